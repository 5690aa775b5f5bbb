// Reverse-mode kernels of the sparse operators (gfx950) -- the training step, emulator.py:457-484 (GradientTape over
// the layers of emulator.py:18-45,225-230).  The dense parts of the backward pass are row GEMMs (the forward kernels
// with transposed weights) and plain weight-gradient GEMMs; what is specific to the graph operators lives here:
//
//   k_gat_bwd_rows : softmax / leaky-relu backward of GATConv along the rows of the pattern (CSR walk)
//   k_gat_bwd_cols : gradient of the transformed features, gathered along the columns (CSR of the transpose)
//   k_csr_sddmm    : gradient of a per-entry support weight (NodeEdge.weight on its support)
//
// Thread mapping as in kernels_sparse.hpp: no atomics, deterministic results.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_sparse.hpp"

namespace uds {

// Forward (per snapshot): l_ij = leaky(s_self_i + s_nbr_j), alpha_ij = softmax_j(l_ij), pre_i = sum_j alpha_ij hx_j.
// Given g_i = dL/dpre_i:   q_ij = <g_i, hx_j>,  c_i = sum_j alpha_ij q_ij,
//   dl_ij = alpha_ij (q_ij - c_i),  de_ij = dl_ij * leaky'(s_self_i + s_nbr_j),  ds_self_i = sum_j de_ij.
// Writes alpha and de per pattern entry (S x nnz each) for the column pass.
struct GatBwdRowsArgs {
  const int32_t *rowptr, *col;
  const float *g, *hx, *s_self, *s_nbr;
  float *alpha, *de, *ds_self;
  int n, d4, S, G;        // G lanes per row (power of two, <= 64, <= d4 rounded down)
  int64_t nnz;
  // attention dropout (k_gat_aggregate_coef): pre_i = sum_j alpha_ij m_ij hx_j with m (S, nnz) = 0 or 1 / (1 - rate), else NULL.
  // Then q_ij = m_ij <g_i, hx_j> in the formulas above, and the alpha handed to the column pass is alpha_ij m_ij.
  const float *coef;
  // per-snapshot edge mask (S, nnz) of uds_gat_backward_ex (use_adj), else NULL: entry p of snapshot s takes part iff
  // mask != 0 or p is the row's diagonal.  The softmax runs over the surviving entries; a masked entry gets alpha = de = 0,
  // so the column pass needs no change.
  const float *mask;
};

__global__ __launch_bounds__(256) void k_gat_bwd_rows(GatBwdRowsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lg = (int)(t % a.G);
  const int64_t r = t / a.G;
  const bool row_ok = r < a.n;
  const int i = (int)(row_ok ? r : a.n - 1);      // surplus groups shadow the last row (they take part in the shuffles)
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + ((int64_t)s * a.n + i) * a.d4;
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4;
  float *al = a.alpha + (int64_t)s * a.nnz, *de = a.de + (int64_t)s * a.nnz;
  const float *cf = a.coef ? a.coef + (int64_t)s * a.nnz : nullptr;
  const float *mk = a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
  float m = -INFINITY;
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    if (!mk || mk[p] != 0.0f || j == i) m = fmaxf(m, leaky02(ss + sn[j]));
  }
  float den = 0.f, cn = 0.f;
  if (end - beg <= a.G) {
    // the usual case (degree <= lanes per row): lane k of the row keeps entry k's (exp, q, logit sign) in registers, the
    // row sums are known to every lane after the loop, and the lanes write alpha / de of their entries side by side --
    // no second walk through memory by one lane.  Same operation order per value as the general path below.
    float wk = 0.f, qk = 0.f;
    bool pos = false, onk = true;
    for (int p = beg; p < end; ++p) {
      const int j = a.col[p];
      const float lgt = ss + sn[j];
      const bool on = !mk || mk[p] != 0.0f || j == i;
      const float w = on ? expf(leaky02(lgt) - m) : 0.f;       // a masked entry: weight 0, alpha = de = 0 below
      float q = 0.f;
      for (int c = lg; c < a.d4; c += a.G) {
        const float4 gv = g4[c], hv = hx4[(int64_t)j * a.d4 + c];
        q = fmaf(gv.x, hv.x, fmaf(gv.y, hv.y, fmaf(gv.z, hv.z, fmaf(gv.w, hv.w, q))));
      }
      for (int o = a.G >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
      if (cf) q *= cf[p];
      den += w;
      cn = fmaf(w, q, cn);
      if (p - beg == lg) {
        wk = w;
        qk = q;
        pos = lgt > 0.0f;
        onk = on;
      }
    }
    const float inv = (mk ? den > 0.0f : end > beg) ? 1.0f / den : 0.0f;     // (a row with every entry masked: den = 0)
    const float cbar = cn * inv;
    const bool mine = lg < end - beg;
    const float w = wk * inv;
    const float dl = w * (qk - cbar);
    const float dv = mine && onk ? (pos ? dl : 0.2f * dl) : 0.f;
    if (mine && row_ok) {
      al[beg + lg] = cf ? w * cf[beg + lg] : w;
      de[beg + lg] = dv;
    }
    // ds_self = sum of the row's de in entry order (the order the one-lane walk below adds them in)
    float dss = 0.f;
    for (int k = 0; k < end - beg; ++k) dss += __shfl(dv, k, a.G);
    if (lg == 0 && row_ok) a.ds_self[(int64_t)s * a.n + i] = dss;
    return;
  }
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    const float w = !mk || mk[p] != 0.0f || j == i ? expf(leaky02(ss + sn[j]) - m) : 0.f;
    float q = 0.f;
    for (int c = lg; c < a.d4; c += a.G) {
      const float4 gv = g4[c], hv = hx4[(int64_t)j * a.d4 + c];
      q = fmaf(gv.x, hv.x, fmaf(gv.y, hv.y, fmaf(gv.z, hv.z, fmaf(gv.w, hv.w, q))));
    }
    for (int o = a.G >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (cf) q *= cf[p];
    den += w;
    cn = fmaf(w, q, cn);
    if (lg == 0 && row_ok) {
      al[p] = w;
      de[p] = q;
    }
  }
  if (lg != 0 || !row_ok) return;
  const float inv = (mk ? den > 0.0f : end > beg) ? 1.0f / den : 0.0f;
  const float cbar = cn * inv;
  float dss = 0.f;
  for (int p = beg; p < end; ++p) {       // same lane wrote al / de above
    const float w = al[p] * inv;
    const float dl = w * (de[p] - cbar);
    const int j = a.col[p];
    const float dv = mk && !(mk[p] != 0.0f || j == i) ? 0.f : (ss + sn[j] > 0.0f ? dl : 0.2f * dl);
    al[p] = cf ? w * cf[p] : w;
    de[p] = dv;
    dss += dv;
  }
  a.ds_self[(int64_t)s * a.n + i] = dss;
}

// Grouped variant (see kernels_sparse.hpp): the G lanes of a row load G entries' indices and scores side by side, each
// lane ends up holding (exp, q, sign) of "its" entry, and alpha / de are written side by side.  Rows of more than G entries
// park the raw (exp, q) pairs in alpha / de per chunk and finish them in a second walk (same lane wrote them).
// EX = true (uds_gat_backward_ex) honours a.mask and a.coef: a masked entry gets weight 0 but stays in every shuffle, the
// row maximum runs over the surviving entries, and q of entry k is multiplied by its coef after the lane reduction (the
// order of k_gat_bwd_rows).  EX = false ignores both (uds_gat_backward; its code is that of the unmasked kernel).
template <int G, int NC, bool EX = false>
__global__ __launch_bounds__(256) void k_gat_bwd_rows_g(GatBwdRowsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % G);
  const int64_t r = t / G;
  const bool row_ok = r < a.n;
  const int i = (int)(row_ok ? r : a.n - 1);
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + ((int64_t)s * a.n + i) * a.d4 + c;
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
  float *al = a.alpha + (int64_t)s * a.nnz, *de = a.de + (int64_t)s * a.nnz;
  const float *mk = EX && a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
  const float *cf = EX && a.coef ? a.coef + (int64_t)s * a.nnz : nullptr;
  float4 gv[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) gv[q] = g4[G * q];
  float m = -INFINITY, l0 = 0.f, c0 = 1.f;
  int j0 = 0;
  bool on0 = true;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    const int pc = min(p, end - 1);
    const int j = a.col[pc];
    const float lgt = ss + sn[j];
    bool on = p < end;
    if (EX && mk) on = on && (mk[pc] != 0.0f || j == i);
    if (b0 == beg) {
      j0 = j;
      l0 = lgt;
      on0 = on;
      if (EX && cf) c0 = cf[pc];
    }
    m = fmaxf(m, on ? leaky02(lgt) : -INFINITY);
  }
  m = group_max<G>(m);
  const bool single = end - beg <= G;
  float den = 0.f, cn = 0.f, wk = 0.f, qk = 0.f, lk = 0.f, ck = 1.f;
  bool onk = true;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    int j = j0;
    float lgt = l0, cv = c0;
    bool on = on0;
    if (b0 != beg) {
      const int pc = min(p, end - 1);
      j = a.col[pc];
      lgt = ss + sn[j];
      on = p < end;
      if (EX && mk) on = on && (mk[pc] != 0.0f || j == i);
      if (EX && cf) cv = cf[pc];
    }
    const float w = (EX ? on : p < end) ? expf(leaky02(lgt) - m) : 0.f;
    const int nk = min(G, end - b0);
    float qm = 0.f;
    for (int k0 = 0; k0 < nk; k0 += GU) {
      float ww[GU], qq[GU], cc[GU];
      float4 hv[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int k = min(k0 + u, nk - 1);
        const int jj = __shfl(j, k, G);
        ww[u] = __shfl(w, k, G);
        if (EX && cf) cc[u] = __shfl(cv, k, G);
#pragma unroll
        for (int v = 0; v < NC; ++v) hv[u][v] = hx4[(int64_t)jj * a.d4 + G * v];
      }
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < NC; ++v)      // the one-lane-per-chunk kernel adds a lane's chunks c, c + G, .. in this order
          q = fmaf(gv[v].x, hv[u][v].x, fmaf(gv[v].y, hv[u][v].y, fmaf(gv[v].z, hv[u][v].z, fmaf(gv[v].w, hv[u][v].w, q))));
        qq[u] = q;
      }
#pragma unroll
      for (int o = G >> 1; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < GU; ++u) qq[u] += __shfl_xor(qq[u], o);
      if (EX && cf)
#pragma unroll
        for (int u = 0; u < GU; ++u) qq[u] *= cc[u];
#pragma unroll
      for (int u = 0; u < GU; ++u)
        if (k0 + u < nk) {
          den += ww[u];
          cn = fmaf(ww[u], qq[u], cn);
          if (k0 + u == c) qm = qq[u];
        }
    }
    if (single) {
      wk = w;
      qk = qm;
      lk = lgt;
      ck = cv;
      onk = on;
    } else if (p < end && row_ok) {
      al[p] = w;
      de[p] = qm;
    }
  }
  const float inv = (EX ? den > 0.0f : end > beg) ? 1.0f / den : 0.0f;
  const float cbar = cn * inv;
  if (single) {
    const bool mine = c < end - beg;
    const float w = wk * inv;
    const float dl = w * (qk - cbar);
    const float dv = (EX ? mine && onk : mine) ? (lk > 0.0f ? dl : 0.2f * dl) : 0.f;
    if (mine && row_ok) {
      al[beg + c] = EX && cf ? w * ck : w;
      de[beg + c] = dv;
    }
    float dss = 0.f;
    for (int k = 0; k < end - beg; ++k) dss += __shfl(dv, k, G);      // entry order, as the one-lane walk adds them
    if (c == 0 && row_ok) a.ds_self[(int64_t)s * a.n + i] = dss;
    return;
  }
  float dss = 0.f;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    float dv = 0.f;
    if (p < end && row_ok) {
      const float w = al[p] * inv;        // EX: a masked entry parked exp = 0, so w = 0 and dl = +-0
      const float dl = w * (de[p] - cbar);
      const int j = a.col[p];
      dv = EX && mk && !(mk[p] != 0.0f || j == i) ? 0.f : (ss + sn[j] > 0.0f ? dl : 0.2f * dl);
      al[p] = EX && cf ? w * cf[p] : w;
      de[p] = dv;
    }
    dss += dv;
  }
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) dss += __shfl_xor(dss, o);
  if (c == 0 && row_ok) a.ds_self[(int64_t)s * a.n + i] = dss;
}

inline hipError_t launch_gat_bwd_rows(const GatBwdRowsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0 && !a.coef)      // (attention dropout: the plain kernel below)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_rows_g<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
  const int64_t total = (int64_t)a.n * a.G;
  hipLaunchKernelGGL(k_gat_bwd_rows, dim3((unsigned)((total + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// uds_gat_backward_ex: the grouped EX instantiations (mask and / or coef), the walking kernel for the other widths.
inline hipError_t launch_gat_bwd_rows_ex(const GatBwdRowsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_rows_g<decltype(g_)::value, decltype(nc_)::value, true>), grid, dim3(256), 0, st, a);
    });
  const int64_t total = (int64_t)a.n * a.G;
  hipLaunchKernelGGL(k_gat_bwd_rows, dim3((unsigned)((total + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// d_hx_j = sum_{i : j in row i} alpha_ij g_i + a_nbr * ds_nbr_j + a_self * ds_self_j,   ds_nbr_j = sum_i de_ij.
// (rowptr_t, col_t) = CSR of the transposed pattern; perm_t[p] = position of that entry in the row-major arrays.
struct GatBwdColsArgs {
  const int32_t *rowptr_t, *col_t, *perm_t;
  const float *g, *alpha, *de, *ds_self, *a_self, *a_nbr;
  float *d_hx, *ds_nbr;
  int n, d4, S;
  int64_t nnz;
};

__global__ __launch_bounds__(256) void k_gat_bwd_cols(GatBwdColsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.n * a.d4) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.d4), j = (int)(t / a.d4);
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + (int64_t)s * a.n * a.d4 + c;
  const float *al = a.alpha + (int64_t)s * a.nnz, *de = a.de + (int64_t)s * a.nnz;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float dsn = 0.f;
  for (int p = a.rowptr_t[j]; p < a.rowptr_t[j + 1]; ++p) {
    const int i = a.col_t[p], k = a.perm_t[p];
    const float w = al[k];
    const float4 gv = g4[(int64_t)i * a.d4];
    acc.x = fmaf(w, gv.x, acc.x);
    acc.y = fmaf(w, gv.y, acc.y);
    acc.z = fmaf(w, gv.z, acc.z);
    acc.w = fmaf(w, gv.w, acc.w);
    dsn += de[k];
  }
  const float dss = a.ds_self[(int64_t)s * a.n + j];
  const float4 as = reinterpret_cast<const float4 *>(a.a_self)[c], an = reinterpret_cast<const float4 *>(a.a_nbr)[c];
  acc.x = fmaf(an.x, dsn, fmaf(as.x, dss, acc.x));
  acc.y = fmaf(an.y, dsn, fmaf(as.y, dss, acc.y));
  acc.z = fmaf(an.z, dsn, fmaf(as.z, dss, acc.z));
  acc.w = fmaf(an.w, dsn, fmaf(as.w, dss, acc.w));
  reinterpret_cast<float4 *>(a.d_hx)[((int64_t)s * a.n + j) * a.d4 + c] = acc;
  if (c == 0) a.ds_nbr[(int64_t)s * a.n + j] = dsn;
}

template <int G, int NC>
__global__ __launch_bounds__(256) void k_gat_bwd_cols_g(GatBwdColsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % G);
  const int64_t r = t / G;
  const bool row_ok = r < a.n;
  const int j = (int)(row_ok ? r : a.n - 1);
  const int s = blockIdx.y;
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + (int64_t)s * a.n * a.d4 + c;
  const float *al = a.alpha + (int64_t)s * a.nnz, *de = a.de + (int64_t)s * a.nnz;
  float4 acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  float dsn = 0.f;
  const int beg = a.rowptr_t[j], end = a.rowptr_t[j + 1];
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = min(b0 + c, end - 1);
    const int i = a.col_t[p], k = a.perm_t[p];
    const float w = al[k], d = de[k];
    const int nk = min(G, end - b0);
    for (int e0 = 0; e0 < nk; e0 += GU) {
      float ww[GU], dd[GU];
      float4 gv[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int e = min(e0 + u, nk - 1);
        const int ii = __shfl(i, e, G);
        ww[u] = __shfl(w, e, G);
        dd[u] = __shfl(d, e, G);
#pragma unroll
        for (int q = 0; q < NC; ++q) gv[u][q] = g4[(int64_t)ii * a.d4 + G * q];
      }
#pragma unroll
      for (int u = 0; u < GU; ++u)
        if (e0 + u < nk) {
          dsn += dd[u];
#pragma unroll
          for (int q = 0; q < NC; ++q) {
            acc[q].x = fmaf(ww[u], gv[u][q].x, acc[q].x);
            acc[q].y = fmaf(ww[u], gv[u][q].y, acc[q].y);
            acc[q].z = fmaf(ww[u], gv[u][q].z, acc[q].z);
            acc[q].w = fmaf(ww[u], gv[u][q].w, acc[q].w);
          }
        }
    }
  }
  if (!row_ok) return;
  const float dss = a.ds_self[(int64_t)s * a.n + j];
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const float4 as = reinterpret_cast<const float4 *>(a.a_self)[c + G * q], an = reinterpret_cast<const float4 *>(a.a_nbr)[c + G * q];
    float4 o;
    o.x = fmaf(an.x, dsn, fmaf(as.x, dss, acc[q].x));
    o.y = fmaf(an.y, dsn, fmaf(as.y, dss, acc[q].y));
    o.z = fmaf(an.z, dsn, fmaf(as.z, dss, acc[q].z));
    o.w = fmaf(an.w, dsn, fmaf(as.w, dss, acc[q].w));
    reinterpret_cast<float4 *>(a.d_hx)[((int64_t)s * a.n + j) * a.d4 + c + G * q] = o;
  }
  if (c == 0) a.ds_nbr[(int64_t)s * a.n + j] = dsn;
}

inline hipError_t launch_gat_bwd_cols(const GatBwdColsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_cols_g<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
  const int64_t total = (int64_t)a.n * a.d4;
  hipLaunchKernelGGL(k_gat_bwd_cols, dim3((unsigned)((total + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// Reverse mode of the multi-head aggregation (uds_gat_backward_heads; layouts as GatHeadsArgs in kernels_sparse.hpp).  A work
// item is one (row, head) in the row pass and one (column, head) in the column pass; alpha / de are (S, H, nnz), ds_* (S, n, H).
// The upstream gradient is (S, n, H * C) for the concatenation; for the mean it is (S, n, C) and every head reads it scaled by
// 1 / H (gscale).  Per head the operations are those of k_gat_bwd_rows_g<G, NC, true> / k_gat_bwd_rows and k_gat_bwd_cols[_g]:
// H = 1 with concatenation is bitwise equal to uds_gat_backward_ex.
struct GatBwdHeadsArgs {
  const int32_t *rowptr, *col, *rowptr_t, *col_t, *perm_t;
  const float *g, *hx, *s_self, *s_nbr, *a_self, *a_nbr, *mask, *coef;
  float *alpha, *de, *d_hx, *ds_self, *ds_nbr;
  int n, H, c4, S, G, mean;       // G: lanes per item of the walking row pass (lanes_per_item(c4))
  int64_t nnz;
};

__device__ __forceinline__ float4 scaled(float4 v, float f) { return make_float4(v.x * f, v.y * f, v.z * f, v.w * f); }

template <int G, int NC>
__global__ __launch_bounds__(256) void k_gat_bwd_rows_hg(GatBwdHeadsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % G);
  const int64_t items = (int64_t)a.n * a.H;
  const bool row_ok = t / G < items;
  const int64_t it = row_ok ? t / G : items - 1;
  const int i = (int)(it / a.H), h = (int)(it % a.H);
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const int rs = a.H * a.c4;
  const float *sn = a.s_nbr + (int64_t)s * a.n * a.H + h;
  const float ss = a.s_self[((int64_t)s * a.n + i) * a.H + h];
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + (a.mean ? ((int64_t)s * a.n + i) * a.c4 : ((int64_t)s * a.n + i) * rs + h * a.c4) + c;
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * rs + h * a.c4 + c;
  float *al = a.alpha + ((int64_t)s * a.H + h) * a.nnz, *de = a.de + ((int64_t)s * a.H + h) * a.nnz;
  const float *mk = a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
  const float *cf = a.coef ? a.coef + ((int64_t)s * a.H + h) * a.nnz : nullptr;
  float4 gv[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) gv[q] = g4[G * q];
  if (a.mean) {
    const float rh = 1.0f / (float)a.H;
#pragma unroll
    for (int q = 0; q < NC; ++q) gv[q] = scaled(gv[q], rh);
  }
  float m = -INFINITY, l0 = 0.f, c0 = 1.f;
  int j0 = 0;
  bool on0 = true;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    const int pc = min(p, end - 1);
    const int j = a.col[pc];
    const float lgt = ss + sn[(int64_t)j * a.H];
    bool on = p < end;
    if (mk) on = on && (mk[pc] != 0.0f || j == i);
    if (b0 == beg) {
      j0 = j;
      l0 = lgt;
      on0 = on;
      if (cf) c0 = cf[pc];
    }
    m = fmaxf(m, on ? leaky02(lgt) : -INFINITY);
  }
  m = group_max<G>(m);
  const bool single = end - beg <= G;
  float den = 0.f, cn = 0.f, wk = 0.f, qk = 0.f, lk = 0.f, ck = 1.f;
  bool onk = true;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    int j = j0;
    float lgt = l0, cv = c0;
    bool on = on0;
    if (b0 != beg) {
      const int pc = min(p, end - 1);
      j = a.col[pc];
      lgt = ss + sn[(int64_t)j * a.H];
      on = p < end;
      if (mk) on = on && (mk[pc] != 0.0f || j == i);
      if (cf) cv = cf[pc];
    }
    const float w = on ? expf(leaky02(lgt) - m) : 0.f;
    const int nk = min(G, end - b0);
    float qm = 0.f;
    for (int k0 = 0; k0 < nk; k0 += GU) {
      float ww[GU], qq[GU], cc[GU];
      float4 hv[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int k = min(k0 + u, nk - 1);
        const int jj = __shfl(j, k, G);
        ww[u] = __shfl(w, k, G);
        if (cf) cc[u] = __shfl(cv, k, G);
#pragma unroll
        for (int v = 0; v < NC; ++v) hv[u][v] = hx4[(int64_t)jj * rs + G * v];
      }
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < NC; ++v)
          q = fmaf(gv[v].x, hv[u][v].x, fmaf(gv[v].y, hv[u][v].y, fmaf(gv[v].z, hv[u][v].z, fmaf(gv[v].w, hv[u][v].w, q))));
        qq[u] = q;
      }
#pragma unroll
      for (int o = G >> 1; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < GU; ++u) qq[u] += __shfl_xor(qq[u], o);
      if (cf)
#pragma unroll
        for (int u = 0; u < GU; ++u) qq[u] *= cc[u];
#pragma unroll
      for (int u = 0; u < GU; ++u)
        if (k0 + u < nk) {
          den += ww[u];
          cn = fmaf(ww[u], qq[u], cn);
          if (k0 + u == c) qm = qq[u];
        }
    }
    if (single) {
      wk = w;
      qk = qm;
      lk = lgt;
      ck = cv;
      onk = on;
    } else if (p < end && row_ok) {
      al[p] = w;
      de[p] = qm;
    }
  }
  const float inv = den > 0.0f ? 1.0f / den : 0.0f;
  const float cbar = cn * inv;
  float *dss_out = a.ds_self + ((int64_t)s * a.n + i) * a.H + h;
  if (single) {
    const bool mine = c < end - beg;
    const float w = wk * inv;
    const float dl = w * (qk - cbar);
    const float dv = mine && onk ? (lk > 0.0f ? dl : 0.2f * dl) : 0.f;
    if (mine && row_ok) {
      al[beg + c] = cf ? w * ck : w;
      de[beg + c] = dv;
    }
    float dss = 0.f;
    for (int k = 0; k < end - beg; ++k) dss += __shfl(dv, k, G);
    if (c == 0 && row_ok) *dss_out = dss;
    return;
  }
  float dss = 0.f;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    float dv = 0.f;
    if (p < end && row_ok) {
      const float w = al[p] * inv;
      const float dl = w * (de[p] - cbar);
      const int j = a.col[p];
      dv = mk && !(mk[p] != 0.0f || j == i) ? 0.f : (ss + sn[(int64_t)j * a.H] > 0.0f ? dl : 0.2f * dl);
      al[p] = cf ? w * cf[p] : w;
      de[p] = dv;
    }
    dss += dv;
  }
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) dss += __shfl_xor(dss, o);
  if (c == 0 && row_ok) *dss_out = dss;
}

// The walking row pass per (row, head): a.G lanes per item, the operations of k_gat_bwd_rows.
__global__ __launch_bounds__(256) void k_gat_bwd_rows_hx(GatBwdHeadsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lg = (int)(t % a.G);
  const int64_t items = (int64_t)a.n * a.H;
  const bool row_ok = t / a.G < items;
  const int64_t it = row_ok ? t / a.G : items - 1;
  const int i = (int)(it / a.H), h = (int)(it % a.H);
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const int rs = a.H * a.c4;
  const float *sn = a.s_nbr + (int64_t)s * a.n * a.H + h;
  const float ss = a.s_self[((int64_t)s * a.n + i) * a.H + h];
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + (a.mean ? ((int64_t)s * a.n + i) * a.c4 : ((int64_t)s * a.n + i) * rs + h * a.c4);
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * rs + h * a.c4;
  float *al = a.alpha + ((int64_t)s * a.H + h) * a.nnz, *de = a.de + ((int64_t)s * a.H + h) * a.nnz;
  const float *mk = a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
  const float *cf = a.coef ? a.coef + ((int64_t)s * a.H + h) * a.nnz : nullptr;
  const float gscale = 1.0f / (float)a.H;
  float *dss_out = a.ds_self + ((int64_t)s * a.n + i) * a.H + h;
  float m = -INFINITY;
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    if (!mk || mk[p] != 0.0f || j == i) m = fmaxf(m, leaky02(ss + sn[(int64_t)j * a.H]));
  }
  float den = 0.f, cn = 0.f;
  const bool single = end - beg <= a.G;
  float wk = 0.f, qk = 0.f;
  bool pos = false, onk = true;
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    const float lgt = ss + sn[(int64_t)j * a.H];
    const bool on = !mk || mk[p] != 0.0f || j == i;
    const float w = on ? expf(leaky02(lgt) - m) : 0.f;
    float q = 0.f;
    for (int c = lg; c < a.c4; c += a.G) {
      float4 gv = g4[c];
      if (a.mean) gv = scaled(gv, gscale);
      const float4 hv = hx4[(int64_t)j * rs + c];
      q = fmaf(gv.x, hv.x, fmaf(gv.y, hv.y, fmaf(gv.z, hv.z, fmaf(gv.w, hv.w, q))));
    }
    for (int o = a.G >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (cf) q *= cf[p];
    den += w;
    cn = fmaf(w, q, cn);
    if (single) {
      if (p - beg == lg) {
        wk = w;
        qk = q;
        pos = lgt > 0.0f;
        onk = on;
      }
    } else if (lg == 0 && row_ok) {
      al[p] = w;
      de[p] = q;
    }
  }
  const float inv = den > 0.0f ? 1.0f / den : 0.0f;
  const float cbar = cn * inv;
  if (single) {
    const bool mine = lg < end - beg;
    const float w = wk * inv;
    const float dl = w * (qk - cbar);
    const float dv = mine && onk ? (pos ? dl : 0.2f * dl) : 0.f;
    if (mine && row_ok) {
      al[beg + lg] = cf ? w * cf[beg + lg] : w;
      de[beg + lg] = dv;
    }
    float dss = 0.f;
    for (int k = 0; k < end - beg; ++k) dss += __shfl(dv, k, a.G);
    if (lg == 0 && row_ok) *dss_out = dss;
    return;
  }
  if (lg != 0 || !row_ok) return;
  float dss = 0.f;
  for (int p = beg; p < end; ++p) {       // same lane wrote al / de above
    const float w = al[p] * inv;
    const float dl = w * (de[p] - cbar);
    const int j = a.col[p];
    const float dv = mk && !(mk[p] != 0.0f || j == i) ? 0.f : (ss + sn[(int64_t)j * a.H] > 0.0f ? dl : 0.2f * dl);
    al[p] = cf ? w * cf[p] : w;
    de[p] = dv;
    dss += dv;
  }
  *dss_out = dss;
}

template <int G, int NC>
__global__ __launch_bounds__(256) void k_gat_bwd_cols_hg(GatBwdHeadsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % G);
  const int64_t items = (int64_t)a.n * a.H;
  const bool row_ok = t / G < items;
  const int64_t it = row_ok ? t / G : items - 1;
  const int j = (int)(it / a.H), h = (int)(it % a.H);
  const int s = blockIdx.y;
  const int rs = a.H * a.c4, gs = a.mean ? a.c4 : rs;
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + (int64_t)s * a.n * gs + (a.mean ? 0 : h * a.c4) + c;
  const float *al = a.alpha + ((int64_t)s * a.H + h) * a.nnz, *de = a.de + ((int64_t)s * a.H + h) * a.nnz;
  const float gscale = 1.0f / (float)a.H;
  float4 acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  float dsn = 0.f;
  const int beg = a.rowptr_t[j], end = a.rowptr_t[j + 1];
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = min(b0 + c, end - 1);
    const int i = a.col_t[p], k = a.perm_t[p];
    const float w = al[k], d = de[k];
    const int nk = min(G, end - b0);
    for (int e0 = 0; e0 < nk; e0 += GU) {
      float ww[GU], dd[GU];
      float4 gv[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int e = min(e0 + u, nk - 1);
        const int ii = __shfl(i, e, G);
        ww[u] = __shfl(w, e, G);
        dd[u] = __shfl(d, e, G);
#pragma unroll
        for (int q = 0; q < NC; ++q) {
          gv[u][q] = g4[(int64_t)ii * gs + G * q];
          if (a.mean) gv[u][q] = scaled(gv[u][q], gscale);
        }
      }
#pragma unroll
      for (int u = 0; u < GU; ++u)
        if (e0 + u < nk) {
          dsn += dd[u];
#pragma unroll
          for (int q = 0; q < NC; ++q) {
            acc[q].x = fmaf(ww[u], gv[u][q].x, acc[q].x);
            acc[q].y = fmaf(ww[u], gv[u][q].y, acc[q].y);
            acc[q].z = fmaf(ww[u], gv[u][q].z, acc[q].z);
            acc[q].w = fmaf(ww[u], gv[u][q].w, acc[q].w);
          }
        }
    }
  }
  if (!row_ok) return;
  const float dss = a.ds_self[((int64_t)s * a.n + j) * a.H + h];
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const float4 as = reinterpret_cast<const float4 *>(a.a_self)[h * a.c4 + c + G * q];
    const float4 an = reinterpret_cast<const float4 *>(a.a_nbr)[h * a.c4 + c + G * q];
    float4 o;
    o.x = fmaf(an.x, dsn, fmaf(as.x, dss, acc[q].x));
    o.y = fmaf(an.y, dsn, fmaf(as.y, dss, acc[q].y));
    o.z = fmaf(an.z, dsn, fmaf(as.z, dss, acc[q].z));
    o.w = fmaf(an.w, dsn, fmaf(as.w, dss, acc[q].w));
    reinterpret_cast<float4 *>(a.d_hx)[((int64_t)s * a.n + j) * rs + h * a.c4 + c + G * q] = o;
  }
  if (c == 0) a.ds_nbr[((int64_t)s * a.n + j) * a.H + h] = dsn;
}

__global__ __launch_bounds__(256) void k_gat_bwd_cols_hx(GatBwdHeadsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.n * a.H * a.c4) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.c4);
  const int64_t it = t / a.c4;
  const int j = (int)(it / a.H), h = (int)(it % a.H);
  const int rs = a.H * a.c4, gs = a.mean ? a.c4 : rs;
  const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + (int64_t)s * a.n * gs + (a.mean ? 0 : h * a.c4) + c;
  const float *al = a.alpha + ((int64_t)s * a.H + h) * a.nnz, *de = a.de + ((int64_t)s * a.H + h) * a.nnz;
  const float gscale = 1.0f / (float)a.H;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float dsn = 0.f;
  for (int p = a.rowptr_t[j]; p < a.rowptr_t[j + 1]; ++p) {
    const int i = a.col_t[p], k = a.perm_t[p];
    const float w = al[k];
    float4 gv = g4[(int64_t)i * gs];
    if (a.mean) gv = scaled(gv, gscale);
    acc.x = fmaf(w, gv.x, acc.x);
    acc.y = fmaf(w, gv.y, acc.y);
    acc.z = fmaf(w, gv.z, acc.z);
    acc.w = fmaf(w, gv.w, acc.w);
    dsn += de[k];
  }
  const float dss = a.ds_self[((int64_t)s * a.n + j) * a.H + h];
  const float4 as = reinterpret_cast<const float4 *>(a.a_self)[h * a.c4 + c], an = reinterpret_cast<const float4 *>(a.a_nbr)[h * a.c4 + c];
  acc.x = fmaf(an.x, dsn, fmaf(as.x, dss, acc.x));
  acc.y = fmaf(an.y, dsn, fmaf(as.y, dss, acc.y));
  acc.z = fmaf(an.z, dsn, fmaf(as.z, dss, acc.z));
  acc.w = fmaf(an.w, dsn, fmaf(as.w, dss, acc.w));
  reinterpret_cast<float4 *>(a.d_hx)[((int64_t)s * a.n + j) * rs + h * a.c4 + c] = acc;
  if (c == 0) a.ds_nbr[((int64_t)s * a.n + j) * a.H + h] = dsn;
}

inline hipError_t launch_gat_bwd_heads(const GatBwdHeadsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.c4, G, NC);
  const int64_t items = (int64_t)a.n * a.H;
  if (G) {
    hipError_t e = launch_grouped(a, items, a.S, a.c4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_rows_hg<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
    if (e != hipSuccess) return e;
    return launch_grouped(a, items, a.S, a.c4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_cols_hg<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
  }
  hipLaunchKernelGGL(k_gat_bwd_rows_hx, dim3((unsigned)((items * a.G + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_gat_bwd_cols_hx, dim3((unsigned)((items * a.c4 + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// out[k] = sum_s <a[s, row(k), :], b[s, col(k), :]> for every pattern entry k: the gradient of a per-entry weight of
// out = A(val) @ x  (a = dL/dout, b = x).  G lanes per entry walk the snapshots.
struct SddmmArgs {
  const int32_t *row, *col;
  const float *a, *b;
  float *out;
  int n_rows, n_cols, f4, S, G;
  int64_t nnz;
};

__global__ __launch_bounds__(256) void k_csr_sddmm(SddmmArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lg = (int)(t % a.G);
  const int64_t e = t / a.G;
  const bool ok = e < a.nnz;
  const int64_t k = ok ? e : a.nnz - 1;
  const int r = a.row[k], c = a.col[k];
  const float4 *a4 = reinterpret_cast<const float4 *>(a.a) + (int64_t)r * a.f4;
  const float4 *b4 = reinterpret_cast<const float4 *>(a.b) + (int64_t)c * a.f4;
  float q = 0.f;
  for (int s = 0; s < a.S; ++s) {
    const float4 *as = a4 + (int64_t)s * a.n_rows * a.f4, *bs = b4 + (int64_t)s * a.n_cols * a.f4;
    for (int f = lg; f < a.f4; f += a.G) {
      const float4 av = as[f], bv = bs[f];
      q = fmaf(av.x, bv.x, fmaf(av.y, bv.y, fmaf(av.z, bv.z, fmaf(av.w, bv.w, q))));
    }
  }
  for (int o = a.G >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
  if (lg == 0 && ok) a.out[k] = q;
}

inline hipError_t launch_csr_sddmm(const SddmmArgs &a, hipStream_t st) {
  const int64_t total = a.nnz * a.G;
  hipLaunchKernelGGL(k_csr_sddmm, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

inline int lanes_per_item(int f4) {     // largest power of two <= min(f4, 16)
  int g = 1;
  while (g * 2 <= f4 && g * 2 <= 16) g *= 2;
  return g;
}

}  // namespace uds
