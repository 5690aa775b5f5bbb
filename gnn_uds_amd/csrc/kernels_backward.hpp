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

#include <type_traits>

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

// ---- The activation-folded operator (uds_gat_backward_act): the row pass takes the layer's output `out` and the upstream
// gradient `gout` instead of g, computes g_i = gout_i * act'(out_i) in registers (the formulas and the fp32 operation order of
// autograd.act_grad, contraction off), stores it once for the column pass and adds up its column sums (the bias gradient); the
// column pass also adds up ds_self[j] hx[j, :] and ds_nbr[j] hx[j, :] (the attention-kernel gradients).  Everything else is the
// code of the plain passes: ACT = false compiles to the kernels as they were (one item per workgroup, no loop).
//
// Partials.  A folded pass cuts a snapshot's rows into the row blocks of the plain pass (256 threads each) and numbers the
// blocks of all snapshots in a row: item = s * nb + block.  Workgroup w takes the `per` consecutive items from w * per on,
// per = ceil(items / GAT_ACT_WG_MAX), adds their contributions per thread in item order, then across its rows in LDS in row
// order, and writes ONE partial (d floats in the row pass, 2 d in the column pass).  So a pass writes at most
// GAT_ACT_WG_MAX partials whatever the batch: (1 + 2) * d * GAT_ACT_WG_MAX floats = 1.5 MiB at d = 64, 6 MiB at the largest
// d = 256.  k_gat_bwd_act_reduce sums them in a fixed order.  No atomics; the result does not depend on scheduling.
constexpr int GAT_ACT_WG_MAX = 2048;       // 8 workgroups of 256 threads per CU on 256 CUs

struct GatActPlan {
  int nb, per, wgs;        // row blocks per snapshot, items per workgroup, workgroups
  int64_t items;
};

inline GatActPlan gat_act_plan(int64_t blocks_per_snapshot, int64_t S) {
  GatActPlan p;
  p.nb = (int)blocks_per_snapshot;
  p.items = blocks_per_snapshot * S;
  p.per = (int)((p.items + GAT_ACT_WG_MAX - 1) / GAT_ACT_WG_MAX);
  if (p.per < 1) p.per = 1;
  p.wgs = (int)((p.items + p.per - 1) / p.per);
  return p;
}

struct GatBwdRowsActArgs : GatBwdRowsArgs {        // g of the base is not read
  const float *out, *gout;      // (S, n, d) each
  float *gw;                    // (S, n, d): g for the column pass; NULL for the linear activation (g = gout, nothing to store)
  float *bpart;                 // (wgs, d) partial column sums of g, or NULL (no bias gradient wanted)
  int act, nb, per;
  int64_t items;
};

// dL/dz from dL/dy for y = act(z): autograd.act_grad, one value, every product and difference rounded on its own as the
// element-wise tensor code rounds them.  Contraction is off for this function: gy * (1 - y * y) must not become an FMA (HIP's
// __fmul_rn / __fsub_rn are plain operators, which the default -ffp-contract=fast may still fuse).
__device__ __forceinline__ float act_grad1(int act, float y, float gy) {
#pragma clang fp contract(off)
  switch (act) {
    case UDS_ACT_RELU: return y > 0.0f ? gy : 0.0f;
    case UDS_ACT_TANH: {
      const float yy = y * y, u = 1.0f - yy;
      return gy * u;
    }
    case UDS_ACT_SIGMOID: {
      const float gyy = gy * y, u = 1.0f - y;
      return gyy * u;
    }
    case UDS_ACT_HARD_SIGMOID: {
      const float t = gy * 0.2f;
      return t * (y > 0.0f && y < 1.0f ? 1.0f : 0.0f);
    }
    default: return gy;
  }
}

__device__ __forceinline__ float4 act_grad4(int act, float4 y, float4 gy) {
  return make_float4(act_grad1(act, y.x, gy.x), act_grad1(act, y.y, gy.y), act_grad1(act, y.z, gy.z), act_grad1(act, y.w, gy.w));
}

__device__ __forceinline__ void add4(float4 &a, float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// ACT (k_gat_bwd_rows<true>, GatBwdRowsActArgs): the folded row pass for the widths without a grouped kernel.  `bias` is the
// workgroup's (256 / a.G, d) tile of column sums: d <= 256 and a.G = lanes_per_item(d / 4) keep it within 4096 floats.
// `continue` ends an item: the only one of the plain kernel.
template <bool ACT = false>
__global__ __launch_bounds__(256) void k_gat_bwd_rows(std::conditional_t<ACT, GatBwdRowsActArgs, GatBwdRowsArgs> a) {
  int64_t blk = blockIdx.x, it = 0, it1 = 0;
  int s = blockIdx.y;
  [[maybe_unused]] float4 *bias = nullptr;
  if constexpr (ACT) {
    __shared__ float4 tile[1024];
    bias = tile;
    if (a.bpart) {
      for (int k = threadIdx.x; k < 256 / a.G * a.d4; k += 256) bias[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      __syncthreads();
    }
    it = (int64_t)blockIdx.x * a.per;
    it1 = min(it + a.per, a.items);
  }
  do {
    if constexpr (ACT) {
      blk = it % a.nb;
      s = (int)(it / a.nb);
    }
    const int64_t t = blk * 256 + threadIdx.x;
    const int lg = (int)(t % a.G);
    const int64_t r = t / a.G;
    const bool row_ok = r < a.n;
    const int i = (int)(row_ok ? r : a.n - 1);      // surplus groups shadow the last row (they take part in the shuffles)
    const int beg = a.rowptr[i], end = a.rowptr[i + 1];
    const float *sn = a.s_nbr + (int64_t)s * a.n;
    const float ss = a.s_self[(int64_t)s * a.n + i];
    const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + ((int64_t)s * a.n + i) * a.d4;
    if constexpr (ACT) {
      // this lane's chunks of g_i: computed, stored, and read back below by the lane that stored them.  Slot (row of the block,
      // chunk) of the LDS tile belongs to the one lane that handles that chunk, so the adds need no ordering.
      const int64_t ro = ((int64_t)s * a.n + i) * a.d4;
      g4 = reinterpret_cast<const float4 *>(a.gw ? a.gw : a.gout) + ro;
      if (row_ok && (a.gw || a.bpart)) {
        float4 *b4 = bias + (threadIdx.x / a.G) * a.d4;
        for (int c = lg; c < a.d4; c += a.G) {
          const float4 gv = act_grad4(a.act, reinterpret_cast<const float4 *>(a.out)[ro + c], reinterpret_cast<const float4 *>(a.gout)[ro + c]);
          if (a.gw) reinterpret_cast<float4 *>(a.gw)[ro + c] = gv;
          if (a.bpart) add4(b4[c], gv);
        }
      }
    }
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
      continue;
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
    if (lg != 0 || !row_ok) continue;
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
  } while (ACT && ++it < it1);
  if constexpr (ACT) {
    if (!a.bpart) return;
    __syncthreads();
    const int d = a.d4 * 4;
    if ((int)threadIdx.x < d) {
      const float *b = reinterpret_cast<const float *>(bias);
      float sum = 0.f;
      for (int r = 0; r < 256 / a.G; ++r) sum += b[r * d + threadIdx.x];
      a.bpart[(int64_t)blockIdx.x * d + threadIdx.x] = sum;
    }
  }
}

// Grouped variant (see kernels_sparse.hpp): the G lanes of a row load G entries' indices and scores side by side, each
// lane ends up holding (exp, q, sign) of "its" entry, and alpha / de are written side by side.  Rows of more than G entries
// park the raw (exp, q) pairs in alpha / de per chunk and finish them in a second walk (same lane wrote them).
// EX = true (uds_gat_backward_ex) honours a.mask and a.coef: a masked entry gets weight 0 but stays in every shuffle, the
// row maximum runs over the surviving entries, and q of entry k is multiplied by its coef after the lane reduction (the
// order of k_gat_bwd_rows).  EX = false ignores both (uds_gat_backward; its code is that of the unmasked kernel).
// The workgroup's partial of a folded pass: thread (row r of the block, lane c) holds the sums of chunks c, c + G, .. of its
// rows; the rows are added in LDS in row order and column k of the result goes to part[k].  red: (256 / G, 4 G NC) floats.
template <int G, int NC>
__device__ __forceinline__ void gat_act_block_sum(const float4 (&v)[NC], float4 *red, float *part) {
  constexpr int D4 = G * NC, ROWS = 256 / G;
  const int r = threadIdx.x / G, c = threadIdx.x % G;
#pragma unroll
  for (int q = 0; q < NC; ++q) red[r * D4 + c + G * q] = v[q];
  __syncthreads();
  if ((int)threadIdx.x < 4 * D4) {
    const float *f = reinterpret_cast<const float *>(red);
    float sum = 0.f;
    for (int k = 0; k < ROWS; ++k) sum += f[k * 4 * D4 + threadIdx.x];
    part[threadIdx.x] = sum;
  }
  __syncthreads();
}

// ACT (GatBwdRowsActArgs): g_i is computed from out / gout, stored, and added into the lane's running column sums bsum.
template <int G, int NC, bool EX = false, bool ACT = false>
__global__ __launch_bounds__(256) void k_gat_bwd_rows_g(std::conditional_t<ACT, GatBwdRowsActArgs, GatBwdRowsArgs> a) {
  int64_t blk = blockIdx.x, it = 0, it1 = 0;
  int s = blockIdx.y;
  [[maybe_unused]] float4 bsum[NC];
  if constexpr (ACT) {
#pragma unroll
    for (int q = 0; q < NC; ++q) bsum[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    it = (int64_t)blockIdx.x * a.per;
    it1 = min(it + a.per, a.items);
  }
  do {
    if constexpr (ACT) {
      blk = it % a.nb;
      s = (int)(it / a.nb);
    }
    const int64_t t = blk * 256 + threadIdx.x;
    const int c = (int)(t % G);
    const int64_t r = t / G;
    const bool row_ok = r < a.n;
    const int i = (int)(row_ok ? r : a.n - 1);
    const int beg = a.rowptr[i], end = a.rowptr[i + 1];
    const float *sn = a.s_nbr + (int64_t)s * a.n;
    const float ss = a.s_self[(int64_t)s * a.n + i];
    const float4 *g4 = reinterpret_cast<const float4 *>(a.g) + ((int64_t)s * a.n + i) * a.d4 + c;
    const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
    float *al = a.alpha + (int64_t)s * a.nnz, *de = a.de + (int64_t)s * a.nnz;
    const float *mk = EX && a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
    const float *cf = EX && a.coef ? a.coef + (int64_t)s * a.nnz : nullptr;
    float4 gv[NC];
    if constexpr (ACT) {
      const int64_t ro = ((int64_t)s * a.n + i) * a.d4 + c;
  #pragma unroll
      for (int q = 0; q < NC; ++q) {
        gv[q] = act_grad4(a.act, reinterpret_cast<const float4 *>(a.out)[ro + G * q], reinterpret_cast<const float4 *>(a.gout)[ro + G * q]);
        if (row_ok) {
          if (a.gw) reinterpret_cast<float4 *>(a.gw)[ro + G * q] = gv[q];
          add4(bsum[q], gv[q]);
        }
      }
    } else {
  #pragma unroll
      for (int q = 0; q < NC; ++q) gv[q] = g4[G * q];
    }
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
      continue;
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
  } while (ACT && ++it < it1);
  if constexpr (ACT) {
    __shared__ float4 red[256 * NC];
    if (a.bpart) gat_act_block_sum<G, NC>(bsum, red, a.bpart + (int64_t)blockIdx.x * (4 * G * NC));
  }
}

inline hipError_t launch_gat_bwd_rows(const GatBwdRowsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0 && !a.coef)      // (attention dropout: the plain kernel below)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_rows_g<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
  const int64_t total = (int64_t)a.n * a.G;
  hipLaunchKernelGGL(k_gat_bwd_rows<false>, dim3((unsigned)((total + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
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
  hipLaunchKernelGGL(k_gat_bwd_rows<false>, dim3((unsigned)((total + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
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

// The folded column pass (uds_gat_backward_act) also reads row j of hx -- the lanes that write d_hx_j, one coalesced row read --
// and adds ds_self[j] hx[j, :] and ds_nbr[j] hx[j, :] into the workgroup's partial of the attention-kernel gradients.
struct GatBwdColsActArgs : GatBwdColsArgs {
  const float *hx;
  float *apart;        // (wgs, 2, d) partials: [0] of d a_self, [1] of d a_nbr
  int nb, per;
  int64_t items;
};

__device__ __forceinline__ void fma4(float4 &acc, float w, float4 v) {
  acc.x = fmaf(w, v.x, acc.x);
  acc.y = fmaf(w, v.y, acc.y);
  acc.z = fmaf(w, v.z, acc.z);
  acc.w = fmaf(w, v.w, acc.w);
}

// ACT (k_gat_bwd_cols<true>, GatBwdColsActArgs): a thread keeps ONE chunk for all its items -- a row block is the 256 / d4 whole
// columns that fit 256 threads (d4 <= 64; the threads past them idle), a.nb = ceil(n / (256 / d4)).  Per value the operations
// are the same.
template <bool ACT = false>
__global__ __launch_bounds__(256) void k_gat_bwd_cols(std::conditional_t<ACT, GatBwdColsActArgs, GatBwdColsArgs> a) {
  int64_t blk = blockIdx.x, it = 0, it1 = 0;
  int s = blockIdx.y;
  [[maybe_unused]] float4 ps = make_float4(0.f, 0.f, 0.f, 0.f), pn = ps;
  if constexpr (ACT) {
    it = (int64_t)blockIdx.x * a.per;
    it1 = min(it + a.per, a.items);
  }
  do {
    if constexpr (ACT) {
      blk = it % a.nb;
      s = (int)(it / a.nb);
    }
    const int64_t t = blk * 256 + threadIdx.x;
    int c, j;
    if constexpr (ACT) {
      const int64_t jj = blk * (256 / a.d4) + threadIdx.x / a.d4;
      if ((int)threadIdx.x / a.d4 >= 256 / a.d4 || jj >= a.n) continue;
      c = threadIdx.x % a.d4;
      j = (int)jj;
    } else {
      if (t >= (int64_t)a.n * a.d4) continue;
      c = (int)(t % a.d4);
      j = (int)(t / a.d4);
    }
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
    if constexpr (ACT) {
      if (a.apart) {
        const float4 hv = reinterpret_cast<const float4 *>(a.hx)[((int64_t)s * a.n + j) * a.d4 + c];
        fma4(ps, dss, hv);
        fma4(pn, dsn, hv);
      }
    }
  } while (ACT && ++it < it1);
  if constexpr (ACT) {
    __shared__ float4 red[2][256];
    if (!a.apart) return;
    red[0][threadIdx.x] = ps;      // (an idle thread holds zeros, in a slot past the rows)
    red[1][threadIdx.x] = pn;
    __syncthreads();
    const int d = a.d4 * 4;
    for (int k = threadIdx.x; k < 2 * d; k += 256) {
      const float *f = reinterpret_cast<const float *>(red[k / d]);
      float sum = 0.f;
      for (int r = 0; r < 256 / a.d4; ++r) sum += f[r * d + k % d];
      a.apart[(int64_t)blockIdx.x * 2 * d + k] = sum;
    }
  }
}

// ACT (GatBwdColsActArgs): ps / pn are the lane's running sums of ds_self[j] hx[j, :] and ds_nbr[j] hx[j, :].
template <int G, int NC, bool ACT = false>
__global__ __launch_bounds__(256) void k_gat_bwd_cols_g(std::conditional_t<ACT, GatBwdColsActArgs, GatBwdColsArgs> a) {
  int64_t blk = blockIdx.x, it = 0, it1 = 0;
  int s = blockIdx.y;
  [[maybe_unused]] float4 ps[NC], pn[NC];
  if constexpr (ACT) {
#pragma unroll
    for (int q = 0; q < NC; ++q) ps[q] = pn[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    it = (int64_t)blockIdx.x * a.per;
    it1 = min(it + a.per, a.items);
  }
  do {
    if constexpr (ACT) {
      blk = it % a.nb;
      s = (int)(it / a.nb);
    }
    const int64_t t = blk * 256 + threadIdx.x;
    const int c = (int)(t % G);
    const int64_t r = t / G;
    const bool row_ok = r < a.n;
    const int j = (int)(row_ok ? r : a.n - 1);
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
    if (!row_ok) continue;
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
      if constexpr (ACT) {
        if (a.apart) {
          const float4 hv = reinterpret_cast<const float4 *>(a.hx)[((int64_t)s * a.n + j) * a.d4 + c + G * q];
          fma4(ps[q], dss, hv);
          fma4(pn[q], dsn, hv);
        }
      }
    }
    if (c == 0) a.ds_nbr[(int64_t)s * a.n + j] = dsn;
  } while (ACT && ++it < it1);
  if constexpr (ACT) {
    __shared__ float4 red[256 * NC];
    if (!a.apart) return;
    float *part = a.apart + (int64_t)blockIdx.x * (8 * G * NC);
    gat_act_block_sum<G, NC>(ps, red, part);
    gat_act_block_sum<G, NC>(pn, red, part + 4 * G * NC);
  }
}

// db[k] = sum_w bpart[w, k], da[h, k] = sum_w apart[w, h, k]: 16 outputs per workgroup, 16 lanes per output that each add
// every 16th partial in index order, then the 16 lane sums in lane order (the pattern of k_wgrad_reduce).  db or da may be NULL.
struct GatActReduceArgs {
  const float *bpart, *apart;
  float *db, *da;
  int nb_part, na_part, d;
};

__global__ __launch_bounds__(256) void k_gat_bwd_act_reduce(GatActReduceArgs a) {
  __shared__ float red[256];
  const int tid = threadIdx.x, o = tid & 15, bl = tid >> 4;
  const int i = blockIdx.x * 16 + o;          // [0, d): db, [d, 3 d): da
  const bool bias = i < a.d;
  const bool ok = i < 3 * a.d && (bias ? a.db != nullptr : a.da != nullptr);
  float s = 0.f;
  if (ok) {
    const float *p = bias ? a.bpart + i : a.apart + (i - a.d);
    const int n_part = bias ? a.nb_part : a.na_part;
    const int64_t stride = bias ? a.d : 2 * a.d;
#pragma unroll 8
    for (int b = bl; b < n_part; b += 16) s += p[b * stride];
  }
  red[tid] = s;
  __syncthreads();
  if (tid < 16 && ok) {
    float t = 0.f;
    for (int b = 0; b < 16; ++b) t += red[b * 16 + tid];
    if (bias) a.db[i] = t;
    else a.da[i - a.d] = t;
  }
}


inline hipError_t launch_gat_bwd_cols(const GatBwdColsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_bwd_cols_g<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
  const int64_t total = (int64_t)a.n * a.d4;
  hipLaunchKernelGGL(k_gat_bwd_cols<false>, dim3((unsigned)((total + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// uds_gat_backward_act: folded rows, folded columns, reduce -- three launches.  `parts`: 3 * d * GAT_ACT_WG_MAX floats at most
// (gat_act_plan), the row pass's partials first.  The row pass takes the kernel autograd.GatFn's chain takes, so that d_hx keeps
// its bits: with an edge mask the route of launch_gat_bwd_rows_ex (grouped EX instantiations, coef or not), without one the route
// of launch_gat_bwd_rows (grouped, but the walking kernel when there is a coef: the two differ in the last bits).
// ra / ca carry everything but the plans and the partial pointers; db / da NULL: that gradient is not wanted.
inline hipError_t launch_gat_bwd_act(GatBwdRowsActArgs ra, GatBwdColsActArgs ca, float *db, float *da, float *parts, hipStream_t st) {
  int G, NC;
  group_shape(ra.d4, G, NC);
  const int d = ra.d4 * 4;
  const bool ex = ra.mask != nullptr;
  const bool rows_grouped = G && (ex || !ra.coef);
  const GatActPlan rp = gat_act_plan(((int64_t)ra.n * (rows_grouped ? G : ra.G) + 255) / 256, ra.S);
  const GatActPlan cp = gat_act_plan(G ? ((int64_t)ra.n * G + 255) / 256 : (ra.n + 256 / ra.d4 - 1) / (256 / ra.d4), ra.S);
  ra.nb = rp.nb, ra.per = rp.per, ra.items = rp.items;
  ca.nb = cp.nb, ca.per = cp.per, ca.items = cp.items;
  ra.bpart = db ? parts : nullptr;
  ca.apart = da ? parts + (int64_t)rp.wgs * d : nullptr;
  const dim3 rgrid((unsigned)rp.wgs), cgrid((unsigned)cp.wgs);
  if (rows_grouped) {
    launch_grouped(ra, ra.n, ra.S, ra.d4, st, [&](auto g_, auto nc_, dim3) {
      if (ex) hipLaunchKernelGGL((k_gat_bwd_rows_g<decltype(g_)::value, decltype(nc_)::value, true, true>), rgrid, dim3(256), 0, st, ra);
      else hipLaunchKernelGGL((k_gat_bwd_rows_g<decltype(g_)::value, decltype(nc_)::value, false, true>), rgrid, dim3(256), 0, st, ra);
    });
  } else {
    hipLaunchKernelGGL(k_gat_bwd_rows<true>, rgrid, dim3(256), 0, st, ra);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (G) {
    launch_grouped(ca, ca.n, ca.S, ca.d4, st, [&](auto g_, auto nc_, dim3) {
      hipLaunchKernelGGL((k_gat_bwd_cols_g<decltype(g_)::value, decltype(nc_)::value, true>), cgrid, dim3(256), 0, st, ca);
    });
  } else {
    hipLaunchKernelGGL(k_gat_bwd_cols<true>, cgrid, dim3(256), 0, st, ca);
  }
  e = hipGetLastError();
  if (e != hipSuccess || (!db && !da)) return e;
  GatActReduceArgs rr{ra.bpart, ca.apart, db, da, rp.wgs, cp.wgs, d};
  hipLaunchKernelGGL(k_gat_bwd_act_reduce, dim3((unsigned)((3 * d + 15) / 16)), dim3(256), 0, st, rr);
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
