// CSR gather kernels (gfx950): weighted neighbour sum (NodeEdge support / GCN / incidence balance)
// and the GAT segmented softmax + aggregation (Spektral GATConv K5+K6, via emulator.py:229-230).
//
// Thread mapping: one lane owns one float4 feature chunk of one destination row, so a row of
// F floats is read by F/4 adjacent lanes with 16-B accesses (a 64-float row = one 256-B request
// from 16 lanes).  Rows are visited in the degree-sorted schedule of the handle so the lanes of
// a wave run equal trip counts.  No cross-lane traffic, no atomics: results are deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_dense.hpp"

namespace uds {

struct SpmmArgs {
  const int32_t *rowptr, *col, *order;
  const float *val, *x, *bias;
  float *out;
  int n_rows, n_cols, f4, act, S;
};

__global__ __launch_bounds__(256) void k_csr_spmm(SpmmArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_snap = (int64_t)a.n_rows * a.f4;
  if (t >= per_snap) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.f4);
  const int i = a.order[t / a.f4];
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float4 *x4 = reinterpret_cast<const float4 *>(a.x) + (int64_t)s * a.n_cols * a.f4 + c;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; ++p) {
    const float v = a.val ? a.val[p] : 1.0f;
    const float4 xv = x4[(int64_t)a.col[p] * a.f4];
    acc.x = fmaf(v, xv.x, acc.x);
    acc.y = fmaf(v, xv.y, acc.y);
    acc.z = fmaf(v, xv.z, acc.z);
    acc.w = fmaf(v, xv.w, acc.w);
  }
  if (a.bias) {
    const float4 b = reinterpret_cast<const float4 *>(a.bias)[c];
    acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
  }
  with_act(a.act, [&](auto act_) {
    constexpr int A = decltype(act_)::value;
    acc.x = act_ct<A>(acc.x, a.act);
    acc.y = act_ct<A>(acc.y, a.act);
    acc.z = act_ct<A>(acc.z, a.act);
    acc.w = act_ct<A>(acc.w, a.act);
  });
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n_rows + i) * a.f4 + c] = acc;
}

// Grouped variants (the ones that run when the row is G * NC float4 chunks wide, G a power of two <= 16).  The kernels
// above walk a row's entries with one dependent load chain per entry and lane (col[p] -> x[col[p]]): ~2 memory latencies
// per entry, 18 per GAT row -- at 2 M rows (the C5 training batch) that chain, not the bandwidth, was the run time.  Here
// the G lanes of a row load G entries' indices / weights / scores side by side (one latency), the softmax terms are
// computed once per entry instead of once per lane, and (index, weight) pairs reach the row's lanes by shuffles, so the
// feature-row gathers of a row are independent loads.  Values are accumulated in entry order exactly as above:
// bit-identical results.
constexpr int GU = 4;      // feature-row gathers a lane keeps in flight

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

template <int G, int NC>
__global__ __launch_bounds__(256) void k_csr_spmm_g(SpmmArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t grp = t / G;
  const int c = (int)(t % G);
  const bool row_ok = grp < a.n_rows;
  const int i = a.order[row_ok ? grp : a.n_rows - 1];       // surplus groups shadow the last row (they take part in the shuffles)
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float4 *x4 = reinterpret_cast<const float4 *>(a.x) + (int64_t)s * a.n_cols * a.f4 + c;
  float4 acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = min(b0 + c, end - 1);
    const int j = a.col[p];
    const float v = a.val ? a.val[p] : 1.0f;
    const int nk = min(G, end - b0);
    for (int k0 = 0; k0 < nk; k0 += GU) {          // GU gathers in flight per lane; entries are still added in order
      float vv[GU];
      float4 xv[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int k = min(k0 + u, nk - 1);
        const int jj = __shfl(j, k, G);
        vv[u] = __shfl(v, k, G);
#pragma unroll
        for (int q = 0; q < NC; ++q) xv[u][q] = x4[(int64_t)jj * a.f4 + G * q];
      }
#pragma unroll
      for (int u = 0; u < GU; ++u)
        if (k0 + u < nk) {
#pragma unroll
          for (int q = 0; q < NC; ++q) {
            acc[q].x = fmaf(vv[u], xv[u][q].x, acc[q].x);
            acc[q].y = fmaf(vv[u], xv[u][q].y, acc[q].y);
            acc[q].z = fmaf(vv[u], xv[u][q].z, acc[q].z);
            acc[q].w = fmaf(vv[u], xv[u][q].w, acc[q].w);
          }
        }
    }
  }
  if (!row_ok) return;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    float4 o = acc[q];
    if (a.bias) {
      const float4 b = reinterpret_cast<const float4 *>(a.bias)[c + G * q];
      o.x += b.x; o.y += b.y; o.z += b.z; o.w += b.w;
    }
    with_act(a.act, [&](auto act_) {
      constexpr int A = decltype(act_)::value;
      o.x = act_ct<A>(o.x, a.act);
      o.y = act_ct<A>(o.y, a.act);
      o.z = act_ct<A>(o.z, a.act);
      o.w = act_ct<A>(o.w, a.act);
    });
    reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n_rows + i) * a.f4 + c + G * q] = o;
  }
}

// (G, NC) of a row of f4 float4 chunks; G = 0: no grouped instance (odd widths take the one-lane-per-chunk kernels)
inline void group_shape(int f4, int &G, int &NC) {
  G = 0;
  NC = 1;
  if (f4 == 2 || f4 == 4 || f4 == 8 || f4 == 16) G = f4;
  else if (f4 == 32) { G = 16; NC = 2; }
}

template <class Args, class F>
inline hipError_t launch_grouped(const Args &a, int64_t rows, int S, int f4, hipStream_t st, F &&pick) {
  int G, NC;
  group_shape(f4, G, NC);
  const dim3 grid((unsigned)((rows * G + 255) / 256), (unsigned)S);
  switch (G * 4 + NC) {
    case 2 * 4 + 1: pick(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}, grid); break;
    case 4 * 4 + 1: pick(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{}, grid); break;
    case 8 * 4 + 1: pick(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{}, grid); break;
    case 16 * 4 + 1: pick(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{}, grid); break;
    default: pick(std::integral_constant<int, 16>{}, std::integral_constant<int, 2>{}, grid); break;
  }
  return hipGetLastError();
}

inline hipError_t launch_csr_spmm(const SpmmArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.f4, G, NC);
  if (G && a.n_rows > 0)
    return launch_grouped(a, a.n_rows, a.S, a.f4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_csr_spmm_g<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a);
    });
  const int64_t per_snap = (int64_t)a.n_rows * a.f4;
  hipLaunchKernelGGL(k_csr_spmm, dim3((unsigned)((per_snap + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

struct GatArgs {
  const int32_t *rowptr, *col, *order;
  const float *hx, *s_self, *s_nbr, *bias;
  float *out;
  int n, d4, act, S;
};

__device__ __forceinline__ float leaky02(float v) { return v > 0.0f ? v : 0.2f * v; }

__global__ __launch_bounds__(256) void k_gat_aggregate(GatArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_snap = (int64_t)a.n * a.d4;
  if (t >= per_snap) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.d4);
  const int i = a.order[t / a.d4];
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  // pass 1: row maximum of the logits (softmax is shift-invariant; this is tf.nn.softmax's shift)
  float m = -INFINITY;
  for (int p = beg; p < end; ++p) m = fmaxf(m, leaky02(ss + sn[a.col[p]]));
  // pass 2: exp, denominator and weighted sum of the neighbours' transformed rows
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
  float den = 0.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    const float w = expf(leaky02(ss + sn[j]) - m);
    const float4 hv = hx4[(int64_t)j * a.d4];
    den += w;
    acc.x = fmaf(w, hv.x, acc.x);
    acc.y = fmaf(w, hv.y, acc.y);
    acc.z = fmaf(w, hv.z, acc.z);
    acc.w = fmaf(w, hv.w, acc.w);
  }
  const float inv = end > beg ? 1.0f / den : 0.0f;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c];
  float4 o;
  with_act(a.act, [&](auto act_) {
    constexpr int A = decltype(act_)::value;
    o.x = act_ct<A>(fmaf(acc.x, inv, b.x), a.act);
    o.y = act_ct<A>(fmaf(acc.y, inv, b.y), a.act);
    o.z = act_ct<A>(fmaf(acc.z, inv, b.z), a.act);
    o.w = act_ct<A>(fmaf(acc.w, inv, b.w), a.act);
  });
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.d4 + c] = o;
}

// Optional operands of the _ex aggregation / row pass (uds_gat_aggregate_ex, uds_gat_backward_ex): a per-snapshot edge
// mask (S, nnz) -- entry p of snapshot s takes part iff mask[s, p] != 0 or p is the row's diagonal -- and the attention
// dropout multiplier coef (S, nnz) on the normalised coefficients.  Either may be NULL.
struct GatEx {
  const float *mask, *coef;
  int64_t nnz;
};

// EX = false: the unmasked instantiations (uds_gat_aggregate / uds_gat_forward), `x` unused.  EX = true: a masked entry
// gets logit -inf exactly like the lanes past the row's end, so it stays in every shuffle with weight 0, and the row
// maximum runs over the surviving entries only.  With an all-ones mask and no coef every value is computed by the same
// operations in the same order as EX = false (a zero weight adds 0 to den and fmaf(0, h, acc) = acc): bitwise equal.
template <int G, int NC, bool EX = false>
__global__ __launch_bounds__(256) void k_gat_aggregate_g(GatArgs a, GatEx x) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t grp = t / G;
  const int c = (int)(t % G);
  const bool row_ok = grp < a.n;
  const int i = a.order[row_ok ? grp : a.n - 1];
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  const float *mk = EX && x.mask ? x.mask + (int64_t)s * x.nnz : nullptr;
  const float *cf = EX && x.coef ? x.coef + (int64_t)s * x.nnz : nullptr;
  // pass 1: row maximum of the logits; the single-chunk row (degree <= G, the usual case) keeps its logits for pass 2
  float m = -INFINITY, l0 = -INFINITY, c0 = 1.0f;
  int j0 = 0;
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    const int pc = min(p, end - 1);
    const int j = a.col[pc];
    bool on = p < end;
    if (EX && mk) on = on && (mk[pc] != 0.0f || j == i);
    const float l = on ? leaky02(ss + sn[j]) : -INFINITY;
    if (b0 == beg) {
      j0 = j;
      l0 = l;
      if (EX && cf) c0 = cf[pc];
    }
    m = fmaxf(m, l);
  }
  m = group_max<G>(m);
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
  float den = 0.0f;
  float4 acc[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b0 = beg; b0 < end; b0 += G) {
    const int p = b0 + c;
    int j = j0;
    float l = l0, cv = c0;
    if (b0 != beg) {
      const int pc = min(p, end - 1);
      j = a.col[pc];
      bool on = p < end;
      if (EX && mk) on = on && (mk[pc] != 0.0f || j == i);
      l = on ? leaky02(ss + sn[j]) : -INFINITY;
      if (EX && cf) cv = cf[pc];
    }
    // one exp per entry (lanes past the row's end hold exp(-inf) = 0, unused); EX: a row whose every entry is masked has
    // m = -inf, so the weight of an off lane is set to 0 instead of exp(-inf - -inf)
    const float w = EX ? (l == -INFINITY ? 0.0f : expf(l - m)) : expf(l - m);
    const float wc = EX && cf ? w * cv : w;      // attention dropout multiplies the numerator only, as k_gat_aggregate_coef
    const int nk = min(G, end - b0);
    for (int k0 = 0; k0 < nk; k0 += GU) {
      float ww[GU], wm[GU];
      float4 hv[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int k = min(k0 + u, nk - 1);
        const int jj = __shfl(j, k, G);
        ww[u] = __shfl(w, k, G);
        wm[u] = EX && cf ? __shfl(wc, k, G) : ww[u];
#pragma unroll
        for (int q = 0; q < NC; ++q) hv[u][q] = hx4[(int64_t)jj * a.d4 + G * q];
      }
#pragma unroll
      for (int u = 0; u < GU; ++u)
        if (k0 + u < nk) {
          den += ww[u];
#pragma unroll
          for (int q = 0; q < NC; ++q) {
            acc[q].x = fmaf(wm[u], hv[u][q].x, acc[q].x);
            acc[q].y = fmaf(wm[u], hv[u][q].y, acc[q].y);
            acc[q].z = fmaf(wm[u], hv[u][q].z, acc[q].z);
            acc[q].w = fmaf(wm[u], hv[u][q].w, acc[q].w);
          }
        }
    }
  }
  if (!row_ok) return;
  const float inv = (EX ? den > 0.0f : end > beg) ? 1.0f / den : 0.0f;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c + G * q];
    float4 o;
    with_act(a.act, [&](auto act_) {
      constexpr int A = decltype(act_)::value;
      o.x = act_ct<A>(fmaf(acc[q].x, inv, b.x), a.act);
      o.y = act_ct<A>(fmaf(acc[q].y, inv, b.y), a.act);
      o.z = act_ct<A>(fmaf(acc[q].z, inv, b.z), a.act);
      o.w = act_ct<A>(fmaf(acc[q].w, inv, b.w), a.act);
    });
    reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.d4 + c + G * q] = o;
  }
}

// k_gat_aggregate with a PER-SNAPSHOT edge mask (`use_adj`, emulator.py:268-271,343-362: the control action rewrites
// adjacency entries of the actuated links per time step; GAT casts the result to int, so a setting < 1 removes the entry).
// mask (S, nnz) floats: entry p of snapshot s takes part iff mask != 0 or it is the diagonal (spektral sets the diagonal
// to one after the rewrite: tf.linalg.set_diag).  A masked logit is -10e9 in the reference: exp underflows to exactly 0.
__global__ __launch_bounds__(256) void k_gat_aggregate_masked(GatArgs a, const float *__restrict__ mask, int64_t nnz) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_snap = (int64_t)a.n * a.d4;
  if (t >= per_snap) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.d4);
  const int i = a.order[t / a.d4];
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float *mk = mask + (int64_t)s * nnz;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  float m = -INFINITY;
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    if (mk[p] != 0.0f || j == i) m = fmaxf(m, leaky02(ss + sn[j]));
  }
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
  float den = 0.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    if (!(mk[p] != 0.0f || j == i)) continue;
    const float w = expf(leaky02(ss + sn[j]) - m);
    const float4 hv = hx4[(int64_t)j * a.d4];
    den += w;
    acc.x = fmaf(w, hv.x, acc.x);
    acc.y = fmaf(w, hv.y, acc.y);
    acc.z = fmaf(w, hv.z, acc.z);
    acc.w = fmaf(w, hv.w, acc.w);
  }
  const float inv = den > 0.0f ? 1.0f / den : 0.0f;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c];
  float4 o;
  o.x = apply_act(fmaf(acc.x, inv, b.x), a.act);
  o.y = apply_act(fmaf(acc.y, inv, b.y), a.act);
  o.z = apply_act(fmaf(acc.z, inv, b.z), a.act);
  o.w = apply_act(fmaf(acc.w, inv, b.w), a.act);
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.d4 + c] = o;
}

// k_gat_aggregate with a per-entry multiplier on the NORMALISED attention coefficients: Spektral's attention dropout
// (`attn_coef_drop = self.dropout(attn_coef)` after the softmax, GATConv._call_dense; rate 0.5, active whenever the model runs
// with training=True, i.e. the emulator's dropout > 0 under fit, emulator.py:411,434).  coef (S, nnz): 0 or 1 / (1 - rate) per
// pattern entry and snapshot.  Training path only: one thread per (row, 16-byte chunk), no grouping.
__global__ __launch_bounds__(256) void k_gat_aggregate_coef(GatArgs a, const float *__restrict__ coef, int64_t nnz) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_snap = (int64_t)a.n * a.d4;
  if (t >= per_snap) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.d4);
  const int i = a.order[t / a.d4];
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float *cf = coef + (int64_t)s * nnz;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  float m = -INFINITY;
  for (int p = beg; p < end; ++p) m = fmaxf(m, leaky02(ss + sn[a.col[p]]));
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
  float den = 0.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    const float w = expf(leaky02(ss + sn[j]) - m);
    den += w;                                   // the softmax is over ALL entries; the dropped ones only leave the sum
    const float wc = w * cf[p];
    const float4 hv = hx4[(int64_t)j * a.d4];
    acc.x = fmaf(wc, hv.x, acc.x);
    acc.y = fmaf(wc, hv.y, acc.y);
    acc.z = fmaf(wc, hv.z, acc.z);
    acc.w = fmaf(wc, hv.w, acc.w);
  }
  const float inv = den > 0.0f ? 1.0f / den : 0.0f;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c];
  float4 o;
  o.x = apply_act(fmaf(acc.x, inv, b.x), a.act);
  o.y = apply_act(fmaf(acc.y, inv, b.y), a.act);
  o.z = apply_act(fmaf(acc.z, inv, b.z), a.act);
  o.w = apply_act(fmaf(acc.w, inv, b.w), a.act);
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.d4 + c] = o;
}

inline hipError_t launch_gat_aggregate_coef(const GatArgs &a, const float *coef, int64_t nnz, hipStream_t st) {
  const int64_t per_snap = (int64_t)a.n * a.d4;
  hipLaunchKernelGGL(k_gat_aggregate_coef, dim3((unsigned)((per_snap + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a, coef, nnz);
  return hipGetLastError();
}

inline hipError_t launch_gat_aggregate_masked(const GatArgs &a, const float *mask, int64_t nnz, hipStream_t st) {
  const int64_t per_snap = (int64_t)a.n * a.d4;
  hipLaunchKernelGGL(k_gat_aggregate_masked, dim3((unsigned)((per_snap + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a, mask, nnz);
  return hipGetLastError();
}

inline hipError_t launch_gat_aggregate(const GatArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_aggregate_g<decltype(g_)::value, decltype(nc_)::value>), grid, dim3(256), 0, st, a, GatEx{});
    });
  const int64_t per_snap = (int64_t)a.n * a.d4;
  hipLaunchKernelGGL(k_gat_aggregate, dim3((unsigned)((per_snap + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// One-lane-per-chunk form of k_gat_aggregate_g<.., EX = true> for widths group_shape does not cover (d / 4 not in
// {2, 4, 8, 16, 32}).  No shuffles here, so a masked entry is skipped; the surviving entries are added in entry order with
// the operations of k_gat_aggregate (bitwise equal to it under an all-ones mask and no coef).
__global__ __launch_bounds__(256) void k_gat_aggregate_x(GatArgs a, GatEx x) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_snap = (int64_t)a.n * a.d4;
  if (t >= per_snap) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.d4);
  const int i = a.order[t / a.d4];
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const float *sn = a.s_nbr + (int64_t)s * a.n;
  const float *mk = x.mask ? x.mask + (int64_t)s * x.nnz : nullptr;
  const float *cf = x.coef ? x.coef + (int64_t)s * x.nnz : nullptr;
  const float ss = a.s_self[(int64_t)s * a.n + i];
  float m = -INFINITY;
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    if (!mk || mk[p] != 0.0f || j == i) m = fmaxf(m, leaky02(ss + sn[j]));
  }
  const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * a.d4 + c;
  float den = 0.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; ++p) {
    const int j = a.col[p];
    if (mk && !(mk[p] != 0.0f || j == i)) continue;
    const float w = expf(leaky02(ss + sn[j]) - m);
    const float wc = cf ? w * cf[p] : w;
    const float4 hv = hx4[(int64_t)j * a.d4];
    den += w;
    acc.x = fmaf(wc, hv.x, acc.x);
    acc.y = fmaf(wc, hv.y, acc.y);
    acc.z = fmaf(wc, hv.z, acc.z);
    acc.w = fmaf(wc, hv.w, acc.w);
  }
  const float inv = den > 0.0f ? 1.0f / den : 0.0f;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c];
  float4 o;
  with_act(a.act, [&](auto act_) {
    constexpr int A = decltype(act_)::value;
    o.x = act_ct<A>(fmaf(acc.x, inv, b.x), a.act);
    o.y = act_ct<A>(fmaf(acc.y, inv, b.y), a.act);
    o.z = act_ct<A>(fmaf(acc.z, inv, b.z), a.act);
    o.w = act_ct<A>(fmaf(acc.w, inv, b.w), a.act);
  });
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.d4 + c] = o;
}

// uds_gat_aggregate_ex: the grouped EX instantiations, the walking k_gat_aggregate_x for the other widths.
inline hipError_t launch_gat_aggregate_ex(const GatArgs &a, const GatEx &x, hipStream_t st) {
  int G, NC;
  group_shape(a.d4, G, NC);
  if (G && a.n > 0)
    return launch_grouped(a, a.n, a.S, a.d4, st, [&](auto g_, auto nc_, dim3 grid) {
      hipLaunchKernelGGL((k_gat_aggregate_g<decltype(g_)::value, decltype(nc_)::value, true>), grid, dim3(256), 0, st, a, x);
    });
  const int64_t per_snap = (int64_t)a.n * a.d4;
  hipLaunchKernelGGL(k_gat_aggregate_x, dim3((unsigned)((per_snap + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a, x);
  return hipGetLastError();
}

// Multi-head GATConv (spektral GATConv with attn_heads = H > 1, concat_heads true or false, return_attn_coef;
// uds_gat_aggregate_heads).  hx (S, n, H * C) with head-major columns, scores (S, n, H), coef and alpha_out (S, H, nnz), the edge
// mask (S, nnz) shared by the heads.  A work item is one (row, head) for the concatenation and one row, walking its heads, for the
// mean: the mean needs the sum over the heads before bias and activation, and the entry has no workspace to park them in.
// Per head the operations and their order are those of k_gat_aggregate_g<G, NC, true> / k_gat_aggregate_x, so H = 1 with
// concatenation is bitwise equal to uds_gat_aggregate_ex.  alpha_out, when given, gets alpha * coef of every entry of every head
// (0 for a masked one) in a third walk that recomputes the weights with the same operations the aggregation used.
struct GatHeadsArgs {
  const int32_t *rowptr, *col, *order;
  const float *hx, *s_self, *s_nbr, *bias, *mask, *coef;
  float *out, *alpha_out;
  int n, H, c4, act, S, mean;
  int64_t nnz;
};

// MEAN: the head loop and the cross-head sum exist in the mean instantiations only (the concatenation keeps the registers of one head)
template <int G, int NC, bool MEAN>
__global__ __launch_bounds__(256) void k_gat_aggregate_hg(GatHeadsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t grp = t / G;
  const int c = (int)(t % G);
  const int per_row = MEAN ? 1 : a.H;                     // items per row
  const int64_t items = (int64_t)a.n * per_row;
  const bool item_ok = grp < items;
  const int64_t it = item_ok ? grp : items - 1;             // surplus groups shadow the last item (they take part in the shuffles)
  const int i = a.order[it / per_row];
  const int h_beg = MEAN ? 0 : (int)(it % per_row), h_end = MEAN ? a.H : h_beg + 1;
  const int s = blockIdx.y;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const int rs = a.H * a.c4;                                // float4 chunks of one hx row
  const float *mk = a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
  float4 tot[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) tot[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int h = h_beg; h < h_end; ++h) {
    const float *sn = a.s_nbr + (int64_t)s * a.n * a.H + h;
    const float ss = a.s_self[((int64_t)s * a.n + i) * a.H + h];
    const float *cf = a.coef ? a.coef + ((int64_t)s * a.H + h) * a.nnz : nullptr;
    float m = -INFINITY, l0 = -INFINITY, c0 = 1.0f;
    int j0 = 0;
    for (int b0 = beg; b0 < end; b0 += G) {
      const int p = b0 + c;
      const int pc = min(p, end - 1);
      const int j = a.col[pc];
      bool on = p < end;
      if (mk) on = on && (mk[pc] != 0.0f || j == i);
      const float l = on ? leaky02(ss + sn[(int64_t)j * a.H]) : -INFINITY;
      if (b0 == beg) {
        j0 = j;
        l0 = l;
        if (cf) c0 = cf[pc];
      }
      m = fmaxf(m, l);
    }
    m = group_max<G>(m);
    const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * rs + h * a.c4 + c;
    float den = 0.0f;
    float4 acc[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = beg; b0 < end; b0 += G) {
      const int p = b0 + c;
      int j = j0;
      float l = l0, cv = c0;
      if (b0 != beg) {
        const int pc = min(p, end - 1);
        j = a.col[pc];
        bool on = p < end;
        if (mk) on = on && (mk[pc] != 0.0f || j == i);
        l = on ? leaky02(ss + sn[(int64_t)j * a.H]) : -INFINITY;
        if (cf) cv = cf[pc];
      }
      const float w = l == -INFINITY ? 0.0f : expf(l - m);
      const float wc = cf ? w * cv : w;
      const int nk = min(G, end - b0);
      for (int k0 = 0; k0 < nk; k0 += GU) {
        float ww[GU], wm[GU];
        float4 hv[GU][NC];
#pragma unroll
        for (int u = 0; u < GU; ++u) {
          const int k = min(k0 + u, nk - 1);
          const int jj = __shfl(j, k, G);
          ww[u] = __shfl(w, k, G);
          wm[u] = cf ? __shfl(wc, k, G) : ww[u];
#pragma unroll
          for (int q = 0; q < NC; ++q) hv[u][q] = hx4[(int64_t)jj * rs + G * q];
        }
#pragma unroll
        for (int u = 0; u < GU; ++u)
          if (k0 + u < nk) {
            den += ww[u];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
              acc[q].x = fmaf(wm[u], hv[u][q].x, acc[q].x);
              acc[q].y = fmaf(wm[u], hv[u][q].y, acc[q].y);
              acc[q].z = fmaf(wm[u], hv[u][q].z, acc[q].z);
              acc[q].w = fmaf(wm[u], hv[u][q].w, acc[q].w);
            }
          }
      }
    }
    const float inv = den > 0.0f ? 1.0f / den : 0.0f;
    if (a.alpha_out && item_ok) {
      float *ao = a.alpha_out + ((int64_t)s * a.H + h) * a.nnz;
      for (int p = beg + c; p < end; p += G) {
        const int j = a.col[p];
        const bool on = !mk || mk[p] != 0.0f || j == i;
        const float w = on ? expf(leaky02(ss + sn[(int64_t)j * a.H]) - m) : 0.0f;
        ao[p] = (cf ? w * cf[p] : w) * inv;
      }
    }
    if (MEAN) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        tot[q].x = fmaf(acc[q].x, inv, tot[q].x);
        tot[q].y = fmaf(acc[q].y, inv, tot[q].y);
        tot[q].z = fmaf(acc[q].z, inv, tot[q].z);
        tot[q].w = fmaf(acc[q].w, inv, tot[q].w);
      }
    } else if (item_ok) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[h * a.c4 + c + G * q];
        float4 o;
        with_act(a.act, [&](auto act_) {
          constexpr int A = decltype(act_)::value;
          o.x = act_ct<A>(fmaf(acc[q].x, inv, b.x), a.act);
          o.y = act_ct<A>(fmaf(acc[q].y, inv, b.y), a.act);
          o.z = act_ct<A>(fmaf(acc[q].z, inv, b.z), a.act);
          o.w = act_ct<A>(fmaf(acc[q].w, inv, b.w), a.act);
        });
        reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * rs + h * a.c4 + c + G * q] = o;
      }
    }
  }
  if (!MEAN || !item_ok) return;
  const float rh = 1.0f / (float)a.H;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c + G * q];
    float4 o;
    with_act(a.act, [&](auto act_) {
      constexpr int A = decltype(act_)::value;
      o.x = act_ct<A>(fmaf(tot[q].x, rh, b.x), a.act);
      o.y = act_ct<A>(fmaf(tot[q].y, rh, b.y), a.act);
      o.z = act_ct<A>(fmaf(tot[q].z, rh, b.z), a.act);
      o.w = act_ct<A>(fmaf(tot[q].w, rh, b.w), a.act);
    });
    reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.c4 + c + G * q] = o;
  }
}

// One lane per (row, head, 16-byte chunk) -- per (row, chunk) for the mean -- for the head widths group_shape does not cover
// (C / 4 = 1, 3, ..): the operations of k_gat_aggregate_x per head.  The lane of chunk 0 writes alpha_out.
__global__ __launch_bounds__(256) void k_gat_aggregate_hx(GatHeadsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = a.mean ? 1 : a.H;
  if (t >= (int64_t)a.n * per_row * a.c4) return;
  const int s = blockIdx.y;
  const int c = (int)(t % a.c4);
  const int64_t it = t / a.c4;
  const int i = a.order[it / per_row];
  const int h_beg = a.mean ? 0 : (int)(it % per_row), h_end = a.mean ? a.H : h_beg + 1;
  const int beg = a.rowptr[i], end = a.rowptr[i + 1];
  const int rs = a.H * a.c4;
  const float *mk = a.mask ? a.mask + (int64_t)s * a.nnz : nullptr;
  float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int h = h_beg; h < h_end; ++h) {
    const float *sn = a.s_nbr + (int64_t)s * a.n * a.H + h;
    const float ss = a.s_self[((int64_t)s * a.n + i) * a.H + h];
    const float *cf = a.coef ? a.coef + ((int64_t)s * a.H + h) * a.nnz : nullptr;
    float m = -INFINITY;
    for (int p = beg; p < end; ++p) {
      const int j = a.col[p];
      if (!mk || mk[p] != 0.0f || j == i) m = fmaxf(m, leaky02(ss + sn[(int64_t)j * a.H]));
    }
    const float4 *hx4 = reinterpret_cast<const float4 *>(a.hx) + (int64_t)s * a.n * rs + h * a.c4 + c;
    float den = 0.0f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = beg; p < end; ++p) {
      const int j = a.col[p];
      if (mk && !(mk[p] != 0.0f || j == i)) continue;
      const float w = expf(leaky02(ss + sn[(int64_t)j * a.H]) - m);
      const float wc = cf ? w * cf[p] : w;
      const float4 hv = hx4[(int64_t)j * rs];
      den += w;
      acc.x = fmaf(wc, hv.x, acc.x);
      acc.y = fmaf(wc, hv.y, acc.y);
      acc.z = fmaf(wc, hv.z, acc.z);
      acc.w = fmaf(wc, hv.w, acc.w);
    }
    const float inv = den > 0.0f ? 1.0f / den : 0.0f;
    if (a.alpha_out && c == 0) {
      float *ao = a.alpha_out + ((int64_t)s * a.H + h) * a.nnz;
      for (int p = beg; p < end; ++p) {
        const int j = a.col[p];
        const bool on = !mk || mk[p] != 0.0f || j == i;
        const float w = on ? expf(leaky02(ss + sn[(int64_t)j * a.H]) - m) : 0.0f;
        ao[p] = (cf ? w * cf[p] : w) * inv;
      }
    }
    if (a.mean) {
      tot.x = fmaf(acc.x, inv, tot.x);
      tot.y = fmaf(acc.y, inv, tot.y);
      tot.z = fmaf(acc.z, inv, tot.z);
      tot.w = fmaf(acc.w, inv, tot.w);
    } else {
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[h * a.c4 + c];
      float4 o;
      with_act(a.act, [&](auto act_) {
        constexpr int A = decltype(act_)::value;
        o.x = act_ct<A>(fmaf(acc.x, inv, b.x), a.act);
        o.y = act_ct<A>(fmaf(acc.y, inv, b.y), a.act);
        o.z = act_ct<A>(fmaf(acc.z, inv, b.z), a.act);
        o.w = act_ct<A>(fmaf(acc.w, inv, b.w), a.act);
      });
      reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * rs + h * a.c4 + c] = o;
    }
  }
  if (!a.mean) return;
  const float rh = 1.0f / (float)a.H;
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.bias) b = reinterpret_cast<const float4 *>(a.bias)[c];
  float4 o;
  with_act(a.act, [&](auto act_) {
    constexpr int A = decltype(act_)::value;
    o.x = act_ct<A>(fmaf(tot.x, rh, b.x), a.act);
    o.y = act_ct<A>(fmaf(tot.y, rh, b.y), a.act);
    o.z = act_ct<A>(fmaf(tot.z, rh, b.z), a.act);
    o.w = act_ct<A>(fmaf(tot.w, rh, b.w), a.act);
  });
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n + i) * a.c4 + c] = o;
}

inline hipError_t launch_gat_aggregate_heads(const GatHeadsArgs &a, hipStream_t st) {
  int G, NC;
  group_shape(a.c4, G, NC);
  const int64_t items = (int64_t)a.n * (a.mean ? 1 : a.H);
  if (G)
    return launch_grouped(a, items, a.S, a.c4, st, [&](auto g_, auto nc_, dim3 grid) {
      if (a.mean) hipLaunchKernelGGL((k_gat_aggregate_hg<decltype(g_)::value, decltype(nc_)::value, true>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((k_gat_aggregate_hg<decltype(g_)::value, decltype(nc_)::value, false>), grid, dim3(256), 0, st, a);
    });
  hipLaunchKernelGGL(k_gat_aggregate_hx, dim3((unsigned)((items * a.c4 + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// out[b,t,r,:] = act(sum_{t' <= t} x[b,t',r,:] + res[b,0,r,:])   -- `cumsum(x_out, axis=1) + tile(res)` then the
// activation (emulator.py:313-320).  One lane owns one float4 feature chunk of one (b, r) and walks the T steps.
struct CumsumArgs {
  const float *x, *res;
  float *out;
  int B, T, R, f4, act;
};

__global__ __launch_bounds__(256) void k_cumsum_res_act(CumsumArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_b = (int64_t)a.R * a.f4;
  if (t >= per_b * a.B) return;
  const int64_t b = t / per_b, rc = t - b * per_b;
  const float4 *x4 = reinterpret_cast<const float4 *>(a.x) + b * a.T * per_b + rc;
  float4 *o4 = reinterpret_cast<float4 *>(a.out) + b * a.T * per_b + rc;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.res) r = reinterpret_cast<const float4 *>(a.res)[b * per_b + rc];
  with_act(a.act, [&](auto act_) {
    constexpr int A = decltype(act_)::value;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < a.T; ++s) {
      const float4 v = x4[(int64_t)s * per_b];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      float4 o;
      o.x = act_ct<A>(acc.x + r.x, a.act);
      o.y = act_ct<A>(acc.y + r.y, a.act);
      o.z = act_ct<A>(acc.z + r.z, a.act);
      o.w = act_ct<A>(acc.w + r.w, a.act);
      o4[(int64_t)s * per_b] = o;
    }
  });
}

inline hipError_t launch_cumsum(const CumsumArgs &a, hipStream_t st) {
  const int64_t total = (int64_t)a.B * a.R * a.f4;
  hipLaunchKernelGGL(k_cumsum_res_act, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// Link -> node flow balance of post_proc_tf (emulator.py:717-724): for node n and every incident link l with
// sign sg (+1 = n is the from-node, -1 = the to-node) and signed flow f:
//   q_out[n] += sg > 0 ? max(f,0) : max(-f,0);   q_in[n] += sg > 0 ? max(-f,0) : max(f,0)
// each scaled per node (the reference divides by norm_y where it exceeds 1e-3, else multiplies by 0).
struct FlowArgs {
  const int32_t *rowptr, *col;
  const float *sign, *flow, *scale_in, *scale_out;
  float *q_in, *q_out;
  int n_node, n_edge, S;
};

__global__ __launch_bounds__(256) void k_flow_balance(FlowArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_node) return;
  const int s = blockIdx.y;
  const float *f = a.flow + (int64_t)s * a.n_edge;
  float qi = 0.f, qo = 0.f;
  for (int p = a.rowptr[n]; p < a.rowptr[n + 1]; ++p) {
    const float v = f[a.col[p]];
    const float fp = fmaxf(v, 0.f), fn = fmaxf(-v, 0.f);
    if (a.sign[p] > 0.f) { qo += fp; qi += fn; } else { qi += fp; qo += fn; }
  }
  a.q_in[(int64_t)s * a.n_node + n] = qi * a.scale_in[n];
  a.q_out[(int64_t)s * a.n_node + n] = qo * a.scale_out[n];
}

inline hipError_t launch_flow_balance(const FlowArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_flow_balance, dim3((unsigned)((a.n_node + 255) / 256), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// One chunk of the autoregressive rollout after the forward (emulator.py:403-423 with post_proc_tf's edge-fusion branch,
// :717-724): de-normalise the predicted link flow, balance it onto the nodes (as k_flow_balance), assemble the node
// prediction [h, q_in, q_out, (flood)], and shift both state windows by `so` steps in place, feeding the prediction back
// (flood bit thresholded at 0.5, runoff appended; link rows get the constant setting 1).  Replaces ~15 elementwise /
// concatenation launches per step.  Same operations in the same order as the tensor code (no fused multiply-add): the
// results are bit-identical.
struct RollArgs {
  const int32_t *rowptr, *col;
  const float *sign, *span_e, *mini_e, *scale_in, *scale_out;
  const float *y, *ey, *b;      // (B,so,N,cy), (B,so,E,ce), (B,so,N,1)
  float *x, *ex, *preds;        // (B,T,N,cy+3), (B,T,E,ce+1) in place; (B,so,N,cy+2)
  int B, so, T, N, E, cy, ce, flood;
};

__global__ __launch_bounds__(256) void k_roll_node(RollArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.B * a.N) return;
  const int b = (int)(t / a.N), n = (int)(t % a.N);
  const int cx = a.cy + 3, cp = a.cy + 2, keep = a.T - a.so;
  float *xw = a.x + ((int64_t)b * a.T * a.N + n) * cx;
  const int64_t xs = (int64_t)a.N * cx;                       // stride of a time step
  for (int k = 0; k < keep; ++k)
    for (int c = 0; c < cx; ++c) xw[k * xs + c] = xw[(k + a.so) * xs + c];
  for (int j = 0; j < a.so; ++j) {
    const float *f = a.ey + ((int64_t)b * a.so + j) * a.E * a.ce + (a.ce - 1);
    float qi = 0.f, qo = 0.f;
    for (int p = a.rowptr[n]; p < a.rowptr[n + 1]; ++p) {
      const int l = a.col[p];
      const float v = __fadd_rn(__fmul_rn(f[(int64_t)l * a.ce], a.span_e[l]), a.mini_e[l]);
      const float fp = fmaxf(v, 0.f), fn = fmaxf(-v, 0.f);
      if (a.sign[p] > 0.f) { qo += fp; qi += fn; } else { qi += fp; qo += fn; }
    }
    qi = __fmul_rn(qi, a.scale_in[n]);
    qo = __fmul_rn(qo, a.scale_out[n]);
    const float *yr = a.y + (((int64_t)b * a.so + j) * a.N + n) * a.cy;
    float *pr = a.preds + (((int64_t)b * a.so + j) * a.N + n) * cp;
    float *xn = xw + (int64_t)(keep + j) * xs;
    pr[0] = xn[0] = yr[0];
    pr[1] = xn[1] = qi;
    pr[2] = xn[2] = qo;
    for (int c = 1; c < a.cy; ++c) {
      const float v = yr[c];
      pr[2 + c] = v;
      xn[2 + c] = (a.flood && c == a.cy - 1) ? (v > 0.5f ? 1.f : 0.f) : v;
    }
    xn[cx - 1] = a.b[((int64_t)b * a.so + j) * a.N + n];
  }
}

__global__ __launch_bounds__(256) void k_roll_edge(RollArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.B * a.E) return;
  const int b = (int)(t / a.E), l = (int)(t % a.E);
  const int cx = a.ce + 1, keep = a.T - a.so;
  float *xw = a.ex + ((int64_t)b * a.T * a.E + l) * cx;
  const int64_t xs = (int64_t)a.E * cx;
  for (int k = 0; k < keep; ++k)
    for (int c = 0; c < cx; ++c) xw[k * xs + c] = xw[(k + a.so) * xs + c];
  for (int j = 0; j < a.so; ++j) {
    const float *er = a.ey + (((int64_t)b * a.so + j) * a.E + l) * a.ce;
    float *xn = xw + (int64_t)(keep + j) * xs;
    for (int c = 0; c < a.ce; ++c) xn[c] = er[c];
    xn[a.ce] = 1.f;
  }
}

inline hipError_t launch_roll_update(const RollArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_roll_node, dim3((unsigned)(((int64_t)a.B * a.N + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_roll_edge, dim3((unsigned)(((int64_t)a.B * a.E + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// Message buffers of the graph-sharded block (dist.py; no reference counterpart -- SURVEY.md 8e).  One buffer per peer:
//   PACK:   buf[s, i, :] = i < nx ? x[s, idx_x[i], :] : e[s, idx_e[i - nx], :]      (own rows a peer holds as halo)
//   UNPACK: the inverse scatter into the halo rows of x / e.
// One thread per 16 bytes; rows are F floats (F % 4 == 0), x is (S, n_x, F), e is (S, n_e, F).
struct HaloArgs {
  float *x, *e, *buf;
  const int32_t *idx_x, *idx_e;
  int64_t n_x, n_e, total;      // total = S * (nx + ne) * F / 4 float4 elements
  int nx, ne, f4;
};

template <bool PACK>
__global__ __launch_bounds__(256) void k_halo_rows(HaloArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int c = (int)(i % a.f4);
  const int64_t r = i / a.f4;
  const int n = a.nx + a.ne, j = (int)(r % n);
  const int64_t s = r / n;
  float4 *row = j < a.nx ? reinterpret_cast<float4 *>(a.x + (s * a.n_x + a.idx_x[j]) * (a.f4 * 4))
                         : reinterpret_cast<float4 *>(a.e + (s * a.n_e + a.idx_e[j - a.nx]) * (a.f4 * 4));
  float4 *slot = reinterpret_cast<float4 *>(a.buf) + i;
  if (PACK) *slot = row[c];
  else row[c] = *slot;
}

inline hipError_t launch_halo_rows(const HaloArgs &a, bool pack, hipStream_t st) {
  const unsigned grid = (unsigned)((a.total + 255) / 256);
  if (pack) hipLaunchKernelGGL(k_halo_rows<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_halo_rows<false>, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

// The messages of ALL peers in one launch (dist.HaloExchangeAll).  Message rows are numbered across peers: peer q owns
// rows [r_q, r_{q+1}), r_q = off_x[q] + off_e[q], node rows first; its block of the buffer is (S, n_q, F) at float offset
// S * F * r_q, so each peer's message stays one contiguous slice.
//   PACK:   buf[S F r_q + (s n_q + j) F + f] = j < nx_q ? x[s, idx_x[off_x[q] + j], f] : e[s, idx_e[off_e[q] + j - nx_q], f]
//   UNPACK: the inverse scatter.
//   CLEAR (with PACK): every source element is zeroed after it is read -- the first half of the exchange's adjoint
//   (the rows must be distinct across peers: each element is read and zeroed by one thread).
// Grid (ceil(n_rows * W / 256), S); thread = (message row, W-th of a row): W = F / 4 float4 (VEC) or F floats.
struct HaloAllArgs {
  float *x, *e, *buf;
  const int32_t *idx_x, *idx_e, *off_x, *off_e;      // off_* (P + 1), device
  int64_t n_x, n_e;
  int n_rows, P, F, W;
};

template <bool PACK, bool VEC, bool CLEAR = false>
__global__ __launch_bounds__(256) void k_halo_rows_all(HaloAllArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.n_rows * a.W) return;
  const int r = (int)(i / a.W), c = (int)(i % a.W);
  const int64_t s = blockIdx.y, S = gridDim.y;
  int lo = 0, hi = a.P;                                  // peer q: r_q <= r < r_{q+1} (peers with no rows are skipped over)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.off_x[mid] + a.off_e[mid] <= r) lo = mid;
    else hi = mid;
  }
  const int q = lo, r0 = a.off_x[q] + a.off_e[q], nx = a.off_x[q + 1] - a.off_x[q];
  const int n = a.off_x[q + 1] + a.off_e[q + 1] - r0, j = r - r0;
  float *row = j < nx ? a.x + (s * a.n_x + a.idx_x[a.off_x[q] + j]) * a.F : a.e + (s * a.n_e + a.idx_e[a.off_e[q] + j - nx]) * a.F;
  float *slot = a.buf + S * a.F * r0 + (s * n + j) * a.F;
  if (VEC) {
    float4 *rv = reinterpret_cast<float4 *>(row) + c, *sv = reinterpret_cast<float4 *>(slot) + c;
    if (PACK) {
      *sv = *rv;
      if (CLEAR) *rv = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      *rv = *sv;
    }
  } else {
    if (PACK) {
      slot[c] = row[c];
      if (CLEAR) row[c] = 0.f;
    } else {
      row[c] = slot[c];
    }
  }
}

inline hipError_t launch_halo_rows_all(const HaloAllArgs &a, int S, bool pack, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)a.n_rows * a.W + 255) / 256), (unsigned)S);
  if (pack && vec) hipLaunchKernelGGL((k_halo_rows_all<true, true>), grid, dim3(256), 0, st, a);
  else if (pack) hipLaunchKernelGGL((k_halo_rows_all<true, false>), grid, dim3(256), 0, st, a);
  else if (vec) hipLaunchKernelGGL((k_halo_rows_all<false, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_halo_rows_all<false, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

inline hipError_t launch_halo_pack_clear_all(const HaloAllArgs &a, int S, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)a.n_rows * a.W + 255) / 256), (unsigned)S);
  if (vec) hipLaunchKernelGGL((k_halo_rows_all<true, true, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_halo_rows_all<true, false, true>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// The second half of the exchange's adjoint: every owner ADDS the gradients its peers return for its rows.  Targets are
// numbered node rows first (t < tx: x row tgt_x[t], else e row tgt_e[t - tx]); target t sums the message rows
// src[ptr[t] .. ptr[t+1]) -- numbered across peers as in HaloAllArgs, so row r lies in peer q's block with
// r_q <= r < r_{q+1} -- in the order listed (ascending peer):
//   row[s, :] = ((row[s, :] + m_0[s, :]) + m_1[s, :]) + ...
// One thread per (target, W-th of a row) and snapshot: no two threads touch one element, no atomics -- the sum is the same
// bits whatever the arrival order of the messages.  Grid (ceil(n_tgt * W / 256), S).
struct HaloAccArgs {
  const float *buf;
  float *x, *e;
  const int32_t *off_x, *off_e, *tgt_x, *tgt_e, *ptr, *src;
  int64_t n_x, n_e;
  int tx, n_tgt, P, F, W;
};

template <bool VEC>
__global__ __launch_bounds__(256) void k_halo_accumulate_all(HaloAccArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.n_tgt * a.W) return;
  const int t = (int)(i / a.W), c = (int)(i % a.W);
  const int64_t s = blockIdx.y, S = gridDim.y;
  float *row = t < a.tx ? a.x + (s * a.n_x + a.tgt_x[t]) * a.F : a.e + (s * a.n_e + a.tgt_e[t - a.tx]) * a.F;
  float4 acc4 = VEC ? reinterpret_cast<const float4 *>(row)[c] : make_float4(row[c], 0.f, 0.f, 0.f);
  for (int k = a.ptr[t]; k < a.ptr[t + 1]; ++k) {
    const int r = a.src[k];
    int lo = 0, hi = a.P;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.off_x[mid] + a.off_e[mid] <= r) lo = mid;
      else hi = mid;
    }
    const int r0 = a.off_x[lo] + a.off_e[lo], n = a.off_x[lo + 1] + a.off_e[lo + 1] - r0;
    const float *slot = a.buf + S * a.F * r0 + (s * n + (r - r0)) * a.F;
    if (VEC) {
      const float4 m = reinterpret_cast<const float4 *>(slot)[c];
      acc4.x += m.x;
      acc4.y += m.y;
      acc4.z += m.z;
      acc4.w += m.w;
    } else {
      acc4.x += slot[c];
    }
  }
  if (VEC) reinterpret_cast<float4 *>(row)[c] = acc4;
  else row[c] = acc4.x;
}

inline hipError_t launch_halo_accumulate_all(const HaloAccArgs &a, int S, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)a.n_tgt * a.W + 255) / 256), (unsigned)S);
  if (vec) hipLaunchKernelGGL(k_halo_accumulate_all<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_halo_accumulate_all<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// spektral DiffusionConv in the reference's dense "mixed" mode (emulator.py:135-138,229): each of the C output channels
// is ONE DiffuseFeatures filter, H_q = reduce_sum(polyval(theta_q, a_hat) @ x, -1), where tf.math.polyval runs Horner's
// rule on the ENTRIES of a_hat.  A zero entry therefore gets the constant coefficient c0_q = theta_q[K], and with
// r[s, j] = sum_f x[s, j, f], tot[s] = sum_j r[s, j]:
//     H_q[s, i] = c0_q * tot[s] + sum_{p in row i} (polyval(theta_q, a_p) - c0_q) * r[s, col[p]]
// -- the dense N x N product collapses to the support.  vals[p, q] = polyval(theta_q, a_p) - c0_q is prepared once per
// parameter update.  One thread per (row, 4 channels), one grid row per snapshot.
struct DiffusionArgs {
  const int32_t *rowptr, *col;
  const float *vals, *c0, *r, *tot;
  float *out;
  int n_rows, n_cols, c4, act;
};

__global__ __launch_bounds__(256) void k_diffusion(DiffusionArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(idx / a.c4), q = (int)(idx % a.c4), s = blockIdx.y;
  if (i >= a.n_rows) return;
  const float4 c = reinterpret_cast<const float4 *>(a.c0)[q];
  const float t = a.tot[s];
  float4 acc = make_float4(c.x * t, c.y * t, c.z * t, c.w * t);
  const float *r = a.r + (int64_t)s * a.n_cols;
  for (int p = a.rowptr[i]; p < a.rowptr[i + 1]; ++p) {
    const float rv = r[a.col[p]];
    const float4 v = reinterpret_cast<const float4 *>(a.vals)[(int64_t)p * a.c4 + q];
    acc.x += v.x * rv, acc.y += v.y * rv, acc.z += v.z * rv, acc.w += v.w * rv;
  }
  acc.x = apply_act(acc.x, a.act), acc.y = apply_act(acc.y, a.act), acc.z = apply_act(acc.z, a.act), acc.w = apply_act(acc.w, a.act);
  reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n_rows + i) * a.c4 + q] = acc;
}

inline hipError_t launch_diffusion(const DiffusionArgs &a, int S, hipStream_t st) {
  const int64_t per_s = (int64_t)a.n_rows * a.c4;
  hipLaunchKernelGGL(k_diffusion, dim3((unsigned)((per_s + 255) / 256), (unsigned)S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// Reverse of k_diffusion.  With gz = act'(y) gy (act' from the output y), K = K1 - 1, M_0[s, i] = tot[s] and
// M_m[s, i] = sum_{p in row i} a_p^m r[s, col p] (m = 1..K):
//     dtheta[q, k] = sum_{s, i} gz[s, i, q] M_{K-k}[s, i]
//     dr[s, j]     = g0[s] + sum_{p : col p = j} sum_q vals[p, q] gz[s, row p, q],     g0[s] = sum_{i, q} c0[q] gz[s, i, q]
// (the c0 tot[s] term reaches every r[s, j]; zero entries of a_hat are off the support in both directions).  Three launches:
//   rows    grid (gx, sy): block (bx, by) owns snapshots [8 by, 8 by + 8) and row slots bx, bx + gx, ...; lr lanes per row
//           (lr = c4 rounded up to a power of two), lane q = channels 4q..4q+3.  Writes gz, the block's partial of the
//           (K1, C) moment products and, per snapshot, of g0.
//   reduce  one block per dtheta element and per g0[s]: strided partial sums and a fixed LDS tree.
//   input   grid (ceil(n_cols / (256 / lr)), S): row j of the TRANSPOSED pattern, vals read through perm_t, lanes summed by a
//           fixed xor tree.
// Every partial has one writer and every sum a fixed order: no atomics, bitwise repeatable.  The block partition depends only
// on (n_rows, S, C), not on the device.
constexpr int DIFF_SCH = 8;        // snapshots per row-pass block
constexpr int DIFF_KMAX = 16;      // largest K1 the row pass takes

struct DiffusionBwdArgs {
  const int32_t *rowptr, *col, *t_rowptr, *t_col, *perm_t;
  const float *a, *vals, *c0, *r, *tot, *y, *gy;
  float *gz, *pth, *pg, *g0, *dr, *dtheta;
  int n_rows, n_cols, S, c4, lr, K1, act, gx, sy;
  int c0s = 1;      // stride of c0 in floats: 1 = a (C,) vector, K1 = the last column of theta (C, K1) (the table-free entry)
};

struct DiffusionBwdPlan {
  int lr, gx, sy;
  int64_t off_pth, off_pg, off_g0, total;     // workspace carve (floats, 16-byte aligned sections); gz at offset 0
};

inline DiffusionBwdPlan diffusion_bwd_plan(int64_t n_rows, int64_t S, int64_t C, int64_t K1) {
  DiffusionBwdPlan p;
  p.lr = 1;
  while (p.lr < C / 4) p.lr <<= 1;
  const int64_t rpb = 256 / p.lr, ng = (n_rows + rpb - 1) / rpb;
  p.sy = (int)((S + DIFF_SCH - 1) / DIFF_SCH);
  const int64_t cap = p.sy > 0 && 2048 / p.sy > 256 ? 2048 / p.sy : 256;      // ~2048 blocks: the whole GPU, few partials
  p.gx = (int)(ng < 1 ? 1 : ng < cap ? ng : cap);
  auto up4 = [](int64_t f) { return (f + 3) & ~int64_t(3); };
  p.off_pth = up4(S * n_rows * C);
  p.off_pg = p.off_pth + up4((int64_t)p.gx * p.sy * K1 * C);
  p.off_g0 = p.off_pg + up4(S * p.gx);
  p.total = p.off_g0 + up4(S);
  return p;
}

__device__ __forceinline__ float act_grad_from_out(float y, float g, int act) {     // autograd.act_grad, element-wise
  switch (act) {
    case UDS_ACT_RELU: return y > 0.f ? g : 0.f;
    case UDS_ACT_TANH: return g * (1.f - y * y);
    case UDS_ACT_SIGMOID: return g * y * (1.f - y);
    case UDS_ACT_HARD_SIGMOID: return y > 0.f && y < 1.f ? g * 0.2f : 0.f;
    default: return g;
  }
}

template <int KMAX>
__global__ __launch_bounds__(256) void k_diffusion_bwd_rows(DiffusionBwdArgs a) {
  __shared__ float4 s_red[256];
  __shared__ float s_g0[4][DIFF_SCH];
  const int tid = threadIdx.x, q = tid % a.lr, rpb = 256 / a.lr, wave = tid >> 6, wl = tid & 63;
  const bool qok = q < a.c4;
  const int s0 = blockIdx.y * DIFF_SCH;
  float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
  if (qok) {
    if (a.c0s == 1) c = reinterpret_cast<const float4 *>(a.c0)[q];
    else c = make_float4(a.c0[(4 * q) * a.c0s], a.c0[(4 * q + 1) * a.c0s], a.c0[(4 * q + 2) * a.c0s], a.c0[(4 * q + 3) * a.c0s]);
  }
  float4 acc[KMAX];
#pragma unroll
  for (int m = 0; m < KMAX; ++m) acc[m] = make_float4(0.f, 0.f, 0.f, 0.f);
  float g0p[DIFF_SCH];
#pragma unroll
  for (int sl = 0; sl < DIFF_SCH; ++sl) g0p[sl] = 0.f;
  for (int i = blockIdx.x * rpb + tid / a.lr; i < a.n_rows; i += gridDim.x * rpb) {
    const int beg = a.rowptr[i], end = a.rowptr[i + 1];
#pragma unroll
    for (int sl = 0; sl < DIFF_SCH; ++sl) {
      const int s = s0 + sl;
      if (s < a.S) {
        float M[KMAX];
        M[0] = a.tot[s];
#pragma unroll
        for (int m = 1; m < KMAX; ++m) M[m] = 0.f;
        const float *rs = a.r + (int64_t)s * a.n_cols;
        for (int p = beg; p < end; ++p) {
          const float av = a.a[p];
          float pw = rs[a.col[p]];
#pragma unroll
          for (int m = 1; m < KMAX; ++m)
            if (m < a.K1) {
              pw *= av;
              M[m] += pw;
            }
        }
        if (qok) {
          const int64_t idx = ((int64_t)s * a.n_rows + i) * a.c4 + q;
          const float4 yv = reinterpret_cast<const float4 *>(a.y)[idx], gv = reinterpret_cast<const float4 *>(a.gy)[idx];
          const float4 z = make_float4(act_grad_from_out(yv.x, gv.x, a.act), act_grad_from_out(yv.y, gv.y, a.act),
                                       act_grad_from_out(yv.z, gv.z, a.act), act_grad_from_out(yv.w, gv.w, a.act));
          reinterpret_cast<float4 *>(a.gz)[idx] = z;
#pragma unroll
          for (int m = 0; m < KMAX; ++m)
            if (m < a.K1) {
              acc[m].x = fmaf(z.x, M[m], acc[m].x);
              acc[m].y = fmaf(z.y, M[m], acc[m].y);
              acc[m].z = fmaf(z.z, M[m], acc[m].z);
              acc[m].w = fmaf(z.w, M[m], acc[m].w);
            }
          g0p[sl] += c.x * z.x + c.y * z.y + c.z * z.z + c.w * z.w;
        }
      }
    }
  }
  // g0 partial per snapshot: wave xor tree, then the 4 waves in order
#pragma unroll
  for (int sl = 0; sl < DIFF_SCH; ++sl) {
    float v = g0p[sl];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (wl == 0) s_g0[wave][sl] = v;
  }
  __syncthreads();
  if (tid < DIFF_SCH && s0 + tid < a.S)
    a.pg[(int64_t)(s0 + tid) * a.gx + blockIdx.x] = ((s_g0[0][tid] + s_g0[1][tid]) + s_g0[2][tid]) + s_g0[3][tid];
  // moment products: lanes of one channel group are lr apart in a wave (xor tree over the row slots), then the 4 waves in order
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
  for (int m = 0; m < KMAX; ++m) {
    if (m >= a.K1) break;
    float4 v = acc[m];
    for (int o = a.lr; o < 64; o <<= 1) {
      v.x += __shfl_xor(v.x, o);
      v.y += __shfl_xor(v.y, o);
      v.z += __shfl_xor(v.z, o);
      v.w += __shfl_xor(v.w, o);
    }
    if (wl < a.lr) s_red[wave * 64 + wl] = v;
    __syncthreads();
    if (tid < a.lr && qok) {
      float4 t = s_red[tid];
      for (int w = 1; w < 4; ++w) {
        const float4 u = s_red[w * 64 + tid];
        t.x += u.x, t.y += u.y, t.z += u.z, t.w += u.w;
      }
      reinterpret_cast<float4 *>(a.pth)[(blk * a.K1 + m) * a.c4 + q] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_diffusion_bwd_reduce(DiffusionBwdArgs a) {
  __shared__ float sh[256];
  const int tid = threadIdx.x, C = a.c4 * 4, nt = a.K1 * C;
  const int o = blockIdx.x;
  float v = 0.f;
  if (o < nt) {
    const int64_t nb = (int64_t)a.gx * a.sy;
    for (int64_t b = tid; b < nb; b += 256) v += a.pth[b * nt + o];
  } else {
    const int64_t s = o - nt;
    for (int b = tid; b < a.gx; b += 256) v += a.pg[s * a.gx + b];
  }
  sh[tid] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    if (o < nt) a.dtheta[(o % C) * a.K1 + (a.K1 - 1 - o / C)] = sh[0];     // moment m = K - k
    else a.g0[o - nt] = sh[0];
  }
}

__global__ __launch_bounds__(256) void k_diffusion_bwd_input(DiffusionBwdArgs a) {
  const int tid = threadIdx.x, q = tid % a.lr;
  const int j = blockIdx.x * (256 / a.lr) + tid / a.lr, s = blockIdx.y;
  const bool live = j < a.n_cols;
  float acc = 0.f;
  if (live && q < a.c4) {
    const float4 *gz = reinterpret_cast<const float4 *>(a.gz) + (int64_t)s * a.n_rows * a.c4 + q;
    const float4 *vals = reinterpret_cast<const float4 *>(a.vals) + q;
    for (int p = a.t_rowptr[j]; p < a.t_rowptr[j + 1]; ++p) {
      const float4 v = vals[(int64_t)a.perm_t[p] * a.c4], z = gz[(int64_t)a.t_col[p] * a.c4];
      acc = fmaf(v.x, z.x, acc);
      acc = fmaf(v.y, z.y, acc);
      acc = fmaf(v.z, z.z, acc);
      acc = fmaf(v.w, z.w, acc);
    }
  }
  for (int o = a.lr >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);      // every lane takes part (no early return above)
  if (live && q == 0) a.dr[(int64_t)s * a.n_cols + j] = a.g0[s] + acc;
}

inline hipError_t launch_diffusion_backward(const DiffusionBwdArgs &a, hipStream_t st) {
  if (a.K1 <= 8) hipLaunchKernelGGL(k_diffusion_bwd_rows<8>, dim3((unsigned)a.gx, (unsigned)a.sy), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_diffusion_bwd_rows<DIFF_KMAX>, dim3((unsigned)a.gx, (unsigned)a.sy), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_diffusion_bwd_reduce, dim3((unsigned)(a.K1 * a.c4 * 4 + a.S)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int rpb = 256 / a.lr;
  hipLaunchKernelGGL(k_diffusion_bwd_input, dim3((unsigned)((a.n_cols + rpb - 1) / rpb), (unsigned)a.S), dim3(256), 0, st, a);
  return hipGetLastError();
}

// DiffusionConv without the (nnz, C) table: the polynomial expanded per row.  With K = K1 - 1, M_0[s, i] = tot[s] and
// M_m[s, i] = sum_{p in row i} a_p^m r[s, col p]:
//     out[s, i, q] = act( sum_{m=0..K} theta[q][K-m] M_m[s, i] )
// A row belongs to a lane group of lr lanes (lr = c4 rounded up to a power of two, 256 / lr rows per block).  With lr >= K lane
// l < K walks the row for moment l + 1; with fewer lanes than moments every lane walks the row once, forms every power by the
// running product and sums the moments l + 1, l + 1 + lr, .. it owns.  Either way a moment is the sum over the row's entries in
// row order of r * a * a * .. (the same bits), left in LDS; after the barrier lane q reads the K moments (one LDS broadcast each)
// and the float4 of theta it needs (theta transposed to [m][C] in LDS: consecutive lanes, consecutive banks), sums m upwards and
// stores its float4 of the output row.  A block keeps theta for all the row tiles it visits (grid-stride), the moment buffer is
// double-buffered so one barrier per tile is enough.  Reads per snapshot: a, col, r -- no table.
struct DiffusionMArgs {
  const int32_t *rowptr, *col;
  const float *a, *theta, *r, *tot;
  float *out;
  int n_rows, n_cols, c4, lr, K1, act, ntiles;
};

inline size_t diffusion_m_lds_bytes(int c4, int lr, int K1) {
  return sizeof(float) * ((size_t)K1 * c4 * 4 + 2 * (size_t)(256 / lr) * (K1 > 1 ? K1 - 1 : 1));
}

__device__ __forceinline__ void diffusion_m_load_theta(float *s_th, const float *theta, int C, int K1, int tid) {
  for (int idx = tid; idx < C * K1; idx += 256) s_th[(K1 - 1 - idx % K1) * C + idx / K1] = theta[idx];     // s_th[m][c] = theta[c][K - m]
}

__global__ __launch_bounds__(256) void k_diffusion_m(DiffusionMArgs a) {
  extern __shared__ float4 s_dyn4[];
  float *s_th = reinterpret_cast<float *>(s_dyn4);
  const int tid = threadIdx.x, C = a.c4 * 4, K = a.K1 - 1, rpb = 256 / a.lr, q = tid % a.lr, slot = tid / a.lr, s = blockIdx.y;
  float *s_M = s_th + a.K1 * C;                         // [2][rpb][K]
  diffusion_m_load_theta(s_th, a.theta, C, a.K1, tid);
  const float t = a.tot[s];
  const float *r = a.r + (int64_t)s * a.n_cols;
  const float4 *th4 = reinterpret_cast<const float4 *>(s_th) + q;
  int buf = 0;
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x, buf ^= 1) {      // uniform trip count: the barrier is safe
    const int i = tile * rpb + slot;
    float *M = s_M + (buf * rpb + slot) * K;
    if (i < a.n_rows) {
      const int beg = a.rowptr[i], end = a.rowptr[i + 1];
      if (a.lr >= K) {                   // one moment per lane (lanes K.. idle until the barrier): m multiplies per entry, sum in a register
        const int m = q + 1;
        if (m <= K) {
          float acc = 0.f;
          for (int p = beg; p < end; ++p) {
            const float av = a.a[p];
            float pw = r[a.col[p]];
            for (int j = 0; j < m; ++j) pw *= av;
            acc += pw;
          }
          M[m - 1] = acc;
        }
      } else {                           // fewer lanes than moments (C <= 32): ONE walk, every power once, lane q sums moments q + 1, q + 1 + lr, .. in LDS
        for (int m = q; m < K; m += a.lr) M[m] = 0.f;
        for (int p = beg; p < end; ++p) {
          const float av = a.a[p];
          float pw = r[a.col[p]];
          for (int j = 0; j < K; ++j) {
            pw *= av;
            if ((j & (a.lr - 1)) == q) M[j] += pw;       // its own slots only: no other lane touches them before the barrier
          }
        }
      }
    }
    __syncthreads();       // moments of this tile (and, first time round, theta) are in LDS
    if (i < a.n_rows && q < a.c4) {
      float4 th = th4[0];
      float4 o = make_float4(th.x * t, th.y * t, th.z * t, th.w * t);
      for (int m = 1; m <= K; ++m) {
        const float Mm = M[m - 1];
        th = th4[m * a.c4];
        o.x = fmaf(th.x, Mm, o.x), o.y = fmaf(th.y, Mm, o.y), o.z = fmaf(th.z, Mm, o.z), o.w = fmaf(th.w, Mm, o.w);
      }
      o.x = apply_act(o.x, a.act), o.y = apply_act(o.y, a.act), o.z = apply_act(o.z, a.act), o.w = apply_act(o.w, a.act);
      reinterpret_cast<float4 *>(a.out)[((int64_t)s * a.n_rows + i) * a.c4 + q] = o;
    }
  }
}

inline hipError_t launch_diffusion_m(DiffusionMArgs a, int S, hipStream_t st) {
  const int rpb = 256 / a.lr;
  a.ntiles = (a.n_rows + rpb - 1) / rpb;
  const int cap = 2048 / S > 256 ? 2048 / S : 256;      // ~2048 blocks or more: a block amortises its theta load over its tiles
  const int gx = a.ntiles < cap ? a.ntiles : cap;
  hipLaunchKernelGGL(k_diffusion_m, dim3((unsigned)gx, (unsigned)S), dim3(256), diffusion_m_lds_bytes(a.c4, a.lr, a.K1), st, a);
  return hipGetLastError();
}

// Reverse of k_diffusion_m.  dtheta needs the moments only: k_diffusion_bwd_rows / k_diffusion_bwd_reduce as they are (c0 read
// from theta's last column), which also leave gz and g0[s] = sum_{i, q} theta[q][K] gz[s, i, q] = sum_i G_0[s, i].  The dr pass
// replaces the table by
//     G_m[s, i] = sum_q theta[q][K-m] gz[s, i, q]      (m = 1..K)       k_diffusion_bwd_gm: lane group per row, fixed xor tree
//     dr[s, j]  = g0[s] + sum_{p : col p = j} sum_{m=1..K} a_p^m G_m[s, row p]      k_diffusion_bwd_input_m: thread per (j, s)
// Every value has one writer and a fixed order: no atomics, bitwise repeatable.
struct DiffusionBwdMArgs {
  DiffusionBwdArgs b;
  const float *theta;
  float *G;               // (S, n_rows, K)
};

__global__ __launch_bounds__(256) void k_diffusion_bwd_gm(DiffusionBwdMArgs m) {
  extern __shared__ float4 s_dyn4[];
  float *s_th = reinterpret_cast<float *>(s_dyn4);
  const DiffusionBwdArgs &a = m.b;
  const int tid = threadIdx.x, C = a.c4 * 4, K = a.K1 - 1, rpb = 256 / a.lr, q = tid % a.lr, slot = tid / a.lr, s = blockIdx.y;
  diffusion_m_load_theta(s_th, m.theta, C, a.K1, tid);
  __syncthreads();
  const bool qok = q < a.c4;
  const float4 *th4 = reinterpret_cast<const float4 *>(s_th) + (qok ? q : 0);
  const int ntiles = (a.n_rows + rpb - 1) / rpb;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // uniform trip count: every lane reaches the shuffles
    const int i = tile * rpb + slot;
    const bool live = i < a.n_rows;
    const float4 z = live && qok ? reinterpret_cast<const float4 *>(a.gz)[((int64_t)s * a.n_rows + i) * a.c4 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int mm = 1; mm <= K; ++mm) {
      const float4 th = th4[mm * a.c4];
      float v = fmaf(th.w, z.w, fmaf(th.z, z.z, fmaf(th.y, z.y, th.x * z.x)));
      for (int o = a.lr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (live && q == 0) m.G[((int64_t)s * a.n_rows + i) * K + (mm - 1)] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_diffusion_bwd_input_m(DiffusionBwdMArgs m) {
  const DiffusionBwdArgs &a = m.b;
  const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, K = a.K1 - 1;
  if (j >= a.n_cols) return;
  const float *G = m.G + (int64_t)s * a.n_rows * K;
  float acc = 0.f;
  for (int p = a.t_rowptr[j]; p < a.t_rowptr[j + 1]; ++p) {
    const float av = a.a[a.perm_t[p]];
    const float *g = G + (int64_t)a.t_col[p] * K;
    float pw = 1.f;
    for (int mm = 0; mm < K; ++mm) {
      pw *= av;
      acc = fmaf(pw, g[mm], acc);
    }
  }
  a.dr[(int64_t)s * a.n_cols + j] = a.g0[s] + acc;
}

inline hipError_t launch_diffusion_backward_m(const DiffusionBwdMArgs &m, hipStream_t st) {
  const DiffusionBwdArgs &a = m.b;
  if (a.K1 <= 8) hipLaunchKernelGGL(k_diffusion_bwd_rows<8>, dim3((unsigned)a.gx, (unsigned)a.sy), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_diffusion_bwd_rows<DIFF_KMAX>, dim3((unsigned)a.gx, (unsigned)a.sy), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_diffusion_bwd_reduce, dim3((unsigned)(a.K1 * a.c4 * 4 + a.S)), dim3(256), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.K1 > 1 && a.n_rows > 0) {
    const int rpb = 256 / a.lr, ntiles = (a.n_rows + rpb - 1) / rpb;
    const int cap = 2048 / a.S > 256 ? 2048 / a.S : 256;
    hipLaunchKernelGGL(k_diffusion_bwd_gm, dim3((unsigned)(ntiles < cap ? ntiles : cap), (unsigned)a.S), dim3(256),
                       sizeof(float) * (size_t)a.K1 * a.c4 * 4, st, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_diffusion_bwd_input_m, dim3((unsigned)((a.n_cols + 255) / 256), (unsigned)a.S), dim3(256), 0, st, m);
  return hipGetLastError();
}

// spektral GlobalAttnSumPool in batch mode (agent.py:93-94: the head of the RL agents' ConvNet): per sample b,
//     alpha = softmax_r(<x[b, r, :], k>),  out[b, :] = sum_r alpha_r x[b, r, :]
// One 256-thread workgroup per sample, one pass over its rows with an online (running-max) softmax: thread (c, part) owns float4
// chunk c of every row it visits (F <= 256), the 64 lanes of a wave visit 64 / (F/4) rows per step; the score of a row is a
// shuffle reduction over its F/4 lanes.  Partial (max, sum, weighted row) triples are merged through LDS at the end.
struct AttnPoolArgs {
  const float *x, *k;
  float *out;
  int R, F4;          // rows per sample, float4 chunks per row (a power of two <= 64)
};

__global__ __launch_bounds__(256) void k_attn_sum_pool(AttnPoolArgs a) {
  __shared__ float s_m[256], s_l[256];
  __shared__ float4 s_acc[256];
  const int tid = threadIdx.x, c = tid % a.F4, part = tid / a.F4, n_part = 256 / a.F4;
  const float4 *xb = reinterpret_cast<const float4 *>(a.x) + (int64_t)blockIdx.x * a.R * a.F4;
  const float4 kc = reinterpret_cast<const float4 *>(a.k)[c];
  float m = -INFINITY, l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r0 = 0; r0 < a.R; r0 += n_part) {          // every thread of the workgroup runs the same number of steps (shuffles below)
    const int r = r0 + part;
    const bool live = r < a.R;
    const float4 v = live ? xb[(int64_t)r * a.F4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    float sc = v.x * kc.x + v.y * kc.y + v.z * kc.z + v.w * kc.w;
    for (int o = a.F4 >> 1; o > 0; o >>= 1) sc += __shfl_xor(sc, o);      // the F4 lanes of a row are consecutive and aligned
    if (live) {
      const float mn = fmaxf(m, sc), f_old = __expf(m - mn), w = __expf(sc - mn);
      l = l * f_old + w;
      acc.x = acc.x * f_old + w * v.x; acc.y = acc.y * f_old + w * v.y; acc.z = acc.z * f_old + w * v.z; acc.w = acc.w * f_old + w * v.w;
      m = mn;
    }
  }
  s_m[tid] = m; s_l[tid] = l; s_acc[tid] = acc;
  __syncthreads();
  if (part == 0) {                                      // chunk c: merge the n_part partial triples in a fixed order (reproducible)
    float M = -INFINITY;
    for (int p = 0; p < n_part; ++p) M = fmaxf(M, s_m[p * a.F4 + c]);
    float L = 0.f;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < n_part; ++p) {
      const int q = p * a.F4 + c;
      if (s_l[q] > 0.f) {
        const float f = __expf(s_m[q] - M);
        L += s_l[q] * f;
        A.x += s_acc[q].x * f; A.y += s_acc[q].y * f; A.z += s_acc[q].z * f; A.w += s_acc[q].w * f;
      }
    }
    const float inv = 1.0f / L;
    reinterpret_cast<float4 *>(a.out)[(int64_t)blockIdx.x * a.F4 + c] = make_float4(A.x * inv, A.y * inv, A.z * inv, A.w * inv);
  }
}

// ---- training-time dropout (emulator.py:199-213,234-235,287-288,314-318; keras Dropout = inverted dropout) ----------------
// out[i] = x[i] / (1 - rate) where bit i is kept, else 0.  The mask is a pure function of (seed, offset + i): Philox4x32-10
// (Salmon et al., SC'11) with key = seed, counter = (offset + i) / 4, word (offset + i) % 4 -- nothing is stored, the backward
// pass calls the same kernel on the gradient with the same (seed, offset).  A word u keeps its element when u >= rate * 2^32.
struct DropoutArgs {
  const float *x;
  float *out;
  int64_t n;
  unsigned long long seed, offset;
  unsigned thresh;
  float scale;
};

__device__ __forceinline__ void philox4x32_10(unsigned long long ctr_lo, unsigned long long ctr_hi, unsigned long long key, unsigned (&r)[4]) {
  unsigned c0 = (unsigned)ctr_lo, c1 = (unsigned)(ctr_lo >> 32), c2 = (unsigned)ctr_hi, c3 = (unsigned)(ctr_hi >> 32);
  unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// one thread = one counter = four consecutive elements (offset % 4 == 0 and 16-byte aligned x / out: the float4 path; else scalar)
__global__ __launch_bounds__(256) void k_dropout(DropoutArgs a) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // index of the group of four ELEMENT POSITIONS offset + 4q ..
  const unsigned long long g0 = a.offset >> 2;
  const int lead = (int)(a.offset & 3);                                    // elements of the first counter that precede x[0]
  // element i uses counter (offset + i) >> 2, word (offset + i) & 3: thread q covers positions p = 4 (g0 + q) + w, i = p - offset
  unsigned r[4];
  philox4x32_10(g0 + (unsigned long long)q, 0ull, a.seed, r);
  const int64_t i0 = 4 * q - lead;
  if (lead == 0 && i0 + 3 < a.n && ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out)) & 15) == 0) {
    const float4 v = *reinterpret_cast<const float4 *>(a.x + i0);
    float4 o;
    o.x = r[0] >= a.thresh ? v.x * a.scale : 0.f;
    o.y = r[1] >= a.thresh ? v.y * a.scale : 0.f;
    o.z = r[2] >= a.thresh ? v.z * a.scale : 0.f;
    o.w = r[3] >= a.thresh ? v.w * a.scale : 0.f;
    *reinterpret_cast<float4 *>(a.out + i0) = o;
    return;
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int64_t i = i0 + w;
    if (i >= 0 && i < a.n) a.out[i] = r[w] >= a.thresh ? a.x[i] * a.scale : 0.f;
  }
}

}  // namespace uds
