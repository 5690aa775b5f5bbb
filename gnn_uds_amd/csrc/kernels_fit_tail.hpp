// Everything `Emulator.fit_eval` / `fit_grad_norm` do after the network forward (emulator.py:400-484: `post_proc_tf`, clamp(0, 1),
// `get_node_loss` plain or in its `balance` form through `constrain_tf`, the weighted flood BCE, the link MSE) as ONE forward
// triple and ONE backward pair:
//   k_fit_link      (b, t, link) rows, grid-stride: the gated flow (tail_link_flow of kernels_tail.hpp)  -> out_ey (B,T,E,ce),
//                   the row's link-MSE term, one partial per workgroup
//   k_fit_node      (b, t, node) rows, grid-stride: flow balance over the node's incidence row (reads out_ey, loop order of
//                   k_flow_balance) or the node pump / a_in / a_out gates, tide                           -> out_y (B,T,N,C),
//                   the row's node-MSE and flood-BCE terms on clamp(out_y, 0, 1), one partial each per workgroup
//   k_fit_reduce    three workgroups: the partials of one loss each, added in a fixed order                -> loss_sums[3]
//   k_fit_node_bwd  (b, t, node) rows: recomputes the row, d loss / d row + the gradient arriving at out_y -> dy, and per node the
//                   gradients of q_in / q_out in the workspace
//   k_fit_link_bwd  (b, t, link) rows: gathers those from the link's two incidence entries, link MSE + the gradient arriving at
//                   out_ey, the gates                                                                     -> dey
// out_y / out_ey repeat the tensor code's operations in its order, rounded one by one (no fused multiply-add): bit-identical to
// `post_proc_tf`.  The loss sums are the sums of the per-sample terms of `_mse` / `_bce` before the division by the sample count;
// no atomics anywhere, so two runs give the same bits.  Derivatives as kernels_tail.hpp states them; clamp(0, 1) and the BCE's clip
// pass on their closed interval, as torch's clamp does.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels_tail.hpp"

namespace uds {

constexpr int FIT_MAX_BLOCKS = 1024;      // workgroups (= partials) per loss at most; rows beyond are taken grid-stride
constexpr float BCE_EPS = 1e-7f;          // keras backend epsilon: probabilities are clipped to [eps, 1 - eps]

struct FitTailArgs {
  TailArgs t;                                     // constants, pattern, y, ey, a, b_norm, out_y / out_ey, g_out_*, dy / dey, ws_qi / ws_qo
  const float *y_true, *ey_true;                  // (B,T,N,cyt) (B,T,E,ce)
  const float *nwei, *poswei, *ewei;              // (N, 3 + balance) (N) (E)
  const float *qw_den, *span_b, *mini_b;          // balance only, per node: norm_y[0, :, -1]; max - min / min of the runoff channel
  const float *g_loss;                            // backward: 3 device values
  float *part_node, *part_flood, *part_edge;      // one partial per workgroup
  float *loss_sums;                               // [node, flood, edge]
  int cyt, balance, node_blocks, link_blocks;
};

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }      // hands a NaN on, as torch.clamp
__device__ __forceinline__ float pass01(float v) { return gate(v >= 0.f && v <= 1.f); }

// sum over the 256 threads of a workgroup, the same order every run: wave butterflies, then the four wave sums
__device__ __forceinline__ float block_sum256(float v, float *sm) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// The normalised row [h, q_in, q_out, (flood)] `post_proc_tf` returns for node n at snapshot bt.  FROM_OUT: the link flows are read
// from out_ey (forward, behind k_fit_link); otherwise they are recomputed (backward).  g = the node gates of the non-edge-fusion form.
template <bool FROM_OUT>
__device__ __forceinline__ void fit_node_row(const TailArgs &t, int64_t bt, int n, float &v0, float &v1, float &v2, float &v3, NodeGates &g) {
  const uds_tail_t &p = t.p;
  const float *yr = t.y + (bt * p.N + n) * p.cy;
  v0 = tail_depth(t, bt, n);
  v3 = p.if_flood ? yr[p.cy - 1] : 0.f;
  if (p.edge_fusion) {
    const int cl = p.ce - 1;
    float qi = 0.f, qo = 0.f;
    for (int q = t.rowptr[n]; q < t.rowptr[n + 1]; ++q) {
      const int l = t.col[q];
      float fl;
      if (FROM_OUT) {
        fl = t.out_ey[(bt * p.E + l) * p.ce + cl];
      } else {
        float pre, dflow, set;
        fl = tail_link_flow(t, bt, l, pre, dflow, set);
      }
      const float v = __fadd_rn(__fmul_rn(fl, p.span_e[(int64_t)l * p.ce + cl]), p.mini_e[(int64_t)l * p.ce + cl]);
      const float fp = fmaxf(v, 0.f), fn = fmaxf(-v, 0.f);
      if (t.sign[q] > 0.f) { qo += fp; qi += fn; } else { qi += fp; qo += fn; }
    }
    v1 = __fmul_rn(qi, p.scale_in[n]);
    v2 = __fmul_rn(qo, p.scale_out[n]);
    g = NodeGates{0.f, 0.f, 1.f, 1.f, 1.f, 1.f};
  } else {
    tail_node_gates(t, bt, n, v0, v1, v2, g);
  }
}

// log(p) and log(1 - p) of the BCE for p clipped to [eps, 1 - eps].  p and 1 - p are clipped apart (1 - v is exact for v >= 1/2), so
// a saturated probability gives log(eps) as the definition has it, not log(1 - fl(1 - eps)) = log(2^-23).  q = the clipped 1 - p.
__device__ __forceinline__ void bce_logs(float v, float &pc, float &qc, float &logp, float &logq) {
  pc = t_min(t_max(v, BCE_EPS), 1.f);
  qc = t_min(t_max(__fsub_rn(1.f, v), BCE_EPS), 1.f);
  if (v >= 0.5f) {
    logp = log1pf(-qc);
    logq = logf(qc);
  } else {
    logp = logf(pc);
    logq = log1pf(-pc);
  }
}

__global__ __launch_bounds__(256) void k_fit_link(FitTailArgs a) {
  __shared__ float sm[4];
  const TailArgs &t = a.t;
  const uds_tail_t &p = t.p;
  const int64_t total = (int64_t)t.B * t.T * p.E;
  const int cl = p.ce - 1;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t bt = i / p.E;
    const int l = (int)(i - bt * p.E);
    float pre, dflow, set;
    const float flow = tail_link_flow(t, bt, l, pre, dflow, set);
    const float *er = t.ey + i * p.ce, *tr = a.ey_true + i * p.ce;
    float *o = t.out_ey + i * p.ce;
    float s = 0.f;
    for (int c = 0; c < cl; ++c) {
      const float v = er[c], d = v - tr[c];
      o[c] = v;
      s += d * d;
    }
    const float d = flow - tr[cl];
    o[cl] = flow;
    s += d * d;
    acc += s / (float)p.ce * a.ewei[l];
  }
  const float sum = block_sum256(acc, sm);
  if (threadIdx.x == 0) a.part_edge[blockIdx.x] = sum;
}

// The four rows of the `balance` node loss (get_node_loss): the clamped prediction de-normalised, constrain_tf, re-normalised and
// clamped again, q_w over its norm.  D = the de-normalised row, pre = the re-normalised one before its clamp, P = the four
// compared values, f / m / s = constrain_tf's flood gate, epsilon gate and q_us + r - q_ds.
struct Balance { float D0, D1, D2, pre0, pre1, pre2, P0, P1, P2, P3, f, m, s; };

__device__ __forceinline__ void fit_balance(const FitTailArgs &a, int64_t row, int n, float c0, float c1, float c2, float c3, Balance &k) {
  const TailArgs &t = a.t;
  const uds_tail_t &p = t.p;
  const float *sp = p.span_y + (int64_t)n * t.C, *mn = p.mini_y + (int64_t)n * t.C;
  k.D0 = __fadd_rn(__fmul_rn(c0, sp[0]), mn[0]);
  k.D1 = __fadd_rn(__fmul_rn(c1, sp[1]), mn[1]);
  k.D2 = __fadd_rn(__fmul_rn(c2, sp[2]), mn[2]);
  const float F = p.if_flood ? __fadd_rn(__fmul_rn(c3, sp[3]), mn[3]) : 0.f;
  const float r = __fadd_rn(__fmul_rn(t.b_norm[row * p.b_channels], a.span_b[n]), a.mini_b[n]);
  float hc, qw;
  tail_constrain(p, n, k.D0, k.D1, k.D2, r, F, hc, qw, k.f, k.m, k.s);
  k.pre0 = __fdiv_rn(__fsub_rn(hc, mn[0]), sp[0]);
  k.pre1 = __fdiv_rn(__fsub_rn(k.D1, mn[1]), sp[1]);
  k.pre2 = __fdiv_rn(__fsub_rn(k.D2, mn[2]), sp[2]);
  k.P0 = clamp01(k.pre0);
  k.P1 = clamp01(k.pre1);
  k.P2 = clamp01(k.pre2);
  k.P3 = __fdiv_rn(qw, a.qw_den[n]);
}

__global__ __launch_bounds__(256) void k_fit_node(FitTailArgs a) {
  __shared__ float sm[4];
  const TailArgs &t = a.t;
  const uds_tail_t &p = t.p;
  const int64_t total = (int64_t)t.B * t.T * p.N;
  const int C = t.C, nw = 3 + a.balance;
  float acc_n = 0.f, acc_f = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t bt = i / p.N;
    const int n = (int)(i - bt * p.N);
    float v0, v1, v2, v3;
    NodeGates g;
    fit_node_row<true>(t, bt, n, v0, v1, v2, v3, g);
    float *o = t.out_y + i * C;
    o[0] = v0;
    o[1] = v1;
    o[2] = v2;
    if (C == 4) o[3] = v3;
    const float c0 = clamp01(v0), c1 = clamp01(v1), c2 = clamp01(v2), c3 = clamp01(v3);
    const float *yt = a.y_true + i * a.cyt, *w = a.nwei + (int64_t)n * nw;
    if (a.balance) {
      Balance k;
      fit_balance(a, i, n, c0, c1, c2, c3, k);
      const float d0 = (k.P0 - yt[0]) * w[0], d1 = (k.P1 - yt[1]) * w[1], d2 = (k.P2 - yt[2]) * w[2], d3 = (k.P3 - yt[a.cyt - 1]) * w[3];
      acc_n += ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * 0.25f;
    } else {
      const float d0 = (c0 - yt[0]) * w[0], d1 = (c1 - yt[1]) * w[1], d2 = (c2 - yt[2]) * w[2];
      acc_n += (d0 * d0 + d1 * d1 + d2 * d2) / 3.f;
      if (p.if_flood) {
        const float ytf = yt[a.cyt - 2];
        float pc, qc, logp, logq;
        bce_logs(c3, pc, qc, logp, logq);
        const float per = -(ytf * logp + (1.f - ytf) * logq);
        acc_f += per * (a.poswei[n] * ytf + w[nw - 1] * (1.f - ytf));
      }
    }
  }
  const float sn = block_sum256(acc_n, sm);
  const float sf = block_sum256(acc_f, sm);
  if (threadIdx.x == 0) {
    a.part_node[blockIdx.x] = sn;
    a.part_flood[blockIdx.x] = sf;
  }
}

__global__ __launch_bounds__(256) void k_fit_reduce(FitTailArgs a) {
  __shared__ float sm[4];
  const float *part = blockIdx.x == 0 ? a.part_node : (blockIdx.x == 1 ? a.part_flood : a.part_edge);
  const int n = blockIdx.x == 2 ? a.link_blocks : a.node_blocks;
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
  const float sum = block_sum256(acc, sm);
  if (threadIdx.x == 0) a.loss_sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_fit_node_bwd(FitTailArgs a) {
  const TailArgs &t = a.t;
  const uds_tail_t &p = t.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)t.B * t.T * p.N) return;
  const int64_t bt = i / p.N;
  const int n = (int)(i - bt * p.N);
  const int C = t.C, nw = 3 + a.balance;
  const float gN = a.g_loss[0], gF = a.g_loss[1];
  float v0, v1, v2, v3;
  NodeGates ng;
  fit_node_row<false>(t, bt, n, v0, v1, v2, v3, ng);
  const float c0 = clamp01(v0), c1 = clamp01(v1), c2 = clamp01(v2), c3 = clamp01(v3);
  const float *yt = a.y_true + i * a.cyt, *w = a.nwei + (int64_t)n * nw;
  // d loss / d clamped row
  float l0, l1, l2, l3 = 0.f;
  if (a.balance) {
    Balance k;
    fit_balance(a, i, n, c0, c1, c2, c3, k);
    const float *sp = p.span_y + (int64_t)n * C;
    const float h = 0.5f * gN;      // 2 / 4
    const float gP0 = h * w[0] * w[0] * (k.P0 - yt[0]), gP1 = h * w[1] * w[1] * (k.P1 - yt[1]), gP2 = h * w[2] * w[2] * (k.P2 - yt[2]);
    const float gqw = h * w[3] * w[3] * (k.P3 - yt[a.cyt - 1]) / a.qw_den[n];
    const float gs = k.s >= 0.f ? gqw * k.m * (1.f - p.is_outfall[n]) : 0.f;
    const float hmin = p.hmin[n], hmax = p.hmax[n];
    const float ghc = gP0 * pass01(k.pre0) / sp[0];
    const float gD0 = ghc * (1.f - k.f) * w_max(k.D0, hmin) * w_min(t_max(k.D0, hmin), hmax);
    const float gD1 = gP1 * pass01(k.pre1) / sp[1] + gs, gD2 = gP2 * pass01(k.pre2) / sp[2] - gs;
    l0 = gD0 * sp[0];
    l1 = gD1 * sp[1];
    l2 = gD2 * sp[2];
  } else {
    const float h = gN * (2.f / 3.f);
    l0 = h * w[0] * w[0] * (c0 - yt[0]);
    l1 = h * w[1] * w[1] * (c1 - yt[1]);
    l2 = h * w[2] * w[2] * (c2 - yt[2]);
    if (p.if_flood) {
      const float ytf = yt[a.cyt - 2];
      float pc, qc, logp, logq;
      bce_logs(c3, pc, qc, logp, logq);
      const float weight = a.poswei[n] * ytf + w[nw - 1] * (1.f - ytf);
      const float inside = gate(c3 >= BCE_EPS && __fsub_rn(1.f, c3) >= BCE_EPS);
      l3 = gF * weight * ((1.f - ytf) / qc - ytf / pc) * inside;
    }
  }
  float g0 = l0 * pass01(v0), g1 = l1 * pass01(v1), g2 = l2 * pass01(v2), g3 = l3 * pass01(v3);
  if (t.g_out_y) {
    const float *g = t.g_out_y + i * C;
    g0 += g[0];
    g1 += g[1];
    g2 += g[2];
    if (C == 4) g3 += g[3];
  }
  float *dy = t.dy + i * p.cy;
  dy[0] = g0 * (p.tide ? 1.f - p.is_outfall[n] : 1.f);
  if (p.edge_fusion) {
    t.ws_qi[i] = g1 * p.scale_in[n];
    t.ws_qo[i] = g2 * p.scale_out[n];
  } else {
    dy[1] = g1 * ng.s_in * ng.z_in;
    dy[2] = g2 * ng.s_out * ng.z_out;
  }
  if (p.if_flood) dy[p.cy - 1] = g3;
}

__global__ __launch_bounds__(256) void k_fit_link_bwd(FitTailArgs a) {
  const TailArgs &t = a.t;
  const uds_tail_t &p = t.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)t.B * t.T * p.E) return;
  const int64_t bt = i / p.E;
  const int l = (int)(i - bt * p.E);
  const int cl = p.ce - 1;
  float pre, dflow, set;
  const float flow = tail_link_flow(t, bt, l, pre, dflow, set);
  const float *er = t.ey + i * p.ce, *tr = a.ey_true + i * p.ce;
  const float *g = t.g_out_ey ? t.g_out_ey + i * p.ce : nullptr;
  float *d = t.dey + i * p.ce;
  const float h = a.g_loss[2] * 2.f / (float)p.ce * a.ewei[l];
  for (int c = 0; c < cl; ++c) d[c] = h * (er[c] - tr[c]) + (g ? g[c] : 0.f);
  float gflow = h * (flow - tr[cl]) + (g ? g[cl] : 0.f);
  if (p.edge_fusion) {
    const float sp = p.span_e[(int64_t)l * p.ce + cl];
    const float v = __fadd_rn(__fmul_rn(flow, sp), p.mini_e[(int64_t)l * p.ce + cl]);
    float pos = 0.f, neg = 0.f;      // as k_tail_link_bwd: what a positive / a negative flow feeds
    for (int j = 0; j < 2; ++j) {
      const int nd = p.link_node[2 * l + j];
      if (nd < 0) continue;
      const float gi = t.ws_qi[bt * p.N + nd], go = t.ws_qo[bt * p.N + nd];
      if (p.link_sign[2 * l + j] > 0.f) { pos += go; neg += gi; } else { pos += gi; neg += go; }
    }
    gflow += (v > 0.f ? pos : (v < 0.f ? -neg : 0.f)) * sp;
  }
  d[cl] = gflow * set * dflow;
}

inline unsigned fit_blocks(int64_t rows) { return (unsigned)std::min<int64_t>((rows + 255) / 256, FIT_MAX_BLOCKS); }

inline hipError_t launch_fit_tail_forward(const FitTailArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_fit_link, dim3(a.link_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_fit_node, dim3(a.node_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_fit_reduce, dim3(3), dim3(256), 0, st, a);
  return hipGetLastError();
}

inline hipError_t launch_fit_tail_backward(const FitTailArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_fit_node_bwd, dim3(tail_grid((int64_t)a.t.B * a.t.T * a.t.p.N)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_fit_link_bwd, dim3(tail_grid((int64_t)a.t.B * a.t.T * a.t.p.E)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace uds
