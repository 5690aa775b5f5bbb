// Everything `Emulator._predict` does after the network forward (emulator.py `_post_proc`, the de-normalisation, the ehmax
// clamp, the pumped-storage depth scan and `constrain_tf`) as ONE forward pair and ONE backward triple:
//   k_tail_link      one thread per (b, t, link):  from-node depth (tide form), offset gate, rated-pump override, setting,
//                    de-normalisation of all ce channels, clamp of channel 0 to [0, ehmax]        -> out_ey (B,T,E,ce)
//   k_tail_node      one thread per (b, node), t in order: flow balance over the node's incidence row (reads out_ey, loop order
//                    of k_flow_balance) or the node pump / a_in / a_out gates, tide, de-normalisation, depth recurrence,
//                    constrain_tf                                                                   -> out_y (B,T,N,4 or 5)
//   k_tail_node_bwd  one thread per (b, node): forward sweep (values kept in the workspace), then t in reverse
//   k_tail_link_bwd  one thread per (b, t, link): gathers the node gradients of its two ends
//   k_tail_da        one thread per (b, t, action): sums the short lists of links / nodes the action drives (no atomics)
// The forward uses the tensor code's operations in the tensor code's order, rounded one by one (__fmul_rn / __fadd_rn /
// __fdiv_rn: no fused multiply-add), so it is bit-identical to that composition.  Derivatives: hard gates (comparisons) carry
// none; maximum / minimum split evenly at a tie; clamp(min=0) passes at the bound; the flow balance passes nothing at a flow
// of exactly 0 (autograd.FlowBalanceFn).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/uds_hip.h"

namespace uds {

struct TailArgs {
  uds_tail_t p;
  const int32_t *rowptr, *col;
  const float *sign;
  const float *y, *ey, *a, *b_norm, *runoff, *h0;      // (B,T,N,cy) (B,T,E,ce) (B,T,n_act) (B,T,N,b_channels) (B,T,N) (B,N)
  float *out_y, *out_ey;                               // (B,T,N,C+1) (B,T,E,ce), C = 3 + flood
  const float *g_out_y, *g_out_ey;
  float *dy, *dey, *da, *dh0;
  float *ws_qi, *ws_qo, *ws_prev, *ws_set;             // (B,T,N) x 3, (B,T,E)
  int B, T, C;
};

// torch.minimum / torch.maximum hand a NaN on; fminf / fmaxf would drop it
__device__ __forceinline__ float t_min(float a, float b) { return (a != a || b != b) ? (a != a ? a : b) : fminf(a, b); }
__device__ __forceinline__ float t_max(float a, float b) { return (a != a || b != b) ? (a != a ? a : b) : fmaxf(a, b); }
__device__ __forceinline__ float t_clamp0(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float gate(bool c) { return c ? 1.f : 0.f; }
// d max(v, lo) / dv and d min(v, hi) / dv as torch.maximum / torch.minimum define them
__device__ __forceinline__ float w_max(float v, float lo) { return v > lo ? 1.f : (v == lo ? 0.5f : 0.f); }
__device__ __forceinline__ float w_min(float v, float hi) { return v < hi ? 1.f : (v == hi ? 0.5f : 0.f); }

// normalised depth of node n at snapshot bt after the tide step: y0 * (1 - is_outfall) + b[..., -1]
__device__ __forceinline__ float tail_depth(const TailArgs &a, int64_t bt, int n) {
  const uds_tail_t &p = a.p;
  float h = a.y[(bt * p.N + n) * p.cy];
  if (p.tide) h = __fadd_rn(__fmul_rn(h, __fsub_rn(1.f, p.is_outfall[n])), a.b_norm[(bt * p.N + n) * p.b_channels + p.b_channels - 1]);
  return h;
}

// The gated, still normalised flow of link l at snapshot bt.  pre = the flow before the setting multiplies it, dflow = the
// derivative of `pre` with respect to the predicted flow (a product of 0/1 gates), set = the link's setting (1 without one).
__device__ __forceinline__ float tail_link_flow(const TailArgs &a, int64_t bt, int l, float &pre, float &dflow, float &set) {
  const uds_tail_t &p = a.p;
  float flow = a.ey[(bt * p.E + l) * p.ce + p.ce - 1];
  dflow = 1.f;
  set = 1.f;
  const bool override_ = p.act && p.pump_override;
  if (p.has_offset || override_) {
    const int fn = p.from_node[l];
    const float ok = p.from_ok[l];
    const float hn = tail_depth(a, bt, fn);
    if (p.has_offset) {
      const float hd = __fadd_rn(__fmul_rn(hn, p.span_y[(int64_t)fn * a.C]), p.mini_y[(int64_t)fn * a.C]);
      const float inoff = __fmul_rn(__fsub_rn(hd, p.hmin[fn]), ok);
      const float off = p.offset[l];
      const float m1 = gate(flow > 0.f), m4 = gate(flow <= 0.f), m2 = gate(off > 0.f), m3 = gate(inoff > off), m5 = gate(off == 0.f);
      const float t1 = __fmul_rn(__fmul_rn(__fmul_rn(flow, m1), m2), m3);
      const float t2 = __fmul_rn(__fmul_rn(flow, m4), m2);
      const float t3 = __fmul_rn(flow, m5);
      flow = __fadd_rn(__fadd_rn(t1, t2), t3);
      dflow = m1 * m2 * m3 + m4 * m2 + m5;
    }
    if (override_) {
      float fl = __fmul_rn(p.pump[l], __fmul_rn(gate(hn > 0.01f), ok));
      fl = __fdiv_rn(__fmul_rn(fl, p.pump_mask[l]), p.pump_den[l]);
      const float z = gate(fl == 0.f);
      flow = __fadd_rn(__fmul_rn(flow, z), fl);
      dflow *= z;
    }
  }
  pre = flow;
  if (p.act) {
    const int k = p.act_link[l];
    if (k > 0) set = a.a[bt * p.n_act + (k - 1)];
    flow = __fmul_rn(flow, set);
  }
  return flow;
}

__global__ __launch_bounds__(256) void k_tail_link(TailArgs a) {
  const uds_tail_t &p = a.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.T * p.E) return;
  const int64_t bt = i / p.E;
  const int l = (int)(i - bt * p.E);
  float pre, dflow, set;
  const float flow = tail_link_flow(a, bt, l, pre, dflow, set);
  const float *er = a.ey + i * p.ce;
  const float *sp = p.span_e + (int64_t)l * p.ce, *mn = p.mini_e + (int64_t)l * p.ce;
  float *o = a.out_ey + i * p.ce;
  o[0] = t_min(t_clamp0(__fadd_rn(__fmul_rn(er[0], sp[0]), mn[0])), p.ehmax[l]);
  for (int c = 1; c < p.ce - 1; ++c) o[c] = __fadd_rn(__fmul_rn(er[c], sp[c]), mn[c]);
  o[p.ce - 1] = __fadd_rn(__fmul_rn(flow, sp[p.ce - 1]), mn[p.ce - 1]);
}

// The normalised node row [h, q_in, q_out] of the non-edge-fusion form: pump gates and a_in / a_out.  in_pre / out_pre = the
// flows before their settings, z_in / z_out = the 0/1 gates on the predicted flows, s_in / s_out = the settings.
struct NodeGates { float in_pre, out_pre, z_in, z_out, s_in, s_out; };

__device__ __forceinline__ void tail_node_gates(const TailArgs &a, int64_t bt, int n, float hn, float &q1, float &q2, NodeGates &g) {
  const uds_tail_t &p = a.p;
  const float *yr = a.y + (bt * p.N + n) * p.cy;
  q1 = yr[1];
  q2 = yr[2];
  g = NodeGates{q1, q2, 1.f, 1.f, 1.f, 1.f};
  if (!p.act) return;
  const float open = gate(hn > p.depth_gate);
  const float fli = __fdiv_rn(__fmul_rn(p.pump_in[n], open), p.ny_in[n]);
  const float flo = __fdiv_rn(__fmul_rn(p.pump_out[n], open), p.ny_out[n]);
  g.z_in = gate(fli == 0.f);
  g.z_out = gate(flo == 0.f);
  g.in_pre = __fadd_rn(__fmul_rn(q1, g.z_in), fli);
  g.out_pre = __fadd_rn(__fmul_rn(q2, g.z_out), flo);
  const int ki = p.act_in[n], ko = p.act_out[n];
  if (ki > 0) g.s_in = a.a[bt * p.n_act + (ki - 1)];
  if (ko > 0) g.s_out = a.a[bt * p.n_act + (ko - 1)];
  q1 = __fmul_rn(g.in_pre, g.s_in);
  q2 = __fmul_rn(g.out_pre, g.s_out);
}

// depth clip, flood bit and q_w of constrain_tf on the de-normalised row; f = the flood gate (0 without a flood channel),
// m = the 0/1 gate the epsilon mode puts on q_w
__device__ __forceinline__ void tail_constrain(const uds_tail_t &p, int n, float H, float QI, float QO, float r, float F, float &hc, float &qw,
                                               float &f, float &m, float &s) {
  const float hmin = p.hmin[n], hmax = p.hmax[n];
  hc = t_min(t_max(H, hmin), hmax);
  s = __fsub_rn(__fadd_rn(QI, r), QO);
  qw = __fmul_rn(t_clamp0(s), __fsub_rn(1.f, p.is_outfall[n]));
  f = 0.f;
  m = 1.f;
  if (p.if_flood) {
    f = gate(F > 0.5f);
    hc = __fadd_rn(__fmul_rn(hmax, f), __fmul_rn(hc, __fsub_rn(1.f, f)));
  }
  if (p.epsilon > 0.f) m = gate(__fsub_rn(hmax, hc) < p.epsilon);
  else if (p.epsilon < 0.f && p.if_flood) m = f;
  if (p.epsilon > 0.f || (p.epsilon < 0.f && p.if_flood)) qw = __fmul_rn(qw, m);
}

__global__ __launch_bounds__(256) void k_tail_node(TailArgs a) {
  const uds_tail_t &p = a.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * p.N) return;
  const int b = (int)(i / p.N), n = (int)(i - (int64_t)b * p.N);
  const int C = a.C;
  const float *sp = p.span_y + (int64_t)n * C, *mn = p.mini_y + (int64_t)n * C;
  const int r0 = a.rowptr[n], r1 = a.rowptr[n + 1];
  float de = 0.f;
  for (int t = 0; t < a.T; ++t) {
    const int64_t bt = (int64_t)b * a.T + t;
    const float hn = tail_depth(a, bt, n);
    const float *yr = a.y + (bt * p.N + n) * p.cy;
    float q1, q2, F = 0.f;
    float *o = a.out_y + (bt * p.N + n) * (C + 1);
    if (p.edge_fusion) {
      const float *f = a.out_ey + bt * p.E * p.ce + (p.ce - 1);
      float qi = 0.f, qo = 0.f;
      for (int q = r0; q < r1; ++q) {
        const float v = f[(int64_t)a.col[q] * p.ce];
        const float fp = fmaxf(v, 0.f), fn = fmaxf(-v, 0.f);
        if (a.sign[q] > 0.f) { qo += fp; qi += fn; } else { qi += fp; qo += fn; }
      }
      q1 = __fmul_rn(qi, p.scale_in[n]);
      q2 = __fmul_rn(qo, p.scale_out[n]);
      for (int c = 1; c < p.cy; ++c) {
        const float v = __fadd_rn(__fmul_rn(yr[c], sp[c + 2]), mn[c + 2]);
        o[c + 2] = v;
        F = v;
      }
    } else {
      NodeGates g;
      tail_node_gates(a, bt, n, hn, q1, q2, g);
      for (int c = 3; c < p.cy; ++c) {
        const float v = __fadd_rn(__fmul_rn(yr[c], sp[c]), mn[c]);
        o[c] = v;
        F = v;
      }
    }
    float H = __fadd_rn(__fmul_rn(hn, sp[0]), mn[0]);
    const float QI = __fadd_rn(__fmul_rn(q1, sp[1]), mn[1]), QO = __fadd_rn(__fmul_rn(q2, sp[2]), mn[2]);
    if (p.any_pump) {
      const float prev = t == 0 ? a.h0[i] : __fadd_rn(de, __fdiv_rn(__fsub_rn(QI, QO), p.area_eps[n]));
      de = t_min(t_max(prev, p.hmin[n]), p.hmax[n]);
      H = __fadd_rn(__fmul_rn(H, __fsub_rn(1.f, p.ps[n])), __fmul_rn(de, p.ps[n]));
    }
    float hc, qw, f, m, s;
    tail_constrain(p, n, H, QI, QO, a.runoff[bt * p.N + n], F, hc, qw, f, m, s);
    o[0] = hc;
    o[1] = QI;
    o[2] = QO;
    o[C] = qw;
  }
}

__global__ __launch_bounds__(256) void k_tail_node_bwd(TailArgs a) {
  const uds_tail_t &p = a.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * p.N) return;
  const int b = (int)(i / p.N), n = (int)(i - (int64_t)b * p.N);
  const int C = a.C;
  const float *sp = p.span_y + (int64_t)n * C, *mn = p.mini_y + (int64_t)n * C;
  const int r0 = a.rowptr[n], r1 = a.rowptr[n + 1];
  const float hmin = p.hmin[n], hmax = p.hmax[n];
  const float ps = p.any_pump ? p.ps[n] : 0.f, area = p.any_pump ? p.area_eps[n] : 1.f;
  // forward sweep: the de-normalised flows and the depth the recurrence proposes, kept for the reverse sweep
  float de = 0.f;
  for (int t = 0; t < a.T; ++t) {
    const int64_t bt = (int64_t)b * a.T + t;
    float q1, q2;
    if (p.edge_fusion) {
      float qi = 0.f, qo = 0.f;
      for (int q = r0; q < r1; ++q) {
        const int l = a.col[q];
        float pre, dflow, set;
        const float fl = tail_link_flow(a, bt, l, pre, dflow, set);
        const float v = __fadd_rn(__fmul_rn(fl, p.span_e[(int64_t)l * p.ce + p.ce - 1]), p.mini_e[(int64_t)l * p.ce + p.ce - 1]);
        const float fp = fmaxf(v, 0.f), fn = fmaxf(-v, 0.f);
        if (a.sign[q] > 0.f) { qo += fp; qi += fn; } else { qi += fp; qo += fn; }
      }
      q1 = __fmul_rn(qi, p.scale_in[n]);
      q2 = __fmul_rn(qo, p.scale_out[n]);
    } else {
      NodeGates g;
      tail_node_gates(a, bt, n, tail_depth(a, bt, n), q1, q2, g);
    }
    const float QI = __fadd_rn(__fmul_rn(q1, sp[1]), mn[1]), QO = __fadd_rn(__fmul_rn(q2, sp[2]), mn[2]);
    float prev = 0.f;
    if (p.any_pump) {
      prev = t == 0 ? a.h0[i] : __fadd_rn(de, __fdiv_rn(__fsub_rn(QI, QO), area));
      de = t_min(t_max(prev, hmin), hmax);
    }
    a.ws_qi[bt * p.N + n] = QI;
    a.ws_qo[bt * p.N + n] = QO;
    a.ws_prev[bt * p.N + n] = prev;
  }
  float carry = 0.f;      // gradient of de_t that the recurrence of step t + 1 sends back
  for (int t = a.T - 1; t >= 0; --t) {
    const int64_t bt = (int64_t)b * a.T + t;
    const int64_t bn = bt * p.N + n;
    const float QI = a.ws_qi[bn], QO = a.ws_qo[bn], prev = a.ws_prev[bn];
    const float hn = tail_depth(a, bt, n);
    const float *yr = a.y + bn * p.cy;
    float H = __fadd_rn(__fmul_rn(hn, sp[0]), mn[0]);
    if (p.any_pump) H = __fadd_rn(__fmul_rn(H, __fsub_rn(1.f, ps)), __fmul_rn(t_min(t_max(prev, hmin), hmax), ps));
    float F = 0.f;
    if (p.if_flood) {
      const int cf = p.cy - 1, co = p.edge_fusion ? cf + 2 : cf;
      F = __fadd_rn(__fmul_rn(yr[cf], sp[co]), mn[co]);
    }
    float hc, qw, f, m, s;
    tail_constrain(p, n, H, QI, QO, a.runoff[bn], F, hc, qw, f, m, s);
    const float *g = a.g_out_y + bn * (C + 1);
    const float gs = s >= 0.f ? g[C] * m * (1.f - p.is_outfall[n]) : 0.f;
    float gQI = g[1] + gs, gQO = g[2] - gs;
    const float gHp = g[0] * (1.f - f) * w_max(H, hmin) * w_min(t_max(H, hmin), hmax);
    float gH = gHp;
    if (p.any_pump) {
      gH = gHp * (1.f - ps);
      const float gprev = (gHp * ps + carry) * w_max(prev, hmin) * w_min(t_max(prev, hmin), hmax);
      if (t > 0) {
        carry = gprev;
        gQI += gprev / area;
        gQO -= gprev / area;
      } else {
        a.dh0[i] = gprev;
      }
    }
    float *dy = a.dy + bn * p.cy;
    dy[0] = gH * sp[0] * (p.tide ? 1.f - p.is_outfall[n] : 1.f);
    const float gp1 = gQI * sp[1], gp2 = gQO * sp[2];
    if (p.edge_fusion) {
      a.ws_qi[bn] = gp1 * p.scale_in[n];
      a.ws_qo[bn] = gp2 * p.scale_out[n];
      for (int c = 1; c < p.cy; ++c) dy[c] = g[c + 2] * sp[c + 2];
    } else {
      float q1, q2;
      NodeGates ng;
      tail_node_gates(a, bt, n, hn, q1, q2, ng);
      dy[1] = gp1 * ng.s_in * ng.z_in;
      dy[2] = gp2 * ng.s_out * ng.z_out;
      a.ws_qi[bn] = gp1 * ng.in_pre;       // gradient of the node's a_in / a_out setting
      a.ws_qo[bn] = gp2 * ng.out_pre;
      for (int c = 3; c < p.cy; ++c) dy[c] = g[c] * sp[c];
    }
  }
  if (!p.any_pump) a.dh0[i] = 0.f;
}

__global__ __launch_bounds__(256) void k_tail_link_bwd(TailArgs a) {
  const uds_tail_t &p = a.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.T * p.E) return;
  const int64_t bt = i / p.E;
  const int l = (int)(i - bt * p.E);
  float pre, dflow, set;
  const float flow = tail_link_flow(a, bt, l, pre, dflow, set);
  const float *er = a.ey + i * p.ce, *g = a.g_out_ey + i * p.ce;
  const float *sp = p.span_e + (int64_t)l * p.ce, *mn = p.mini_e + (int64_t)l * p.ce;
  float *d = a.dey + i * p.ce;
  const int cl = p.ce - 1;
  float gV = g[cl];
  if (p.edge_fusion) {
    const float v = __fadd_rn(__fmul_rn(flow, sp[cl]), mn[cl]);
    float pos = 0.f, neg = 0.f;      // what a positive / a negative flow feeds: q_out of the from-node + q_in of the to-node, and the reverse
    for (int j = 0; j < 2; ++j) {
      const int nd = p.link_node[2 * l + j];
      if (nd < 0) continue;
      const float gi = a.ws_qi[bt * p.N + nd], go = a.ws_qo[bt * p.N + nd];
      if (p.link_sign[2 * l + j] > 0.f) { pos += go; neg += gi; } else { pos += gi; neg += go; }
    }
    gV += v > 0.f ? pos : (v < 0.f ? -neg : 0.f);
  }
  const float gflow = gV * sp[cl];
  if (p.act) a.ws_set[i] = gflow * pre;
  d[cl] = gflow * set * dflow;
  const float e0 = __fadd_rn(__fmul_rn(er[0], sp[0]), mn[0]);
  d[0] = g[0] * w_min(t_clamp0(e0), p.ehmax[l]) * gate(e0 >= 0.f) * sp[0];
  for (int c = 1; c < cl; ++c) d[c] = g[c] * sp[c];
}

// da[b, t, k] = the setting gradients of the links action k drives, then of the nodes whose inflow, then whose outflow it gates
__global__ __launch_bounds__(256) void k_tail_da(TailArgs a) {
  const uds_tail_t &p = a.p;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.T * p.n_act) return;
  const int64_t bt = i / p.n_act;
  const int k = (int)(i - bt * p.n_act);
  float acc = 0.f;
  for (int q = p.al_ptr[k]; q < p.al_ptr[k + 1]; ++q) acc += a.ws_set[bt * p.E + p.al_idx[q]];
  if (!p.edge_fusion) {
    for (int q = p.ai_ptr[k]; q < p.ai_ptr[k + 1]; ++q) acc += a.ws_qi[bt * p.N + p.ai_idx[q]];
    for (int q = p.ao_ptr[k]; q < p.ao_ptr[k + 1]; ++q) acc += a.ws_qo[bt * p.N + p.ao_idx[q]];
  }
  a.da[i] = acc;
}

inline unsigned tail_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

inline hipError_t launch_tail_forward(const TailArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_tail_link, dim3(tail_grid((int64_t)a.B * a.T * a.p.E)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_tail_node, dim3(tail_grid((int64_t)a.B * a.p.N)), dim3(256), 0, st, a);
  return hipGetLastError();
}

inline hipError_t launch_tail_backward(const TailArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_tail_node_bwd, dim3(tail_grid((int64_t)a.B * a.p.N)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_tail_link_bwd, dim3(tail_grid((int64_t)a.B * a.T * a.p.E)), dim3(256), 0, st, a);
  if (a.p.act && a.da) hipLaunchKernelGGL(k_tail_da, dim3(tail_grid((int64_t)a.B * a.T * a.p.n_act)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace uds
