// GlobalAttnSumPool over two row blocks and its backward (the RL agents' graph encoder under training: agent.py:93-94 inside the
// GradientTape of the SAC / PPO / TD3 updates).  Per sample b the rows r = 0 .. Rx+Re-1 are the rows of x[b] followed by the rows
// of e[b] -- the stack torch.cat([x, e], -2) that is never built:
//     s_r = <row_r, k>,  M = max_r s_r,  L = sum_r exp(s_r - M),  alpha_r = exp(s_r - M) / L,  out = sum_r alpha_r row_r
// Thread layout of k_attn_sum_pool (kernels_sparse.hpp): one 256-thread workgroup per sample, thread (c, part) owns float4 chunk c
// of every row it visits, the F/4 lanes of a row are consecutive and aligned, a row's dot products are xor-shuffle reductions.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace uds {

// <a, b> of two float4 chunks with every product and sum rounded on its own, in source order: what k_attn_sum_pool's score compiles
// to.  The forward, the backward's recomputed score and both halves of t_r = <g, row_r> - <g, out> go through this one function,
// so a recomputed score equals the saved maximum bit for bit where it should (alpha = 1 exactly for a row that carries the whole
// weight) and t_r cancels exactly for a row equal to the output; a fused multiply-add in one of them would leave an ulp of the
// score, 1.5e-5 at |s| = 190, in alpha.
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

struct AttnPoolPairArgs {
  const float *x, *e, *k;
  float *out, *stat;   // stat (B, 2) = (M, L) or NULL
  int Rx, Re, F4;      // rows of x / of e per sample, float4 chunks per row (a power of two <= 64)
};

// The forward.  Row r of the stack is visited at the step, by the thread and with the operations of k_attn_sum_pool on the
// concatenated tensor -- only the address of the row differs -- so `out` carries the same bits.
__global__ __launch_bounds__(256) void k_attn_sum_pool_pair(AttnPoolPairArgs a) {
  __shared__ float s_m[256], s_l[256];
  __shared__ float4 s_acc[256];
  const int tid = threadIdx.x, c = tid % a.F4, part = tid / a.F4, n_part = 256 / a.F4, R = a.Rx + a.Re;
  const float4 *xb = reinterpret_cast<const float4 *>(a.x) + (int64_t)blockIdx.x * a.Rx * a.F4;
  const float4 *eb = reinterpret_cast<const float4 *>(a.e) + (int64_t)blockIdx.x * a.Re * a.F4;      // never read when Re = 0
  const float4 kc = reinterpret_cast<const float4 *>(a.k)[c];
  float m = -INFINITY, l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r0 = 0; r0 < R; r0 += n_part) {          // every thread of the workgroup runs the same number of steps (shuffles below)
    const int r = r0 + part;
    const bool live = r < R;
    const float4 v = live ? (r < a.Rx ? xb[(int64_t)r * a.F4 + c] : eb[(int64_t)(r - a.Rx) * a.F4 + c]) : make_float4(0.f, 0.f, 0.f, 0.f);
    float sc = dot4(v, kc);
    for (int o = a.F4 >> 1; o > 0; o >>= 1) sc += __shfl_xor(sc, o);
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
    if (a.stat && c == 0) {                             // the lanes of a row share its score: (m, l), hence (M, L), is the same for every c
      a.stat[(int64_t)blockIdx.x * 2] = M;
      a.stat[(int64_t)blockIdx.x * 2 + 1] = L;
    }
  }
}

// The backward.  With g = grad[b], t_r = <g, row_r> - <g, out[b]>:
//     ds_r = alpha_r t_r,  d row_r = alpha_r g + ds_r k,  dk_ws[b] = sum_r ds_r row_r
// alpha_r is recomputed from the row and the saved (M, L); one pass, every row read once and its gradient written once, two rows
// per thread in flight.  dx / de / dk_ws may each be NULL: rows whose gradient nobody wants are read only when dk_ws needs them.
struct AttnPoolBwdArgs {
  const float *x, *e, *k, *out, *stat, *grad;
  float *dx, *de, *dk_ws;
  int Rx, Re, F4;
};

__global__ __launch_bounds__(256) void k_attn_sum_pool_bwd(AttnPoolBwdArgs a) {
  __shared__ float4 s_dk[256];
  const int tid = threadIdx.x, c = tid % a.F4, part = tid / a.F4, n_part = 256 / a.F4, R = a.Rx + a.Re;
  const int64_t b = blockIdx.x;
  const float4 *xb = reinterpret_cast<const float4 *>(a.x) + b * a.Rx * a.F4;
  const float4 *eb = reinterpret_cast<const float4 *>(a.e) + b * a.Re * a.F4;
  float4 *dxb = a.dx ? reinterpret_cast<float4 *>(a.dx) + b * a.Rx * a.F4 : nullptr;
  float4 *deb = a.de ? reinterpret_cast<float4 *>(a.de) + b * a.Re * a.F4 : nullptr;
  const float4 kc = reinterpret_cast<const float4 *>(a.k)[c];
  const float4 gc = reinterpret_cast<const float4 *>(a.grad)[b * a.F4 + c];
  const float M = a.stat[b * 2], inv_l = 1.0f / a.stat[b * 2 + 1];
  float go = dot4(gc, reinterpret_cast<const float4 *>(a.out)[b * a.F4 + c]);
  for (int o = a.F4 >> 1; o > 0; o >>= 1) go += __shfl_xor(go, o);
  const bool want_dk = a.dk_ws != nullptr;
  float4 dk = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r0 = 0; r0 < R; r0 += 2 * n_part) {      // every thread runs the same number of steps (shuffles below)
    float4 v[2];
    float4 *dst[2];
    bool live[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = r0 + u * n_part + part;
      const bool in_x = r < a.Rx;
      dst[u] = r < R ? (in_x ? (dxb ? dxb + (int64_t)r * a.F4 + c : nullptr) : (deb ? deb + (int64_t)(r - a.Rx) * a.F4 + c : nullptr)) : nullptr;
      live[u] = r < R && (want_dk || dst[u]);
      v[u] = live[u] ? (in_x ? xb[(int64_t)r * a.F4 + c] : eb[(int64_t)(r - a.Rx) * a.F4 + c]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float sc = dot4(v[u], kc), gv = dot4(gc, v[u]);
      for (int o = a.F4 >> 1; o > 0; o >>= 1) {
        sc += __shfl_xor(sc, o);
        gv += __shfl_xor(gv, o);
      }
      if (live[u]) {
        const float alpha = __expf(sc - M) * inv_l, ds = alpha * (gv - go);
        if (dst[u]) *dst[u] = make_float4(alpha * gc.x + ds * kc.x, alpha * gc.y + ds * kc.y, alpha * gc.z + ds * kc.z, alpha * gc.w + ds * kc.w);
        dk.x += ds * v[u].x; dk.y += ds * v[u].y; dk.z += ds * v[u].z; dk.w += ds * v[u].w;
      }
    }
  }
  if (!want_dk) return;                               // uniform over the workgroup
  s_dk[tid] = dk;
  __syncthreads();
  if (part == 0) {                                    // chunk c: the n_part partial sums in a fixed order
    float4 A = s_dk[c];
    for (int p = 1; p < n_part; ++p) {
      const float4 q = s_dk[p * a.F4 + c];
      A.x += q.x; A.y += q.y; A.z += q.z; A.w += q.w;
    }
    reinterpret_cast<float4 *>(a.dk_ws)[b * a.F4 + c] = A;
  }
}

// dk[f] = sum_b dk_ws[b, f] in a fixed order (no float atomics): workgroup j owns cw = min(F/4, 16) float4 chunks, thread
// (chunk, bp) sums the samples b = bp, bp + 256 / cw, .. in ascending order, then a tree over bp through LDS.
struct AttnPoolDkArgs {
  const float *dk_ws;
  float *dk;
  int B, F4, cw;
};

__global__ __launch_bounds__(256) void k_attn_sum_pool_dk(AttnPoolDkArgs a) {
  __shared__ float4 s[256];
  const int tid = threadIdx.x, c = blockIdx.x * a.cw + tid % a.cw, bp = tid / a.cw, n_bp = 256 / a.cw;
  const float4 *ws = reinterpret_cast<const float4 *>(a.dk_ws) + c;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = bp; b < a.B; b += n_bp) {
    const float4 q = ws[(int64_t)b * a.F4];
    acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
  }
  s[tid] = acc;
  __syncthreads();
  for (int o = n_bp >> 1; o > 0; o >>= 1) {
    if (bp < o) {
      const float4 q = s[tid + o * a.cw];
      acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
      s[tid] = acc;
    }
    __syncthreads();
  }
  if (bp == 0) reinterpret_cast<float4 *>(a.dk)[c] = acc;
}

}  // namespace uds
