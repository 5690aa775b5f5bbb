// Optimizer kernels: keras.optimizers.Adam(learning_rate, clipnorm) as TF 2.10 applies it (emulator.py:111 of the reference),
// every gradient clipped by ITS OWN norm (tf.clip_by_norm), for a whole list of tensors in two passes (uds_adam_step).
//
//   pass 1  k_adam_sumsq    one workgroup = one span of ADAM_SPAN elements of one tensor: sum of g^2 in double -> one partial
//   pass 2  k_adam_update   the same workgroups: add the tensor's partials in a fixed order, n = sqrt(sum),
//                           g *= clipnorm / max(n, clipnorm), m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
//                           p -= lr_t m / (sqrt(v) + eps) with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), t = state[0] + 1
//   then    k_adam_commit   one thread: status word, t += 1 unless the step was refused
//
// The (p, g, m, v, numel) tables travel BY VALUE in the kernel arguments (AdamTable, ADAM_TABLE tensors per launch, under the
// 4 KiB kernarg segment), so a captured graph keeps them in its kernel nodes and nothing on the host is read at replay.
// No atomics: partials have one writer each and are added in index order, so two calls on the same inputs give the same bits.
// state (int32[4], device): [0] t, [1] status of the LAST call (bit 0: loss not finite, bit 1: a gradient not finite),
// [2] scratch flag raised by pass 1 (plain stores of the same value), [3] unused.  With either status bit set pass 2 and the
// commit change none of p, m, v, t.  Sums of squares are kept in double: a finite fp32 gradient cannot overflow them, so
// "norm not finite" is exactly "some gradient element is NaN or Inf".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uds {

constexpr int ADAM_TABLE = 64;        // tensors per launch: 5 * 8 * 64 + 4 * 65 + 4 bytes of table, under the 4 KiB kernarg segment
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_SPAN = 4096;       // elements per workgroup (a multiple of 4: a span of an aligned tensor starts aligned)

struct AdamTable {
  float *p[ADAM_TABLE];
  const float *g[ADAM_TABLE];
  float *m[ADAM_TABLE];
  float *v[ADAM_TABLE];
  int64_t numel[ADAM_TABLE];
  int32_t block0[ADAM_TABLE + 1];     // first workgroup of tensor i in this launch; block0[n] = the grid
  int32_t n;
};

struct AdamHyper {
  double lr, b1, b2;
  float b1f, one_minus_b1, b2f, one_minus_b2, eps, clipnorm;     // clipnorm <= 0: no clipping
};

// the tensor whose span workgroup `b` covers: the last i with block0[i] <= b (block0 is increasing, every tensor has a block)
__device__ __forceinline__ int adam_tensor_of(const AdamTable &t, int b) {
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.block0[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum over the workgroup in a fixed order (lanes by halving, then the four waves in order), returned to every thread
__device__ __forceinline__ double adam_block_sum(double x, double *lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                   // lds may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) lds[wave] = x;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__device__ __forceinline__ bool adam_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(ADAM_THREADS) void k_adam_sumsq(AdamTable t, double *partial, int32_t *state) {
  __shared__ double lds[4];
  const int i = adam_tensor_of(t, (int)blockIdx.x);
  const int64_t start = (int64_t)((int)blockIdx.x - t.block0[i]) * ADAM_SPAN;
  const int64_t left = t.numel[i] - start;
  const int cnt = left < ADAM_SPAN ? (int)left : ADAM_SPAN;
  const float *g = t.g[i] + start;
  double acc = 0.0;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int n4 = cnt >> 2;
    for (int q = threadIdx.x; q < n4; q += ADAM_THREADS) {
      const float4 x = reinterpret_cast<const float4 *>(g)[q];
      acc += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
    }
    done = n4 << 2;
  }
  for (int j = done + threadIdx.x; j < cnt; j += ADAM_THREADS) acc += (double)g[j] * g[j];
  const double s = adam_block_sum(acc, lds);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s;
    if (!(s <= 1.7976931348623157e308)) state[2] = 1;          // NaN or Inf: a gradient element is
  }
}

__device__ __forceinline__ double adam_ipow(double b, int t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, float scale, float neg_lr_t, const AdamHyper &h) {
  g *= scale;
  m = m * h.b1f + h.one_minus_b1 * g;
  v = v * h.b2f + h.one_minus_b2 * (g * g);
  p = p + neg_lr_t * (m / (sqrtf(v) + h.eps));
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam_update(AdamTable t, const double *partial, const float *loss, const int32_t *state,
                                                              AdamHyper h) {
  __shared__ double lds[4];
  if (state[2] != 0 || (loss != nullptr && !adam_finite(*loss))) return;       // uniform: the whole grid leaves
  const int i = adam_tensor_of(t, (int)blockIdx.x);
  const int b0 = t.block0[i], nb = t.block0[i + 1] - b0;
  double acc = 0.0;
  for (int j = threadIdx.x; j < nb; j += ADAM_THREADS) acc += partial[b0 + j];
  const double norm = sqrt(adam_block_sum(acc, lds));
  float scale = 1.0f;
  if (h.clipnorm > 0.f) {
    const float nf = (float)norm;                    // tf.clip_by_norm: clip / max(norm, clip) in the tensor's precision
    scale = h.clipnorm / (nf > h.clipnorm ? nf : h.clipnorm);
  }
  const int step = state[0] + 1;
  const float neg_lr_t = -(float)(h.lr * sqrt(1.0 - adam_ipow(h.b2, step)) / (1.0 - adam_ipow(h.b1, step)));
  const int64_t start = (int64_t)((int)blockIdx.x - b0) * ADAM_SPAN;
  const int64_t left = t.numel[i] - start;
  const int cnt = left < ADAM_SPAN ? (int)left : ADAM_SPAN;
  float *p = t.p[i] + start, *m = t.m[i] + start, *v = t.v[i] + start;
  const float *g = t.g[i] + start;
  int done = 0;
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0) {
    const int n4 = cnt >> 2;
    for (int q = threadIdx.x; q < n4; q += ADAM_THREADS) {
      float4 P = reinterpret_cast<float4 *>(p)[q], M = reinterpret_cast<float4 *>(m)[q], V = reinterpret_cast<float4 *>(v)[q];
      const float4 G = reinterpret_cast<const float4 *>(g)[q];
      adam_one(P.x, G.x, M.x, V.x, scale, neg_lr_t, h);
      adam_one(P.y, G.y, M.y, V.y, scale, neg_lr_t, h);
      adam_one(P.z, G.z, M.z, V.z, scale, neg_lr_t, h);
      adam_one(P.w, G.w, M.w, V.w, scale, neg_lr_t, h);
      reinterpret_cast<float4 *>(p)[q] = P;
      reinterpret_cast<float4 *>(m)[q] = M;
      reinterpret_cast<float4 *>(v)[q] = V;
    }
    done = n4 << 2;
  }
  for (int j = done + threadIdx.x; j < cnt; j += ADAM_THREADS) {
    float P = p[j], M = m[j], V = v[j];
    adam_one(P, g[j], M, V, scale, neg_lr_t, h);
    p[j] = P;
    m[j] = M;
    v[j] = V;
  }
}

// after the last pass 2: the status word of this call, the step count, and the scratch flag cleared for the next call
__global__ void k_adam_commit(const float *loss, int32_t *state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int bad = ((loss != nullptr && !adam_finite(*loss)) ? 1 : 0) | (state[2] != 0 ? 2 : 0);
  state[1] = bad;
  if (!bad) state[0] = state[0] + 1;
  state[2] = 0;
}

}  // namespace uds
