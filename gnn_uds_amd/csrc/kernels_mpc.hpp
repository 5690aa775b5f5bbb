// Model-predictive control on the device (gnn_uds_amd/mpc.py: `Problem`): the scenario objective of a population of predicted
// horizons with its reverse mode, and the two steps of a cross-entropy iteration.
//
//   k_mpc_objective           obj[p] = sum_t gamma_t sum_n (w_flood[n] q_w + w_out[n] q_in[t] + w_smooth[n] |q_in[t] - q_in[t-1]|)
//   k_mpc_objective_backward  ALL of d_preds (pop, T, N, C): zero in every channel no weight reaches
//   k_ce_draw                 pop candidates from N(mean, std) clipped to [0, 1]: Philox4x32-10 counter (count + i, v), Box-Muller;
//                             then k_window_bump (kernels_data.hpp): count += pop in a launch of its own
//   k_ce_update               rank the candidates, mean / std of the elites, one variable per workgroup; reads best_obj
//   k_ce_commit               one workgroup after it on the same stream: best_obj and status (nothing reads them before)
//
// preds (pop, T, N, C): q_w is channel C - 1, q_in channel 1; q_in[-1] = q_in0[p * q0_stride + n].  A term whose weight is 0 (or
// whose vector is NULL) is not formed: its channel is not read, as the index lists of `mpc.objective_pred` never touch it.
//
// Order of k_mpc_objective, the same in every call (no atomics, a second call gives the same bits): one workgroup of 256 threads
// per candidate; thread i takes the nodes i, i + 256, ... and walks the T steps of each, so q_in[t-1] stays in a register; the
// thread's terms are added in that order, then the 64 lanes by halving (6 levels), then the four waves as (0 + 1) + (2 + 3).
// Every product, term and partial sum is fp64 -- a product of two fp32 numbers is exact there -- and the result is rounded to
// fp32 once.  Roundings on the longest path: 1 of 2^-24 (the result, in fact half of it) and 3 + ceil(N / 256) * T + 8 of 2^-53;
// with T * N <= 2^36 (the entry's limit) the fp64 part stays below 2^-25 * sum|term|, so against the exact sum
//        |obj - exact| <= D * 2^-24 * sum|term|   with D = 2.
// k_mpc_objective_backward forms every element in fp64 too and rounds it once: within 2^-24 of the sum of its contributions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_data.hpp"        // k_window_bump; philox4x32_10 through kernels_sparse.hpp

namespace uds {

constexpr int MPC_THREADS = 256;
constexpr int CE_MAX = 1024;       // candidates and variables of a cross-entropy call

struct MpcObjectiveArgs {
  const float *preds, *q_in0, *g;                       // g (pop): backward only
  const float *w_flood, *w_out, *w_smooth, *gamma;      // (N) each or NULL; gamma (T) or NULL
  float *obj, *d_preds;
  int64_t q0_stride;
  int64_t pop;
  int T, N, C;
};

// sum over the workgroup in a fixed order (lanes by halving, then the four waves), returned to every thread
__device__ __forceinline__ double mpc_block_sum(double x, double *lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(MPC_THREADS) void k_mpc_objective(MpcObjectiveArgs a) {
  __shared__ double lds[4];
  const int64_t p = blockIdx.x;
  const int64_t step = (int64_t)a.N * a.C;                            // floats between two time steps of one node
  const float *pr = a.preds + p * a.T * step;
  const float *q0 = a.q_in0 + p * a.q0_stride;
  double acc = 0.0;
  for (int n = threadIdx.x; n < a.N; n += MPC_THREADS) {
    const float wf = a.w_flood ? a.w_flood[n] : 0.f, wo = a.w_out ? a.w_out[n] : 0.f, ws = a.w_smooth ? a.w_smooth[n] : 0.f;
    if (wf == 0.f && wo == 0.f && ws == 0.f) continue;
    const bool inflow = wo != 0.f || ws != 0.f;
    const float *row = pr + (int64_t)n * a.C;
    double prev = ws != 0.f ? (double)q0[n] : 0.0;
    for (int t = 0; t < a.T; ++t, row += step) {
      double term = 0.0;
      if (wf != 0.f) term = (double)wf * (double)row[a.C - 1];
      if (inflow) {
        const double q = (double)row[1];
        if (wo != 0.f) term += (double)wo * q;
        if (ws != 0.f) term += (double)ws * fabs(q - prev);
        prev = q;
      }
      acc += a.gamma ? (double)a.gamma[t] * term : term;
    }
  }
  const double s = mpc_block_sum(acc, lds);
  if (threadIdx.x == 0) a.obj[p] = (float)s;
}

// sign of q[t] - q[t-1] as torch.abs differentiates it: 0 at 0, NaN stays NaN
__device__ __forceinline__ double mpc_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d); }

// one thread per (candidate, step, node): its C channels, every one written
__global__ __launch_bounds__(MPC_THREADS) void k_mpc_objective_backward(MpcObjectiveArgs a) {
  const int64_t i = (int64_t)blockIdx.x * MPC_THREADS + threadIdx.x;
  if (i >= a.pop * a.T * a.N) return;
  const int64_t pt = i / a.N;
  const int n = (int)(i - pt * a.N);
  const int64_t p = pt / a.T;
  const int t = (int)(pt - p * a.T);
  const int64_t step = (int64_t)a.N * a.C;
  const float *row = a.preds + i * a.C;
  const double g = (double)a.g[p];
  const double gt = a.gamma ? (double)a.gamma[t] : 1.0;
  const float wf = a.w_flood ? a.w_flood[n] : 0.f, wo = a.w_out ? a.w_out[n] : 0.f, ws = a.w_smooth ? a.w_smooth[n] : 0.f;
  const double d_w = wf != 0.f ? g * gt * (double)wf : 0.0;
  double d_q = wo != 0.f ? g * gt * (double)wo : 0.0;
  if (ws != 0.f) {
    const double q = (double)row[1];
    const double prev = t ? (double)row[1 - step] : (double)a.q_in0[p * a.q0_stride + n];
    d_q += g * gt * (double)ws * mpc_sign(q - prev);
    if (t + 1 < a.T) {
      const double gn = a.gamma ? (double)a.gamma[t + 1] : 1.0;
      d_q -= g * gn * (double)ws * mpc_sign((double)row[1 + step] - q);
    }
  }
  float *out = a.d_preds + i * a.C;
  for (int c = 0; c < a.C; ++c) {
    double v = 0.0;
    if (c == 1) v += d_q;
    if (c == a.C - 1) v += d_w;
    out[c] = (float)v;
  }
}

// ---- cross-entropy method ---------------------------------------------------------------------------------------------------
struct CeDrawArgs {
  const float *mean, *std;                // (n_var)
  const unsigned long long *count;        // candidates drawn so far
  float *out;                             // (pop, n_var)
  unsigned long long seed;
  int n_var, pop;
};

// one thread per (candidate, variable).  k = word >> 8 is a 24-bit integer; k + 0.5 is formed in fp32 (exact below 2^23, rounded
// to even above: 25 bits) and scaled by 2^-24 (exact), so u lies in (0, 1] and the logarithm is finite (u1 = 1 gives z = 0).  A
// restatement that rounds k + 0.5 to fp32 the same way holds the same u.  Precise logf / cosf / sqrtf.
__global__ __launch_bounds__(MPC_THREADS) void k_ce_draw(CeDrawArgs a) {
  const int idx = blockIdx.x * MPC_THREADS + threadIdx.x;
  if (idx >= a.pop * a.n_var) return;
  const int i = idx / a.n_var, v = idx - i * a.n_var;
  unsigned r[4];
  philox4x32_10(*a.count + (unsigned long long)i, (unsigned long long)v, a.seed, r);
  const float u1 = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;      // 2^-24
  const float u2 = ((float)(r[1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
  const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
  a.out[idx] = fminf(fmaxf(a.mean[v] + a.std[v] * z, 0.0f), 1.0f);
}

struct CeUpdateArgs {
  const float *y, *obj;                   // (pop, n_var), (pop)
  float *mean, *std, *best_y, *best_obj;  // (n_var) x 3, one float
  int32_t *status;
  float smooth, std_min;
  int pop, n_var, n_elite;
};

constexpr unsigned CE_KEY_TOP = 0xFFFFFFFFu;

// order-preserving integer image of an objective: NaN / +-Inf -> the top (as +inf), -0 = +0
__device__ __forceinline__ unsigned ce_key(float x) {
  unsigned b = __float_as_uint(x);
  if ((b & 0x7F800000u) == 0x7F800000u) return CE_KEY_TOP;
  if ((b & 0x7FFFFFFFu) == 0) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// sum of the workgroup's values as a balanced tree (lanes by xor butterfly: 6 levels, the four waves as (0 + 1) + (2 + 3)),
// returned to every thread; a + b = b + a, so every lane holds the same bits
__device__ __forceinline__ float ce_tree_sum(float x, float *lds) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// Workgroup v handles variable v; every workgroup ranks the candidates itself (pop^2 integer comparisons on keys in the LDS).
// rank[p] = #{q: key[q] < key[p] or (key[q] == key[p] and q < p)}; sel[r] = the candidate of rank r < n_elite when it is finite,
// so the K elites are sel[0 .. K - 1].  Mean and standard deviation (two passes, ddof 0) are trees over 1024 leaves in rank order,
// leaves past K zero: thread i adds (x[4i] + x[4i+1]) + (x[4i+2] + x[4i+3]), then ce_tree_sum -- 10 levels whatever K is.
__global__ __launch_bounds__(MPC_THREADS) void k_ce_update(CeUpdateArgs a) {
  __shared__ unsigned key[CE_MAX];
  __shared__ int sel[CE_MAX + 1];
  __shared__ float lds[4];
  __shared__ int k_sh;
  const int v = blockIdx.x;
  for (int p = threadIdx.x; p < a.pop; p += MPC_THREADS) key[p] = ce_key(a.obj[p]);
  for (int r = threadIdx.x; r <= CE_MAX; r += MPC_THREADS) sel[r] = -1;
  if (threadIdx.x == 0) k_sh = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < a.pop; p += MPC_THREADS) {
    const unsigned kp = key[p];
    int rank = 0;
    for (int q = 0; q < a.pop; ++q) rank += (key[q] < kp || (key[q] == kp && q < p)) ? 1 : 0;
    if (rank < a.n_elite && kp != CE_KEY_TOP) sel[rank] = p;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < a.n_elite; r += MPC_THREADS)
    if (sel[r] >= 0 && (r + 1 == a.n_elite || sel[r + 1] < 0)) k_sh = r + 1;      // finite candidates hold ranks 0 .. K - 1: one writer
  __syncthreads();
  const int K = k_sh;
  if (K == 0) return;                      // no finite candidate: nothing changes (k_ce_commit raises status)
  float x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 4 * threadIdx.x + j;
    x[j] = r < K ? a.y[(int64_t)sel[r] * a.n_var + v] : 0.f;
  }
  const float m = ce_tree_sum((x[0] + x[1]) + (x[2] + x[3]), lds) / (float)K;
  float d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float dj = x[j] - m;
    d[j] = 4 * threadIdx.x + j < K ? dj * dj : 0.f;
  }
  const float s = sqrtf(ce_tree_sum((d[0] + d[1]) + (d[2] + d[3]), lds) / (float)K);
  if (threadIdx.x == 0) {
    const float keep = a.smooth, take = 1.0f - a.smooth;
    a.mean[v] = keep * a.mean[v] + take * m;
    a.std[v] = fmaxf(keep * a.std[v] + take * s, a.std_min);
    if (a.obj[sel[0]] < *a.best_obj) a.best_y[v] = a.y[(int64_t)sel[0] * a.n_var + v];
  }
}

// the rank-0 candidate again (the smallest key, the lower index on a tie: an integer minimum, whatever the order), then the two
// words every workgroup of k_ce_update only read
__global__ __launch_bounds__(MPC_THREADS) void k_ce_commit(CeUpdateArgs a) {
  __shared__ unsigned long long lds[4];
  unsigned long long best = ~0ull;
  for (int p = threadIdx.x; p < a.pop; p += MPC_THREADS) {
    const unsigned long long c = ((unsigned long long)ce_key(a.obj[p]) << 32) | (unsigned)p;
    best = c < best ? c : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off, 64);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) best = lds[w] < best ? lds[w] : best;
    if ((unsigned)(best >> 32) == CE_KEY_TOP) {
      a.status[0] = 1;
    } else {
      const float o = a.obj[(unsigned)best];
      if (o < *a.best_obj) *a.best_obj = o;
    }
  }
}

}  // namespace uds
