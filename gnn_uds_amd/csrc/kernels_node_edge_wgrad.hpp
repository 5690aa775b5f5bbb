// Parameter gradient of a dense-parameter NodeEdge on the matrix cores (gfx950): for out[s] = (weight o inci + bias) @ x[s],
//     d_bias[r, m] = sum_s sum_k g[s, r, k] x[s, m, k],   d_weight = d_bias o inci,
// g (S, R, h) the upstream gradient, x (S, M, h) the layer's input, both read where they lie: inside a row of a snapshot the h
// values are contiguous, and that is the K-contiguous layout the MFMA operands want (lane (row, q) holds k = 8q .. 8q + 7 of
// its row: two 16-byte loads).  No permuted copy, no transposed copy, no library.
//
// The output is cut into 64 x 64 tiles, the snapshots into `pieces` runs of `spp` snapshots: one 4-wave workgroup per (tile,
// piece).  Wave w of a workgroup takes the snapshots w, w + 4, .. of the piece and keeps the WHOLE tile in accumulators (4 x 4
// MFMA tiles of 16 x 16, K = 32 per step: KS = 1 step per snapshot for h <= 32, 2 for h <= 64; an h that is no multiple of 32
// reads zeros for the k past it, decided per 16-byte load).  Operands are split into bf16 hi + lo, three products, fp32
// accumulation: the numerics of k_wgrad_mfma and of the forward GEMM.  16-row blocks past R or M are skipped, loads and MFMAs
// (wave-uniform: a 30 x 29 network does 4 of the 16 tile products).  The waves add their accumulators in LDS in wave order,
// the workgroup stores its (R, M) part of the partial -- every element of partial (pieces, R, M) is written by exactly one
// workgroup -- and k_node_edge_wgrad_reduce sums the pieces in a fixed order and writes d_bias and d_weight.  No atomics: the
// same inputs give the same bits.
//
// Every address is clamped into its tensor BEFORE the load is predicated (row past R -> row 0, k past h -> 0), so a load that
// the compiler hoists above its predicate still reads inside the tensor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels_fused.hpp"

namespace uds {

constexpr int NEW_TILE = 64;             // output tile edge: 4 MFMA tiles of 16
constexpr int NEW_WAVES = 4;
constexpr int NEW_MIN_SPP = 8;           // least snapshots per piece: two per wave
constexpr int NEW_TARGET_WG = 512;       // workgroups wanted in flight: two 4-wave workgroups per CU

struct NodeEdgeWgradPlan {
  int ks;                    // the instantiation k_node_edge_wgrad<KS>: k-steps of 32 per snapshot, 1 or 2; 0 = refused
  int pieces, spp;           // pieces of the reduction over S, snapshots per piece (the last piece may be shorter)
  int padded;                // h is no multiple of 32: the k past h are zeros on chip
  int64_t tiles_r, tiles_m;
};

// The shapes the entry takes: h % 4 == 0, 4 <= h <= 64, R, M >= 1, 0 <= S <= 2^24, at most 2^20 tiles.  The piece count is a
// function of (R, M, S, h) alone: enough pieces that tiles * pieces reaches NEW_TARGET_WG, no piece under NEW_MIN_SPP snapshots.
inline NodeEdgeWgradPlan node_edge_wgrad_plan(int64_t R, int64_t M, int64_t S, int64_t h) {
  NodeEdgeWgradPlan p{};
  if (h < 4 || h > 64 || h % 4 || R < 1 || M < 1 || S < 0 || S > ((int64_t)1 << 24) || R > ((int64_t)1 << 24) || M > ((int64_t)1 << 24)) return p;
  p.tiles_r = (R + NEW_TILE - 1) / NEW_TILE;
  p.tiles_m = (M + NEW_TILE - 1) / NEW_TILE;
  const int64_t tiles = p.tiles_r * p.tiles_m;
  if (tiles > ((int64_t)1 << 20)) return p;
  p.ks = h <= 32 ? 1 : 2;
  p.padded = h % 32 != 0;
  const int64_t want = std::max<int64_t>(1, NEW_TARGET_WG / tiles);
  p.spp = (int)std::max<int64_t>(NEW_MIN_SPP, (S + want - 1) / want);
  p.pieces = (int)((S + p.spp - 1) / p.spp);      // 0 at S = 0: nothing is launched
  return p;
}

struct NodeEdgeWgradArgs {
  const float *g, *x;        // (S, R, h), (S, M, h)
  float *partial;            // (pieces, R, M)
  int64_t S;
  int R, M, h;
  int spp, tiles_m;
};

// 16-byte load number `half` (0, 1) of this lane's 8 k values of row `row_off` (floats from the snapshot's start, clamped by the
// caller), zeros where `ok` is false; koff is clamped to 0 where the k are past h
__device__ __forceinline__ float4 new_load4(const float *snap, int64_t row_off, int koff, bool ok) {
  const float4 v = *reinterpret_cast<const float4 *>(snap + row_off + koff);
  return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int KS>
__global__ __launch_bounds__(NEW_WAVES * 64) void k_node_edge_wgrad(NodeEdgeWgradArgs a) {
  __shared__ float red[NEW_TILE * NEW_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, qd = lane >> 4;
  const int r0 = (int)(blockIdx.x / a.tiles_m) * NEW_TILE, m0 = (int)(blockIdx.x % a.tiles_m) * NEW_TILE;
  const int64_t s_begin = (int64_t)blockIdx.y * a.spp, s_end = min(a.S, s_begin + a.spp);
  // how many 16-row blocks of the tile hold rows of g / x at all (wave-uniform)
  const int nb_r = min(4, (a.R - r0 + 15) / 16), nb_m = min(4, (a.M - m0 + 15) / 16);

  int64_t goff[4], xoff[4];      // this lane's row in each 16-row block: floats from the snapshot's start, clamped to row 0
  bool gv[4], xv[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = r0 + 16 * t + r16, m = m0 + 16 * t + r16;
    gv[t] = r < a.R;
    xv[t] = m < a.M;
    goff[t] = (int64_t)(gv[t] ? r : 0) * a.h;
    xoff[t] = (int64_t)(xv[t] ? m : 0) * a.h;
  }
  int koff[KS][2];               // the two 16-byte loads of a k-step: k = 32 ks + 8 qd + 4 half, clamped to 0 past h
  bool kv[KS][2];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int k = 32 * ks + 8 * qd + 4 * hf;
      kv[ks][hf] = k + 4 <= a.h;
      koff[ks][hf] = kv[ks][hf] ? k : 0;
    }

  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t g_snap = (int64_t)a.R * a.h, x_snap = (int64_t)a.M * a.h;
  for (int64_t s = s_begin + wave; s < s_end; s += NEW_WAVES) {
    const float *gs = a.g + s * g_snap, *xs = a.x + s * x_snap;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 xh[4], xl[4];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (n < nb_m)
          split8(new_load4(xs, xoff[n], koff[ks][0], xv[n] && kv[ks][0]), new_load4(xs, xoff[n], koff[ks][1], xv[n] && kv[ks][1]), xh[n], xl[n]);
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (m < nb_r) {
          bf16x8 gh, gl;
          split8(new_load4(gs, goff[m], koff[ks][0], gv[m] && kv[ks][0]), new_load4(gs, goff[m], koff[ks][1], gv[m] && kv[ks][1]), gh, gl);
#pragma unroll
          for (int n = 0; n < 4; ++n)
            if (n < nb_m) acc[m][n] = mfma3(gh, gl, xh[n], xl[n], acc[m][n]);
        }
    }
  }

  // the waves add their accumulators into the zeroed LDS tile in wave order (fixed summation order): acc[m][n][j] =
  // tile[16 m + 4 qd + j][16 n + r16].  One code path for every wave (0 + acc is exact).
  for (int i = tid; i < NEW_TILE * NEW_TILE; i += NEW_WAVES * 64) red[i] = 0.f;
  __syncthreads();
  for (int w = 0; w < NEW_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) red[(16 * m + 4 * qd + j) * NEW_TILE + 16 * n + r16] += acc[m][n][j];
    }
    __syncthreads();
  }
  float *part = a.partial + (int64_t)blockIdx.y * a.R * a.M;
  for (int i = tid; i < NEW_TILE * NEW_TILE; i += NEW_WAVES * 64) {
    const int r = r0 + i / NEW_TILE, m = m0 + i % NEW_TILE;
    if (r < a.R && m < a.M) part[(int64_t)r * a.M + m] = red[i];
  }
}

// d_bias[i] = sum_p partial[p, i] over the n_out = R * M outputs, d_weight[i] = d_bias[i] * inci[i] where d_weight is given.  As
// k_wgrad_reduce: a block sums 16 outputs, 16 lanes per output take every 16th piece (independent loads in flight), then the 16
// lane sums are added in lane order -- a fixed order.
__global__ __launch_bounds__(256) void k_node_edge_wgrad_reduce(const float *partial, int n_part, int64_t n_out, const float *inci, float *d_bias,
                                                                float *d_weight) {
  __shared__ float red[256];
  const int tid = threadIdx.x, o = tid & 15, bl = tid >> 4;
  const int64_t i = (int64_t)blockIdx.x * 16 + o;
  const bool ok = i < n_out;
  const float *p = partial + (ok ? i : 0);
  float s = 0.f;
#pragma unroll 8
  for (int b = bl; b < n_part; b += 16) s += p[b * n_out];
  red[tid] = s;
  __syncthreads();
  if (tid < 16 && ok) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k * 16 + tid];
    d_bias[i] = t;
    if (d_weight) d_weight[i] = t * inci[i];
  }
}

inline hipError_t launch_node_edge_wgrad(const NodeEdgeWgradArgs &a, const NodeEdgeWgradPlan &p, hipStream_t st) {
  const dim3 grid((unsigned)(p.tiles_r * p.tiles_m), (unsigned)p.pieces);
  if (p.ks == 1)
    hipLaunchKernelGGL(k_node_edge_wgrad<1>, grid, dim3(NEW_WAVES * 64), 0, st, a);
  else if (p.ks == 2)
    hipLaunchKernelGGL(k_node_edge_wgrad<2>, grid, dim3(NEW_WAVES * 64), 0, st, a);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace uds
