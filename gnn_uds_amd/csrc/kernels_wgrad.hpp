// Weight gradient of a row GEMM on the matrix cores (gfx950): dW[f, n] = sum_r A[r, f] * G[r, n] over ALL rows r
// (rows = S * N is 1e5..1e7, f <= 128, n <= 64) -- the `X^T dZ` products of the training step (emulator.py:457-484
// via GradientTape), plus the bias gradient (column sums of G) as one extra output row.  A library GEMM handles this
// tall-skinny reduction poorly (no split over the reduction dimension: ~480 us per call at 250k rows where the HBM
// floor is ~30 us), hence this kernel.
//
// HBM-bound: every wave streams its own contiguous range of rows once, 32 rows (one MFMA k-step) at a time, and keeps
// the whole (MT*16) x (NT*16) partial in accumulators.  Operand fragments are read straight from HBM in the transposed
// shape MFMA wants (lane (m, q) holds A[32 k0 + 8q + j][f0 + m], j = 0..7: sixteen lanes read 64 contiguous bytes of a
// row), split into bf16 hi + lo (three products, fp32 accumulate: the numerics of the forward kernels).  The waves of
// a workgroup add their partials in LDS in a fixed order, the workgroup writes ONE partial, and k_wgrad_reduce sums
// the workgroups' partials in index order: no atomics, bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_fused.hpp"

namespace uds {

struct WgradArgs {
  const float *a, *g;        // A (rows, F) possibly time-shifted, G (rows, H)
  float *partial;            // (grid, MT*16, NT*16)
  int64_t rows;
  int F, H, ones_row;        // ones_row = F when the bias gradient is wanted (A[., F] := 1), else -1
  int shift, T, t_rows;      // causal tap: A row of r is r - shift * t_rows, zero where the time index of r is < shift
  int rows_per_wave;         // multiple of 32
};

template <int MT, int NT>
__global__ __launch_bounds__(256, 2) void k_wgrad_mfma(WgradArgs a) {
  __shared__ float red[MT * 16 * NT * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t r_begin = ((int64_t)blockIdx.x * 4 + wave) * a.rows_per_wave;
  const int64_t r_end = min(a.rows, r_begin + a.rows_per_wave);

  for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
    // this lane's 8 rows of the k-step, their validity and (for a causal tap) the shifted source row
    int64_t ra[8], rg[8];
    bool va[8], vg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t r = r0 + 8 * qd + j;
      vg[j] = r < r_end;
      rg[j] = vg[j] ? r : r_begin;
      va[j] = vg[j];
      ra[j] = rg[j];
      if (a.shift) {
        const int t = (int)((rg[j] / a.t_rows) % a.T);
        va[j] = vg[j] && t >= a.shift;
        ra[j] = va[j] ? rg[j] - (int64_t)a.shift * a.t_rows : r_begin;
      }
    }
    bf16x8 gh[NT], gl[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int c = 16 * n + r16;
      const bool cv = c < a.H;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (cv && vg[j]) ? a.g[rg[j] * a.H + c] : 0.f;
      split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), gh[n], gl[n]);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int f = 16 * m + r16;
      float v[8];
      if (f < a.F) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = va[j] ? a.a[ra[j] * a.F + f] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (f == a.ones_row && vg[j]) ? 1.f : 0.f;
      }
      bf16x8 ah, al;
      split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), ah, al);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = mfma3(ah, al, gh[n], gl[n], acc[m][n]);
    }
  }

  // waves add their partials in wave order (fixed summation order), then the workgroup stores one partial
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float *p = red + (16 * m + 4 * qd + j) * (NT * 16) + 16 * n + r16;     // acc[m][n][j] = dW[16m + 4qd + j][16n + r16]
            *p = w == 0 ? acc[m][n][j] : *p + acc[m][n][j];
          }
    }
    __syncthreads();
  }
  float *out = a.partial + (int64_t)blockIdx.x * (MT * 16 * NT * 16);
  for (int i = tid; i < MT * 16 * NT * 16; i += 256) out[i] = red[i];
}

// out[f, n] = sum_b partial[b, f, n] for f < f_rows, n < H (partials are (MT*16) x (NT*16) padded).  A block sums 16
// outputs: 16 lanes per output take every 16th partial (independent loads in flight), then the 16 lane sums are added
// in lane order -- a fixed order, so the result is reproducible.
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float *partial, int n_part, int ld_f, int ld_n, int f_rows, int H, float *out) {
  __shared__ float red[256];
  const int tid = threadIdx.x, o = tid & 15, bl = tid >> 4;
  const int i = blockIdx.x * 16 + o;
  const bool ok = i < f_rows * H;
  const int f = ok ? i / H : 0, n = ok ? i - f * H : 0;
  const float *p = partial + (int64_t)f * ld_n + n;
  const int64_t stride = (int64_t)ld_f * ld_n;
  float s = 0.f;
#pragma unroll 8
  for (int b = bl; b < n_part; b += 16) s += p[b * stride];
  red[tid] = s;
  __syncthreads();
  if (tid < 16 && ok) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k * 16 + tid];
    out[i] = t;
  }
}

template <int MT, int NT>
inline hipError_t launch_wgrad_t(const WgradArgs &a, int grid, hipStream_t st) {
  hipLaunchKernelGGL((k_wgrad_mfma<MT, NT>), dim3((unsigned)grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

inline int wgrad_mt(int f_rows) {           // instantiated row-tile counts
  const int need = (f_rows + 15) / 16;
  const int have[6] = {1, 2, 3, 5, 7, 8};
  for (int k = 0; k < 6; ++k)
    if (have[k] >= need) return have[k];
  return 0;
}
inline int wgrad_nt(int H) { return H <= 16 ? 1 : (H <= 32 ? 2 : (H <= 64 ? 4 : 0)); }
inline int wgrad_grid(int64_t rows) { return (int)std::min<int64_t>(512, (rows + 127) / 128); }

inline hipError_t launch_wgrad(const WgradArgs &a, int mt, int nt, int grid, hipStream_t st) {
#define UDS_WG(M, N) if (mt == M && nt == N) return launch_wgrad_t<M, N>(a, grid, st);
  UDS_WG(1, 1) UDS_WG(1, 2) UDS_WG(1, 4) UDS_WG(2, 1) UDS_WG(2, 2) UDS_WG(2, 4) UDS_WG(3, 1) UDS_WG(3, 2) UDS_WG(3, 4)
  UDS_WG(5, 1) UDS_WG(5, 2) UDS_WG(5, 4) UDS_WG(7, 1) UDS_WG(7, 2) UDS_WG(7, 4) UDS_WG(8, 1) UDS_WG(8, 2) UDS_WG(8, 4)
#undef UDS_WG
  return hipErrorInvalidValue;
}

// ---- the wide form: d_kernel up to 256 x 256 plus the bias gradient (uds_wgrad_wide) -------------------------------------
// The output no longer fits one wave's accumulators, so it is cut into rb x cb blocks of MT x NT MFMA tiles: rb = 1 up to
// 8 row tiles (F <= 128), else 2; cb = ceil(column tiles / 4) blocks of 64 columns.  ONE workgroup holds all nb = rb * cb
// blocks: wave w owns block w % nb and walks the split w / nb of the workgroup's row span, one 32-row k-step per iteration,
// exactly as k_wgrad_mfma does, so the waves that share a split read the same rows of A and G at about the same time --
// every element comes from HBM once per call, the siblings' re-reads are L1 / L2 hits (the direct form, no LDS staging of
// the k-step).  ks = waves per block: 4, 4, 2, 2, 1, 1 at nb = 1, 2, 3, 4, 6, 8, that is 4, 8, 6, 8, 6, 8 waves.
// A choice that differs from k_wgrad_mfma: the bias gradient is NOT a row of ones in A (at F = 128 or 256 that row would
// open a tile row of its own, and 9 x 4 tiles plus the operands do not fit 256 registers without scratch).  Every wave
// already holds the G values of its columns for the split, so it adds them up in fp32 (fixed order: the 8 rows of a lane, the
// k-steps, then the 4 lane groups); the block's bias sums travel as one more row of the partial.
// At the end the ks waves of a block add their accumulators and bias sums into one LDS tile in split order, block after
// block, and the workgroup stores ONE (rb MT 16 + 1) x (cb NT 16) partial, every element of it; k_wgrad_reduce sums the
// workgroups' partials in index order.  No atomics: bitwise reproducible.  Tiles past F or H compute on zeros (their loads
// are masked off); wgrad_wide_plan keeps a workgroup's rows at 4 x its partial's size or more, so that the partials stay
// small beside A and G.
struct WgradWideArgs {
  const float *a, *g;        // A (rows, F) possibly time-shifted, G (rows, H)
  float *partial;            // (grid, rb * MT * 16 + 1, cb * NT * 16); the last row holds the column sums of G
  int64_t rows;
  int F, H;
  int shift, T, t_rows;      // as WgradArgs
  int rows_per_wave;         // multiple of 32
  int rb, cb, ks;            // row blocks, column blocks, waves per block
};

// 512 threads = two waves per SIMD = 256 registers a wave.  <8, 4> uses 254 of them (128 accumulators, 32 for the split G
// tiles, the rest addresses and loads in flight): one more live value in the loop spills.  Read the resource report of
// `python -m gnn_uds_amd.build --force -v` after any change to the loop (scratch must stay 0).
template <int MT, int NT>
__global__ __launch_bounds__(512) void k_wgrad_wide(WgradWideArgs a) {
  __shared__ float red[MT * 16 * NT * 16 + NT * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // row ranges in scalar registers
  const int r16 = lane & 15, qd = lane >> 4;
  const int nb = a.rb * a.cb;
  const int blk = wave % nb, split = wave / nb;
  const int f0 = (blk / a.cb) * (MT * 16), c0 = (blk % a.cb) * (NT * 16);      // this wave's block of the output
  f32x4 acc[MT][NT];
  float bsum[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    bsum[n] = 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int64_t r_begin = ((int64_t)blockIdx.x * a.ks + split) * a.rows_per_wave;
  const int64_t r_end = min(a.rows, r_begin + a.rows_per_wave);

  for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
    // this lane's 8 rows of the k-step, their validity and (for a causal tap) the shifted source row: k_wgrad_mfma's
    int64_t ra[8], rg[8];
    bool va[8], vg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t r = r0 + 8 * qd + j;
      vg[j] = r < r_end;
      rg[j] = vg[j] ? r : r_begin;
      va[j] = vg[j];
      ra[j] = rg[j];
      if (a.shift) {
        const int t = (int)((rg[j] / a.t_rows) % a.T);
        va[j] = vg[j] && t >= a.shift;
        ra[j] = va[j] ? rg[j] - (int64_t)a.shift * a.t_rows : r_begin;
      }
    }
    bf16x8 gh[NT], gl[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int c = c0 + 16 * n + r16;
      const bool cv = c < a.H;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (cv && vg[j]) ? a.g[rg[j] * a.H + c] : 0.f;
      bsum[n] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
      split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), gh[n], gl[n]);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int f = f0 + 16 * m + r16;
      float v[8];
      if (f < a.F) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = va[j] ? a.a[ra[j] * a.F + f] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
      }
      bf16x8 ah, al;
      split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), ah, al);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = mfma3(ah, al, gh[n], gl[n], acc[m][n]);
    }
  }
  // column sums: the 4 lane groups of a column, pairwise (every lane of the column ends with the same sum)
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    bsum[n] += __shfl_xor(bsum[n], 16);
    bsum[n] += __shfl_xor(bsum[n], 32);
  }

  // block after block: its ks waves add their partials in split order (fixed summation order) into one LDS tile, then the
  // whole workgroup stores the tile into the block's place in the partial (the bias sums: the row blocks at f0 = 0 only)
  constexpr int TILE = MT * 16 * NT * 16;
  const int ld_f = a.rb * (MT * 16), ldp = a.cb * (NT * 16);
  float *part = a.partial + (int64_t)blockIdx.x * (ld_f + 1) * ldp;
  for (int b = 0; b < nb; ++b) {
    for (int s = 0; s < a.ks; ++s) {
      if (blk == b && split == s) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float *p = red + (16 * m + 4 * qd + j) * (NT * 16) + 16 * n + r16;     // acc[m][n][j] = dW[f0 + 16m + 4qd + j][c0 + 16n + r16]
              *p = s == 0 ? acc[m][n][j] : *p + acc[m][n][j];
            }
        if (qd == 0) {
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            float *p = red + TILE + 16 * n + r16;
            *p = s == 0 ? bsum[n] : *p + bsum[n];
          }
        }
      }
      __syncthreads();
    }
    const int bf0 = (b / a.cb) * (MT * 16), bc0 = (b % a.cb) * (NT * 16);
    for (int i = tid; i < TILE; i += (int)blockDim.x) part[(bf0 + i / (NT * 16)) * ldp + bc0 + i % (NT * 16)] = red[i];
    if (bf0 == 0 && tid < NT * 16) part[ld_f * ldp + bc0 + tid] = red[TILE + tid];
    __syncthreads();
  }
}

struct WgradWidePlan {
  int mt, nt;                // the instantiation
  int rb, cb, ks;
  int ld_f, ld_n;            // the partial is (ld_f + 1) x ld_n
  int min_span, grid_cap;    // least rows per workgroup, most workgroups
  bool ok;
};

inline WgradWidePlan wgrad_wide_plan(int64_t F, int64_t H) {
  WgradWidePlan p{};
  if (F < 1 || F > 256 || H < 1 || H > 256) return p;
  const int ft = ((int)F + 15) / 16, ht = ((int)H + 15) / 16;
  p.rb = ft > 8 ? 2 : 1;
  const int need = (ft + p.rb - 1) / p.rb;
  p.mt = need <= 2 ? 2 : (need <= 4 ? 4 : (need <= 6 ? 6 : 8));
  p.cb = (ht + 3) / 4;
  p.nt = ht == 1 ? 1 : 4;
  const int nb = p.rb * p.cb;
  p.ks = nb <= 2 ? 4 : (nb <= 4 ? 2 : 1);
  p.ld_f = p.rb * p.mt * 16;
  p.ld_n = p.cb * p.nt * 16;
  const int unit = 32 * p.ks;                                  // a workgroup's rows: 4 x its partial's size or more
  p.min_span = (int)((4 * (int64_t)(p.ld_f + 1) * p.ld_n / (F + H) + unit - 1) / unit * unit);
  if (p.min_span < unit) p.min_span = unit;
  p.grid_cap = nb * p.ks <= 4 ? 512 : 256;                     // two 4-wave workgroups per CU, else one
  p.ok = true;
  return p;
}
inline int wgrad_wide_grid(const WgradWidePlan &p, int64_t rows) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(p.grid_cap, (rows + p.min_span - 1) / p.min_span));
}

inline hipError_t launch_wgrad_wide(const WgradWideArgs &a, int mt, int nt, int grid, hipStream_t st) {
  const unsigned threads = 64u * (unsigned)(a.rb * a.cb * a.ks);
#define UDS_WGW(M, N)                                                                            \
  if (mt == M && nt == N) {                                                                      \
    hipLaunchKernelGGL((k_wgrad_wide<M, N>), dim3((unsigned)grid), dim3(threads), 0, st, a);     \
    return hipGetLastError();                                                                    \
  }
  UDS_WGW(2, 1) UDS_WGW(2, 4) UDS_WGW(4, 1) UDS_WGW(4, 4) UDS_WGW(6, 1) UDS_WGW(6, 4) UDS_WGW(8, 1) UDS_WGW(8, 4)
#undef UDS_WGW
  return hipErrorInvalidValue;
}

}  // namespace uds
