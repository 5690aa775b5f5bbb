// Dense remainder of a trained NodeEdge layer on a SMALL network (gfx950): rest @ act(e W + b) in one launch, x_e on chip.
//
// The tiled path (kernels_gemm.hpp) was built for 10k-row networks: k_dense_split_planes writes the transposed bf16 image of
// x_e = act(e W + b) to global memory, k_remainder_gemm / k_remainder_gemm2 read it back in 128 x 128 / 256 x 256 tiles.  On the
// networks the reference ships (30 .. 444 rows) most of a tile is padding and the layer is launch-bound.  Here a workgroup owns G
// consecutive snapshots and does both steps:
//   phase A  x_e of its snapshots, as k_dense_split_planes computes it (16-row blocks per wave, MFMA 16x16x32 split-bf16, weight
//            fragments of uds_rowgemm_pack from L2), written as bf16 hi / lo straight into an LDS image [column (g, f)][m]:
//            rows of Kp + 8 bf16 (Kp = M rounded up to 64), so 8 consecutive m of one column are one 16-byte read and the 16
//            columns of a fragment read fall on 16 different 16-byte bank groups (the row stride in 16-byte units is odd).
//            Rows m >= M -- and whole snapshots past S in the last workgroup -- are written as zeros: 0 x NaN is NaN.
//   phase B  out[s][r][:] = sum_m rest[r][m] x_e[s][m][:]: x_e is the MFMA A operand from LDS, `rest` the B operand, loaded
//            from the planes of uds_remainder_pack straight into registers (the packed row layout IS the fragment layout: one
//            16-byte load per lane, plane and k-step of 32; the next step's loads are in flight during the current one's
//            MFMAs).  A wave pass is RB blocks of 16 rows of r times one group of 64 columns; the passes of a workgroup are
//            dealt to its 8 waves round robin.  A lane ends with 4 consecutive features of one out[s][r] row: 16-byte stores.
// Numerics as everywhere else: hi hi + lo hi + hi lo, fp32 accumulation.  No workspace.
// Lanes whose r >= R neither load nor store; every LDS word that is read was written in phase A.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels_dense.hpp"
#include "kernels_fused.hpp"

namespace uds {

constexpr int SNAP_WAVES = 8;                  // 512 threads
constexpr int SNAP_PAD = 8;                    // bf16 behind the Kp of an image row
constexpr int SNAP_MAX_GROUPS = 4;             // column groups of 64 per workgroup: at most 256 columns
constexpr int64_t SNAP_LDS_MAX = 160 * 1024;   // the CU's LDS
constexpr int64_t SNAP_LDS_TWO = 80 * 1024;    // an image up to here leaves room for a second workgroup on the CU
constexpr int64_t SNAP_MAX_ROWS = 1 << 20;

// The plan (host only).  A workgroup holds NG groups of 64 columns (G = 64 NG / h snapshots), NG = the largest count <= 4 whose
// image stays within half the LDS -- two workgroups per CU, one in phase A while the other is in phase B -- or 1 when even one
// group needs more than half; a shape whose single group exceeds 160 KiB is refused (NG = 0).  RB = 2 row blocks per wave pass
// (every x_e fragment read from LDS then feeds six MFMAs) when that still leaves a pass for each of the 8 waves, else 1.
struct SnapPlan {
  int G, NG, RB;
  int64_t lds;
};

inline int64_t snap_group_bytes(int64_t M) { return 2 * 64 * ((M + 63) / 64 * 64 + SNAP_PAD) * 2; }      // hi + lo planes of 64 columns

inline SnapPlan snapshot_plan(int64_t R, int64_t M, int64_t F, int64_t h) {
  SnapPlan p{0, 0, 0, 0};
  if (R <= 0 || M <= 0 || R > SNAP_MAX_ROWS || M > SNAP_MAX_ROWS || (F != 64 && F != 128) || (h != 32 && h != 64)) return p;
  const int64_t per = snap_group_bytes(M);
  if (per > SNAP_LDS_MAX) return p;
  p.NG = (int)std::max<int64_t>(1, std::min<int64_t>(SNAP_MAX_GROUPS, SNAP_LDS_TWO / per));
  p.G = p.NG * 64 / (int)h;
  p.lds = p.NG * per;
  const int64_t nrb = (R + 15) / 16;
  p.RB = ((nrb + 1) / 2) * p.NG >= SNAP_WAVES ? 2 : 1;
  return p;
}

struct SnapSide {
  const __bf16 *rest;      // hi plane (R x Kp) of uds_remainder_pack; the lo plane follows
  const float *e;          // (S, M, F)
  const uint4 *wq;         // uds_rowgemm_pack image of W (F x h)
  const float *bias;       // (h,) or NULL
  float *out;              // (S, R, h)
  int R, M, Kp, NG, RB, nwg;      // nwg: workgroups of this side, ceil(S / G); 0: the side is absent
};

struct SnapArgs {
  SnapSide side[2];
  int h, act;
  int64_t S;
};

template <int RB>
__device__ __forceinline__ void snap_phase_b(const SnapSide &sd, const __bf16 *xh, const __bf16 *xl, int ldw, int64_t s0, int64_t S, int h,
                                             int wave, int lane) {
  const int fr = lane & 15, qd = lane >> 4;
  const int nrb = (sd.R + 15) / 16, nrg = (nrb + RB - 1) / RB, units = nrg * sd.NG, nk = sd.Kp / 32;
  const __bf16 *rh = sd.rest, *rl = sd.rest + (int64_t)sd.R * sd.Kp;
  const bf16x8 zero = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
  for (int u = wave; u < units; u += SNAP_WAVES) {
    const int cg = u / nrg, rg = u - cg * nrg;
    f32x4 acc[RB][4];
    int64_t roff[RB];
    bool rok[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int r = (rg * RB + i) * 16 + fr;
      rok[i] = r < sd.R;
      roff[i] = (int64_t)min(r, sd.R - 1) * sd.Kp + 8 * qd;
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const __bf16 *ah = xh + (cg * 64 + fr) * ldw + 8 * qd, *al = xl + (cg * 64 + fr) * ldw + 8 * qd;
    bf16x8 bh[RB], bl[RB], nh[RB], nl[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      bh[i] = rok[i] ? *reinterpret_cast<const bf16x8 *>(rh + roff[i]) : zero;
      bl[i] = rok[i] ? *reinterpret_cast<const bf16x8 *>(rl + roff[i]) : zero;
    }
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          nh[i] = rok[i] ? *reinterpret_cast<const bf16x8 *>(rh + roff[i] + (kt + 1) * 32) : zero;
          nl[i] = rok[i] ? *reinterpret_cast<const bf16x8 *>(rl + roff[i] + (kt + 1) * 32) : zero;
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 vh = *reinterpret_cast<const bf16x8 *>(ah + c * 16 * ldw + kt * 32);
        const bf16x8 vl = *reinterpret_cast<const bf16x8 *>(al + c * 16 * ldw + kt * 32);
#pragma unroll
        for (int i = 0; i < RB; ++i) acc[i][c] = mfma3(vh, vl, bh[i], bl[i], acc[i][c]);
      }
      if (kt + 1 < nk) {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          bh[i] = nh[i];
          bl[i] = nl[i];
        }
      }
    }
    // D[row = 4 qd + j][col = fr] of tile (c, i): column cg 64 + 16 c + 4 qd + j of the image (snapshot s0 + col / h, feature
    // col % h), row r = 16 (rg RB + i) + fr of the result
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = cg * 64 + c * 16 + 4 * qd;
      const int sl = col / h, f = col - sl * h;
      const int64_t s = s0 + sl;
      if (s >= S) continue;
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int r = (rg * RB + i) * 16 + fr;
        if (rok[i]) *reinterpret_cast<f32x4 *>(sd.out + ((s * sd.R + r) * h + f)) = acc[i][c];
      }
    }
  }
}

template <int KT>
__global__ __launch_bounds__(SNAP_WAVES * 64) void k_remainder_snapshot(SnapArgs a) {
  constexpr int F = 32 * KT;
  extern __shared__ __attribute__((aligned(16))) unsigned char snap_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, qd = lane >> 4;
  const bool second = (int)blockIdx.x >= a.side[0].nwg;      // the workgroup index is partitioned between the two sides
  const SnapSide sd = second ? a.side[1] : a.side[0];
  const int wg = (int)blockIdx.x - (second ? a.side[0].nwg : 0);
  const int h = a.h, G = sd.NG * 64 / h, ldw = sd.Kp + SNAP_PAD;
  const int64_t s0 = (int64_t)wg * G;
  __bf16 *xh = reinterpret_cast<__bf16 *>(snap_lds), *xl = xh + sd.NG * 64 * ldw;

  // ---- phase A: x_e of snapshots s0 .. s0 + G - 1 into the image, every row m < Kp of every column written
  const int MB = h / 16, nblk = sd.Kp / 16;                   // MB = the block count of the packed weight image at h = 32, 64
  for (int u = wave; u < G * nblk; u += SNAP_WAVES) {
    const int g = u / nblk, blk = u - g * nblk;
    const int64_t s = s0 + g;
    const int m = 16 * blk + fr;
    const bool any = s < a.S && 16 * blk < sd.M;              // wave-uniform: a block of padding rows is zeros without the product
    f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (any) {
      const float *row = sd.e + (s * sd.M + min(m, sd.M - 1)) * F;
      if (sd.bias) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (b < MB) acc[b] = *reinterpret_cast<const f32x4 *>(sd.bias + 16 * b + 4 * qd);
      }
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const f32x4 u0 = *reinterpret_cast<const f32x4 *>(row + 32 * t + 4 * qd), u1 = *reinterpret_cast<const f32x4 *>(row + 32 * t + 16 + 4 * qd);
        bf16x8 dh, dl;
        split8(make_float4(u0[0], u0[1], u0[2], u0[3]), make_float4(u1[0], u1[1], u1[2], u1[3]), dh, dl);
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (b < MB) {
            const bf16x8 wh = __builtin_bit_cast(bf16x8, sd.wq[((t * MB + b) * 2 + 0) * 64 + lane]), wl = __builtin_bit_cast(bf16x8, sd.wq[((t * MB + b) * 2 + 1) * 64 + lane]);
            acc[b] = mfma3(wh, wl, dh, dl, acc[b]);
          }
      }
    }
    const bool live = any && m < sd.M;
    with_act(a.act, [&](auto act_) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (b < MB) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {      // acc[b][j]: feature 16 b + 4 qd + j of row m
            const float v = live ? act_ct<decltype(act_)::value>(acc[b][j], a.act) : 0.f;
            const __bf16 vh = (__bf16)v;
            const int o = (g * h + 16 * b + 4 * qd + j) * ldw + m;
            xh[o] = vh;
            xl[o] = (__bf16)(v - (float)vh);
          }
        }
    });
  }
  __syncthreads();

  // ---- phase B
  if (sd.RB == 2) snap_phase_b<2>(sd, xh, xl, ldw, s0, a.S, h, wave, lane);
  else snap_phase_b<1>(sd, xh, xl, ldw, s0, a.S, h, wave, lane);
}

}  // namespace uds
