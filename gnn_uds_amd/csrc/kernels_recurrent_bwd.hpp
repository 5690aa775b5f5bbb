// Reverse mode of the keras GRU / LSTM(H, return_sequences=True) time recurrence, H = 64 (k_recurrent_bwd) and every other
// multiple of 16 from 16 to 128 (k_recurrent_bwd_h, at the end of this file) (emulator.py:158-161 under the
// GradientTape of fit_eval, emulator.py:457-484): back-propagation through time as ONE time-streaming kernel on the matrix
// cores (gfx950), the mirror image of k_recurrent_mfma (kernels_recurrent.hpp).
//
// Forward (uds_recurrent_forward, exact fp32; gate order and reset_after=True form as in kernels_dense.hpp: k_recurrent):
//     a_rec = h[t-1] U + b_rec ;  GRU:  z = sig(xp_z + a_z), r = sig(xp_r + a_r), cand = tanh(xp_h + r a_h), h[t] = z h[t-1] + (1 - z) cand
//                                 LSTM: i, f, g, o from xp + a_rec ;  c[t] = f c[t-1] + i g ;  h[t] = o tanh(c[t])
// Backward: a wave owns 16 rows (series) of one batch element and walks t = T-1 .. 0 with the carried gradient dh (and dc):
//     1. a_rec is RECOMPUTED from the saved h[t-1] (one 16 x 64 x G*64 product, split-bf16, three MFMA products), the gates
//        from it and the saved input projection xp[t]: nothing but the layer output (and the LSTM's cell states) is kept
//        from the forward pass;
//     2. the gate derivatives give d_xp[t] (gradient of the input projection: handed to the Dense backward) and d_arec[t]
//        (gradient of the recurrent pre-activation; differs from d_xp only in the GRU's candidate gate: r * d_cand);
//     3. dh[t-1] = direct path + d_arec[t] U^T (one 16 x G*64 x 64 product).  The accumulator layout of step 2's values is
//        the B-operand fragment layout of step 3's product (the identity the forward kernel uses): no LDS round trip.
// d_arec is written gate-major, (G, B, T, R, 64), so that dU_g = h[t-1]^T d_arec_g is one call of the split-K weight-
// gradient kernel per gate (uds_wgrad with a time shift of one) and d b_rec its bias row.
// LDS: U as G packed 64 x 64 slices (uds_rowgemm_pack layout) and U^T as G more: 96 KB (GRU) / 128 KB (LSTM).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_recurrent.hpp"

namespace uds {

struct RecurrentBwdArgs {
  const float *xp, *b_rec;             // xp (B, T, R, G*64) input projection incl. input bias; b_rec (G*64) or NULL
  const uint4 *packed;                 // G slices of U (64 x 64 each), then G slices of U_g^T: [(kt * 4 + m) * 2 + hl] * 64 + lane
  const float *h, *c, *gh;             // h (B, T, R, 64) forward output; c (B, T, R, 64) cell states (LSTM) or NULL; gh = dL/dh
  float *dxp, *darec;                  // dxp (B, T, R, G*64); darec (G, B, T, R, 64)
  int B, T, R, n_blocks;
};

template <int G>
__global__ __launch_bounds__(RC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_recurrent_bwd(RecurrentBwdArgs a) {
  constexpr int MB = 4, KT = 2, SLICE = KT * MB * 2 * 64;      // uint4 per packed 64 x 64 slice
  extern __shared__ __attribute__((aligned(16))) uint4 wl_rb[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, qd = lane >> 4;
  for (int i = tid; i < 2 * G * SLICE; i += RC_WAVES * 64) wl_rb[i] = a.packed[i];
  __syncthreads();
  const int unit = blockIdx.x * RC_WAVES + wave;       // (batch element, 16-row block)
  if (unit >= a.B * a.n_blocks) return;
  const int b = unit / a.n_blocks, nb = unit - b * a.n_blocks;
  const int n_valid = min(16, a.R - nb * 16);
  const bool live = r16 < n_valid;
  const int64_t row0 = (int64_t)b * a.T * a.R + nb * 16 + min(r16, n_valid - 1);      // this lane's row at t = 0
  const int64_t t_rows = a.R;
  const int64_t gate_stride = (int64_t)a.B * a.T * a.R * 64;                           // floats between the gate planes of darec

  f32x4 br[G][MB];                                     // recurrent bias in accumulator layout: feature 16 m + 4 qd + q of gate g
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int m = 0; m < MB; ++m)
      br[g][m] = a.b_rec ? *reinterpret_cast<const f32x4 *>(a.b_rec + g * 64 + 16 * m + 4 * qd) : f32x4{0.f, 0.f, 0.f, 0.f};

  int wl_lane = lane;      // laundered once per step: the weight fragments are re-read from LDS every step, not hoisted out of the loop
  auto wfrag = [&](int slice, int kt, int m, int hl) __attribute__((always_inline)) {
    return __builtin_bit_cast(bf16x8, wl_rb[slice * SLICE + ((kt * MB + m) * 2 + hl) * 64 + wl_lane]);
  };
  // acc[m] += W_slice (k-step kt) x data fragment: three MFMA products per feature block
  auto mma = [&](int slice, int kt, f32x4 (&acc)[MB], const bf16x8 &dh_, const bf16x8 &dl_) __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const bf16x8 wh = wfrag(slice, kt, m, 0), wl = wfrag(slice, kt, m, 1);
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, dl_, acc[m], 0, 0, 0);
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, dh_, acc[m], 0, 0, 0);
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, dh_, acc[m], 0, 0, 0);
    }
  };
  auto frag = [&](const f32x4 &u0, const f32x4 &u1, bf16x8 &hi, bf16x8 &lo) __attribute__((always_inline)) {
    split8(make_float4(u0[0], u0[1], u0[2], u0[3]), make_float4(u1[0], u1[1], u1[2], u1[3]), hi, lo);
  };

  f32x4 dh[MB], dc[MB];                                // carried gradients (zero beyond the last step)
#pragma unroll
  for (int m = 0; m < MB; ++m) dh[m] = dc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // registers of the step being processed, loaded one step ahead
  f32x4 xq[G][MB], hp[MB], cp[MB], gq[MB];
  auto load_step = [&](int t) __attribute__((always_inline)) {
    const int64_t row = row0 + (int64_t)t * t_rows;
    const float *xr = a.xp + row * (G * 64) + 4 * qd;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int m = 0; m < MB; ++m) xq[g][m] = *reinterpret_cast<const f32x4 *>(xr + g * 64 + 16 * m);
    const float *gr = a.gh + row * 64 + 4 * qd;
#pragma unroll
    for (int m = 0; m < MB; ++m) gq[m] = *reinterpret_cast<const f32x4 *>(gr + 16 * m);
    if (t > 0) {
      const float *hr = a.h + (row - t_rows) * 64 + 4 * qd;
#pragma unroll
      for (int m = 0; m < MB; ++m) hp[m] = *reinterpret_cast<const f32x4 *>(hr + 16 * m);
      if (G == 4) {
        const float *cr = a.c + (row - t_rows) * 64 + 4 * qd;
#pragma unroll
        for (int m = 0; m < MB; ++m) cp[m] = *reinterpret_cast<const f32x4 *>(cr + 16 * m);
      }
    } else {
#pragma unroll
      for (int m = 0; m < MB; ++m) hp[m] = cp[m] = f32x4{0.f, 0.f, 0.f, 0.f};      // zero initial state
    }
  };

  for (int t = a.T - 1; t >= 0; --t) {
    asm volatile("" : "+v"(wl_lane));
    load_step(t);
    // ---- 1. a_rec = h[t-1] U + b_rec ----
    bf16x8 hh[KT], hl[KT];
    frag(hp[0], hp[1], hh[0], hl[0]);
    frag(hp[2], hp[3], hh[1], hl[1]);
    f32x4 ar[G][MB];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int m = 0; m < MB; ++m) ar[g][m] = br[g][m];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) mma(g, kt, ar[g], hh[kt], hl[kt]);
    }
    // ---- 2. gates and their derivatives ----
    f32x4 dx[G][MB], da[G][MB], direct[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dht = gq[m][q] + dh[m][q];
        if (G == 3) {
          const float z = rc_sigmoid(xq[0][m][q] + ar[0][m][q]), r = rc_sigmoid(xq[1][m][q] + ar[1][m][q]);
          const float ah = ar[2][m][q];
          const float cand = rc_tanh(xq[2][m][q] + r * ah);
          const float dcand = dht * (1.0f - z) * (1.0f - cand * cand);      // d / d(pre-activation of the candidate)
          const float dz = dht * (hp[m][q] - cand) * z * (1.0f - z);
          const float dr = dcand * ah * r * (1.0f - r);
          dx[0][m][q] = dz; dx[1][m][q] = dr; dx[2][m][q] = dcand;
          da[0][m][q] = dz; da[1][m][q] = dr; da[2][m][q] = dcand * r;
          direct[m][q] = dht * z;
        } else {
          const float ig = rc_sigmoid(xq[0][m][q] + ar[0][m][q]), fg = rc_sigmoid(xq[1][m][q] + ar[1][m][q]);
          const float gg = rc_tanh(xq[2][m][q] + ar[2][m][q]), og = rc_sigmoid(xq[G - 1][m][q] + ar[G - 1][m][q]);
          const float ct = fg * cp[m][q] + ig * gg, tc = rc_tanh(ct);
          const float dct = dc[m][q] + dht * og * (1.0f - tc * tc);
          dx[0][m][q] = dct * gg * ig * (1.0f - ig);
          dx[1][m][q] = dct * cp[m][q] * fg * (1.0f - fg);
          dx[2][m][q] = dct * ig * (1.0f - gg * gg);
          dx[G - 1][m][q] = dht * tc * og * (1.0f - og);
#pragma unroll
          for (int g = 0; g < G; ++g) da[g][m][q] = dx[g][m][q];
          dc[m][q] = dct * fg;
          direct[m][q] = 0.f;
        }
      }
    if (live) {
      const int64_t row = row0 + (int64_t)t * t_rows;
      float *xo = a.dxp + row * (G * 64) + 4 * qd;
      float *ao = a.darec + row * 64 + 4 * qd;
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          *reinterpret_cast<f32x4 *>(xo + g * 64 + 16 * m) = dx[g][m];
          *reinterpret_cast<f32x4 *>(ao + g * gate_stride + 16 * m) = da[g][m];
        }
    }
    // ---- 3. dh[t-1] = direct + sum_g d_arec_g U_g^T ----
#pragma unroll
    for (int m = 0; m < MB; ++m) dh[m] = direct[m];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      bf16x8 fh[KT], fl[KT];
      frag(da[g][0], da[g][1], fh[0], fl[0]);
      frag(da[g][2], da[g][3], fh[1], fl[1]);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) mma(G + g, kt, dh, fh[kt], fl[kt]);
    }
  }
}

inline size_t recurrent_bwd_lds(int G) { return (size_t)2 * G * (2 * 4 * 2 * 64) * sizeof(uint4); }

template <int G>
inline hipError_t launch_recurrent_bwd_t(const RecurrentBwdArgs &a, hipStream_t st) {
  static unsigned long long attr_done = 0;
  const size_t lds = recurrent_bwd_lds(G);
  if (hipError_t e = set_max_lds_once(reinterpret_cast<const void *>(&k_recurrent_bwd<G>), (int)lds, attr_done); e != hipSuccess) return e;
  const int units = a.B * a.n_blocks;
  hipLaunchKernelGGL((k_recurrent_bwd<G>), dim3((unsigned)((units + RC_WAVES - 1) / RC_WAVES)), dim3(RC_WAVES * 64), lds, st, a);
  return hipGetLastError();
}

// ---- other widths: H a multiple of 16 from 16 to 128 (the 64-unit kernel above stays the code it is) ----
// Same scheme, same outputs, the packed image generalised: 2 G slices (U_g, then U_g^T) of KT = ceil(H / 32) k-steps x
// MB = H / 16 feature blocks, [(kt * MB + m) * 2 + hl] * 64 + lane, rows H .. 32 KT - 1 of the K dimension zero (a width
// that is not a multiple of 32 sums over a zero half fragment).  At H = 64 this is the layout above.
// A wave still owns 16 series, but walks a step in K-PAIRS of feature blocks instead of holding every gate of every block
// at once (G * MB accumulators alone would be 128 VGPRs at H = 128, four times over for xp, a_rec, d_xp and d_arec):
//     for p = 0 .. KT-1:   blocks 2p, 2p+1:  a_rec (all gates) from the h[t-1] fragments, gates, derivatives, stores;
//                          the two blocks' d_arec are exactly k-step p of  dh[t-1] += d_arec_g U_g^T  (all MB output blocks).
// Weights: where the 2 G slices fit the 160 KiB LDS (H <= 64: at most 72 / 96 KiB at 48) they are staged once per
// workgroup as above.  Above 64 they do not (GRU 180 .. 384 KiB, LSTM 240 .. 512 KiB): every fragment is then read where
// it is used, one coalesced 1 KiB load per wave from the packed image -- at most 0.5 MiB, read by every wave of the
// grid at every step and so cache-resident; the loads of a k-pair are independent of the MFMA chain and issue ahead of it.
// No cross-wave exchange, no barrier inside the time loop, nothing depends on arrival order.
constexpr int recurrent_bwd_kt(int H) { return (H + 31) / 32; }
constexpr int recurrent_bwd_slice(int H) { return recurrent_bwd_kt(H) * (H / 16) * 2 * 64; }      // uint4 per packed slice
constexpr size_t recurrent_bwd_packed_bytes(int G, int H) { return (size_t)2 * G * recurrent_bwd_slice(H) * 16; }
constexpr bool recurrent_bwd_in_lds(int G, int H) { return recurrent_bwd_packed_bytes(G, H) <= 160 * 1024; }
inline bool recurrent_bwd_width_ok(int64_t H) { return H >= 16 && H <= 128 && H % 16 == 0; }

// U (H, G*H) row-major -> the packed image: slice s < G is U[:, sH:(s+1)H], slice G + g its transpose
__global__ void k_pack_recurrent_bwd(const float *__restrict__ U, int H, int G, uint4 *__restrict__ out) {
  const int MB = H / 16, KT = (H + 31) / 32, per = KT * MB * 64;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * G * per) return;
  const int s = idx / per, rem = idx - s * per;
  const int lane = rem & 63, m = (rem >> 6) % MB, t = (rem >> 6) / MB;
  const int qd = lane >> 4, f = 16 * m + (lane & 15), g = s < G ? s : s - G;
  bf16x8 hi, lo;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const int k = frag_k(t, qd, jj);
    const float w = k < H ? (s < G ? U[(int64_t)k * G * H + g * H + f] : U[(int64_t)f * G * H + g * H + k]) : 0.0f;
    const __bf16 h = (__bf16)w;
    hi[jj] = h;
    lo[jj] = (__bf16)(w - (float)h);
  }
  out[(int64_t)s * (KT * MB * 2 * 64) + ((t * MB + m) * 2 + 0) * 64 + lane] = __builtin_bit_cast(uint4, hi);
  out[(int64_t)s * (KT * MB * 2 * 64) + ((t * MB + m) * 2 + 1) * 64 + lane] = __builtin_bit_cast(uint4, lo);
}

template <int G, int H>
__global__ __launch_bounds__(RC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_recurrent_bwd_h(RecurrentBwdArgs a) {
  constexpr int MB = H / 16, KT = recurrent_bwd_kt(H), SLICE = recurrent_bwd_slice(H);
  constexpr bool IN_LDS = recurrent_bwd_in_lds(G, H);
  extern __shared__ __attribute__((aligned(16))) uint4 wl_rh[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, qd = lane >> 4;
  if constexpr (IN_LDS) {
    for (int i = tid; i < 2 * G * SLICE; i += RC_WAVES * 64) wl_rh[i] = a.packed[i];
    __syncthreads();
  }
  const int unit = blockIdx.x * RC_WAVES + wave;       // (batch element, 16-row block)
  if (unit >= a.B * a.n_blocks) return;
  const int b = unit / a.n_blocks, nb = unit - b * a.n_blocks;
  const int n_valid = min(16, a.R - nb * 16);
  const bool live = r16 < n_valid;
  const int64_t row0 = (int64_t)b * a.T * a.R + nb * 16 + min(r16, n_valid - 1);      // this lane's row at t = 0
  const int64_t t_rows = a.R;
  const int64_t gate_stride = (int64_t)a.B * a.T * a.R * H;                            // floats between the gate planes of darec
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  int wl_lane = lane;      // laundered once per step: the weight fragments are re-read every step, not hoisted out of the loop
  auto wfrag = [&](int slice, int kt, int m, int hl) __attribute__((always_inline)) {
    const int i = slice * SLICE + ((kt * MB + m) * 2 + hl) * 64 + wl_lane;
    if constexpr (IN_LDS) return __builtin_bit_cast(bf16x8, wl_rh[i]);
    else return __builtin_bit_cast(bf16x8, a.packed[i]);
  };
  auto mma3 = [&](int slice, int kt, int m, f32x4 &acc, const bf16x8 &dh_, const bf16x8 &dl_) __attribute__((always_inline)) {
    const bf16x8 wh = wfrag(slice, kt, m, 0), wl = wfrag(slice, kt, m, 1);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, dl_, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, dh_, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, dh_, acc, 0, 0, 0);
  };
  auto frag = [&](const f32x4 &u0, const f32x4 &u1, bf16x8 &hi, bf16x8 &lo) __attribute__((always_inline)) {
    split8(make_float4(u0[0], u0[1], u0[2], u0[3]), make_float4(u1[0], u1[1], u1[2], u1[3]), hi, lo);
  };

  f32x4 dh[MB], dc[MB];                                // carried gradients (zero beyond the last step)
#pragma unroll
  for (int m = 0; m < MB; ++m) dh[m] = dc[m] = zero4;

  for (int t = a.T - 1; t >= 0; --t) {
    asm volatile("" : "+v"(wl_lane));
    const int64_t row = row0 + (int64_t)t * t_rows;
    // the previous state, every block: the B operand of the a_rec product (zero initial state; zero beyond an odd last block)
    f32x4 hp[MB];
    bf16x8 hh[KT], hl[KT];
    if (t > 0) {
      const float *hr = a.h + (row - t_rows) * H + 4 * qd;
#pragma unroll
      for (int m = 0; m < MB; ++m) hp[m] = *reinterpret_cast<const f32x4 *>(hr + 16 * m);
    } else {
#pragma unroll
      for (int m = 0; m < MB; ++m) hp[m] = zero4;
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) frag(hp[2 * kt], 2 * kt + 1 < MB ? hp[2 * kt + 1] : zero4, hh[kt], hl[kt]);
    f32x4 dhn[MB];                                     // sum_g d_arec_g U_g^T
#pragma unroll
    for (int m = 0; m < MB; ++m) dhn[m] = zero4;

#pragma unroll
    for (int p = 0; p < KT; ++p) {
      f32x4 da[G][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int m = 2 * p + j;
        if (m >= MB) {
#pragma unroll
          for (int g = 0; g < G; ++g) da[g][j] = zero4;
          continue;
        }
        // ---- 1. a_rec = h[t-1] U + b_rec, block m of every gate ----
        f32x4 ar[G], xq[G], dx[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          xq[g] = *reinterpret_cast<const f32x4 *>(a.xp + row * (G * H) + g * H + 16 * m + 4 * qd);
          ar[g] = a.b_rec ? *reinterpret_cast<const f32x4 *>(a.b_rec + g * H + 16 * m + 4 * qd) : zero4;
        }
        const f32x4 gq = *reinterpret_cast<const f32x4 *>(a.gh + row * H + 16 * m + 4 * qd);
        f32x4 cp = zero4;
        if (G == 4 && t > 0) cp = *reinterpret_cast<const f32x4 *>(a.c + (row - t_rows) * H + 16 * m + 4 * qd);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) mma3(g, kt, m, ar[g], hh[kt], hl[kt]);
        // ---- 2. gates and their derivatives ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float dht = gq[q] + dh[m][q];
          if (G == 3) {
            const float z = rc_sigmoid(xq[0][q] + ar[0][q]), r = rc_sigmoid(xq[1][q] + ar[1][q]);
            const float ah = ar[2][q];
            const float cand = rc_tanh(xq[2][q] + r * ah);
            const float dcand = dht * (1.0f - z) * (1.0f - cand * cand);      // d / d(pre-activation of the candidate)
            const float dz = dht * (hp[m][q] - cand) * z * (1.0f - z);
            const float dr = dcand * ah * r * (1.0f - r);
            dx[0][q] = dz; dx[1][q] = dr; dx[2][q] = dcand;
            da[0][j][q] = dz; da[1][j][q] = dr; da[2][j][q] = dcand * r;
            dh[m][q] = dht * z;                                               // the direct path; the products are added below
          } else {
            const float ig = rc_sigmoid(xq[0][q] + ar[0][q]), fg = rc_sigmoid(xq[1][q] + ar[1][q]);
            const float gg = rc_tanh(xq[2][q] + ar[2][q]), og = rc_sigmoid(xq[G - 1][q] + ar[G - 1][q]);
            const float ct = fg * cp[q] + ig * gg, tc = rc_tanh(ct);
            const float dct = dc[m][q] + dht * og * (1.0f - tc * tc);
            dx[0][q] = dct * gg * ig * (1.0f - ig);
            dx[1][q] = dct * cp[q] * fg * (1.0f - fg);
            dx[2][q] = dct * ig * (1.0f - gg * gg);
            dx[G - 1][q] = dht * tc * og * (1.0f - og);
#pragma unroll
            for (int g = 0; g < G; ++g) da[g][j][q] = dx[g][q];
            dc[m][q] = dct * fg;
            dh[m][q] = 0.f;
          }
        }
        if (live) {
          float *xo = a.dxp + row * (G * H) + 16 * m + 4 * qd;
          float *ao = a.darec + row * H + 16 * m + 4 * qd;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            *reinterpret_cast<f32x4 *>(xo + g * H) = dx[g];
            *reinterpret_cast<f32x4 *>(ao + g * gate_stride) = da[g][j];
          }
        }
      }
      // ---- 3. k-step p of  dh[t-1] += sum_g d_arec_g U_g^T ----
#pragma unroll
      for (int g = 0; g < G; ++g) {
        bf16x8 fh, fl;
        frag(da[g][0], da[g][1], fh, fl);
#pragma unroll
        for (int m = 0; m < MB; ++m) mma3(G + g, p, m, dhn[m], fh, fl);
      }
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) dh[m] += dhn[m];
  }
}

template <int G, int H>
inline hipError_t launch_recurrent_bwd_h_t(const RecurrentBwdArgs &a, hipStream_t st) {
  static unsigned long long attr_done = 0;
  const size_t lds = recurrent_bwd_in_lds(G, H) ? recurrent_bwd_packed_bytes(G, H) : 0;
  if (lds)
    if (hipError_t e = set_max_lds_once(reinterpret_cast<const void *>(&k_recurrent_bwd_h<G, H>), (int)lds, attr_done); e != hipSuccess) return e;
  const int units = a.B * a.n_blocks;
  hipLaunchKernelGGL((k_recurrent_bwd_h<G, H>), dim3((unsigned)((units + RC_WAVES - 1) / RC_WAVES)), dim3(RC_WAVES * 64), lds, st, a);
  return hipGetLastError();
}

// any supported width; 64 is the kernel above, launched exactly as uds_recurrent_backward launches it
template <int G>
inline hipError_t launch_recurrent_bwd_h(const RecurrentBwdArgs &a, int H, hipStream_t st) {
  switch (H) {
    case 16: return launch_recurrent_bwd_h_t<G, 16>(a, st);
    case 32: return launch_recurrent_bwd_h_t<G, 32>(a, st);
    case 48: return launch_recurrent_bwd_h_t<G, 48>(a, st);
    case 64: return launch_recurrent_bwd_t<G>(a, st);
    case 80: return launch_recurrent_bwd_h_t<G, 80>(a, st);
    case 96: return launch_recurrent_bwd_h_t<G, 96>(a, st);
    case 112: return launch_recurrent_bwd_h_t<G, 112>(a, st);
    case 128: return launch_recurrent_bwd_h_t<G, 128>(a, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace uds
