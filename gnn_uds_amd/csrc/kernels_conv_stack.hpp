// A whole temporal Conv1D stack in ONE launch (gfx950): L in {2, 3} causal dilated Conv1D(64 -> 64, kernel 3) layers with
// dilations 1, 2[, 4] applied back to back to the same rows (`tem1_x`, `tem1_e`, `tem2_x`, `tem2_e`,
// emulator.py:154-157,244-257,299-310).  The input is read once and the last layer written once; the layers in between never
// reach memory.
//
// A wave owns 16 rows of one batch element and walks time, as k_conv3_stream does.  Step t loads x[t] straight into registers in
// B-operand fragment order (four 16-byte pieces per lane, prefetched CK_PREF steps ahead), splits it once and scatters it
// through layer 0's three taps into layer 0's ring of accumulator blocks:
//   out_0[t] += x[t] W_2,   out_0[t+1] += x[t] W_1,   out_0[t+2] += x[t] W_0.
// out_0[t] is then complete: bias, activation -- and the finished 16 x 64 block, lane (r16, qd) holding features 16 m + 4 qd + j,
// IS the fragment layout of the next product (the identity k_dense_cumsum_heads uses), so it is split in registers and scattered
// into layer 1's ring, and so on.  The last layer's block goes through a per-wave LDS tile and out as whole 128-B lines.
//
// Per layer and output block the operation order is exactly k_conv3_stream's (tap 0, 1, 2 into a given block; k-halves 0, 1; the
// three products of mfma3 in its order; split8; bias, then fused_act): the result equals, bit for bit, L successive
// streaming-Conv1D launches.  What differs is the issue order ACROSS blocks, which no value depends on: the wave is its SIMD's
// only one, so (as in k_recurrent_mfma) a GROUP = one (tap, k-half) = 8 weight fragments + 12 MFMAs on four independent
// accumulators, the fragments of group i+1 are fetched from LDS before the MFMAs of group i are issued, and out[t] -- complete
// after the first two groups, tap 2 -- gets its bias / activation / split under the MFMAs of the four groups that follow.
//
// Rings: layer i needs 2 D_i + 1 blocks in flight.  The time loop is unrolled CK_UNROLL times; a ring whose size divides
// CK_UNROLL is indexed at compile time, any other is kept in "block 0 = out[t]" order and shifted down one block per step
// (register moves under the next layer's MFMAs).  L = 2: rings 3 + 6, unrolled 6, no moves; L = 3: rings 3 + 5 + 9, unrolled 9,
// the middle ring shifts.  L = 3 holds 17 blocks = 272 accumulator registers per lane: one wave per SIMD on the unified
// VGPR + AGPR file, as k_recurrent_mfma runs.  LDS: 48 KB of pre-split weights per layer (96 / 144 KB), the biases, a 16 x 36
// tile per wave.
//
// Time segments as in launch_conv_stream: a segment that writes steps [s0, s1) starts HALO = sum_i 2 D_i steps early (6 / 14)
// and drops every block of the last layer before s0.  Intermediate values inside the halo are incomplete but finite; every
// written output depends only on complete ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_rowgemm.hpp"

namespace uds {

struct ConvStackArgs {
  const float *x;
  const uint4 *packed[3];     // k_pack_weight_frags layout of each layer's (3*64, 64) kernel: k-step kt = 2*tap + half
  const float *bias[3];       // 64 floats or nullptr
  float *out;
  int B, T, R, act;
  int n_blocks;               // ceil(R / 16)
  int n_seg, seg_len;
};

constexpr int CK_WAVES = 4;       // one wave per SIMD, one workgroup per CU
constexpr int CK_PREF = 1;        // time steps of input in flight (a step is ~3 us of MFMA issue)
constexpr int CK_CUS = 256;
constexpr int conv_stack_halo(int L) { return L == 2 ? 6 : 14; }
constexpr int conv_stack_ring(int L, int i) { return i == 0 ? 3 : i == 1 ? (L == 2 ? 6 : 5) : 9; }
constexpr int conv_stack_unroll(int L) { return L == 2 ? 6 : 9; }
constexpr int conv_stack_slots() { return CK_CUS * CK_WAVES; }      // resident waves of one launch

template <int N>
__device__ __forceinline__ void conv_stack_clear(f32x4 (&acc)[N][4]) {
#pragma unroll
  for (int s = 0; s < N; ++s)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[s][m] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ring kept in "block 0 = out[t]" order: one block down after a step
template <int N>
__device__ __forceinline__ void conv_stack_shift(f32x4 (&acc)[N][4]) {
#pragma unroll
  for (int s = 0; s + 1 < N; ++s)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[s][m] = acc[s + 1][m];
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[N - 1][m] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// the hi (HL = 0) or lo (1) weight fragments of k-step kt, one per feature block
template <int HL>
__device__ __forceinline__ void conv_stack_frags(const uint4 *w, int kt, int lane, bf16x8 (&f)[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) f[m] = __builtin_bit_cast(bf16x8, w[((kt * 4 + m) * 2 + HL) * 64 + lane]);
}

// One layer's share of step t (unrolled position U): the split input block (dh, dl) through the three taps into the ring, out[t]
// finished into y (bias + activation) and its ring block freed.  Six groups, tap 2 first (it completes out[t]); fh holds group 0's
// hi fragments on entry and those of the first group of `w_next` (the next layer, or layer 0 of the next step) on return.  The lo
// fragments are fetched inside their group: its first four MFMAs need the hi ones only (the register file does not hold both ahead).  under0() is
// issued under the MFMAs of group 0, under3(y) under those of group 3 (y is complete there).  A shifting ring is NOT shifted here.
// AHEAD = false fetches every group's fragments inside the group (three layers with a run-time activation: its inlined tanh / exp
// bodies take the registers the fragments held ahead would).
template <int ACT, int D, int N, int UNROLL, int U, bool AHEAD, class F0, class F3>
__device__ __forceinline__ void conv_stack_layer(f32x4 (&acc)[N][4], const uint4 *w, const uint4 *w_next, const float *bias_s, int lane, int qd,
                                                 int act, const bf16x8 (&dh)[2], const bf16x8 (&dl)[2], bf16x8 (&fh)[2][4],
                                                 f32x4 (&y)[4], F0 &&under0, F3 &&under3) {
  constexpr int MB = 4;
  constexpr bool SHIFT = UNROLL % N != 0;
  constexpr int CUR = SHIFT ? 0 : U % N, MID = SHIFT ? D : (U + D) % N, FAR = SHIFT ? 2 * D : (U + 2 * D) % N;
  static_assert(N >= 2 * D + 1, "ring too short");
  static_for<6>([&](auto i_) {
    constexpr int I = decltype(i_)::value, TAP = 2 - I / 2, H = I % 2, BUF = I % 2;
    constexpr int DST = TAP == 2 ? CUR : TAP == 1 ? MID : FAR;
    if constexpr (!AHEAD) conv_stack_frags<0>(w, 2 * TAP + H, lane, fh[BUF]);
    else if constexpr (I + 1 < 6) conv_stack_frags<0>(w, 2 * (2 - (I + 1) / 2) + (I + 1) % 2, lane, fh[BUF ^ 1]);
    else conv_stack_frags<0>(w_next, 4, lane, fh[0]);
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 fl[MB];
    conv_stack_frags<1>(w, 2 * TAP + H, lane, fl);
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[DST][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh[BUF][m], dl[H], acc[DST][m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[DST][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl[m], dh[H], acc[DST][m], 0, 0, 0);
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[DST][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh[BUF][m], dh[H], acc[DST][m], 0, 0, 0);
    if constexpr (I == 0) under0();
    if constexpr (I == 2) {
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(bias_s + 16 * m + 4 * qd);
        f32x4 o = acc[CUR][m];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fused_act<ACT>(o[j] + bb[j], act);
        y[m] = o;
        if constexpr (!SHIFT) acc[CUR][m] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if constexpr (I == 3) under3(y);
    __builtin_amdgcn_sched_barrier(0);
  });
}

template <int L, int ACT>
__global__ __launch_bounds__(CK_WAVES * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_conv3_stack(ConvStackArgs a) {
  static_assert(L == 2 || L == 3, "stacks of two or three layers");
  constexpr int F = 64, MB = 4, KT = 6, LD = 36, WL = KT * MB * 2 * 64;      // WL: uint4 entries of one layer's weights
  constexpr int UNROLL = conv_stack_unroll(L), HALO = conv_stack_halo(L);
  constexpr bool AHEAD = !(L == 3 && ACT == -1);
  constexpr int N0 = conv_stack_ring(L, 0), N1 = conv_stack_ring(L, 1), N2 = L == 3 ? conv_stack_ring(L, 2) : 1;
  static_assert(UNROLL % N0 == 0 && UNROLL % conv_stack_ring(L, L - 1) == 0, "only the middle ring may shift");
  extern __shared__ __attribute__((aligned(16))) float smem_ck[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, qd = lane >> 4;
  uint4 *wlds = reinterpret_cast<uint4 *>(smem_ck);
  float *bias_s = smem_ck + L * WL * 4;
  float *tile = bias_s + L * 64 + wave * (16 * LD);
#pragma unroll
  for (int l = 0; l < L; ++l) {
    for (int i = tid; i < WL; i += CK_WAVES * 64) wlds[l * WL + i] = a.packed[l][i];
    if (tid < 64) bias_s[l * 64 + tid] = a.bias[l] ? a.bias[l][tid] : 0.f;
  }
  __syncthreads();

  const int unit = blockIdx.x * CK_WAVES + wave;          // (time segment, batch element, 16-row block)
  if (unit >= a.n_seg * a.B * a.n_blocks) return;
  const int seg = unit / (a.B * a.n_blocks), bn = unit - seg * (a.B * a.n_blocks);
  const int b = bn / a.n_blocks, nb = bn - b * a.n_blocks;
  const int s0 = seg * a.seg_len, s1 = min(a.T, s0 + a.seg_len);       // steps whose outputs this wave writes
  const int t_first = max(0, s0 - HALO);                                 // ... after the halo steps that feed them
  const int n_valid = min(16, a.R - nb * 16);
  const int64_t row0 = (int64_t)b * a.T * a.R + nb * 16;   // row of time step 0
  const float *src_lane = a.x + (row0 + min(r16, n_valid - 1)) * F + 4 * qd;      // rows past the block re-read the last valid row
  const int64_t t_stride = (int64_t)a.R * F;
  // x[t] in fragment order: k-step h of the lane is the 16-byte pieces 32 h + 4 qd and 32 h + 16 + 4 qd of its row
  // (past the segment: a re-fetch of its last step, never used)
  auto load = [&](int t, float4 (&v)[4]) {
    const float4 *s = reinterpret_cast<const float4 *>(src_lane + (int64_t)min(t, s1 - 1) * t_stride);
    v[0] = s[0], v[1] = s[4], v[2] = s[8], v[3] = s[12];
  };
  float4 pre[CK_PREF][4];
#pragma unroll
  for (int q = 0; q < CK_PREF; ++q) load(t_first + q, pre[q]);

  f32x4 acc0[N0][MB], acc1[N1][MB], acc2[N2][MB];
  conv_stack_clear(acc0), conv_stack_clear(acc1), conv_stack_clear(acc2);
  int wl_lane = lane;
  bf16x8 fh[2][MB];
  conv_stack_frags<0>(wlds, 4, wl_lane, fh[0]);      // layer 0, tap 2, half 0

  for (int t0 = t_first; t0 < s1; t0 += UNROLL) {
    static_for<UNROLL>([&](auto u_) {
      constexpr int U = decltype(u_)::value;
      const int t = t0 + U;
      if (t < s1) {
        float4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = pre[0][i];
#pragma unroll
        for (int q = 0; q + 1 < CK_PREF; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i) pre[q][i] = pre[q + 1][i];
        load(t + CK_PREF, pre[CK_PREF - 1]);
        asm volatile("" : "+v"(wl_lane));      // the weight reads stay inside the time loop
        bf16x8 dh[2], dl[2], eh[2], el[2];
        f32x4 y[MB];
        auto nothing = [] {};
        // a finished block of a layer below the last: split into the next layer's operand (layer 0 -> eh / el, layer 1 -> dh / dl)
        auto to_e = [&](f32x4 (&o)[MB]) {
          split8(*reinterpret_cast<const float4 *>(&o[0]), *reinterpret_cast<const float4 *>(&o[1]), eh[0], el[0]);
          split8(*reinterpret_cast<const float4 *>(&o[2]), *reinterpret_cast<const float4 *>(&o[3]), eh[1], el[1]);
        };
        auto to_d = [&](f32x4 (&o)[MB]) {
          split8(*reinterpret_cast<const float4 *>(&o[0]), *reinterpret_cast<const float4 *>(&o[1]), dh[0], dl[0]);
          split8(*reinterpret_cast<const float4 *>(&o[2]), *reinterpret_cast<const float4 *>(&o[3]), dh[1], dl[1]);
        };
        // the last layer's out[t]: 16 x 64 block through the tile in two 32-column halves -> 4 stores
        // (halo steps only feed later outputs: their block is dropped)
        auto store = [&](f32x4 (&o)[MB]) {
          if (t >= s0) {
            const int64_t orow = row0 + (int64_t)t * a.R;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
#pragma unroll
              for (int mm = 0; mm < 2; ++mm) *reinterpret_cast<f32x4 *>(tile + r16 * LD + 16 * mm + 4 * qd) = o[2 * g + mm];
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
              for (int i = 0; i < 2; ++i) {
                const int rr = min(i * 8 + (lane >> 3), n_valid - 1), cc = 4 * (lane & 7);    // rows past the block repeat the last valid row
                const f32x4 ov = *reinterpret_cast<const f32x4 *>(tile + rr * LD + cc);
                *reinterpret_cast<f32x4 *>(a.out + (orow + rr) * 64 + 32 * g + cc) = ov;
              }
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
          }
        };
        split8(v[0], v[1], dh[0], dl[0]);
        split8(v[2], v[3], dh[1], dl[1]);
        conv_stack_layer<ACT, 1, N0, UNROLL, U, AHEAD>(acc0, wlds, wlds + WL, bias_s, wl_lane, qd, a.act, dh, dl, fh, y, nothing, to_e);
        if constexpr (L == 2) {
          conv_stack_layer<ACT, 2, N1, UNROLL, U, AHEAD>(acc1, wlds + WL, wlds, bias_s + 64, wl_lane, qd, a.act, eh, el, fh, y, nothing, store);
        } else {
          conv_stack_layer<ACT, 2, N1, UNROLL, U, AHEAD>(acc1, wlds + WL, wlds + 2 * WL, bias_s + 64, wl_lane, qd, a.act, eh, el, fh, y, nothing,
                                                  to_d);
          conv_stack_layer<ACT, 4, N2, UNROLL, U, AHEAD>(acc2, wlds + 2 * WL, wlds, bias_s + 128, wl_lane, qd, a.act, dh, dl, fh, y,
                                                  [&] { if constexpr (UNROLL % N1 != 0) conv_stack_shift(acc1); }, store);
        }
      }
    });
  }
}

inline int64_t conv_stack_lds_bytes(int L) { return (int64_t)L * (6 * 4 * 2 * 1024 + 256) + CK_WAVES * 16 * 36 * 4; }

// The default segmentation: enough units for ONE resident round, segments at least two halos long (the halo a segment
// re-computes stays <= 50 % of it).
inline void conv_stack_plan(int64_t B, int64_t T, int64_t R, int L, int64_t &n_seg, int64_t &seg_len) {
  const int64_t streams = std::max<int64_t>(1, B * ((R + 15) / 16));
  n_seg = std::max<int64_t>(1, std::min<int64_t>(conv_stack_slots() / streams, T / (2 * conv_stack_halo(L))));
  seg_len = (T + n_seg - 1) / n_seg;
  n_seg = (T + seg_len - 1) / seg_len;
}

template <int L, int ACT>
inline hipError_t launch_conv_stack_a(const ConvStackArgs &a, hipStream_t st) {
  static unsigned long long attr_done = 0;
  if (hipError_t e = set_max_lds_once(reinterpret_cast<const void *>(&k_conv3_stack<L, ACT>), 160 * 1024, attr_done); e != hipSuccess) return e;
  const int units = a.n_seg * a.B * a.n_blocks;
  hipLaunchKernelGGL((k_conv3_stack<L, ACT>), dim3((unsigned)((units + CK_WAVES - 1) / CK_WAVES)), dim3(CK_WAVES * 64),
                     (size_t)conv_stack_lds_bytes(L), st, a);
  return hipGetLastError();
}

template <int L>
inline hipError_t launch_conv_stack_t(const ConvStackArgs &a, hipStream_t st) {
  if (a.act == 1) return launch_conv_stack_a<L, 1>(a, st);     // relu
  if (a.act == 0) return launch_conv_stack_a<L, 0>(a, st);     // linear
  return launch_conv_stack_a<L, -1>(a, st);
}

// a.n_seg / a.seg_len set by the caller (conv_stack_plan, or a forced count)
inline hipError_t launch_conv_stack(const ConvStackArgs &a, int L, hipStream_t st) {
  return L == 2 ? launch_conv_stack_t<2>(a, st) : launch_conv_stack_t<3>(a, st);
}

}  // namespace uds
