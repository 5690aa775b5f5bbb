// Wave-specialised form of the fused spatial-layer kernel for 64-wide rows (every layer of a d = 64 block but the
// 96-wide first layer of block 2): same tiles, same tile blocks, same arithmetic and the same results, bit for bit,
// as k_fused_tile<64, 64> (kernels_fused.hpp) -- what changes is WHO does what and WHEN.
//
// k_fused_tile runs its eight waves through the phases in lock-step (all multiply, then all gather), every wave keeps
// all the weights (128 VGPRs), every input row passes through an LDS stage, and there are two workgroup barriers per
// snapshot.  Here the workgroup is two teams, software-pipelined over the snapshots, ONE barrier per snapshot:
//
//   interval k     "Y" team (waves 0 .. NY-1): the big weights (96 VGPRs)      "X" team (the rest): the small weights (32 VGPRs)
//                  P2(s):  [prim | agg] @ Wbig -> hx[k & 1], scores[k & 1]      P1(s+1): secondary MLP -> sec[(k+1) & 1]
//                          prim rows of s+1 -> registers                                 secondary rows of s+2 -> registers
//                                                                               P3(s-1): softmax + neighbour sum from hx[(k-1) & 1] -> HBM
//   ---- barrier ----
//
// * No input row touches LDS: each Y wave loads the primary blocks it multiplies straight into the registers its split
//   reads, each X wave the secondary blocks it feeds to the small GEMM, both one interval ahead.  LDS holds only what is
//   shared: sec (x2), hx (x2), the attention scalars (x2) and the tile block: 135 KB instead of 157, and ~30 % less LDS
//   traffic per snapshot (the stage's writes and reads are gone).
// * Registers follow the roles: Y keeps Wbig and no P3 state, X keeps Wsmall, the rows in flight and the P3 state.
// * One barrier per interval orders everything: P1(s+1) writes the sec buffer P2(s-1) read an interval ago, P2(s) writes
//   the hx buffer P3(s-2) read an interval ago.
// * Global accesses: Y's row loads are ordinary loads (it stores nothing: the compiler's vmcnt counting is exact).  X
//   stores its outputs behind its row loads, and the compiler -- which merges its pending-operation state over the
//   exec-masked store branches -- would wait vmcnt(0) for those fresh stores before the next P1; X's row loads are
//   therefore inline asm and their one wait is counted by hand: vmcnt(number of stores issued since).
// * Set-up (paid once per (tile, chunk) workgroup: 1 010 times per launch at the headline) is two vector-memory round trips
//   behind one scalar one, where it used to be four.  Trip 0 (scalar): the tile's side and the eight-int header of its block
//   from global memory -- the section offsets are known before anything is in LDS.  Trip 1, issued back to back: the tile block,
//   the attention vectors, each lane's row ids straight from the global block (clamped indices stay inside the block) and the
//   team's weights into their final registers; one wait for the block, one __syncthreads.  Trip 2: the first snapshot's rows
//   (Y: pp / rm, X: the asm loads) and the NodeEdge gather incl. the overflow list; X's static P3 state and Y's ag_locs are
//   computed under it.  The gathered values are read by Y's aggregate only, from behind the first lds_barrier of the
//   pipeline (the one after P1(0)), so no second set-up barrier is needed.  Each team still drains with ONE
//   __builtin_amdgcn_s_waitcnt(vmcnt(0)) on every path into its snapshot loop.
#pragma once
#include "kernels_fused.hpp"

namespace uds {

// Tuning values: to sweep one, edit its line.
constexpr int WS_NY = 4, WS_NX = FUSED_WAVES - WS_NY;      // team sizes (the 32-row P2 needs four Y waves: see the static_assert there)
constexpr int WS_XPRIO = 1;       // s_setprio of the X team's waves (the Y team stays at 0)
constexpr int WS_OCT_WD = 4;      // neighbour slots per step of the octet P3 (each step: WS_OCT_WD x 2 x octets ds_read_b128 in flight)
constexpr int WS_OCT_GRP = 1;     // octets per batch of reads in a P3 step (registers: 8 x WS_OCT_GRP x WS_OCT_WD for the pieces)

// LDS bytes: tile block + 2 x (s_self, s_nbr) + attention vectors / bias + 2 x sec rows + 2 x hx rows
inline int64_t fused_ws_lds_bytes(int p_cap, int q_cap, int meta_cap) {
  return 4 * ((int64_t)meta_cap + 4 * p_cap + 3 * FUSED_D + FUSED_H + 2 * (int64_t)q_cap * SEC_STRIDE + 2 * (int64_t)p_cap * FUSED_D);
}

// 16 bytes per lane from base (wave-uniform, SGPR pair) + voff (per-lane byte offset) + IMM, invisible to the compiler's
// vmcnt bookkeeping (see the header): the value is NOT there when the statement ends -- ws_vmcnt() makes it so.
template <int IMM>
__device__ __forceinline__ void ws_gld16(f32x4 &dst, const float *base, unsigned voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(base), "n"(IMM) : "memory");
}
// tie four row registers to a point of the program: nothing that reads them is scheduled above it, nothing that writes them below
__device__ __forceinline__ void ws_pin4(f32x4 &a0, f32x4 &a1, f32x4 &a2, f32x4 &a3) {
  asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
}
// 8-lane all-reduce (max / sum) of FOUR values at once with the DPP move folded into the operation, as row16_max4 / row16_sum4
// (kernels_fused.hpp) but for the octet layout of P3 (8 lanes per output row): quad_perm x2, then row_half_mirror (lane i <-> 7 - i
// inside every 8 lanes) joins the two quads.
__device__ __forceinline__ void row8_max4(const float (&in)[4], float (&out)[4]) {
  asm("s_nop 1\n\t" UDS_DPP4_FIRST("v_max_f32_dpp", "quad_perm:[1,0,3,2]") UDS_DPP4("v_max_f32_dpp", "quad_perm:[2,3,0,1]")
      UDS_DPP4("v_max_f32_dpp", "row_half_mirror")
      : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3])
      : "v"(in[0]), "v"(in[1]), "v"(in[2]), "v"(in[3]));
}
__device__ __forceinline__ void row8_sum4(const float (&in)[4], float (&out)[4]) {
  asm("s_nop 1\n\t" UDS_DPP4_FIRST("v_add_f32_dpp", "quad_perm:[1,0,3,2]") UDS_DPP4("v_add_f32_dpp", "quad_perm:[2,3,0,1]")
      UDS_DPP4("v_add_f32_dpp", "row_half_mirror")
      : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3])
      : "v"(in[0]), "v"(in[1]), "v"(in[2]), "v"(in[3]));
}
// 16-bit half HI of pk (zero-extended) + base, one SDWA instruction.  Written as C the compiler unpacks every half it will
// need into a register of its own ahead of the snapshot loop: 32 registers the octet P3 does not have.
template <int HI>
__device__ __forceinline__ unsigned ws_add_half(unsigned pk, unsigned base) {
  unsigned r;
  if (HI) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD" : "=v"(r) : "v"(pk), "v"(base));
  else asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(r) : "v"(pk), "v"(base));
  return r;
}
// wait until all but the n youngest vector-memory operations of this wave are done (n <= 8, exact)
__device__ __forceinline__ void ws_vmcnt(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
  }
}

template <int ACT>
__global__ __launch_bounds__(FUSED_WAVES * 64, 2) void k_fused_ws(FusedArgs a) {
  constexpr int NT = FUSED_WAVES * 64, NY = WS_NY, NX = WS_NX;
  constexpr int FP = 64, FS = 64;
  constexpr int U = FUSED_U;
  extern __shared__ __attribute__((aligned(16))) int32_t smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool team_y = wave < NY;                 // wave-uniform role
  const int yw = wave, xw = wave - NY;           // index inside the team

  // XCD-aware bijective remap (as k_fused_tile): workgroups b, b+8, .. share an XCD and get a contiguous range of items
  const int W = gridDim.x, b = blockIdx.x;
  const int q8 = W / 8, r8 = W % 8, xcd = b % 8;
  const int w = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + b / 8;
  const int tile = w % a.n_tiles;
  const int chunk_id = w / a.n_tiles;
  const int s_begin = chunk_id * a.chunk;
  const int s_end = min(a.S, (chunk_id + 1) * a.chunk);
#ifdef UDS_PHASE_TIMING
  unsigned long long tm_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl_ = clock64();      // stamp 0 runs from kernel entry to the first lds_barrier
  const unsigned long long rt0_ = __builtin_amdgcn_s_memrealtime(), mt0_ = tl_;
#endif
  // ---- set-up, trip 0 (scalar): the tile's side and the header of its block, both from global memory ----
  // The header (the same eight ints the block copy puts at smem[0..7]) gives the section offsets before anything is in LDS, so
  // every address of trip 1 can be formed at once.
  const int32_t *gblk = a.blocks + (int64_t)tile * a.meta_cap;
  const int sd = __builtin_amdgcn_readfirstlane(a.hdr[tile * TILE_HDR_INTS + 6]);
  int hd_[TILE_HDR_INTS];
#pragma unroll
  for (int q = 0; q < TILE_HDR_INTS; ++q) hd_[q] = __builtin_amdgcn_readfirstlane(gblk[q]);
  if (!((a.side_mask >> sd) & 1)) return;
  const FusedSide &S_ = a.side[sd];
  const int n_own = hd_[0], n_prim = hd_[1], n_sec = hd_[2], flags = hd_[3], n_ovf = hd_[4], n_adj = hd_[5], inc_width = hd_[7];
  const EllOffsets off = ell_offsets(n_own, n_prim, n_sec, flags, n_ovf, n_adj);

  float *s_self = reinterpret_cast<float *>(smem + a.meta_cap);         // [2][p_cap]
  float *s_nbr = s_self + 2 * a.p_cap;                                   // [2][p_cap]
  float *attn = s_nbr + 2 * a.p_cap;             // a_self[64] | a_nbr[64] | b_small[32] | b_out[64]
  float *sec = attn + 3 * FUSED_D + FUSED_H;     // [2][q_cap * SEC_STRIDE]
  float *hx = sec + 2 * a.q_cap * SEC_STRIDE;    // [2][p_cap * 64]
  const int sec_buf = a.q_cap * SEC_STRIDE, hx_buf = a.p_cap * FUSED_D;

  const int32_t *prim_ids = smem + off.prim;
  const uint32_t *inc_loc = reinterpret_cast<const uint32_t *>(smem + off.inc_loc);
  int32_t *inc_w = smem + off.inc_w;
  const f32x4 *inc_val4 = reinterpret_cast<const f32x4 *>(inc_w);
  const unsigned char *adj_b = reinterpret_cast<const unsigned char *>(smem + off.adj);
  const int32_t *ovf_ptr = smem + off.ovf_ptr, *ovf_loc = smem + off.ovf_loc;
  int32_t *ovf_w = smem + off.ovf_w;
  const int32_t *adj_ptr = smem + off.adj_ptr, *adj_loc = smem + off.adj_loc;
  const float *ovf_val = reinterpret_cast<const float *>(ovf_w);

  // ---- set-up, trip 1: every load whose address is known now, issued back to back; nothing waits until all are in flight ----
  // Common to both teams: the tile block (first 16 bytes per thread; a block longer than NT x 16 B finishes in block_to_lds) and
  // the attention vectors.  Each team adds, in its branch, its row ids straight from the global block and its weights.
  // (issue_block is called inside the team's branch: loaded in front of it, blk0 was spilled to scratch behind a vmcnt(0).)
  const int n4 = a.meta_cap / 4;
  const uint4 *blk4 = reinterpret_cast<const uint4 *>(gblk);
  uint4 blk0;
  float at_s = 0.f, at_n = 0.f, at_bs = 0.f, at_bo = 0.f;
  auto issue_block = [&]() __attribute__((always_inline)) {
    blk0 = blk4[min(tid, n4 - 1)];
    if (wave == 0) {       // lane = tid < FUSED_D
      at_s = S_.a_self[lane];
      at_n = S_.a_nbr[lane];
      if (lane < FUSED_H && S_.b_small) at_bs = S_.b_small[lane];
      if (S_.b_out) at_bo = S_.b_out[lane];
    }
  };
  // one wait, one barrier: the tile block and the attention vectors are in LDS.  The compiler barrier in front keeps the stores
  // (and the wait they need) behind every load the caller has issued.
  auto block_to_lds = [&]() __attribute__((always_inline)) {
    asm volatile("" ::: "memory");
    uint4 *dst = reinterpret_cast<uint4 *>(smem);
    if (tid < n4) dst[tid] = blk0;
    for (int i = tid + NT; i < n4; i += NT) dst[i] = blk4[i];
    if (wave == 0) {   // scaled by log2(e): scores are logits in base-2 units, P3 needs no multiply in front of its exp2
      attn[lane] = at_s * 1.44269504088896340736f;
      attn[FUSED_D + lane] = at_n * 1.44269504088896340736f;
      if (lane < FUSED_H) attn[2 * FUSED_D + lane] = at_bs;
      attn[2 * FUSED_D + FUSED_H + lane] = at_bo;
    }
    __syncthreads();
  };
  // ---- set-up, trip 2 (behind that barrier, next to the team's first-snapshot rows): the NodeEdge values of the fixed-width lists
  // (0 for padding) and of the overflow list replace their indices in the tile block.  One element per thread covers the
  // fixed-width lists (ELL_INC * n_prim <= NT: p_cap <= 128).  gather_issue puts the loads in flight, gather_land stores what
  // came back; only the Y team's aggregate reads the values, from behind the first lds_barrier of the pipeline.
  static_assert(ELL_INC * 32 * NY <= NT, "one gather element per thread covers the rows the Y team multiplies");
  const int n_inc = ELL_INC * n_prim;
  float ne_v = 0.f, ov_v = 0.f;
  auto gather_issue = [&]() __attribute__((always_inline)) {
    if (tid < n_inc) {
      const int k = inc_w[tid];
      if (k >= 0) ne_v = S_.ne_val[k];
    }
    if ((flags & ELL_FLAG_INC_OVF) && tid < n_ovf) ov_v = S_.ne_val[ovf_w[tid]];
  };
  auto gather_land = [&]() __attribute__((always_inline)) {
    if (tid < n_inc) reinterpret_cast<float *>(inc_w)[tid] = ne_v;
    if (flags & ELL_FLAG_INC_OVF) {
      if (tid < n_ovf) reinterpret_cast<float *>(ovf_w)[tid] = ov_v;
      for (int i = tid + NT; i < n_ovf; i += NT) reinterpret_cast<float *>(ovf_w)[i] = S_.ne_val[ovf_w[i]];
    }
  };

#ifdef UDS_PHASE_TIMING
#define WS_STAMP(k) do { const unsigned long long n_ = clock64(); tm_[k] += n_ - tl_; tl_ = n_; } while (0)
#define WS_DUMP() do { if (a.dbg && lane == 0) { unsigned long long *o = a.dbg + ((size_t)blockIdx.x * 8 + wave) * 16; \
    for (int q_ = 0; q_ < 7; ++q_) o[q_] = tm_[q_]; o[12] = wave; \
    o[15] = ((__builtin_amdgcn_s_memrealtime() - rt0_) << 32) | ((clock64() - mt0_) & 0xffffffffull); \
    o[7] = 1ull | ((unsigned long long)sd << 8) | ((unsigned long long)n_own << 16) | ((unsigned long long)n_prim << 32) | ((unsigned long long)n_sec << 48); } } while (0)
#else
#define WS_STAMP(k) do { } while (0)
#define WS_DUMP() do { } while (0)
#endif
  const int64_t sec_stride = (int64_t)S_.n_sec_glob * FS, prim_stride = (int64_t)S_.n_prim_glob * FP;      // floats per snapshot
  const int n_snap = s_end - s_begin;

  // The two teams run two separate loops (the same number of barriers in each): what a team keeps in registers across the
  // snapshots -- the big weights here, the small weights, rows in flight and P3 state there -- is live in its own loop only.
  if (team_y) {
    // =========================== Y team: P2 on v_mfma_f32_32x32x16_bf16 ===========================
    // One 32-row block per wave (rows 32 yw ..).  Same flops per cycle as 16x16x32 (k_fused_tile), but an MFMA holds its SIMD's
    // vector issue for 8 of its 32 cycles instead of 8 of 16 (MI355X_MICROARCH.md): the X wave on this SIMD -- the long
    // instruction stream of the kernel -- loses half as many issue slots to this wave's matrix work.  Lane l: n = l & 31 is
    // the row, hf = l >> 5 the k half: B fragment of k-step t = floats 16 t + 8 hf .. + 7 of the row; the accumulators hold
    // features (r & 3) + 8 (r >> 2) + 4 hf (+ 32 m) of row n (cdna_hip_programming.md section 3).
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    constexpr int KT32 = (FP + FUSED_H) / 16, KX32 = FP / 16, MB32 = FUSED_D / 32;      // 6 k-steps (4 of x, 2 of agg), 2 feature blocks
    static_assert(NY == 4, "one 32-row block per Y wave: four waves cover p_cap = 128");
    const int n32 = lane & 31, hf = lane >> 5;
    const int lrow = 32 * yw + n32;
    const bool valid = lrow < n_prim;
    const int lr = min(lrow, n_prim - 1);
    // trip 1, Y's part: this lane's row id from the tile's block in global memory (a clamped row -- and the word in front of the
    // section, should it be empty -- lies inside the block), then the weights into the registers they stay in
    issue_block();
    const int prim_id = gblk[off.prim + lr];
    bf16x8 wh[KT32][MB32], wl[KT32][MB32];       // 96 VGPRs, resident across the snapshot loop
#pragma unroll
    for (int t = 0; t < KT32; ++t)
#pragma unroll
      for (int m = 0; m < MB32; ++m) {
        wh[t][m] = __builtin_bit_cast(bf16x8, S_.w_big32[((t * MB32 + m) * 2 + 0) * 64 + lane]);
        wl[t][m] = __builtin_bit_cast(bf16x8, S_.w_big32[((t * MB32 + m) * 2 + 1) * 64 + lane]);
      }
    block_to_lds();
    const unsigned prow = (unsigned)prim_id * FP + 8u * hf;      // element offset of this lane's 8-float piece of k-step 0
    f32x4 pp[2 * KX32];           // the primary row of the snapshot P2 multiplies next: piece i = floats 16 (i >> 1) + 8 hf + 4 (i & 1)
    // the dense remainder of a trained NodeEdge (FusedSide::rem, (S, n_prim_glob, 32)): this lane's 16 aggregate features of its
    // row, fetched with the row itself one interval ahead and used as the initial value of the aggregate
    const bool has_rem = S_.rem != nullptr;
    const unsigned rrow = (unsigned)prim_id * FUSED_H + 8u * hf;
    f32x4 rm[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int64_t rem_stride = (int64_t)S_.n_prim_glob * FUSED_H;
    // trip 2, Y's part: the first snapshot's row (and remainder piece), then the NodeEdge gather; the LDS read of ag_locs rides under it
    if (n_snap > 0) {
      const float *base = S_.prim_in + s_begin * prim_stride;
      static_for<2 * KX32>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        pp[i] = *reinterpret_cast<const f32x4 *>(base + prow + 16 * (i >> 1) + 4 * (i & 1));
      });
      if (has_rem) {
        const float *rb = S_.rem + s_begin * rem_stride + rrow;
        rm[0] = *reinterpret_cast<const f32x4 *>(rb);
        rm[1] = *reinterpret_cast<const f32x4 *>(rb + 4);
        rm[2] = *reinterpret_cast<const f32x4 *>(rb + 16);
        rm[3] = *reinterpret_cast<const f32x4 *>(rb + 20);
      }
    }
    gather_issue();
    const unsigned ag_locs = inc_loc[lr];
    gather_land();
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): drain the set-up loads on every path (see the X team's note)
    WS_STAMP(0);
    lds_barrier();      // the X team has computed the secondary MLP of the first snapshot; every thread's NodeEdge values are in LDS
    const f32x4 ag_vals = inc_val4[lr];      // the only reader of those values (with ovf_val in the loop): behind that barrier

    auto mfma3_32 = [&](const bf16x8 &a_h, const bf16x8 &a_l, const bf16x8 &d_h, const bf16x8 &d_l, f32x16 acc) __attribute__((always_inline)) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, d_l, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l, d_h, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, d_h, acc, 0, 0, 0);
      return acc;
    };
    for (int k = 0; k <= n_snap; ++k) {
      if (k < n_snap && 32 * yw < n_prim) {
        const bool more = k + 1 < n_snap;
        const float *next = S_.prim_in + (s_begin + k + 1) * prim_stride;
        const float *secr = sec + (k & 1) * sec_buf;
        float *hxw = hx + (k & 1) * hx_buf;
        float *ssw = s_self + (k & 1) * a.p_cap, *snw = s_nbr + (k & 1) * a.p_cap;
        bf16x8 dh[KT32], dl[KT32];
        static_for<KX32>([&](auto t_) {
          constexpr int t = decltype(t_)::value;
          const f32x4 u0 = pp[2 * t], u1 = pp[2 * t + 1];
          split8(make_float4(u0[0], u0[1], u0[2], u0[3]), make_float4(u1[0], u1[1], u1[2], u1[3]), dh[t], dl[t]);
        });
        if (more)      // the registers are free: the next snapshot's row, a whole interval ahead
          static_for<2 * KX32>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            pp[i] = *reinterpret_cast<const f32x4 *>(next + prow + 16 * (i >> 1) + 4 * (i & 1));
          });
        f32x16 acc[MB32];
#pragma unroll
        for (int m = 0; m < MB32; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
#pragma unroll
        for (int t = 0; t < KX32; ++t)
#pragma unroll
          for (int m = 0; m < MB32; ++m) acc[m] = mfma3_32(wh[t][m], wl[t][m], dh[t], dl[t], acc[m]);
        // NodeEdge aggregate of this row in fragment shape: features 8 hf .. + 7 (k-step 4) and 16 + 8 hf .. + 7 (k-step 5)
        float4 g0 = make_float4(rm[0][0], rm[0][1], rm[0][2], rm[0][3]), g1 = make_float4(rm[1][0], rm[1][1], rm[1][2], rm[1][3]),
               g2 = make_float4(rm[2][0], rm[2][1], rm[2][2], rm[2][3]), g3 = make_float4(rm[3][0], rm[3][1], rm[3][2], rm[3][3]);
        if (more && has_rem) {      // consumed: the next snapshot's remainder piece
          const float *rb = S_.rem + (s_begin + k + 1) * rem_stride + rrow;
          rm[0] = *reinterpret_cast<const f32x4 *>(rb);
          rm[1] = *reinterpret_cast<const f32x4 *>(rb + 4);
          rm[2] = *reinterpret_cast<const f32x4 *>(rb + 16);
          rm[3] = *reinterpret_cast<const f32x4 *>(rb + 20);
        }
        auto fma4 = [&](float4 &g, float wv, const float4 &u) { g.x = fmaf(wv, u.x, g.x); g.y = fmaf(wv, u.y, g.y); g.z = fmaf(wv, u.z, g.z); g.w = fmaf(wv, u.w, g.w); };
        auto add_row = [&](unsigned la, float wa) {
          const float *ra = secr + la * SEC_STRIDE + 8 * hf;
          const float4 u0 = *reinterpret_cast<const float4 *>(ra), u1 = *reinterpret_cast<const float4 *>(ra + 4);
          const float4 u2 = *reinterpret_cast<const float4 *>(ra + 16), u3 = *reinterpret_cast<const float4 *>(ra + 20);
          fma4(g0, wa, u0); fma4(g1, wa, u1); fma4(g2, wa, u2); fma4(g3, wa, u3);
        };
        add_row(ag_locs & 0xffu, ag_vals[0]);
        add_row((ag_locs >> 8) & 0xffu, ag_vals[1]);
        if (inc_width > 2) {
          add_row((ag_locs >> 16) & 0xffu, ag_vals[2]);
          add_row(ag_locs >> 24, ag_vals[3]);
        }
        if (flags & ELL_FLAG_INC_OVF)      // rows with more than four incident rows
          for (int p = ovf_ptr[lr]; p < ovf_ptr[lr + 1]; ++p) add_row((unsigned)ovf_loc[p], ovf_val[p]);
        split8(g0, g1, dh[KX32], dl[KX32]);
        split8(g2, g3, dh[KX32 + 1], dl[KX32 + 1]);
#pragma unroll
        for (int t = KX32; t < KT32; ++t)
#pragma unroll
          for (int m = 0; m < MB32; ++m) acc[m] = mfma3_32(wh[t][m], wl[t][m], dh[t], dl[t], acc[m]);
        // attention scalars: this lane holds 32 of the row's 64 features, lane l ^ 32 the others
        float ps = 0.f, pn = 0.f;
#pragma unroll
        for (int m = 0; m < MB32; ++m)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            const f32x4 as4 = *reinterpret_cast<const f32x4 *>(attn + 32 * m + 8 * gq + 4 * hf);
            const f32x4 an4 = *reinterpret_cast<const f32x4 *>(attn + FUSED_D + 32 * m + 8 * gq + 4 * hf);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              ps = fmaf(acc[m][4 * gq + q], as4[q], ps);
              pn = fmaf(acc[m][4 * gq + q], an4[q], pn);
            }
          }
        ps += __shfl_xor(ps, 32);
        pn += __shfl_xor(pn, 32);
        if (valid) {
          if (hf == 0) {
            ssw[lrow] = ps;
            snw[lrow] = pn;
          }
#pragma unroll
          for (int m = 0; m < MB32; ++m)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {      // 16-byte chunk 8 m + 2 gq + hf of the row, XOR (row & 7): the layout k_fused_tile's P2 writes
              const f32x4 o = {acc[m][4 * gq], acc[m][4 * gq + 1], acc[m][4 * gq + 2], acc[m][4 * gq + 3]};
              *reinterpret_cast<f32x4 *>(hxw + lrow * FUSED_D + (((8 * m + 2 * gq + hf) ^ (lrow & 7)) << 2)) = o;
            }
        }
      }
      WS_STAMP(1);
      lds_barrier();      // hx / scores of snapshot k are in LDS (and the X team's sec rows of snapshot k + 1)
      WS_STAMP(2);
    }
    WS_DUMP();
  } else {
    // =========================== X team: P1 and P3 ===========================
    __builtin_amdgcn_s_setprio(WS_XPRIO);      // the longer instruction stream of the two, and the younger half of the workgroup (-2 %)
    // P1 on v_mfma_f32_32x32x16_bf16 too: half as many matrix instructions in this team's (issue-bound) stream.  32-row blocks
    // blk = xw + NX j; lane l: n = l & 31 the row, hf = l >> 5: piece i of the row = floats 16 (i >> 1) + 8 hf + 4 (i & 1).
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    constexpr int KS32 = FS / 16, SJ32 = (8 + NX - 1) / NX;      // 4 k-steps; 32-row secondary blocks per X wave (q_cap <= 256)
    const int n32 = lane & 31, hf = lane >> 5;
    // trip 1, X's part: this lane's row ids from the tile's block in global memory (a clamped row -- and the word in front of the
    // section, should it be empty -- lies inside the block), then the weights into the registers they stay in
    issue_block();
    int sec_id[SJ32];
#pragma unroll
    for (int j = 0; j < SJ32; ++j) sec_id[j] = gblk[off.sec + min((xw + NX * j) * 32 + n32, n_sec - 1)];
    bf16x8 w1h[KS32], w1l[KS32];      // 32 VGPRs
#pragma unroll
    for (int t = 0; t < KS32; ++t) {
      w1h[t] = __builtin_bit_cast(bf16x8, S_.w_small32[(t * 2 + 0) * 64 + lane]);
      w1l[t] = __builtin_bit_cast(bf16x8, S_.w_small32[(t * 2 + 1) * 64 + lane]);
    }
    block_to_lds();
    unsigned srow[SJ32];              // BYTE offsets of this lane's rows
#pragma unroll
    for (int j = 0; j < SJ32; ++j) srow[j] = ((unsigned)sec_id[j] * FS + 8u * hf) * 4u;
    f32x4 sp[SJ32][2 * KS32];         // the secondary rows of the snapshot P1 multiplies next (asm loads: see the header)
    auto load_sec_at = [&](const float *base) __attribute__((always_inline)) {      // unconditional (rows are clamped): a fixed number of loads
      static_for<SJ32>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        ws_gld16<0>(sp[j][0], base, srow[j]);
        ws_gld16<16>(sp[j][1], base, srow[j]);
        ws_gld16<64>(sp[j][2], base, srow[j]);
        ws_gld16<80>(sp[j][3], base, srow[j]);
        ws_gld16<128>(sp[j][4], base, srow[j]);
        ws_gld16<144>(sp[j][5], base, srow[j]);
        ws_gld16<192>(sp[j][6], base, srow[j]);
        ws_gld16<208>(sp[j][7], base, srow[j]);
      });
    };
    auto load_sec = [&](int s) __attribute__((always_inline)) { load_sec_at(S_.sec_in + s * sec_stride); };
    // P3 in the OCTET layout: 8 lanes x 2 float4 per output row, 8 rows per wave-instruction (ro = lane >> 3, c8 = lane & 7 owns
    // features 4 c8 .. + 3 and 32 + 4 c8 .. + 3: the two 16-byte pieces sit 128 B apart in a swizzled hx row, ONE address).
    // Against 16 lanes x float4 (k_fused_tile, and the form this kernel started with) every instruction of the softmax
    // prologue and of the output epilogue covers twice the rows, and a neighbour slot costs 7 vector + 2 LDS instructions per
    // 8 rows instead of 10 + 2.  Lane c8 of a row scores neighbour slots c8 and (rows with more than eight neighbours: 7 %
    // of the line graph at the headline, none of the shipped networks) c8 + 8.  The LDS byte offsets of slots 0..7 are
    // static per tile: every lane keeps its own eight as 16-bit halves of four registers (p3_pk); slot K's weight reaches
    // the row's lanes by two bank-masked DPP row broadcasts.  The second slot set goes through ds_bpermute instead (the
    // LDS crossbar).  Rows are degree-sorted inside the tile and dealt in octets: unit u (0..3) of wave xw -> octet NX u + xw.
    const int ro = lane >> 3, c8 = lane & 7, hf8 = ro & 1;      // hf8: which 128-B half of a row this lane takes first (see phase3o)
    // trip 2, X's part: the first snapshot's rows, then the NodeEdge gather; the static P3 state below (LDS reads and ballots on the
    // tile block) is computed while both are in flight
    if (n_snap > 0) load_sec(s_begin);
    gather_issue();
    int p3_dmax[U];
    unsigned p3_pk[U][4];      // (the row's output row is re-read from the tile block per snapshot: registers are short)
    unsigned p3_jb4 = 0;          // this lane's own slot byte of the four octets, 8 bits each: the index of the score it gathers
    int n_st = 0;                 // output-store instructions this wave issues per snapshot (two per octet that has a row)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = 8 * (NX * u + xw) + ro;
      const int ic = min(i, n_own - 1);
      int dmx;
      if (flags & ELL_FLAG_LONG_ROWS) {
        dmx = i < n_own ? adj_ptr[ic + 1] - adj_ptr[ic] : 0;
      } else {
        const unsigned long long m0 = __ballot(i < n_own && adj_b[ic * ELL_ADJ + c8] != 0xFF);
        const unsigned long long m1 = __ballot(i < n_own && adj_b[ic * ELL_ADJ + 8 + c8] != 0xFF);
        dmx = __builtin_popcountll((m0 >> (8 * ro)) & 0xffull) + __builtin_popcountll((m1 >> (8 * ro)) & 0xffull);
      }
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) dmx = max(dmx, __shfl_xor(dmx, o));
      p3_dmax[u] = __builtin_amdgcn_readfirstlane(dmx);
#pragma unroll
      for (int k2 = 0; k2 < 4; ++k2) {
        unsigned pk = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned jb = adj_b[ic * ELL_ADJ + 2 * k2 + h];
          const unsigned j = (i < n_own && jb != 0xFFu) ? jb : 0u;
          pk |= (j * (FUSED_D * 4) + (((j & 7) ^ c8) << 4)) << (16 * h);      // < 2^16: q_cap <= 256 rows of 256 B
        }
        p3_pk[u][k2] = pk;
      }
      p3_jb4 |= (i < n_own ? (unsigned)adj_b[i * ELL_ADJ + c8] : 0xFFu) << (8 * u);
      if (8 * (NX * u + xw) < n_own) n_st += 2;
    }
    const float *bias_l = attn + 2 * FUSED_D + FUSED_H + 4 * c8;      // + 32 hf8 / + 32 - 32 hf8 for the lane's first / second piece      // the output bias, read back per snapshot (registers are short)
    gather_land();
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): drain the set-up loads on every path (see the Y team's note)

    // ---------------- P1: secondary MLP, registers -> MFMA (32x32x16) -> sec ----------------
    auto phase1 = [&](int buf) __attribute__((always_inline)) {
      float *secw = sec + buf * sec_buf;
      static_for<SJ32>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        const int blk = xw + NX * j;
        if (blk * 32 < n_sec) {
          f32x16 acc;
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {      // bias of this lane's features (r & 3) + 8 (r >> 2) + 4 hf
            const f32x4 b4 = *reinterpret_cast<const f32x4 *>(attn + 2 * FUSED_D + 8 * gq + 4 * hf);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[4 * gq + q] = b4[q];
          }
          static_for<KS32>([&](auto t_) {
            constexpr int t = decltype(t_)::value;
            const f32x4 u0 = sp[j][2 * t], u1 = sp[j][2 * t + 1];
            bf16x8 dh, dl;
            split8(make_float4(u0[0], u0[1], u0[2], u0[3]), make_float4(u1[0], u1[1], u1[2], u1[3]), dh, dl);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1h[t], dl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1l[t], dh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1h[t], dh, acc, 0, 0, 0);
          });
          const int lrow = blk * 32 + n32;
          if (lrow < n_sec) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              f32x4 o;
#pragma unroll
              for (int q = 0; q < 4; ++q) o[q] = fused_act<ACT>(acc[4 * gq + q], a.act);
              *reinterpret_cast<f32x4 *>(secw + lrow * SEC_STRIDE + 8 * gq + 4 * hf) = o;
            }
          }
        }
      });
    };
    auto pin_rows = [&]() __attribute__((always_inline)) {
      static_for<SJ32>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        ws_pin4(sp[j][0], sp[j][1], sp[j][2], sp[j][3]);
        ws_pin4(sp[j][4], sp[j][5], sp[j][6], sp[j][7]);
      });
    };

    // first snapshot: rows (requested in trip 2) -> registers -> P1 -> sec[0]; the second snapshot's rows into the registers
    if (n_snap > 0) {
      ws_vmcnt(0);
      pin_rows();
      phase1(0);
      if (n_snap > 1) load_sec(s_begin + 1);
    }
    WS_STAMP(0);
    lds_barrier();

    // ---------------- P3 (octets): segmented softmax + neighbour sum -> HBM, the wave's four octets in one pass ----------------
    auto phase3o = [&](float *out_snap, int buf) __attribute__((always_inline)) {      // out_snap: the snapshot's (n_prim_glob, 64) output
      const float *hxr = hx + buf * hx_buf;
      const float *ssr = s_self + buf * a.p_cap, *snr = s_nbr + buf * a.p_cap;
      int d0 = p3_dmax[0], d1 = p3_dmax[1], d2 = p3_dmax[2], d3 = p3_dmax[3];
      asm volatile("" : "+s"(d0), "+s"(d1), "+s"(d2), "+s"(d3));      // keep the slot tests on the scalar unit
      const int e3 = d3, e2 = max(e3, d2), e1 = max(e2, d1), e0 = max(e1, d0);
      if (e0 == 0) return;            // this wave has no row in the tile

      float ss[U], lg0[U], lg1[U], w0[U], w1[U], den[U];
      bool ok[U], has0[U], has1[U];
      unsigned jb0[U], jb1[U];
      int joff1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = 8 * (NX * u + xw) + ro < n_own;
        // every LDS read of this prologue is unconditional (a row past n_own reads some other word of the tile block, a missing
        // slot the score of row 255; the selects below discard both): under a condition the compiler branches around each read
        // and waits for it alone
        jb0[u] = (p3_jb4 >> (8 * u)) & 0xFFu;      // static per tile (one packed register): no LDS round trip in front of the score gather
        ss[u] = ssr[8 * (NX * u + xw) + ro];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) has0[u] = ok[u] && jb0[u] != 0xFFu;
      f32x4 acc0[U], acc1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) acc0[u] = acc1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e0 <= 16) {
        const bool ext = e0 > 8;      // some row of this wave has more than eight neighbours: the second slot set takes part
        float sn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) sn[u] = snr[jb0[u]];
        asm volatile("" : "+v"(sn[0]), "+v"(sn[1]), "+v"(sn[2]), "+v"(sn[3]));
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float sv = ss[u] + sn[u];
          lg0[u] = has0[u] ? fmaxf(sv, 0.2f * sv) : -INFINITY;      // leaky_relu(0.2)
        }
        float mx[U];
        row8_max4(lg0, mx);
        if (ext) {
          float m1[U];
#pragma unroll
          for (int u = 0; u < U; ++u) jb1[u] = adj_b[(8 * (NX * u + xw) + ro) * ELL_ADJ + 8 + c8];
          asm volatile("" : "+v"(jb1[0]), "+v"(jb1[1]), "+v"(jb1[2]), "+v"(jb1[3]));
#pragma unroll
          for (int u = 0; u < U; ++u) sn[u] = snr[jb1[u]];
          asm volatile("" : "+v"(sn[0]), "+v"(sn[1]), "+v"(sn[2]), "+v"(sn[3]));
#pragma unroll
          for (int u = 0; u < U; ++u) {
            has1[u] = ok[u] && jb1[u] != 0xFFu;
            const int j1 = has1[u] ? (int)jb1[u] : 0;
            joff1[u] = j1 * (FUSED_D * 4) + ((j1 & 7) << 4);
            const float sv = ss[u] + sn[u];
            lg1[u] = has1[u] ? fmaxf(sv, 0.2f * sv) : -INFINITY;
          }
          row8_max4(lg1, m1);
#pragma unroll
          for (int u = 0; u < U; ++u) mx[u] = fmaxf(mx[u], m1[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) w0[u] = has0[u] ? __builtin_amdgcn_exp2f(lg0[u] - mx[u]) : 0.f;
        row8_sum4(w0, den);
        if (ext) {
          float d1s[U];
#pragma unroll
          for (int u = 0; u < U; ++u) w1[u] = has1[u] ? __builtin_amdgcn_exp2f(lg1[u] - mx[u]) : 0.f;
          row8_sum4(w1, d1s);
#pragma unroll
          for (int u = 0; u < U; ++u) den[u] += d1s[u];
        }
        typedef const __attribute__((address_space(3))) f32x4 *lds_f4;
        // the first piece a lane reads is the 128-B half `hf8` of the neighbour's row, the second the other one: the 16 lanes
        // ds_read_b128 serves per LDS cycle hold two rows' low-numbered and two rows' high-numbered lanes, and rows of
        // opposite parity among them -- both halves of the 256-B bank row are in use, as in the 16-lane layout
        const unsigned hxa0 = lds_addr(hxr) + 128 * hf8, hxa1 = lds_addr(hxr) + 128 - 128 * hf8;
        const int cx = c8 << 4;                        // this lane's first 16-byte piece as a byte offset inside a row
        const int bp = (lane & 56) << 2;               // ds_bpermute address of lane 0 of this row's octet
        using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>;
        // slots K .. K + Wd - 1 (0 <= K < 8) of slot set SET for the first A octets of the wave
        auto step = [&](auto SET_, auto K_, auto A_) __attribute__((always_inline)) {
          constexpr int SET = decltype(SET_)::value, K = decltype(K_)::value, A = decltype(A_)::value,
                        Wd = (8 - K < WS_OCT_WD ? 8 - K : WS_OCT_WD);
          constexpr int G = WS_OCT_GRP;           // octets per batch of reads (registers: 8 x G x Wd for the pieces)
          static_for<(A + G - 1) / G>([&](auto g_) {
            constexpr int u0 = decltype(g_)::value * G, GA = (A - u0 < G ? A - u0 : G);
            f32x4 h0[GA][Wd], h1[GA][Wd];
            static_for<GA>([&](auto u_) {
              constexpr int ul = decltype(u_)::value, u = u0 + ul;
              static_for<Wd>([&](auto i_) {
                constexpr int i = decltype(i_)::value, k = K + i;
                unsigned ad = 0;
                if (SET) ad = (unsigned)__builtin_amdgcn_ds_bpermute(bp + 4 * k, joff1[u]) ^ cx;
                unsigned ad0, ad1;
                if (SET) {
                  ad0 = ad + hxa0;
                  ad1 = ad + hxa1;
                } else {                 // half k & 1 of the packed pair + the buffer's base in one instruction (ws_add_half)
                  ad0 = ws_add_half<k & 1>(p3_pk[u][k >> 1], hxa0);
                  ad1 = ws_add_half<k & 1>(p3_pk[u][k >> 1], hxa1);
                }
                h0[ul][i] = *(lds_f4)(uintptr_t)ad0;
                h1[ul][i] = *(lds_f4)(uintptr_t)ad1;
              });
            });
            static_for<GA>([&](auto u_) {
              constexpr int ul = decltype(u_)::value, u = u0 + ul;
              static_for<Wd>([&](auto i_) {
                constexpr int i = decltype(i_)::value, k = K + i;
                float wv;
                if (SET) wv = __int_as_float(__builtin_amdgcn_ds_bpermute(bp + 4 * k, __float_as_int(w1[u])));
                else {     // lane k of the octet: row broadcast of lane k into the low eight lanes of every 16, of lane 8 + k into the high eight
                  const int wi = __float_as_int(w0[u]);
                  int t = __builtin_amdgcn_update_dpp(wi, wi, 0x150 + k, 0xf, 0xf, true);      // every lane written: no `old` to set up
                  t = __builtin_amdgcn_update_dpp(t, wi, 0x150 + 8 + k, 0xf, 0xc, false);
                  wv = __int_as_float(t);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  acc0[u][q] = fmaf(wv, h0[ul][i][q], acc0[u][q]);
                  acc1[u][q] = fmaf(wv, h1[ul][i][q], acc1[u][q]);
                }
              });
            });
          });
        };
        static_for<(8 + WS_OCT_WD - 1) / WS_OCT_WD>([&](auto t_) {                  // slot set 0: slots 0..7, WS_OCT_WD per step
          constexpr int K = decltype(t_)::value * WS_OCT_WD;
          using IK = std::integral_constant<int, K>;
          using S0 = std::integral_constant<int, 0>;
          if (K < e3) step(S0{}, IK{}, I4{});
          else if (K < e2) step(S0{}, IK{}, I3{});
          else if (K < e1) step(S0{}, IK{}, I2{});
          else if (K < e0) step(S0{}, IK{}, I1{});
        });
        if (ext)
          static_for<(8 + WS_OCT_WD - 1) / WS_OCT_WD>([&](auto t_) {                // slot set 1: slots 8..15
            constexpr int K = decltype(t_)::value * WS_OCT_WD;
            using IK = std::integral_constant<int, K>;
            using S1 = std::integral_constant<int, 1>;
            if (K + 8 < e3) step(S1{}, IK{}, I4{});
            else if (K + 8 < e2) step(S1{}, IK{}, I3{});
            else if (K + 8 < e1) step(S1{}, IK{}, I2{});
            else if (K + 8 < e0) step(S1{}, IK{}, I1{});
          });
      } else {   // some row has more than 16 neighbours: every lane walks its row's whole list (tiles with ELL_FLAG_LONG_ROWS)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = 8 * (NX * u + xw) + ro;
          const int b0 = i < n_own ? adj_ptr[i] : 0;
          const int dg = i < n_own ? adj_ptr[i + 1] - b0 : 0;
          float mx = -INFINITY;
          for (int p = b0; p < b0 + dg; ++p) mx = fmaxf(mx, leaky02(ss[u] + snr[adj_loc[p]]));
          den[u] = 0.f;
          for (int p = b0; p < b0 + dg; ++p) {
            const int jj = adj_loc[p];
            const float wv = __builtin_amdgcn_exp2f(leaky02(ss[u] + snr[jj]) - mx);
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(hxr + jj * FUSED_D + 32 * hf8 + ((c8 ^ (jj & 7)) << 2));
            const f32x4 v1 = *reinterpret_cast<const f32x4 *>(hxr + jj * FUSED_D + 32 - 32 * hf8 + ((c8 ^ (jj & 7)) << 2));
            den[u] += wv;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc0[u][q] = fmaf(wv, v0[q], acc0[u][q]);
              acc1[u][q] = fmaf(wv, v1[q], acc1[u][q]);
            }
          }
        }
      }
      // Epilogue.  The six LDS reads it needs (bias pieces, the four output row ids) are issued together and waited for once, and the
      // snapshot's output base is formed once: written the plain way the compiler put an id read + its wait, a reload of the output
      // pointer from the kernel arguments and a 64-bit multiply inside each of the four exec-masked store branches -- five dependent
      // round trips per snapshot.
      f32x4 bo0 = *reinterpret_cast<const f32x4 *>(bias_l + 32 * hf8), bo1 = *reinterpret_cast<const f32x4 *>(bias_l + 32 - 32 * hf8);
      int pid[U];
#pragma unroll
      for (int u = 0; u < U; ++u) pid[u] = prim_ids[8 * (NX * u + xw) + ro];      // rows past n_own: some other word of the tile block, unused
      asm volatile("" : "+v"(pid[0]), "+v"(pid[1]), "+v"(pid[2]), "+v"(pid[3]), "+v"(bo0), "+v"(bo1));
      float *out_s = out_snap + (4 * c8 + 32 * hf8);
      const int o1_off = 32 - 64 * hf8;      // the second piece relative to the first
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u]) {
          const float inv = __builtin_amdgcn_rcpf(den[u]);
          f32x4 o0, o1;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            o0[q] = fused_act<ACT>(fmaf(acc0[u][q], inv, bo0[q]), a.act);
            o1[q] = fused_act<ACT>(fmaf(acc1[u][q], inv, bo1[q]), a.act);
          }
          float *orow = out_s + (int64_t)pid[u] * FUSED_D;
          *reinterpret_cast<f32x4 *>(orow) = o0;
          *reinterpret_cast<f32x4 *>(orow + o1_off) = o1;
        }
      }
    };
    // the base of the rows requested next and of the snapshot P3 writes next, as running pointers: formed from the kernel arguments
    // inside the loop, each costs a scalar load + s_waitcnt lgkmcnt(0) per interval -- a wait that also drains the wave's LDS queue
    const float *sec_next = S_.sec_in + (int64_t)(s_begin + 2) * sec_stride;
    float *out_next = S_.out + (int64_t)s_begin * S_.n_prim_glob * FUSED_D;
    const int64_t out_stride = (int64_t)S_.n_prim_glob * FUSED_D;
    for (int k = 0; k <= n_snap; ++k) {
      if (k + 1 < n_snap) {
        // the rows of snapshot k + 1 were requested in interval k - 1, right after its P1; the only younger vector-memory
        // operations of this wave are the output stores of THAT interval's P3 -- which exists from interval 1 on.  (k >= 1
        // here was a race found by the C3-size repeatability test: interval 0 stores nothing, so in interval 1 vmcnt(n_st)
        // let n_st of the sixteen row loads themselves stay in flight.)
        ws_vmcnt(k >= 2 ? n_st : 0);
        pin_rows();
        phase1((k + 1) & 1);
        if (k + 2 < n_snap) load_sec_at(sec_next);
        sec_next += sec_stride;
      }
      WS_STAMP(3);
      if (k >= 1) {
        phase3o(out_next, (k - 1) & 1);
        out_next += out_stride;
        WS_STAMP(4);
      }
      WS_STAMP(1);
      lds_barrier();
      WS_STAMP(2);
    }
    WS_DUMP();
  }
}

}  // namespace uds
