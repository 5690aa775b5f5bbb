// libuds_hip.so -- C ABI + launchers (gfx950 only).  Kernels live in kernels_*.hpp.
// Interface contract and the reference call sites each entry replaces: include/uds_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/uds_hip.h"
#include <cstdlib>

#include "kernels_dense.hpp"
#include "kernels_sparse.hpp"
#include "kernels_pool.hpp"
#include "kernels_backward.hpp"
#include "kernels_fused.hpp"
#include "kernels_fused_ws.hpp"
#include "kernels_rowgemm.hpp"
#include "kernels_wgrad.hpp"
#include "kernels_node_edge_wgrad.hpp"
#include "kernels_conv_stream.hpp"
#include "kernels_conv_stack.hpp"
#include "kernels_fused128.hpp"
#include "kernels_gemm.hpp"
#include "kernels_remainder_snapshot.hpp"
#include "kernels_recurrent.hpp"
#include "kernels_recurrent_bwd.hpp"
#include "kernels_tail.hpp"
#include "kernels_fit_tail.hpp"
#include "kernels_optim.hpp"
#include "kernels_data.hpp"
#include "kernels_mpc.hpp"
#include "tile_plan.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// The tail of an entry that ends in a launch: UDS_OK, or UDS_EHIP with the entry's name and the runtime's text.
int launched(const char *entry, hipError_t e) {
  if (e != hipSuccess) return fail(UDS_EHIP, "%s: launch -> %s", entry, hipGetErrorString(e));
  return UDS_OK;
}

#define UDS_HIP_TRY(call)                                                             \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) return fail(UDS_EHIP, "%s -> %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define UDS_REQUIRE(cond, ...) \
  do {                         \
    if (!(cond)) return fail(UDS_EINVAL, __VA_ARGS__); \
  } while (0)

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int64_t align4(int64_t floats) { return (floats + 3) & ~int64_t(3); }  // keep 16-B carve offsets

}  // namespace

struct uds_csr {
  int64_t n_rows = 0, n_cols = 0, nnz = 0;
  int32_t max_degree = 0;
  int32_t *d_rowptr = nullptr, *d_col = nullptr, *d_order = nullptr, *d_rowidx = nullptr;   // rowidx: row of every entry
  std::vector<int32_t> h_order;
  uds::HostCsr host;   // kept for the tile planner
};

struct uds_tile_plan {
  uds::NetworkPlan plan;
};

// One tile plan per input width class: the DMA stage holds raw rows, so wider rows need smaller tiles.
struct uds_plan_slot {
  bool built = false;             // planning was attempted
  bool ok = false;                // a tile plan that fits the LDS budget exists
  int fp = 0, fs = 0;             // primary / secondary row widths (floats) of the kernel variant the plan was sized for
  uds::NetworkPlan plan;
  int32_t *d_hdr = nullptr, *d_pool = nullptr;
  int32_t *d_hdr_side[2] = {nullptr, nullptr};   // headers of one side's tiles only (same pool): single-side launches
  // k_fused_tile: header + metadata of every tile as one fixed-stride block (tile_block_ints(meta_cap) ints), so a workgroup
  // fetches both in ONE round trip without knowing the header first; one array per tile list
  int32_t *d_blocks = nullptr, *d_blocks_side[2] = {nullptr, nullptr};
  int blk_cap = 0;                // ints per tile block of k_fused_tile (tile_plan.hpp: ell_block_cap)
  int64_t lds_bytes = 0;
};

struct uds_network {
  const uds_csr *adj = nullptr, *edge_adj = nullptr, *inc_n = nullptr, *inc_e = nullptr;
  uds_plan_slot slot[7];          // d = 64 variants <FP, FS>: [0] <64,64>, [1] <64,96>, [2] <96,64>, [3] <96,96>; d = 128: [4] <128,128>, [5] <128,64>, [6] <64,128>
};

namespace {

constexpr int64_t FUSED_LDS_BUDGET = 160 * 1024;   // one 8-wave workgroup per CU owns the whole 160 KiB LDS
constexpr int WS_BIG32_OFF = 2 * (768 + 2048), WS_BIG32_LEN = 6 * 2 * 2 * 64;      // uint4: behind the four 16x16x32-order kernels of a d = 64 layer
constexpr int WS_SMALL32_OFF = WS_BIG32_OFF + 2 * WS_BIG32_LEN, WS_SMALL32_LEN = 4 * 1 * 2 * 64;
constexpr int64_t PACKED_WEIGHT_FLOATS = 2 * (2048 + 6144) * 4;   // both sides at d = 128 (128->64 and 192->128 kernels): uint4 = 4 floats

inline int slot_index(int fp, int fs) {
  if (fp == 128 || fs == 128) return fp == 128 ? (fs == 128 ? 4 : 5) : 6;      // the d = 128 kernel's variants
  return (fp > 64 ? 2 : 0) + (fs > 64 ? 1 : 0);
}

// the wave-specialised d = 64 kernel (k_fused_ws) can hold this plan's tiles; uds_network_plan_info reports it as bit 32
inline bool ws_plan_ok(const uds_plan_slot &u) {
  return uds::fused_ws_lds_bytes(u.plan.p_cap, u.plan.q_cap, u.blk_cap) <= FUSED_LDS_BUDGET && u.plan.p_cap <= 128 && u.plan.q_cap <= 256;
}

// Tile plan for the kernel variant <fp, fs> (primary / secondary input rows of fp / fs floats: they set the size of the
// DMA stage) under the LDS budget: fix the footprint limits (primary / secondary rows staged per tile, multiples of 16)
// first; the planner then fills them (tile_plan.hpp: merge_clusters, TileRefiner).
bool plan_network(const uds::HostCsr &adj, const uds::HostCsr &eadj, const uds::HostCsr &inc_n, const uds::HostCsr &inc_e,
                  int fp, int fs, uds::NetworkPlan &out, int64_t &lds, int &blk_cap) {
  // candidate (p_limit, q_limit) pairs, largest first; meta is bounded by the limits (checked after planning)
  const int cand[][2] = {{128, 208}, {128, 192}, {128, 176}, {128, 160}, {128, 144}, {112, 160}, {112, 144}, {96, 144}, {96, 128},
                         {80, 128}, {64, 96}, {48, 64}, {32, 48}, {16, 32}};
  for (const auto &c : cand) {
    int p_lim = c[0], q_lim = c[1];
#ifdef UDS_KNOBS
    if (const char *ov = std::getenv("UDS_PLIM")) p_lim = std::min(p_lim, std::atoi(ov));      // experiment builds: smaller tiles
    if (const char *ov = std::getenv("UDS_QLIM")) q_lim = std::min(q_lim, std::atoi(ov));
#endif
    if (uds::fused_lds_bytes(p_lim, q_lim, 0, uds::FUSED_H, uds::FUSED_D, fp, fs) > FUSED_LDS_BUDGET) continue;
    const int t = std::min(p_lim, 4 * uds::FUSED_WAVES * uds::FUSED_U);        // own rows: P3 covers a tile in one trip
    out = uds::build_network_plan(adj, eadj, inc_n, inc_e, t, t, p_lim, q_lim);
    blk_cap = uds::ell_block_cap(out.hdr, out.pool, out.n_tiles);      // the kernel's tile blocks: fixed-width index lists
    if (blk_cap < 0) continue;                                           // a tile beyond the byte-wide local indices (a hub row)
    lds = uds::fused_lds_bytes(out.p_cap, out.q_cap, blk_cap, uds::FUSED_H, uds::FUSED_D, fp, fs);
    if (lds <= FUSED_LDS_BUDGET && out.p_cap <= 4 * uds::FUSED_WAVES * uds::FUSED_U) return true;   // P3 covers a tile in one trip
  }
  return false;
}

// Tile plan of the d = 128 kernel (k_fused128): <= 64 own / primary rows, secondary rows as the LDS allows.
bool plan_network128(const uds::HostCsr &adj, const uds::HostCsr &eadj, const uds::HostCsr &inc_n, const uds::HostCsr &inc_e, int fp, int fs,
                     uds::NetworkPlan &out, int64_t &lds) {
  const int cand[][2] = {{64, 128}, {64, 112}, {64, 96}, {64, 80}, {64, 64}, {48, 64}, {32, 48}, {16, 32}};
  for (const auto &c : cand) {
    const int p_lim = c[0], q_lim = c[1];
    if (uds::fused128_lds_bytes(p_lim, q_lim, 0, fp, fs) > FUSED_LDS_BUDGET) continue;
    const int t = std::min(p_lim, 4 * uds::FUSED_WAVES * uds::F128_U);
    out = uds::build_network_plan(adj, eadj, inc_n, inc_e, t, t, p_lim, q_lim);
    lds = uds::fused128_lds_bytes(out.p_cap, out.q_cap, out.meta_cap, fp, fs);
    if (lds <= FUSED_LDS_BUDGET && out.p_cap <= 4 * uds::FUSED_WAVES * uds::F128_U) return true;
  }
  return false;
}

}  // namespace

namespace {

template <int FP, int FS, int ACT>
hipError_t launch_fused128_act(const uds::FusedArgs &a, int grid, int64_t lds, hipStream_t st) {
  static unsigned long long attr_done = 0;
  if (hipError_t e = uds::set_max_lds_once(reinterpret_cast<const void *>(&uds::k_fused_cs<128, FP, FS, uds::FUSED_WAVES, ACT>), (int)FUSED_LDS_BUDGET, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((uds::k_fused_cs<128, FP, FS, uds::FUSED_WAVES, ACT>), dim3(grid), dim3(uds::FUSED_WAVES * 64), (size_t)lds, st, a);
  return hipGetLastError();
}

template <int FP, int FS>
hipError_t launch_fused128(const uds::FusedArgs &a, int grid, int64_t lds, hipStream_t st) {
  if (a.act == UDS_ACT_RELU) return launch_fused128_act<FP, FS, UDS_ACT_RELU>(a, grid, lds, st);
  return launch_fused128_act<FP, FS, -1>(a, grid, lds, st);
}

template <int FP, int FS, int ACT>
hipError_t launch_fused_act(const uds::FusedArgs &a, int grid, int64_t lds, hipStream_t st) {
  static unsigned long long attr_done = 0;
  if (hipError_t e = uds::set_max_lds_once(reinterpret_cast<const void *>(&uds::k_fused_tile<FP, FS, ACT>), (int)FUSED_LDS_BUDGET, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((uds::k_fused_tile<FP, FS, ACT>), dim3(grid), dim3(uds::FUSED_WAVES * 64), (size_t)lds, st, a);
  return hipGetLastError();
}

template <int ACT>
hipError_t launch_fused_ws_act(const uds::FusedArgs &a, int grid, int64_t lds, hipStream_t st) {
  static unsigned long long attr_done = 0;
  if (hipError_t e = uds::set_max_lds_once(reinterpret_cast<const void *>(&uds::k_fused_ws<ACT>), (int)FUSED_LDS_BUDGET, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((uds::k_fused_ws<ACT>), dim3(grid), dim3(uds::FUSED_WAVES * 64), (size_t)lds, st, a);
  return hipGetLastError();
}
// the wave-specialised kernel (kernels_fused_ws.hpp): 64-wide rows on both sides, one tensor per side
hipError_t launch_fused_ws(const uds::FusedArgs &a, int grid, int64_t lds, hipStream_t st) {
  if (a.act == UDS_ACT_RELU) return launch_fused_ws_act<UDS_ACT_RELU>(a, grid, lds, st);
  return launch_fused_ws_act<-1>(a, grid, lds, st);
}

// relu (the reference's activation in every shipped model) is compiled in; other activations are decided at run time
template <int FP, int FS>
hipError_t launch_fused(const uds::FusedArgs &a, int grid, int64_t lds, hipStream_t st) {
  if (a.act == UDS_ACT_RELU) return launch_fused_act<FP, FS, UDS_ACT_RELU>(a, grid, lds, st);
  return launch_fused_act<FP, FS, -1>(a, grid, lds, st);
}

// Snapshots of a fused spatial launch are cut into chunks; one workgroup = (tile, chunk).  All working workgroups take about
// the same time (setup ~1.5 snapshots' worth + its snapshots), one per CU at a time, so a launch lasts ~ceil(working / 256)
// rounds: the chunk length that minimises rounds * (setup + chunk), in half snapshots, ties to the shorter chunk.  (Metadata,
// weights and the DMA pipeline are set up once per workgroup, so long chunks are cheap.)
int64_t pick_chunk(int64_t S, int64_t working_tiles) {
  int64_t chunk = S, best = INT64_MAX;
  for (int64_t c = 1; c <= S; ++c) {
    const int64_t rounds = (((S + c - 1) / c) * working_tiles + 255) / 256;
    const int64_t cost = rounds * (3 + 2 * c);
    if (cost < best || (cost == best && c < chunk)) {
      best = cost;
      chunk = c;
    }
  }
  return chunk;
}

// One launch of the fused spatial layer: the kernel (UDS_KERNEL_*) and its variant <fp, fs>, the plan slot it reads, the side
// whose tiles it takes (< 0: the merged list of both sides) and how many those are.
struct fused_launch {
  int kernel, fp, fs, slot, side, n_tiles, side_mask;
};

// The launches of a layer (fx, fe, h, d) on the plans this network holds -> their number, 0 when the fused kernels do not take
// it.  uds_spatial_layer_forward launches what this returns and uds_network_fused_launches reports it.  (Split inputs are
// 64 + 32 columns, so a 64 / 64 or a 128-wide layer never has them: the choice does not depend on how the rows arrive.)
int fused_launches(const uds_network *net, int64_t fx, int64_t fe, int64_t h, int64_t d, fused_launch out[2]) {
  auto put = [&](int i, int kernel, int fp, int fs, int side) {
    const int slot = slot_index(fp, fs);
    const uds::NetworkPlan &pl = net->slot[slot].plan;
    out[i] = fused_launch{kernel, fp, fs, slot, side, side < 0 ? pl.n_tiles : pl.side[side].n_tiles, side < 0 ? 3 : (1 << side)};
  };
  if (h == uds::F128_H && d == uds::F128_D && fx == 128 && (fe == 128 || fe == 64) && net->slot[slot_index(128, (int)fe)].ok &&
      net->slot[slot_index((int)fe, 128)].ok) {
    // d = 128: the column-split fused kernel (kernels_fused128.hpp); 64-wide link rows -> one launch per side
    if (fe == 128) {
      put(0, UDS_KERNEL_FUSED_CS, 128, 128, -1);
      return 1;
    }
    put(0, UDS_KERNEL_FUSED_CS, 128, 64, 0);      // node tiles: 128-wide nodes fed by 64-wide links
    put(1, UDS_KERNEL_FUSED_CS, 64, 128, 1);      // link tiles: 64-wide links fed by 128-wide nodes
    return 2;
  }
  // (rows of one snapshot are addressed with a 32-bit byte offset from a per-snapshot base: N, E < 2^31 / 384)
  const bool shape_ok = h == uds::FUSED_H && d == uds::FUSED_D && (fx == 64 || fx == 96) && (fe == 64 || fe == 96) &&
                        std::max(net->adj->n_rows, net->edge_adj->n_rows) * 384 < ((int64_t)1 << 31);
  // node tiles run the variant <fx, fe>, link tiles <fe, fx>: one launch when they coincide, else one per side
  if (!shape_ok || !net->slot[slot_index((int)fx, (int)fe)].ok || !net->slot[slot_index((int)fe, (int)fx)].ok) return 0;
  if (fx == fe) {
    bool ws = fx == 64 && ws_plan_ok(net->slot[0]);
#ifdef UDS_KNOBS
    if (std::getenv("UDS_NO_WS")) ws = false;      // experiment builds only: k_fused_tile<64, 64> in place of k_fused_ws
#endif
    put(0, ws ? UDS_KERNEL_FUSED_WS : UDS_KERNEL_FUSED_TILE, (int)fx, (int)fe, -1);
    return 1;
  }
  put(0, UDS_KERNEL_FUSED_TILE, (int)fx, (int)fe, 0);      // workgroups go round-robin to the XCDs: a grid of working tiles only keeps the XCDs level
  put(1, UDS_KERNEL_FUSED_TILE, (int)fe, (int)fx, 1);
  return 2;
}

hipError_t pack_weights(const float *W, int K, int F_out, uint4 *out, hipStream_t st) {
  const int total = (K / 32) * (F_out / 16) * 64;
  hipLaunchKernelGGL(uds::k_pack_weight_frags, dim3((total + 255) / 256), dim3(256), 0, st, W, K, F_out, out);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int uds_abi_version(void) { return UDS_ABI_VERSION; }
const char *uds_last_error(void) { return g_err.c_str(); }

int uds_csr_create(const int32_t *rowptr, const int32_t *col, int64_t n_rows, int64_t n_cols,
                   int64_t nnz, uds_csr_t **out) {
  UDS_REQUIRE(out != nullptr, "uds_csr_create: out is NULL");
  *out = nullptr;
  UDS_REQUIRE(rowptr != nullptr && (col != nullptr || nnz == 0), "uds_csr_create: NULL index array");
  UDS_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0 && n_rows < INT32_MAX && nnz < INT32_MAX,
              "uds_csr_create: sizes out of int32 range");
  UDS_REQUIRE(rowptr[0] == 0 && rowptr[n_rows] == nnz, "uds_csr_create: rowptr[0]=%d rowptr[n]=%d nnz=%lld",
              rowptr[0], rowptr[n_rows], (long long)nnz);
  int32_t max_deg = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    UDS_REQUIRE(rowptr[r + 1] >= rowptr[r], "uds_csr_create: rowptr decreases at row %lld", (long long)r);
    max_deg = std::max(max_deg, rowptr[r + 1] - rowptr[r]);
  }
  for (int64_t p = 0; p < nnz; ++p)
    UDS_REQUIRE(col[p] >= 0 && col[p] < n_cols, "uds_csr_create: col[%lld]=%d outside [0,%lld)",
                (long long)p, col[p], (long long)n_cols);
  uds_csr *c = new (std::nothrow) uds_csr;
  if (!c) return fail(UDS_ENOMEM, "uds_csr_create: host allocation failed");
  c->n_rows = n_rows;
  c->n_cols = n_cols;
  c->nnz = nnz;
  c->max_degree = max_deg;
  c->host.n_rows = n_rows;
  c->host.n_cols = n_cols;
  c->host.rowptr.assign(rowptr, rowptr + n_rows + 1);
  c->host.col.assign(col, col + nnz);
  // degree-sorted schedule inside windows of 1024 consecutive rows: descending degree, ties by row index (stable).
  // Windowed so that neighbouring workgroups gather neighbouring rows (L2 hits); a global sort scatters them.
  constexpr int64_t ORDER_WINDOW = 1024;
  c->h_order.resize(n_rows);
  std::iota(c->h_order.begin(), c->h_order.end(), 0);
  for (int64_t r0 = 0; r0 < n_rows; r0 += ORDER_WINDOW)
    std::stable_sort(c->h_order.begin() + r0, c->h_order.begin() + std::min(n_rows, r0 + ORDER_WINDOW), [&](int32_t a, int32_t b) {
      return (rowptr[a + 1] - rowptr[a]) > (rowptr[b + 1] - rowptr[b]);
    });
  auto cleanup = [&](int code) {
    hipFree(c->d_rowptr);
    hipFree(c->d_col);
    hipFree(c->d_order);
    hipFree(c->d_rowidx);
    delete c;
    return code;
  };
  hipError_t e;
  if ((e = hipMalloc(&c->d_rowptr, sizeof(int32_t) * (n_rows + 1))) != hipSuccess ||
      (e = hipMalloc(&c->d_col, sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess ||
      (e = hipMalloc(&c->d_order, sizeof(int32_t) * std::max<int64_t>(n_rows, 1))) != hipSuccess ||
      (e = hipMalloc(&c->d_rowidx, sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess)
    return cleanup(fail(UDS_ENOMEM, "uds_csr_create: hipMalloc -> %s", hipGetErrorString(e)));
  std::vector<int32_t> rowidx((size_t)nnz);
  for (int64_t r = 0; r < n_rows; ++r)
    for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p) rowidx[p] = (int32_t)r;
  if ((e = hipMemcpy(c->d_rowptr, rowptr, sizeof(int32_t) * (n_rows + 1), hipMemcpyHostToDevice)) != hipSuccess ||
      (nnz && (e = hipMemcpy(c->d_rowidx, rowidx.data(), sizeof(int32_t) * nnz, hipMemcpyHostToDevice)) != hipSuccess) ||
      (nnz && (e = hipMemcpy(c->d_col, col, sizeof(int32_t) * nnz, hipMemcpyHostToDevice)) != hipSuccess) ||
      (n_rows && (e = hipMemcpy(c->d_order, c->h_order.data(), sizeof(int32_t) * n_rows, hipMemcpyHostToDevice)) != hipSuccess))
    return cleanup(fail(UDS_EHIP, "uds_csr_create: hipMemcpy -> %s", hipGetErrorString(e)));
  *out = c;
  return UDS_OK;
}

int uds_csr_destroy(uds_csr_t *c) {
  if (!c) return UDS_OK;
  hipFree(c->d_rowptr);
  hipFree(c->d_col);
  hipFree(c->d_order);
  hipFree(c->d_rowidx);
  delete c;
  return UDS_OK;
}

int uds_csr_shape(const uds_csr_t *c, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int32_t *max_degree) {
  UDS_REQUIRE(c != nullptr, "uds_csr_shape: NULL handle");
  if (n_rows) *n_rows = c->n_rows;
  if (n_cols) *n_cols = c->n_cols;
  if (nnz) *nnz = c->nnz;
  if (max_degree) *max_degree = c->max_degree;
  return UDS_OK;
}

int uds_csr_row_order(const uds_csr_t *c, int32_t *out_host) {
  UDS_REQUIRE(c != nullptr && out_host != nullptr, "uds_csr_row_order: NULL argument");
  std::memcpy(out_host, c->h_order.data(), sizeof(int32_t) * c->n_rows);
  return UDS_OK;
}

int uds_dense_act(const float *xa, int64_t fa, const float *xb, int64_t fb, int64_t rows, const float *W,
                  const float *bias, int64_t f_out, int act, const float *a_self, const float *a_nbr,
                  float *out, float *s_self, float *s_nbr, uds_stream_t stream) {
  UDS_REQUIRE(xa && W && out, "uds_dense_act: NULL xa/W/out");
  UDS_REQUIRE(((f_out & 3) != 0 || aligned16(out)), "uds_dense_act: out must be 16-byte aligned");
  UDS_REQUIRE(fa > 0 && fb >= 0 && (fb == 0) == (xb == nullptr), "uds_dense_act: fa=%lld fb=%lld xb=%p inconsistent",
              (long long)fa, (long long)fb, (const void *)xb);
  UDS_REQUIRE(rows >= 0 && f_out > 0 && f_out <= 256 && fa + fb <= 4096, "uds_dense_act: rows=%lld f_out=%lld (max 256) f_in=%lld",
              (long long)rows, (long long)f_out, (long long)(fa + fb));
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_dense_act: unknown activation %d", act);
  const bool attn = a_self != nullptr;
  UDS_REQUIRE(attn == (a_nbr != nullptr) && attn == (s_self != nullptr) && attn == (s_nbr != nullptr),
              "uds_dense_act: a_self/a_nbr/s_self/s_nbr must be given together");
  if (rows == 0) return UDS_OK;
  uds::DenseArgs a{xa, xb, W, bias, a_self, a_nbr, out, s_self, s_nbr, (int)fa, (int)fb, (int)f_out, act, rows};
  return launched("uds_dense_act", uds::launch_dense_act(a, static_cast<hipStream_t>(stream)));
}

int uds_conv1d_causal(const float *x, int64_t B, int64_t T, int64_t R, int64_t F, const float *kernel, const float *bias,
                      int64_t taps, int64_t dil, int64_t H, int act, float *out, uds_stream_t stream) {
  UDS_REQUIRE(x && kernel && out, "uds_conv1d_causal: NULL x/kernel/out");
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0 && F > 0 && taps > 0 && taps <= 16 && dil != 0 && H > 0 && H <= 256 && taps * F <= 4096,
              "uds_conv1d_causal: bad sizes B=%lld T=%lld R=%lld F=%lld taps=%lld dil=%lld H=%lld", (long long)B, (long long)T,
              (long long)R, (long long)F, (long long)taps, (long long)dil, (long long)H);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_conv1d_causal: unknown activation %d", act);
  UDS_REQUIRE(((H & 3) != 0 || aligned16(out)), "uds_conv1d_causal: out must be 16-byte aligned");
  if (B == 0) return UDS_OK;
  uds::DenseArgs a{x, nullptr, kernel, bias, nullptr, nullptr, out, nullptr, nullptr, (int)F, 0, (int)H, act, B * T * R};
  a.taps = (int)taps;
  a.dil = (int)dil;
  a.T = (int)T;
  a.t_rows = (int)R;
  return launched("uds_conv1d_causal", uds::launch_dense_act(a, static_cast<hipStream_t>(stream)));
}

// Host only: what launch_dense_act would launch for this shape (the same uds::dense_route), under the size checks of the two entries
int uds_dense_route(int64_t fa, int64_t fb, int64_t taps, int attn, int64_t f_out, int64_t rows, int wb_aligned, int32_t *info5) {
  UDS_REQUIRE(info5 != nullptr, "uds_dense_route: info5 is NULL");
  UDS_REQUIRE(fa > 0 && fb >= 0 && rows >= 0 && rows <= ((int64_t)1 << 40) && f_out > 0 && f_out <= 256 && fa + fb <= 4096,
              "uds_dense_route: fa=%lld fb=%lld rows=%lld (max 2^40) f_out=%lld (max 256) f_in=%lld (max 4096)", (long long)fa, (long long)fb,
              (long long)rows, (long long)f_out, (long long)(fa + fb));
  UDS_REQUIRE(taps >= 0 && taps <= 16 && (taps == 0 || (fb == 0 && !attn && taps * fa <= 4096)),
              "uds_dense_route: taps=%lld (0 .. 16; a convolution has no xb and no attention scalars, taps * fa = %lld <= 4096)",
              (long long)taps, (long long)(taps * fa));
  const uds::DenseRoute r = uds::dense_route((int)fa, (int)fb, (int)taps, attn != 0, (int)f_out, rows, wb_aligned != 0);
  UDS_REQUIRE(r.blocks <= INT32_MAX, "uds_dense_route: rows=%lld need %lld workgroups, more than a launch grid holds", (long long)rows,
              (long long)r.blocks);
  info5[0] = r.kernel;
  info5[1] = r.param;
  info5[2] = r.rows_per_wg;
  info5[3] = (int32_t)r.blocks;
  info5[4] = (int32_t)r.stride;
  return UDS_OK;
}

int uds_recurrent_fused(const float *x, int64_t F, const void *packed, const float *b_in, const float *b_rec, int64_t B, int64_t T, int64_t R,
                        int kind, float *out, uds_stream_t stream) {
  UDS_REQUIRE(x && packed && out && (F == 0 || b_in), "uds_recurrent_fused: NULL argument");
  UDS_REQUIRE(kind == 0 || kind == 1, "uds_recurrent_fused: kind %d (0 = GRU, 1 = LSTM)", kind);
  const int G = kind == 0 ? 3 : 4;
  UDS_REQUIRE(uds::recurrent_mfma_supported(G, (int)F), "uds_recurrent_fused: input width %lld (64 or 128 where W + U fit the LDS, 0 = given projection)",
              (long long)F);
  UDS_REQUIRE(B >= 0 && T >= 0 && R >= 0, "uds_recurrent_fused: bad sizes B=%lld T=%lld R=%lld", (long long)B, (long long)T, (long long)R);
  UDS_REQUIRE(aligned16(x) && aligned16(out) && aligned16(packed) && aligned16(b_in) && aligned16(b_rec),
              "uds_recurrent_fused: buffers must be 16-byte aligned");
  if (B == 0 || T == 0 || R == 0) return UDS_OK;
  const int64_t n_blocks = (R + 15) / 16;
  UDS_REQUIRE(B * n_blocks < INT32_MAX && T < INT32_MAX, "uds_recurrent_fused: too many rows");
  uds::RecurrentMfmaArgs a{x, b_in, b_rec, reinterpret_cast<const uint4 *>(packed), out, (int)B, (int)T, (int)R, (int)n_blocks};
  return launched("uds_recurrent_fused", uds::launch_recurrent_mfma(a, G, (int)F, static_cast<hipStream_t>(stream)));
}

int uds_recurrent_fused_supported(int64_t F, int kind) { return uds::recurrent_mfma_supported(kind == 0 ? 3 : 4, (int)F) ? 1 : 0; }

int uds_recurrent_forward(const float *xp, const float *U, const float *rb, int64_t B, int64_t T, int64_t R, int64_t H, int kind,
                          float *out, uds_stream_t stream) {
  return uds_recurrent_forward_train(xp, U, rb, B, T, R, H, kind, out, nullptr, stream);
}

int uds_recurrent_forward_train(const float *xp, const float *U, const float *rb, int64_t B, int64_t T, int64_t R, int64_t H, int kind,
                                float *out, float *c_out, uds_stream_t stream) {
  UDS_REQUIRE(xp && U && out, "uds_recurrent_forward: NULL argument");
  UDS_REQUIRE(kind == 0 || kind == 1, "uds_recurrent_forward: kind %d (0 = GRU, 1 = LSTM)", kind);
  UDS_REQUIRE(B >= 0 && T >= 0 && R >= 0 && H > 0 && H <= 256, "uds_recurrent_forward: bad sizes B=%lld T=%lld R=%lld H=%lld", (long long)B,
              (long long)T, (long long)R, (long long)H);
  if (B == 0 || T == 0 || R == 0) return UDS_OK;
  const int G = kind == 0 ? 3 : 4;
  const int rows = (int)std::max<int64_t>(1, 256 / H);
  const size_t lds = ((size_t)H * G * H + (size_t)rows * H) * sizeof(float);
  hipError_t e;
  if (lds <= 160 * 1024) {
    UDS_REQUIRE((B * R + rows - 1) / rows < INT32_MAX, "uds_recurrent_forward: too many rows");
    uds::RecurrentArgs a{xp, U, rb, out, c_out, (int)B, (int)T, (int)R, (int)H, G, rows};
    e = uds::launch_recurrent(a, static_cast<hipStream_t>(stream));
  } else {      // U (H x G*H floats) does not fit the LDS: streamed from global memory, the same arithmetic
    const int srows = uds::recurrent_stream_groups((int)H) * uds::RC_STREAM_RPT;
    UDS_REQUIRE((B * R + srows - 1) / srows < INT32_MAX, "uds_recurrent_forward: too many rows");
    uds::RecurrentArgs a{xp, U, rb, out, c_out, (int)B, (int)T, (int)R, (int)H, G, srows};
    e = uds::launch_recurrent_stream(a, static_cast<hipStream_t>(stream));
  }
  return launched("uds_recurrent_forward", e);
}

// uds_recurrent_backward (64 units: `width` NULL) and uds_recurrent_backward_h (*width units): one set of checks, two launchers
static int recurrent_backward(const char *what, const int64_t *width, const float *xp, const void *packed, const float *b_rec, const float *h,
                              const float *c, const float *gh, int64_t B, int64_t T, int64_t R, int kind, float *dxp, float *darec,
                              uds_stream_t stream) {
  UDS_REQUIRE(xp && packed && h && gh && dxp && darec, "%s: NULL argument", what);
  UDS_REQUIRE(kind == 0 || kind == 1, "%s: kind %d (0 = GRU, 1 = LSTM)", what, kind);
  UDS_REQUIRE(!width || uds::recurrent_bwd_width_ok(*width), "%s: %lld units (a multiple of 16 from 16 to 128)", what, (long long)*width);
  UDS_REQUIRE(kind == 0 || c, "%s: the LSTM needs the cell states of the forward pass (uds_recurrent_forward_train)", what);
  UDS_REQUIRE(B >= 0 && T >= 0 && R >= 0, "%s: bad sizes B=%lld T=%lld R=%lld", what, (long long)B, (long long)T, (long long)R);
  UDS_REQUIRE(aligned16(xp) && aligned16(packed) && aligned16(b_rec) && aligned16(h) && aligned16(c) && aligned16(gh) && aligned16(dxp) &&
                  aligned16(darec), "%s: buffers must be 16-byte aligned", what);
  if (B == 0 || T == 0 || R == 0) return UDS_OK;
  const int64_t n_blocks = (R + 15) / 16;
  UDS_REQUIRE(B * n_blocks < INT32_MAX && T < INT32_MAX, "%s: too many rows", what);
  uds::RecurrentBwdArgs a{xp, b_rec, reinterpret_cast<const uint4 *>(packed), h, c, gh, dxp, darec, (int)B, (int)T, (int)R, (int)n_blocks};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!width) return launched(what, kind == 0 ? uds::launch_recurrent_bwd_t<3>(a, st) : uds::launch_recurrent_bwd_t<4>(a, st));
  return launched(what, kind == 0 ? uds::launch_recurrent_bwd_h<3>(a, (int)*width, st) : uds::launch_recurrent_bwd_h<4>(a, (int)*width, st));
}

int uds_recurrent_backward(const float *xp, const void *packed, const float *b_rec, const float *h, const float *c, const float *gh,
                           int64_t B, int64_t T, int64_t R, int kind, float *dxp, float *darec, uds_stream_t stream) {
  return recurrent_backward("uds_recurrent_backward", nullptr, xp, packed, b_rec, h, c, gh, B, T, R, kind, dxp, darec, stream);
}

int64_t uds_recurrent_bwd_packed_bytes(int64_t H, int kind) {
  if (!uds::recurrent_bwd_width_ok(H) || (kind != 0 && kind != 1)) return 0;
  return (int64_t)2 * (kind == 0 ? 3 : 4) * uds::recurrent_bwd_slice((int)H) * 16;
}

int uds_recurrent_pack_bwd(const float *U, int64_t H, int kind, void *packed, uds_stream_t stream) {
  UDS_REQUIRE(U && packed && aligned16(packed), "uds_recurrent_pack_bwd: NULL / misaligned argument");
  const int64_t bytes = uds_recurrent_bwd_packed_bytes(H, kind);
  UDS_REQUIRE(bytes > 0, "uds_recurrent_pack_bwd: H=%lld kind=%d (H a multiple of 16 from 16 to 128; kind 0 = GRU, 1 = LSTM)", (long long)H, kind);
  const int total = (int)(bytes / 16 / 2);      // one thread per (slice, k-step, block, lane): a hi and a lo fragment
  hipLaunchKernelGGL(uds::k_pack_recurrent_bwd, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), U, (int)H,
                     kind == 0 ? 3 : 4, reinterpret_cast<uint4 *>(packed));
  return launched("uds_recurrent_pack_bwd", hipGetLastError());
}

int uds_recurrent_backward_h(const float *xp, const void *packed, const float *b_rec, const float *h, const float *c, const float *gh,
                             int64_t B, int64_t T, int64_t R, int64_t H, int kind, float *dxp, float *darec, uds_stream_t stream) {
  return recurrent_backward("uds_recurrent_backward_h", &H, xp, packed, b_rec, h, c, gh, B, T, R, kind, dxp, darec, stream);
}

int64_t uds_rowgemm_packed_bytes(int64_t k_total, int64_t f_out) {
  if (k_total <= 0 || k_total % 32 || f_out <= 0 || f_out > 64) return 0;
  return (k_total / 32) * uds::rowgemm_mb((int)f_out) * 2 * 64 * 16;
}

int uds_rowgemm_pack(const float *W, int64_t k_total, int64_t f_out, void *packed, uds_stream_t stream) {
  UDS_REQUIRE(W && packed && aligned16(packed), "uds_rowgemm_pack: NULL / misaligned argument");
  UDS_REQUIRE(uds_rowgemm_packed_bytes(k_total, f_out) > 0, "uds_rowgemm_pack: needs K %% 32 == 0 and f_out <= 64 (K=%lld f_out=%lld)",
              (long long)k_total, (long long)f_out);
  const int mb = uds::rowgemm_mb((int)f_out);
  const int total = (int)(k_total / 32) * mb * 64;
  hipLaunchKernelGGL(uds::k_pack_weight_frags_padded, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), W,
                     (int)k_total, (int)f_out, mb, reinterpret_cast<uint4 *>(packed));
  return launched("uds_rowgemm_pack", hipGetLastError());
}

static int64_t pad_k(int64_t k) { return (k + 63) / 64 * 64; }      // the remainder GEMM's k-step
constexpr int REMAINDER_MAX_PIECES = 512;      // (tile, K piece) pairs of the cut tiles of k_remainder_gemm2: at most two rounds of workgroups

int64_t uds_remainder_packed_bytes(int64_t R, int64_t M) {
  if (R <= 0 || M <= 0) return 0;
  return 2 * R * pad_k(M) * 2;
}

int uds_remainder_pack(const float *rest, int64_t R, int64_t M, void *packed, uds_stream_t stream) {
  UDS_REQUIRE(rest && packed && aligned16(packed), "uds_remainder_pack: NULL / misaligned argument");
  UDS_REQUIRE(R > 0 && M > 0 && R * pad_k(M) / 8 < (int64_t)INT32_MAX * 256, "uds_remainder_pack: bad shape (%lld, %lld)", (long long)R,
              (long long)M);
  const int64_t Kp = pad_k(M), n = R * Kp / 8;
  __bf16 *hi = reinterpret_cast<__bf16 *>(packed), *lo = hi + R * Kp;
  hipLaunchKernelGGL(uds::k_split_rows_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rest, R, M,
                     Kp, hi, lo);
  return launched("uds_remainder_pack", hipGetLastError());
}

namespace {
// How uds_remainder_forward tiles (R x Kp) x (Nc x Kp): k_remainder_gemm2<2> (256 x 256 tiles, one 8-wave workgroup per CU) when
// the shape has at least one tile's worth of columns; the tiles that fill whole rounds of 256 workgroups go out as they are, the
// rest are cut along K into ks pieces each so that they fill (most of) one more round.
struct RemainderPlan {
  bool v2;
  int64_t n_ctile, t_main, t_rest, ks;
};
RemainderPlan remainder_plan(int64_t R, int64_t Nc, int64_t Kp) {
  RemainderPlan q{false, 0, 0, 0, 1};
  q.v2 = Nc * Kp * 2 < ((int64_t)1 << 32) && R * Kp * 2 < ((int64_t)1 << 32) && Nc >= 256 && R >= 128;
  if (!q.v2) return q;
  q.n_ctile = (Nc + 255) / 256;
  const int64_t tiles = q.n_ctile * ((R + 255) / 256);
  q.t_main = tiles / 256 * 256;
  q.t_rest = tiles - q.t_main;
  if (q.t_rest) {      // pieces per cut tile: the fewest rounds-of-256 per piece length, ties to the fewer pieces (each piece = 256 KB out and back)
    double best = 1e300;
    for (int64_t k = 1; k <= std::min<int64_t>({(int64_t)REMAINDER_MAX_PIECES / q.t_rest, 8, Kp / 32 / 8}); ++k) {
      const double cost = (double)((q.t_rest * k + 255) / 256) / (double)k + 0.01 * (double)k;
      if (cost < best - 1e-9) {
        best = cost;
        q.ks = k;
      }
    }
  }
#ifdef UDS_KNOBS
  if (const char *ov = std::getenv("UDS_GEMM_KS")) q.ks = std::max<int64_t>(1, std::min<int64_t>(std::atoll(ov), REMAINDER_MAX_PIECES / std::max<int64_t>(1, q.t_rest)));
#endif
  if (q.ks == 1) {
    q.t_main = tiles;
    q.t_rest = 0;
  }
  return q;
}
}  // namespace

int64_t uds_remainder_workspace_bytes(int64_t R, int64_t M, int64_t S, int64_t h) {
  if (R <= 0 || M <= 0 || S <= 0 || h <= 0) return 0;
  // the split activation planes + the accumulator pieces of the K-cut tiles (256 x 256 floats each)
  const RemainderPlan q = remainder_plan(R, S * h, pad_k(M));
  return 2 * S * h * pad_k(M) * 2 + (q.v2 ? q.t_rest * q.ks * 256 * 256 * 4 : 0);
}

namespace {
// the GEMM of uds_remainder_forward on operand planes that are already in the workspace
int remainder_gemm_from_planes(const void *packed, int64_t R, int64_t Kp, int64_t Nc, int64_t h, void *workspace, float *out, hipStream_t st) {
  const __bf16 *wh = reinterpret_cast<const __bf16 *>(packed), *wl = wh + R * Kp;
  __bf16 *xh = reinterpret_cast<__bf16 *>(workspace), *xl = xh + Nc * Kp;
  hipError_t e = hipSuccess;
  // k_remainder_gemm2<2> (256 x 256 tiles, LDS-DMA staged, one 8-wave workgroup per CU): the tiles that fill whole rounds of 256
  // workgroups go out as they are; the rest are cut along K into ks pieces each so that they fill (most of) one more round, their
  // accumulators land in the workspace behind the activation planes and a third launch adds the pieces in a fixed order
  const RemainderPlan plan = remainder_plan(R, Nc, Kp);
  if (plan.v2) {
    using C = uds::Gemm2Cfg<2>;
    static unsigned long long done = 0;
    if ((e = uds::set_max_lds_once(reinterpret_cast<const void *>(&uds::k_remainder_gemm2<2>), C::LDS_BYTES, done)) != hipSuccess)
      return fail(UDS_EHIP, "uds_remainder_forward: LDS attribute -> %s", hipGetErrorString(e));
    const int64_t n_ctile = plan.n_ctile, t_main = plan.t_main, t_rest = plan.t_rest, ks = plan.ks;
    float *partial = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + 2 * Nc * Kp * 2);
    hipLaunchKernelGGL((uds::k_remainder_gemm2<2>), dim3((unsigned)(t_main + t_rest * ks)), dim3(512), C::LDS_BYTES, st, xh, xl, wh, wl, Nc, R, Kp, (int)h,
                       (int)n_ctile, out, (int)t_main, (int)ks, partial);
    if (t_rest)
      hipLaunchKernelGGL((uds::k_remainder_gemm2_reduce<2>), dim3((unsigned)t_rest), dim3(512), 0, st, partial, (int)ks, (int)t_main, Nc, R, (int)h,
                         (int)n_ctile, out);
    return launched("uds_remainder_forward", hipGetLastError());
  }
  {
    const int64_t n_ctile = (Nc + 127) / 128, n_rtile = (R + 127) / 128;
    hipLaunchKernelGGL(uds::k_remainder_gemm, dim3((unsigned)(n_ctile * n_rtile)), dim3(256), 0, st, xh, xl, wh, wl, Nc, R, Kp, (int)h,
                       (int)n_ctile, out);
  }
  return launched("uds_remainder_forward", hipGetLastError());
}
}  // namespace

int uds_remainder_forward(const void *packed, int64_t R, int64_t M, const float *x, int64_t S, int64_t h, void *workspace, float *out,
                          uds_stream_t stream) {
  UDS_REQUIRE(S >= 0 && R > 0 && M > 0, "uds_remainder_forward: bad shape");
  if (S == 0) return UDS_OK;
  UDS_REQUIRE(packed && x && workspace && out, "uds_remainder_forward: NULL argument");
  UDS_REQUIRE(h > 0 && h <= 64 && h % 4 == 0, "uds_remainder_forward: h = %lld (needs h %% 4 == 0, h <= 64)", (long long)h);
  UDS_REQUIRE(aligned16(packed) && aligned16(workspace) && aligned16(out), "uds_remainder_forward: buffers must be 16-byte aligned");
  const int64_t Kp = pad_k(M), Nc = S * h;
  UDS_REQUIRE(S <= 65535 && ((Nc + 127) / 128) * ((R + 127) / 128) < INT32_MAX, "uds_remainder_forward: shape exceeds the launch grid");
  const __bf16 *wh = reinterpret_cast<const __bf16 *>(packed), *wl = wh + R * Kp;
  __bf16 *xh = reinterpret_cast<__bf16 *>(workspace), *xl = xh + Nc * Kp;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(uds::k_split_transpose_bf16, dim3((unsigned)(Kp / 64 + (Kp % 64 != 0)), (unsigned)S), dim3(256), 0, st, x, M, (int)h, Kp,
                     xh, xl);
  return remainder_gemm_from_planes(packed, R, Kp, Nc, h, workspace, out, st);
}

int uds_remainder_forward_dense(const void *packed, int64_t R, int64_t M, const float *e, int64_t F, const void *packed_w, const float *bias,
                                int act, int64_t S, int64_t h, void *workspace, float *out, uds_stream_t stream) {
  UDS_REQUIRE(S >= 0 && R > 0 && M > 0, "uds_remainder_forward_dense: bad shape");
  if (S == 0) return UDS_OK;
  UDS_REQUIRE(packed && e && packed_w && workspace && out, "uds_remainder_forward_dense: NULL argument");
  UDS_REQUIRE((F == 64 || F == 128) && (h == 32 || h == 64), "uds_remainder_forward_dense: F = %lld, h = %lld (F 64 or 128, h 32 or 64)", (long long)F,
              (long long)h);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_remainder_forward_dense: unknown activation %d", act);
  UDS_REQUIRE(aligned16(packed) && aligned16(e) && aligned16(packed_w) && aligned16(bias) && aligned16(workspace) && aligned16(out),
              "uds_remainder_forward_dense: buffers must be 16-byte aligned");
  const int64_t Kp = pad_k(M), Nc = S * h;
  UDS_REQUIRE(S <= 65535 && ((Nc + 127) / 128) * ((R + 127) / 128) < INT32_MAX, "uds_remainder_forward_dense: shape exceeds the launch grid");
  __bf16 *xh = reinterpret_cast<__bf16 *>(workspace), *xl = xh + Nc * Kp;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(Kp / 64), (unsigned)S);
  if (F == 64)
    hipLaunchKernelGGL(uds::k_dense_split_planes<2>, grid, dim3(256), 0, st, e, M, (int)h, Kp, reinterpret_cast<const uint4 *>(packed_w), bias, act, xh, xl);
  else
    hipLaunchKernelGGL(uds::k_dense_split_planes<4>, grid, dim3(256), 0, st, e, M, (int)h, Kp, reinterpret_cast<const uint4 *>(packed_w), bias, act, xh, xl);
  if (int rc = launched("uds_remainder_forward_dense", hipGetLastError())) return rc;
  return remainder_gemm_from_planes(packed, R, Kp, Nc, h, workspace, out, st);
}

// ---- rest @ act(e W + b) with x_e kept on chip: one launch per side, or one for both sides of a layer (kernels_remainder_snapshot.hpp)
int uds_remainder_snapshot_plan(int64_t R, int64_t M, int64_t F, int64_t h, int32_t *info4) {
  UDS_REQUIRE(info4 != nullptr, "uds_remainder_snapshot_plan: info4 is NULL");
  const uds::SnapPlan p = uds::snapshot_plan(R, M, F, h);
  info4[0] = p.G;
  info4[1] = (int32_t)p.lds;
  info4[2] = p.RB;
  info4[3] = 0;
  return UDS_OK;
}

namespace {
struct SnapSideIn {
  const void *packed;
  int64_t R, M;
  const float *e;
  const void *packed_w;
  const float *bias;
  float *out;
};

// One checked implementation behind uds_remainder_snapshot and uds_remainder_snapshot_pair: a side with packed == NULL is skipped.
int remainder_snapshot_run(const char *entry, const SnapSideIn (&in)[2], int64_t F, int act, int64_t S, int64_t h, uds_stream_t stream) {
  UDS_REQUIRE(in[0].packed || in[1].packed, "%s: both sides are NULL", entry);
  UDS_REQUIRE((F == 64 || F == 128) && (h == 32 || h == 64), "%s: F = %lld, h = %lld (F 64 or 128, h 32 or 64)", entry, (long long)F, (long long)h);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "%s: unknown activation %d", entry, act);
  UDS_REQUIRE(S >= 0 && S <= ((int64_t)1 << 24), "%s: S = %lld (0 .. 2^24)", entry, (long long)S);
  uds::SnapArgs a{};
  a.h = (int)h;
  a.act = act;
  a.S = S;
  int64_t lds = 0;
  for (int i = 0; i < 2; ++i) {
    const SnapSideIn &q = in[i];
    if (!q.packed) continue;
    UDS_REQUIRE(q.R > 0 && q.M > 0, "%s: side %d: bad shape (%lld, %lld)", entry, i, (long long)q.R, (long long)q.M);
    const uds::SnapPlan p = uds::snapshot_plan(q.R, q.M, F, h);
    UDS_REQUIRE(p.G > 0, "%s: side %d: rest (%lld, %lld) is refused by uds_remainder_snapshot_plan (M <= %lld: the image of 64 columns must fit the LDS)",
                entry, i, (long long)q.R, (long long)q.M, (long long)((uds::SNAP_LDS_MAX / 256 - uds::SNAP_PAD) / 64 * 64));
    if (S == 0) continue;
    UDS_REQUIRE(q.e && q.packed_w && q.out, "%s: side %d: NULL argument", entry, i);
    UDS_REQUIRE(aligned16(q.packed) && aligned16(q.e) && aligned16(q.packed_w) && aligned16(q.bias) && aligned16(q.out),
                "%s: side %d: buffers must be 16-byte aligned", entry, i);
    uds::SnapSide &sd = a.side[i];
    sd.rest = reinterpret_cast<const __bf16 *>(q.packed);
    sd.e = q.e;
    sd.wq = reinterpret_cast<const uint4 *>(q.packed_w);
    sd.bias = q.bias;
    sd.out = q.out;
    sd.R = (int)q.R;
    sd.M = (int)q.M;
    sd.Kp = (int)pad_k(q.M);
    sd.NG = p.NG;
    sd.RB = p.RB;
    sd.nwg = (int)((S + p.G - 1) / p.G);
    lds = std::max(lds, p.lds);
  }
  if (S == 0) return UDS_OK;
  const unsigned grid = (unsigned)(a.side[0].nwg + a.side[1].nwg);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  if (F == 64) {
    static unsigned long long done = 0;
    if ((e = uds::set_max_lds_once(reinterpret_cast<const void *>(&uds::k_remainder_snapshot<2>), (int)uds::SNAP_LDS_MAX, done)) != hipSuccess)
      return fail(UDS_EHIP, "%s: LDS attribute -> %s", entry, hipGetErrorString(e));
    hipLaunchKernelGGL(uds::k_remainder_snapshot<2>, dim3(grid), dim3(uds::SNAP_WAVES * 64), (size_t)lds, st, a);
  } else {
    static unsigned long long done = 0;
    if ((e = uds::set_max_lds_once(reinterpret_cast<const void *>(&uds::k_remainder_snapshot<4>), (int)uds::SNAP_LDS_MAX, done)) != hipSuccess)
      return fail(UDS_EHIP, "%s: LDS attribute -> %s", entry, hipGetErrorString(e));
    hipLaunchKernelGGL(uds::k_remainder_snapshot<4>, dim3(grid), dim3(uds::SNAP_WAVES * 64), (size_t)lds, st, a);
  }
  return launched(entry, hipGetLastError());
}
}  // namespace

int uds_remainder_snapshot(const void *packed, int64_t R, int64_t M, const float *e, int64_t F, const void *packed_w, const float *bias, int act,
                           int64_t S, int64_t h, float *out, uds_stream_t stream) {
  UDS_REQUIRE(packed != nullptr, "uds_remainder_snapshot: NULL argument");
  const SnapSideIn in[2] = {{packed, R, M, e, packed_w, bias, out}, {nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr}};
  return remainder_snapshot_run("uds_remainder_snapshot", in, F, act, S, h, stream);
}

int uds_remainder_snapshot_pair(const void *packed0, int64_t R0, int64_t M0, const float *e0, const void *packed_w0, const float *bias0, float *out0,
                                const void *packed1, int64_t R1, int64_t M1, const float *e1, const void *packed_w1, const float *bias1, float *out1,
                                int64_t F, int act, int64_t S, int64_t h, uds_stream_t stream) {
  const SnapSideIn in[2] = {{packed0, R0, M0, e0, packed_w0, bias0, out0}, {packed1, R1, M1, e1, packed_w1, bias1, out1}};
  return remainder_snapshot_run("uds_remainder_snapshot_pair", in, F, act, S, h, stream);
}

int uds_rowgemm_forward(const float *x, int64_t B, int64_t T, int64_t R, int64_t F, const void *packed, const float *bias,
                        int64_t taps, int64_t dil, int64_t f_out, int act, float *out, uds_stream_t stream) {
  return uds_rowgemm_forward_cat(x, F, nullptr, 0, B, T, R, packed, bias, taps, dil, f_out, act, out, f_out, 0, stream);
}

int uds_rowgemm_forward_cat(const float *x, int64_t F1, const float *x2, int64_t F2, int64_t B, int64_t T, int64_t R, const void *packed,
                            const float *bias, int64_t taps, int64_t dil, int64_t f_out, int act, float *out, int64_t ldo, int64_t col0,
                            uds_stream_t stream) {
  const int64_t F = F1 + F2;
  UDS_REQUIRE((x2 != nullptr) == (F2 > 0), "uds_rowgemm_forward_cat: x2 / F2 disagree");
  UDS_REQUIRE(!x2 || (taps == 1 && F1 % 32 == 0 && F2 % 32 == 0 && aligned16(x2)),
              "uds_rowgemm_forward_cat: a two-tensor row needs taps = 1 and both widths multiples of 32");
  UDS_REQUIRE(ldo >= col0 + f_out && col0 >= 0 && (ldo == f_out || (ldo % 4 == 0 && col0 % 4 == 0)),
              "uds_rowgemm_forward_cat: output block [%lld, %lld) does not fit rows of %lld floats (4-float aligned)", (long long)col0,
              (long long)(col0 + f_out), (long long)ldo);
  UDS_REQUIRE(x && packed && out, "uds_rowgemm_forward: NULL x/packed/out");
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0 && F > 0 && F % 32 == 0 && taps > 0 && taps <= 16 && dil != 0 && f_out > 0 && f_out <= 64,
              "uds_rowgemm_forward: needs F %% 32 == 0, f_out <= 64 (B=%lld T=%lld R=%lld F=%lld taps=%lld f_out=%lld)", (long long)B,
              (long long)T, (long long)R, (long long)F, (long long)taps, (long long)f_out);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_rowgemm_forward: unknown activation %d", act);
  UDS_REQUIRE(aligned16(x) && aligned16(packed) && aligned16(out) && aligned16(bias), "uds_rowgemm_forward: pointers must be 16-byte aligned");
  UDS_REQUIRE(uds::rowgemm_ring((int)(taps * F), uds::rowgemm_mb((int)f_out)) != 0,
              "uds_rowgemm_forward: K=%lld x f_out=%lld weights do not fit the LDS", (long long)(taps * F), (long long)f_out);
  UDS_REQUIRE(B * T * R < INT32_MAX, "uds_rowgemm_forward: %lld rows exceed the int32 row index", (long long)(B * T * R));
  if (B == 0) return UDS_OK;
  const int64_t n_blocks = (R + 15) / 16;
  bool stream_conv = uds::conv_stream_supported((int)taps, (int)F, (int)f_out, (int)dil) && B * n_blocks >= 256 && ldo == f_out;
#ifdef UDS_KNOBS
  if (std::getenv("UDS_NO_CONV_STREAM")) stream_conv = false;      // experiment builds only: the row GEMM in place of the streaming conv
#endif
  if (stream_conv) {
    // enough (batch element, 16-row block) streams to fill the CUs: read every row once instead of once per tap
    uds::ConvStreamArgs ca{x, bias, reinterpret_cast<const uint4 *>(packed), out, (int)B, (int)T, (int)R, act, dil > 0 ? 1 : -1, (int)n_blocks, 1, (int)T};
    hipError_t ec = uds::launch_conv_stream(ca, (int)dil, static_cast<hipStream_t>(stream));
    if (ec != hipSuccess) return fail(UDS_EHIP, "uds_rowgemm_forward: streaming conv launch -> %s", hipGetErrorString(ec));
    return UDS_OK;
  }
  uds::RowGemmArgs a{x, bias, reinterpret_cast<const uint4 *>(packed), out, B * T * R, (int)F, (int)taps, (int)dil, (int)T, (int)R,
                     (int)f_out, act, 0, x2, (int)F1, (int)ldo, (int)col0};
  return launched("uds_rowgemm_forward", uds::launch_rowgemm(a, static_cast<hipStream_t>(stream)));
}

int uds_rowgemm_forward_pair(const float *x0, int64_t R0, const void *packed0, const float *bias0, float *out0, const float *x1, int64_t R1,
                             const void *packed1, const float *bias1, float *out1, int64_t B, int64_t T, int64_t F, int64_t taps, int64_t dil,
                             int64_t f_out, int act, uds_stream_t stream) {
  UDS_REQUIRE(x0 && x1 && packed0 && packed1 && out0 && out1, "uds_rowgemm_forward_pair: NULL argument");
  UDS_REQUIRE(B >= 0 && T > 0 && R0 > 0 && R1 > 0 && F > 0 && F % 32 == 0 && taps > 0 && taps <= 16 && dil > 0 && f_out > 0 && f_out <= 64,
              "uds_rowgemm_forward_pair: needs F %% 32 == 0, f_out <= 64, dil > 0");
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_rowgemm_forward_pair: unknown activation %d", act);
  UDS_REQUIRE(aligned16(x0) && aligned16(x1) && aligned16(packed0) && aligned16(packed1) && aligned16(out0) && aligned16(out1) && aligned16(bias0) &&
                  aligned16(bias1), "uds_rowgemm_forward_pair: pointers must be 16-byte aligned");
  if (B == 0) return UDS_OK;
  uds::RowGemmArgs a0{x0, bias0, reinterpret_cast<const uint4 *>(packed0), out0, B * T * R0, (int)F, (int)taps, (int)dil, (int)T, (int)R0,
                      (int)f_out, act, 0, nullptr, 0, (int)f_out, 0};
  uds::RowGemmArgs a1{x1, bias1, reinterpret_cast<const uint4 *>(packed1), out1, B * T * R1, (int)F, (int)taps, (int)dil, (int)T, (int)R1,
                      (int)f_out, act, 0, nullptr, 0, (int)f_out, 0};
  hipError_t e = hipSuccess;
  bool done = false;
  switch (uds::rowgemm_mb((int)f_out)) {
    case 1: done = uds::launch_rowgemm_small_pair<1>(a0, a1, static_cast<hipStream_t>(stream), e); break;
    case 2: done = uds::launch_rowgemm_small_pair<2>(a0, a1, static_cast<hipStream_t>(stream), e); break;
    default: done = uds::launch_rowgemm_small_pair<4>(a0, a1, static_cast<hipStream_t>(stream), e); break;
  }
  if (!done) {      // too large (or a depth the pair kernel is not built for): the two ordinary launches
    int rc = uds_rowgemm_forward(x0, B, T, R0, F, packed0, bias0, taps, dil, f_out, act, out0, stream);
    if (rc != UDS_OK) return rc;
    return uds_rowgemm_forward(x1, B, T, R1, F, packed1, bias1, taps, dil, f_out, act, out1, stream);
  }
  return launched("uds_rowgemm_forward_pair", e);
}

// uds_dense_cumsum and uds_dense_cumsum_heads (with_heads): the same checks around those of the heads, one DenseCumsumArgs
static int dense_cumsum(const char *what, bool with_heads, const float *x, int64_t B, int64_t T, int64_t R, const void *packed, const float *bias,
                        const float *res, int act, const uds_heads_t *heads, float *out, uds_stream_t stream) {
  UDS_REQUIRE(x && packed && out && (!with_heads || heads), "%s: NULL x/packed/%sout", what, with_heads ? "heads/" : "");
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0, "%s: bad sizes B=%lld T=%lld R=%lld", what, (long long)B, (long long)T, (long long)R);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "%s: unknown activation %d", what, act);
  if (with_heads) {
    UDS_REQUIRE(heads->a_packed && heads->n_a >= 1 && heads->n_a <= 4, "%s: first head needs 1..4 outputs (got %d)", what, heads->n_a);
    UDS_REQUIRE(heads->n_hidden >= 0 && heads->n_hidden <= 5, "%s: 0..5 hidden layers in the second head (got %d)", what, heads->n_hidden);
    for (int i = 0; i < heads->n_hidden; ++i) UDS_REQUIRE(heads->h_packed[i], "%s: hidden layer %d has no weights", what, i);
    UDS_REQUIRE(heads->n_hidden == 0 || heads->f_packed, "%s: the second head has no output layer", what);
    for (int v : {heads->act_a, heads->act_h, heads->act_f})
      UDS_REQUIRE(v >= UDS_ACT_LINEAR && v <= UDS_ACT_HARD_SIGMOID, "%s: unknown head activation %d", what, v);
  }
  // with heads, `out` holds rows of n_a (+ 1) floats and its alignment is not asked for; the heads' packed weights are
  UDS_REQUIRE(aligned16(x) && aligned16(packed) && aligned16(bias) && aligned16(res) &&
                  (with_heads ? aligned16(heads->a_packed) && aligned16(heads->f_packed) : aligned16(out)),
              "%s: pointers must be 16-byte aligned", what);
  UDS_REQUIRE(B * T * R < INT32_MAX, "%s: %lld rows exceed the int32 row index", what, (long long)(B * T * R));
  if (B == 0) return UDS_OK;
  uds::DenseCumsumArgs a{x, bias, res, reinterpret_cast<const uint4 *>(packed), out, (int)B, (int)T, (int)R, act, (int)((R + 15) / 16)};
  if (!with_heads) return launched(what, uds::launch_dense_cumsum(a, static_cast<hipStream_t>(stream)));
  uds::HeadsArgs hd{};
  hd.a_packed = reinterpret_cast<const uint4 *>(heads->a_packed);
  hd.a_bias = heads->a_bias;
  for (int i = 0; i < 5; ++i) {
    hd.h_packed[i] = reinterpret_cast<const uint4 *>(heads->h_packed[i]);
    hd.h_bias[i] = heads->h_bias[i];
  }
  hd.f_packed = reinterpret_cast<const uint4 *>(heads->f_packed);
  hd.f_bias = heads->f_bias;
  hd.n_a = heads->n_a, hd.act_a = heads->act_a, hd.n_hidden = heads->n_hidden, hd.act_h = heads->act_h, hd.act_f = heads->act_f;
  return launched(what, uds::launch_dense_cumsum_heads(a, hd, static_cast<hipStream_t>(stream)));
}

int uds_dense_cumsum(const float *x, int64_t B, int64_t T, int64_t R, const void *packed, const float *bias, const float *res, int act,
                     float *out, uds_stream_t stream) {
  return dense_cumsum("uds_dense_cumsum", false, x, B, T, R, packed, bias, res, act, nullptr, out, stream);
}

int uds_dense_cumsum_heads(const float *x, int64_t B, int64_t T, int64_t R, const void *packed, const float *bias, const float *res, int act,
                           const uds_heads_t *heads, float *out, uds_stream_t stream) {
  return dense_cumsum("uds_dense_cumsum_heads", true, x, B, T, R, packed, bias, res, act, heads, out, stream);
}

int uds_conv_stack_plan(int64_t B, int64_t T, int64_t R, int n_layers, int64_t *n_seg, int64_t *seg_len, int64_t *halo) {
  UDS_REQUIRE(n_seg && seg_len && halo, "uds_conv_stack_plan: NULL n_seg/seg_len/halo");
  UDS_REQUIRE(n_layers == 2 || n_layers == 3, "uds_conv_stack_plan: stacks of 2 or 3 layers (got %d)", n_layers);
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0, "uds_conv_stack_plan: bad sizes B=%lld T=%lld R=%lld", (long long)B, (long long)T, (long long)R);
  uds::conv_stack_plan(B, T, R, n_layers, *n_seg, *seg_len);
  *halo = uds::conv_stack_halo(n_layers);
  return UDS_OK;
}

int uds_conv_stack_forward(const float *x, int64_t B, int64_t T, int64_t R, const uds_conv_stack_t *layers, int64_t n_seg, float *out,
                           uds_stream_t stream) {
  UDS_REQUIRE(x && out && layers, "uds_conv_stack_forward: NULL x/out/layers");
  const int L = layers->n_layers;
  UDS_REQUIRE(L == 2 || L == 3, "uds_conv_stack_forward: stacks of 2 or 3 layers (got %d)", L);
  for (int i = 0; i < L; ++i) UDS_REQUIRE(layers->packed[i], "uds_conv_stack_forward: layer %d has no weights", i);
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0, "uds_conv_stack_forward: bad sizes B=%lld T=%lld R=%lld", (long long)B, (long long)T, (long long)R);
  UDS_REQUIRE(layers->act >= UDS_ACT_LINEAR && layers->act <= UDS_ACT_HARD_SIGMOID, "uds_conv_stack_forward: unknown activation %d",
              (int)layers->act);
  for (int i = 0; i < L; ++i)
    UDS_REQUIRE(aligned16(layers->packed[i]) && aligned16(layers->bias[i]), "uds_conv_stack_forward: pointers must be 16-byte aligned");
  UDS_REQUIRE(aligned16(x) && aligned16(out), "uds_conv_stack_forward: pointers must be 16-byte aligned");
  UDS_REQUIRE(n_seg >= 0 && n_seg <= T, "uds_conv_stack_forward: n_seg %lld outside [0, T = %lld]", (long long)n_seg, (long long)T);
  UDS_REQUIRE(B * T * R < INT32_MAX, "uds_conv_stack_forward: %lld rows exceed the int32 row index", (long long)(B * T * R));
  {      // segments re-read halo steps of x that another segment's wave may already have overwritten
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x), ob = reinterpret_cast<uintptr_t>(out), bytes = (uintptr_t)(B * T * R) * 64 * 4;
    UDS_REQUIRE(xb + bytes <= ob || ob + bytes <= xb, "uds_conv_stack_forward: out overlaps x");
  }
  if (B == 0) return UDS_OK;
  uds::ConvStackArgs a{};
  a.x = x, a.out = out;
  for (int i = 0; i < L; ++i) a.packed[i] = reinterpret_cast<const uint4 *>(layers->packed[i]), a.bias[i] = layers->bias[i];
  a.B = (int)B, a.T = (int)T, a.R = (int)R, a.act = layers->act, a.n_blocks = (int)((R + 15) / 16);
  int64_t ns = n_seg, sl = 0;
  if (ns == 0) {
    uds::conv_stack_plan(B, T, R, L, ns, sl);
  } else {
    sl = (T + ns - 1) / ns;
    ns = (T + sl - 1) / sl;
  }
  a.n_seg = (int)ns, a.seg_len = (int)sl;
  return launched("uds_conv_stack_forward", uds::launch_conv_stack(a, L, static_cast<hipStream_t>(stream)));
}

int uds_cumsum_act(const float *x, const float *res, int64_t B, int64_t T, int64_t R, int64_t F, int act, float *out,
                   uds_stream_t stream) {
  UDS_REQUIRE(x && out, "uds_cumsum_act: NULL x/out");
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0 && F > 0 && F % 4 == 0, "uds_cumsum_act: bad sizes (F must be a multiple of 4)");
  UDS_REQUIRE(aligned16(x) && aligned16(out) && aligned16(res), "uds_cumsum_act: x/res/out must be 16-byte aligned");
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_cumsum_act: unknown activation %d", act);
  if (B == 0) return UDS_OK;
  uds::CumsumArgs a{x, res, out, (int)B, (int)T, (int)R, (int)(F / 4), act};
  return launched("uds_cumsum_act", uds::launch_cumsum(a, static_cast<hipStream_t>(stream)));
}

int uds_attn_sum_pool(const float *x, const float *k, int64_t B, int64_t R, int64_t F, float *out, uds_stream_t stream) {
  UDS_REQUIRE(x && k && out, "uds_attn_sum_pool: NULL argument");
  UDS_REQUIRE(B >= 0 && R > 0 && F >= 4 && F <= 256 && (F & (F - 1)) == 0, "uds_attn_sum_pool: B=%lld R=%lld F=%lld (F a power of two, 4 .. 256)",
              (long long)B, (long long)R, (long long)F);
  UDS_REQUIRE(aligned16(x) && aligned16(k) && aligned16(out), "uds_attn_sum_pool: x/k/out must be 16-byte aligned");
  UDS_REQUIRE(B < INT32_MAX && R < INT32_MAX, "uds_attn_sum_pool: too many rows");
  if (B == 0) return UDS_OK;
  uds::AttnPoolArgs a{x, k, out, (int)R, (int)(F / 4)};
  hipLaunchKernelGGL(uds::k_attn_sum_pool, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launched("uds_attn_sum_pool", hipGetLastError());
}

int uds_attn_sum_pool_pair(const float *x, int64_t Rx, const float *e, int64_t Re, const float *k, int64_t B, int64_t F, float *out, float *stat,
                           uds_stream_t stream) {
  UDS_REQUIRE(x && k && out && (e || Re == 0), "uds_attn_sum_pool_pair: NULL argument");
  UDS_REQUIRE(B >= 0 && Rx > 0 && Re >= 0 && F >= 4 && F <= 256 && (F & (F - 1)) == 0,
              "uds_attn_sum_pool_pair: B=%lld Rx=%lld Re=%lld F=%lld (F a power of two, 4 .. 256)", (long long)B, (long long)Rx, (long long)Re, (long long)F);
  UDS_REQUIRE(aligned16(x) && aligned16(e) && aligned16(k) && aligned16(out), "uds_attn_sum_pool_pair: x/e/k/out must be 16-byte aligned");
  UDS_REQUIRE(B < INT32_MAX && Rx < INT32_MAX && Re < INT32_MAX && Rx + Re < INT32_MAX, "uds_attn_sum_pool_pair: too many rows");
  if (B == 0) return UDS_OK;
  uds::AttnPoolPairArgs a{x, Re ? e : nullptr, k, out, stat, (int)Rx, (int)Re, (int)(F / 4)};
  hipLaunchKernelGGL(uds::k_attn_sum_pool_pair, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launched("uds_attn_sum_pool_pair", hipGetLastError());
}

int uds_attn_sum_pool_backward(const float *x, int64_t Rx, const float *e, int64_t Re, const float *k, const float *out, const float *stat,
                               const float *grad, int64_t B, int64_t F, float *dx, float *de, float *dk_ws, float *dk, uds_stream_t stream) {
  UDS_REQUIRE(x && k && out && stat && grad && (e || Re == 0), "uds_attn_sum_pool_backward: NULL argument");
  UDS_REQUIRE(B >= 0 && Rx > 0 && Re >= 0 && F >= 4 && F <= 256 && (F & (F - 1)) == 0,
              "uds_attn_sum_pool_backward: B=%lld Rx=%lld Re=%lld F=%lld (F a power of two, 4 .. 256)", (long long)B, (long long)Rx, (long long)Re,
              (long long)F);
  UDS_REQUIRE(!dk || dk_ws, "uds_attn_sum_pool_backward: dk needs the workspace dk_ws (B, F)");
  UDS_REQUIRE(aligned16(x) && aligned16(e) && aligned16(k) && aligned16(out) && aligned16(grad) && aligned16(dx) && aligned16(de) &&
                  aligned16(dk_ws) && aligned16(dk),
              "uds_attn_sum_pool_backward: x/e/k/out/grad/dx/de/dk_ws/dk must be 16-byte aligned");
  UDS_REQUIRE(B < INT32_MAX && Rx < INT32_MAX && Re < INT32_MAX && Rx + Re < INT32_MAX, "uds_attn_sum_pool_backward: too many rows");
  if (!Re) de = nullptr;
  if (!dx && !de && !dk) return UDS_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int f4 = (int)(F / 4);
  if (B > 0) {
    uds::AttnPoolBwdArgs a{x, Re ? e : nullptr, k, out, stat, grad, dx, de, dk ? dk_ws : nullptr, (int)Rx, (int)Re, f4};
    hipLaunchKernelGGL(uds::k_attn_sum_pool_bwd, dim3((unsigned)B), dim3(256), 0, st, a);
    if (int rc = launched("uds_attn_sum_pool_backward", hipGetLastError())) return rc;
  }
  if (dk) {                                           // B = 0: the sum over no samples, zeros
    const int cw = std::min(f4, 16);
    uds::AttnPoolDkArgs r{dk_ws, dk, (int)B, f4, cw};
    hipLaunchKernelGGL(uds::k_attn_sum_pool_dk, dim3((unsigned)(f4 / cw)), dim3(256), 0, st, r);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(UDS_EHIP, "uds_attn_sum_pool_backward: dk reduction launch -> %s", hipGetErrorString(err));
  }
  return UDS_OK;
}

int uds_dropout(const float *x, int64_t n, float rate, uint64_t seed, uint64_t offset, float *out, uds_stream_t stream) {
  UDS_REQUIRE(n >= 0 && (n == 0 || (x && out)), "uds_dropout: NULL argument");
  UDS_REQUIRE(rate >= 0.f && rate < 1.f, "uds_dropout: rate=%g outside [0, 1)", (double)rate);
  if (n == 0) return UDS_OK;
  const int64_t groups = (n + (int64_t)(offset & 3) + 3) / 4;
  UDS_REQUIRE((groups + 255) / 256 < INT32_MAX, "uds_dropout: n=%lld too large for one launch", (long long)n);
  uds::DropoutArgs a{x, out, n, (unsigned long long)seed, (unsigned long long)offset,
                     (unsigned)std::min<double>(4294967295.0, std::ceil((double)rate * 4294967296.0)), 1.0f / (1.0f - rate)};
  hipLaunchKernelGGL(uds::k_dropout, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launched("uds_dropout", hipGetLastError());
}

// ---- Keras Adam with per-variable clipnorm over a list of tensors (kernels_optim.hpp).  Workgroups per tensor: one per
// ADAM_SPAN elements; the partial of workgroup b of launch k sits at partial[first block of launch k + b].
namespace {
inline int64_t adam_blocks(int64_t numel) { return (numel + uds::ADAM_SPAN - 1) / uds::ADAM_SPAN; }
}  // namespace

int64_t uds_adam_workspace_floats(const int64_t *numel, int64_t n_tensors) {
  if (!numel || n_tensors < 0) return -1;
  int64_t blocks = 0;
  for (int64_t i = 0; i < n_tensors; ++i) {
    if (numel[i] < 0) return -1;
    blocks += adam_blocks(numel[i]);
  }
  return 2 * blocks;                                  // one double per workgroup
}

int uds_adam_step(const uds_adam_tensor_t *tensors, int64_t n_tensors, const float *loss, double lr, double beta_1, double beta_2,
                  double epsilon, double clipnorm, int32_t *state, float *workspace, int64_t workspace_floats, uds_stream_t stream) {
  const char *what = "uds_adam_step";
  UDS_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || tensors) && state, "%s: NULL argument", what);
  UDS_REQUIRE((reinterpret_cast<uintptr_t>(state) & 3) == 0 && (reinterpret_cast<uintptr_t>(loss) & 3) == 0, "%s: state / loss not 4-byte aligned", what);
  UDS_REQUIRE(lr == lr && beta_1 >= 0 && beta_1 < 1 && beta_2 >= 0 && beta_2 < 1 && epsilon >= 0, "%s: lr=%g beta_1=%g beta_2=%g epsilon=%g", what, lr,
              beta_1, beta_2, epsilon);
  int64_t blocks = 0;
  for (int64_t i = 0; i < n_tensors; ++i) {
    const uds_adam_tensor_t &x = tensors[i];
    UDS_REQUIRE(x.numel >= 0, "%s: tensor %lld has numel=%lld", what, (long long)i, (long long)x.numel);
    if (x.numel == 0) continue;
    UDS_REQUIRE(x.p && x.g && x.m && x.v, "%s: tensor %lld has a NULL pointer", what, (long long)i);
    UDS_REQUIRE(((reinterpret_cast<uintptr_t>(x.p) | reinterpret_cast<uintptr_t>(x.g) | reinterpret_cast<uintptr_t>(x.m) | reinterpret_cast<uintptr_t>(x.v)) & 3) == 0,
                "%s: tensor %lld is not 4-byte aligned", what, (long long)i);
    UDS_REQUIRE(adam_blocks(x.numel) < INT32_MAX / 2, "%s: tensor %lld (numel=%lld) too large for one launch", what, (long long)i, (long long)x.numel);
    blocks += adam_blocks(x.numel);
  }
  UDS_REQUIRE(blocks == 0 || (workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0), "%s: workspace NULL or not 8-byte aligned", what);
  UDS_REQUIRE(workspace_floats >= 2 * blocks, "%s: workspace of %lld floats, %lld needed (uds_adam_workspace_floats)", what, (long long)workspace_floats,
              (long long)(2 * blocks));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *partial = reinterpret_cast<double *>(workspace);
  uds::AdamHyper h{lr, beta_1, beta_2, (float)beta_1, (float)(1.0 - beta_1), (float)beta_2, (float)(1.0 - beta_2), (float)epsilon,
                   clipnorm > 0 ? (float)clipnorm : 0.f};
  // both passes cut the list into the same launches: up to ADAM_TABLE tensors and 2^30 workgroups each
  for (int pass = 0; pass < 2; ++pass) {
    int64_t i = 0, base = 0;
    while (i < n_tensors) {
      uds::AdamTable t;
      std::memset(&t, 0, sizeof t);
      int32_t grid = 0;
      for (; i < n_tensors && t.n < uds::ADAM_TABLE; ++i) {
        const uds_adam_tensor_t &x = tensors[i];
        if (x.numel == 0) continue;
        const int64_t nb = adam_blocks(x.numel);
        if (t.n > 0 && grid + nb > (int64_t)1 << 30) break;
        t.p[t.n] = x.p; t.g[t.n] = x.g; t.m[t.n] = x.m; t.v[t.n] = x.v;
        t.numel[t.n] = x.numel;
        t.block0[t.n] = grid;
        grid += (int32_t)nb;
        t.block0[++t.n] = grid;
      }
      if (t.n == 0) break;
      if (pass == 0)
        hipLaunchKernelGGL(uds::k_adam_sumsq, dim3((unsigned)grid), dim3(uds::ADAM_THREADS), 0, st, t, partial + base, state);
      else
        hipLaunchKernelGGL(uds::k_adam_update, dim3((unsigned)grid), dim3(uds::ADAM_THREADS), 0, st, t, (const double *)(partial + base), loss,
                           (const int32_t *)state, h);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(UDS_EHIP, "%s: pass %d launch -> %s", what, pass + 1, hipGetErrorString(e));
      base += grid;
    }
  }
  hipLaunchKernelGGL(uds::k_adam_commit, dim3(1), dim3(64), 0, st, loss, state);
  return launched(what, hipGetLastError());
}

// ---- Device-resident training data (kernels_data.hpp).  uds_window_batch: x, a, b, y, ex, ey of B sliding windows, normalised, in
// one launch (the windows of dataloader.py:93-95,144-169, the batch of dataloader.py:106-143, the normalisations and uploads of
// main.py:209-232).
int uds_window_batch(const uds_window_series_t *series, const uds_window_norm_t *norm, const int32_t *starts, int64_t B, int64_t seq_in,
                     int64_t t_out, int if_flood, float *x, float *a, float *b, float *y, float *ex, float *ey, uds_stream_t stream) {
  const char *what = "uds_window_batch";
  UDS_REQUIRE(series && starts && x && b && y && ex && ey, "%s: NULL argument", what);
  const uds_window_series_t &s = *series;
  UDS_REQUIRE(s.states && s.flood && s.edge_states, "%s: NULL series (states, flood and edge_states are required)", what);
  UDS_REQUIRE(s.Ttot >= 1 && s.N >= 1 && s.E >= 1 && s.n_act >= 0 && s.N <= INT32_MAX / 8 && s.E <= INT32_MAX / 8 && s.n_act <= 65536,
              "%s: Ttot=%lld N=%lld E=%lld n_act=%lld", what, (long long)s.Ttot, (long long)s.N, (long long)s.E, (long long)s.n_act);
  UDS_REQUIRE((s.n_act > 0) == (s.settings != nullptr) && (s.n_act > 0) == (a != nullptr), "%s: settings / a must be given exactly when n_act > 0 (n_act=%lld)",
              what, (long long)s.n_act);
  UDS_REQUIRE(seq_in >= 1 && t_out >= 1 && seq_in + t_out <= 65536, "%s: seq_in=%lld t_out=%lld", what, (long long)seq_in, (long long)t_out);
  UDS_REQUIRE(B >= 1 && B <= (INT32_MAX - 1) / (seq_in + t_out), "%s: B=%lld outside [1, %lld]", what, (long long)B,
              (long long)((INT32_MAX - 1) / (seq_in + t_out)));
  UDS_REQUIRE(aligned16(s.states) && aligned16(s.flood) && aligned16(s.edge_states) && aligned16(s.settings) && aligned16(s.tide),
              "%s: every series must be 16-byte aligned", what);
  UDS_REQUIRE(aligned16(x) && aligned16(a) && aligned16(b) && aligned16(y) && aligned16(ex) && aligned16(ey), "%s: every output must be 16-byte aligned", what);
  UDS_REQUIRE((reinterpret_cast<uintptr_t>(starts) & 3) == 0, "%s: starts not 4-byte aligned", what);
  uds::WindowBatchArgs k{};
  if (norm) {
    const float *q[8] = {norm->span_x, norm->min_x, norm->span_b, norm->min_b, norm->span_y, norm->min_y, norm->span_e, norm->min_e};
    for (int i = 0; i < 8; i += 2)
      UDS_REQUIRE((q[i] != nullptr) == (q[i + 1] != nullptr), "%s: norm pair %d needs both its span and its minimum, or neither", what, i / 2);
    for (int i = 0; i < 8; ++i) UDS_REQUIRE((reinterpret_cast<uintptr_t>(q[i]) & 3) == 0, "%s: norm pointer %d not 4-byte aligned", what, i);
    k.span_x = q[0]; k.min_x = q[1]; k.span_b = q[2]; k.min_b = q[3]; k.span_y = q[4]; k.min_y = q[5]; k.span_e = q[6]; k.min_e = q[7];
  }
  const int64_t chunks = (s.N + s.E + s.n_act + uds::WINDOW_THREADS - 1) / uds::WINDOW_THREADS;
  UDS_REQUIRE(chunks <= 65535, "%s: N + E + n_act = %lld too large for one launch", what, (long long)(s.N + s.E + s.n_act));
  k.states = s.states; k.flood = s.flood; k.edge_states = s.edge_states; k.settings = s.settings; k.tide = s.tide;
  k.starts = starts;
  k.x = x; k.a = a; k.b = b; k.y = y; k.ex = ex; k.ey = ey;
  k.Ttot = s.Ttot;
  k.N = (int)s.N; k.E = (int)s.E; k.n_act = (int)s.n_act; k.seq_in = (int)seq_in; k.t_out = (int)t_out; k.if_flood = if_flood ? 1 : 0;
  hipLaunchKernelGGL(uds::k_window_batch, dim3((unsigned)(B * (seq_in + t_out)), (unsigned)chunks), dim3(uds::WINDOW_THREADS), 0,
                     static_cast<hipStream_t>(stream), k);
  return launched(what, hipGetLastError());
}

// uds_window_draw: the weighted random draw of a batch of window starts (DataGenerator.prepare_batch, dataloader.py:106-143 over
// the windows of dataloader.py:93-95,144-169; once per epoch and table, main.py:209-232), then the count bump as a launch of its own.
int uds_window_draw(const int32_t *starts_table, const uint64_t *cum, int64_t W, int64_t B, uint64_t seed, uint64_t *count, int32_t *out,
                    uds_stream_t stream) {
  const char *what = "uds_window_draw";
  UDS_REQUIRE(starts_table && cum && count && out, "%s: NULL argument", what);
  UDS_REQUIRE(W >= 1 && W < INT32_MAX, "%s: W=%lld (a table needs at least one window)", what, (long long)W);
  UDS_REQUIRE(B >= 1 && B <= uds::WINDOW_DRAW_MAX, "%s: B=%lld outside [1, %d]", what, (long long)B, uds::WINDOW_DRAW_MAX);
  UDS_REQUIRE(((reinterpret_cast<uintptr_t>(cum) | reinterpret_cast<uintptr_t>(count)) & 7) == 0, "%s: cum / count not 8-byte aligned", what);
  UDS_REQUIRE(((reinterpret_cast<uintptr_t>(starts_table) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, "%s: starts_table / out not 4-byte aligned", what);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uds::WindowDrawArgs k{starts_table, reinterpret_cast<const unsigned long long *>(cum), reinterpret_cast<const unsigned long long *>(count), out,
                        (unsigned long long)seed, (int)W, (int)B};
  hipLaunchKernelGGL(uds::k_window_draw, dim3((unsigned)((B + uds::WINDOW_THREADS - 1) / uds::WINDOW_THREADS)), dim3(uds::WINDOW_THREADS), 0, st, k);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(UDS_EHIP, "%s: draw launch -> %s", what, hipGetErrorString(e));
  hipLaunchKernelGGL(uds::k_window_bump, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long *>(count), (unsigned long long)B);
  return launched(what, hipGetLastError());
}

// ---- Model-predictive control (kernels_mpc.hpp).  The scenario objective of a population of predicted horizons
// (objective_pred_tf, envs/scenario/astlingen.py:75-99) and its reverse mode share their checks; `out` is obj or d_preds.
static int mpc_objective(const char *what, const float *preds, const float *q_in0, int64_t q0_stride, const float *g, bool backward, int64_t pop,
                         int64_t T, int64_t N, int64_t C, const float *w_flood, const float *w_out, const float *w_smooth, const float *gamma,
                         float *out, uds_stream_t stream) {
  UDS_REQUIRE(preds && q_in0 && out && (g || !backward), "%s: NULL argument", what);
  UDS_REQUIRE(C >= 2 && C <= 8, "%s: C=%lld outside [2, 8]", what, (long long)C);
  UDS_REQUIRE(T >= 1 && T <= 4096, "%s: T=%lld outside [1, 4096]", what, (long long)T);
  UDS_REQUIRE(pop >= 0 && pop <= ((int64_t)1 << 20) && N >= 1 && N <= ((int64_t)1 << 24), "%s: pop=%lld (at most 2^20) N=%lld (1 to 2^24)", what,
              (long long)pop, (long long)N);
  UDS_REQUIRE((pop * T * N + uds::MPC_THREADS - 1) / uds::MPC_THREADS < INT32_MAX, "%s: pop * T * N = %lld too large for one launch", what,
              (long long)(pop * T * N));
  UDS_REQUIRE(q0_stride == 0 || q0_stride == N, "%s: q0_stride=%lld (0 = one shared row, N = %lld = one row per candidate)", what, (long long)q0_stride,
              (long long)N);
  UDS_REQUIRE(w_flood || w_out || w_smooth, "%s: no weight vector given", what);
  UDS_REQUIRE(aligned16(preds) && aligned16(q_in0) && aligned16(g) && aligned16(w_flood) && aligned16(w_out) && aligned16(w_smooth) && aligned16(gamma) &&
                  aligned16(out),
              "%s: every pointer must be 16-byte aligned", what);
  if (pop == 0) return UDS_OK;
  uds::MpcObjectiveArgs a{preds, q_in0, g, w_flood, w_out, w_smooth, gamma, backward ? nullptr : out, backward ? out : nullptr, q0_stride, pop,
                          (int)T, (int)N, (int)C};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (backward)
    hipLaunchKernelGGL(uds::k_mpc_objective_backward, dim3((unsigned)((pop * T * N + uds::MPC_THREADS - 1) / uds::MPC_THREADS)), dim3(uds::MPC_THREADS), 0,
                       st, a);
  else
    hipLaunchKernelGGL(uds::k_mpc_objective, dim3((unsigned)pop), dim3(uds::MPC_THREADS), 0, st, a);
  return launched(what, hipGetLastError());
}

int uds_mpc_objective(const float *preds, const float *q_in0, int64_t q0_stride, int64_t pop, int64_t T, int64_t N, int64_t C, const float *w_flood,
                      const float *w_out, const float *w_smooth, const float *gamma, float *obj, uds_stream_t stream) {
  return mpc_objective("uds_mpc_objective", preds, q_in0, q0_stride, nullptr, false, pop, T, N, C, w_flood, w_out, w_smooth, gamma, obj, stream);
}

int uds_mpc_objective_backward(const float *preds, const float *q_in0, int64_t q0_stride, const float *g, int64_t pop, int64_t T, int64_t N, int64_t C,
                               const float *w_flood, const float *w_out, const float *w_smooth, const float *gamma, float *d_preds,
                               uds_stream_t stream) {
  return mpc_objective("uds_mpc_objective_backward", preds, q_in0, q0_stride, g, true, pop, T, N, C, w_flood, w_out, w_smooth, gamma, d_preds, stream);
}

// The two steps of a cross-entropy iteration share the limits of their sizes.
static int ce_check_sizes(const char *what, int64_t pop, int64_t n_var) {
  UDS_REQUIRE(pop >= 2 && pop <= uds::CE_MAX, "%s: pop=%lld outside [2, %d]", what, (long long)pop, uds::CE_MAX);
  UDS_REQUIRE(n_var >= 1 && n_var <= uds::CE_MAX, "%s: n_var=%lld outside [1, %d]", what, (long long)n_var, uds::CE_MAX);
  return UDS_OK;
}

int uds_ce_draw(const float *mean, const float *std, int64_t n_var, int64_t pop, uint64_t seed, uint64_t *count, float *out, uds_stream_t stream) {
  const char *what = "uds_ce_draw";
  UDS_REQUIRE(mean && std && count && out, "%s: NULL argument", what);
  if (int rc = ce_check_sizes(what, pop, n_var)) return rc;
  UDS_REQUIRE(aligned16(mean) && aligned16(std) && aligned16(count) && aligned16(out), "%s: every pointer must be 16-byte aligned", what);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uds::CeDrawArgs k{mean, std, reinterpret_cast<const unsigned long long *>(count), out, (unsigned long long)seed, (int)n_var, (int)pop};
  hipLaunchKernelGGL(uds::k_ce_draw, dim3((unsigned)((pop * n_var + uds::MPC_THREADS - 1) / uds::MPC_THREADS)), dim3(uds::MPC_THREADS), 0, st, k);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(UDS_EHIP, "%s: draw launch -> %s", what, hipGetErrorString(e));
  hipLaunchKernelGGL(uds::k_window_bump, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long *>(count), (unsigned long long)pop);
  return launched(what, hipGetLastError());
}

int uds_ce_update(const float *y, const float *obj, int64_t pop, int64_t n_var, int64_t n_elite, double smooth, double std_min, float *mean, float *std,
                  float *best_y, float *best_obj, int32_t *status, uds_stream_t stream) {
  const char *what = "uds_ce_update";
  UDS_REQUIRE(y && obj && mean && std && best_y && best_obj && status, "%s: NULL argument", what);
  if (int rc = ce_check_sizes(what, pop, n_var)) return rc;
  UDS_REQUIRE(n_elite >= 1 && n_elite <= pop, "%s: n_elite=%lld outside [1, pop=%lld]", what, (long long)n_elite, (long long)pop);
  UDS_REQUIRE(smooth >= 0 && smooth <= 1 && std_min >= 0 && std_min < INFINITY, "%s: smooth=%g (0 to 1) std_min=%g (finite, not negative)", what, smooth,
              std_min);
  UDS_REQUIRE(aligned16(y) && aligned16(obj) && aligned16(mean) && aligned16(std) && aligned16(best_y) && aligned16(best_obj) && aligned16(status),
              "%s: every pointer must be 16-byte aligned", what);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uds::CeUpdateArgs k{y, obj, mean, std, best_y, best_obj, status, (float)smooth, (float)std_min, (int)pop, (int)n_var, (int)n_elite};
  hipLaunchKernelGGL(uds::k_ce_update, dim3((unsigned)n_var), dim3(uds::MPC_THREADS), 0, st, k);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(UDS_EHIP, "%s: update launch -> %s", what, hipGetErrorString(e));
  hipLaunchKernelGGL(uds::k_ce_commit, dim3(1), dim3(uds::MPC_THREADS), 0, st, k);
  return launched(what, hipGetLastError());
}

int uds_flow_balance(const uds_csr_t *inc_n, const float *sign, const float *flow, int64_t S, const float *scale_in,
                     const float *scale_out, float *q_in, float *q_out, uds_stream_t stream) {
  UDS_REQUIRE(inc_n && sign && flow && scale_in && scale_out && q_in && q_out, "uds_flow_balance: NULL argument");
  UDS_REQUIRE(S >= 0 && S <= 65535, "uds_flow_balance: S=%lld outside [0,65535]", (long long)S);
  if (S == 0 || inc_n->n_rows == 0) return UDS_OK;
  uds::FlowArgs a{inc_n->d_rowptr, inc_n->d_col, sign, flow, scale_in, scale_out, q_in, q_out, (int)inc_n->n_rows,
                  (int)inc_n->n_cols, (int)S};
  return launched("uds_flow_balance", uds::launch_flow_balance(a, static_cast<hipStream_t>(stream)));
}

int uds_diffusion_forward(const uds_csr_t *csr, const float *vals, const float *c0, const float *r, const float *tot, int64_t S, int64_t C,
                          int act, float *out, uds_stream_t stream) {
  UDS_REQUIRE(csr && vals && c0 && r && tot && out, "uds_diffusion_forward: NULL argument");
  UDS_REQUIRE(S >= 0 && S <= 65535 && C > 0 && C % 4 == 0, "uds_diffusion_forward: S=%lld C=%lld (needs S <= 65535, C %% 4 == 0)", (long long)S,
              (long long)C);
  UDS_REQUIRE(act >= 0 && act <= 4, "uds_diffusion_forward: unknown activation %d", act);
  UDS_REQUIRE(aligned16(vals) && aligned16(c0) && aligned16(out), "uds_diffusion_forward: vals / c0 / out must be 16-byte aligned");
  if (S == 0 || csr->n_rows == 0) return UDS_OK;
  uds::DiffusionArgs a{csr->d_rowptr, csr->d_col, vals, c0, r, tot, out, (int)csr->n_rows, (int)csr->n_cols, (int)(C / 4), act};
  return launched("uds_diffusion_forward", uds::launch_diffusion(a, (int)S, static_cast<hipStream_t>(stream)));
}

int64_t uds_diffusion_backward_workspace_floats(int64_t n_rows, int64_t S, int64_t C, int64_t K1) {
  if (n_rows < 0 || S < 0 || C <= 0 || C % 4 || C > 256 || K1 < 1 || K1 > uds::DIFF_KMAX) return -1;
  return uds::diffusion_bwd_plan(n_rows, S, C, K1).total;
}

// The S / C / K1 ranges and the activation of the Diffusion entries that take the layer's (C, K1) kernel
static int diffusion_check_ranges(const char *what, int64_t S, int64_t C, int64_t K1, int act) {
  UDS_REQUIRE(S >= 0 && S <= 65535 && C > 0 && C % 4 == 0 && C <= 256 && K1 >= 1 && K1 <= uds::DIFF_KMAX,
              "%s: S=%lld C=%lld K1=%lld (needs S <= 65535, C %% 4 == 0, C <= 256, 1 <= K1 <= %d)", what, (long long)S, (long long)C,
              (long long)K1, uds::DIFF_KMAX);
  UDS_REQUIRE(act >= 0 && act <= 4, "%s: unknown activation %d", what, act);
  return UDS_OK;
}

// uds_diffusion_backward (table: the (nnz, C) table `vals` and c0 (C,)) and uds_diffusion_backward_m (theta (C, K1) alone)
static int diffusion_backward(const char *what, bool table, const uds_csr_t *csr, const uds_csr_t *csr_t, const int32_t *perm_t, const float *a,
                              const float *vals, const float *c0, const float *theta, const float *r, const float *tot, const float *y,
                              const float *gy, int64_t S, int64_t C, int64_t K1, int act, float *workspace, float *dr, float *dtheta,
                              uds_stream_t stream) {
  UDS_REQUIRE(csr && csr_t && (table ? c0 : theta) && dtheta, "%s: NULL argument", what);
  if (int rc = diffusion_check_ranges(what, S, C, K1, act)) return rc;
  UDS_REQUIRE(csr_t->n_rows == csr->n_cols && csr_t->n_cols == csr->n_rows && csr_t->nnz == csr->nnz,
              "%s: csr_t (%lld x %lld, %lld entries) is not the transpose of a %lld x %lld pattern with %lld entries", what,
              (long long)csr_t->n_rows, (long long)csr_t->n_cols, (long long)csr_t->nnz, (long long)csr->n_rows, (long long)csr->n_cols,
              (long long)csr->nnz);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (S == 0 || csr->n_cols == 0) {           // no dr to write; dtheta = 0 (no snapshot, or no column to sum over)
    UDS_HIP_TRY(hipMemsetAsync(dtheta, 0, sizeof(float) * C * K1, st));
    return UDS_OK;
  }
  UDS_REQUIRE(r && tot && workspace && dr && (csr->nnz == 0 || (perm_t && a && (!table || vals))) && (csr->n_rows == 0 || (y && gy)),
              "%s: NULL argument", what);
  UDS_REQUIRE((table ? aligned16(vals) && aligned16(c0) : aligned16(theta)) && aligned16(y) && aligned16(gy) && aligned16(workspace),
              "%s: %s / y / gy / workspace must be 16-byte aligned", what, table ? "vals / c0" : "theta");
  const uds::DiffusionBwdPlan p = uds::diffusion_bwd_plan(csr->n_rows, S, C, K1);
  uds::DiffusionBwdArgs args{csr->d_rowptr, csr->d_col, csr_t->d_rowptr, csr_t->d_col, perm_t, a, table ? vals : nullptr,
                             table ? c0 : theta + (K1 - 1), r, tot, y, gy,
                             workspace, workspace + p.off_pth, workspace + p.off_pg, workspace + p.off_g0, dr, dtheta,
                             (int)csr->n_rows, (int)csr->n_cols, (int)S, (int)(C / 4), p.lr, (int)K1, act, p.gx, p.sy};
  if (table) return launched(what, uds::launch_diffusion_backward(args, st));
  args.c0s = (int)K1;      // c0 = the last column of theta; G goes behind the table entry's carve
  return launched(what, uds::launch_diffusion_backward_m(uds::DiffusionBwdMArgs{args, theta, workspace + p.total}, st));
}

int uds_diffusion_backward(const uds_csr_t *csr, const uds_csr_t *csr_t, const int32_t *perm_t, const float *a, const float *vals,
                           const float *c0, const float *r, const float *tot, const float *y, const float *gy, int64_t S, int64_t C,
                           int64_t K1, int act, float *workspace, float *dr, float *dtheta, uds_stream_t stream) {
  return diffusion_backward("uds_diffusion_backward", true, csr, csr_t, perm_t, a, vals, c0, nullptr, r, tot, y, gy, S, C, K1, act, workspace, dr,
                            dtheta, stream);
}

int uds_diffusion_forward_m(const uds_csr_t *csr, const float *a, const float *theta, const float *r, const float *tot, int64_t S, int64_t C,
                            int64_t K1, int act, float *out, uds_stream_t stream) {
  UDS_REQUIRE(csr && theta && r && tot && out && (csr->nnz == 0 || a), "uds_diffusion_forward_m: NULL argument");
  if (int rc = diffusion_check_ranges("uds_diffusion_forward_m", S, C, K1, act)) return rc;
  UDS_REQUIRE(aligned16(theta) && aligned16(out), "uds_diffusion_forward_m: theta / out must be 16-byte aligned");
  if (S == 0 || csr->n_rows == 0) return UDS_OK;
  int lr = 1;
  while (lr < C / 4) lr <<= 1;
  uds::DiffusionMArgs args{csr->d_rowptr, csr->d_col, a, theta, r, tot, out, (int)csr->n_rows, (int)csr->n_cols, (int)(C / 4), lr, (int)K1, act, 0};
  return launched("uds_diffusion_forward_m", uds::launch_diffusion_m(args, (int)S, static_cast<hipStream_t>(stream)));
}

static int64_t up4f(int64_t f) { return (f + 3) & ~int64_t(3); }

int64_t uds_diffusion_backward_m_workspace_floats(int64_t n_rows, int64_t S, int64_t C, int64_t K1) {
  if (n_rows < 0 || S < 0 || C <= 0 || C % 4 || C > 256 || K1 < 1 || K1 > uds::DIFF_KMAX) return -1;
  return uds::diffusion_bwd_plan(n_rows, S, C, K1).total + up4f(S * n_rows * (K1 - 1));       // the table entry's carve, then G
}

int uds_diffusion_backward_m(const uds_csr_t *csr, const uds_csr_t *csr_t, const int32_t *perm_t, const float *a, const float *theta,
                             const float *r, const float *tot, const float *y, const float *gy, int64_t S, int64_t C, int64_t K1, int act,
                             float *workspace, float *dr, float *dtheta, uds_stream_t stream) {
  return diffusion_backward("uds_diffusion_backward_m", false, csr, csr_t, perm_t, a, nullptr, nullptr, theta, r, tot, y, gy, S, C, K1, act,
                            workspace, dr, dtheta, stream);
}

static int halo_rows(const char *what, bool pack, float *x, int64_t n_x, float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x,
                     int64_t nx, const int32_t *idx_e, int64_t ne, float *buf, uds_stream_t stream) {
  UDS_REQUIRE(S >= 0 && nx >= 0 && ne >= 0 && n_x >= 0 && n_e >= 0 && F > 0 && F % 4 == 0, "%s: bad sizes (S=%lld nx=%lld ne=%lld F=%lld)", what,
              (long long)S, (long long)nx, (long long)ne, (long long)F);
  if (S == 0 || nx + ne == 0) return UDS_OK;
  UDS_REQUIRE(buf && (nx == 0 || (x && idx_x)) && (ne == 0 || (e && idx_e)), "%s: NULL argument", what);
  UDS_REQUIRE(aligned16(buf) && aligned16(x) && aligned16(e), "%s: buffers must be 16-byte aligned", what);
  UDS_REQUIRE(nx + ne < INT32_MAX && S * (nx + ne) * (F / 4) < (int64_t)INT32_MAX * 256, "%s: message too large", what);
  uds::HaloArgs a{x, e, buf, idx_x, idx_e, n_x, n_e, S * (nx + ne) * (F / 4), (int)nx, (int)ne, (int)(F / 4)};
  return launched(what, uds::launch_halo_rows(a, pack, static_cast<hipStream_t>(stream)));
}

int uds_halo_pack(const float *x, int64_t n_x, const float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx,
                  const int32_t *idx_e, int64_t ne, float *buf, uds_stream_t stream) {
  return halo_rows("uds_halo_pack", true, const_cast<float *>(x), n_x, const_cast<float *>(e), n_e, S, F, idx_x, nx, idx_e, ne, buf, stream);
}

int uds_halo_unpack(const float *buf, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx, const int32_t *idx_e, int64_t ne, float *x,
                    int64_t n_x, float *e, int64_t n_e, uds_stream_t stream) {
  return halo_rows("uds_halo_unpack", false, x, n_x, e, n_e, S, F, idx_x, nx, idx_e, ne, const_cast<float *>(buf), stream);
}

enum HaloAllOp { HALO_UNPACK, HALO_PACK, HALO_PACK_CLEAR };

static int halo_rows_all(const char *what, HaloAllOp op, float *x, int64_t n_x, float *e, int64_t n_e, int64_t S, int64_t F,
                         const int32_t *idx_x, int64_t nx, const int32_t *idx_e, int64_t ne, const int32_t *off_x, const int32_t *off_e,
                         int64_t P, float *buf, uds_stream_t stream) {
  UDS_REQUIRE(S >= 0 && S <= 65535 && nx >= 0 && ne >= 0 && n_x >= 0 && n_e >= 0 && F >= 1 && P >= 1,
              "%s: bad sizes (S=%lld nx=%lld ne=%lld F=%lld P=%lld; needs S <= 65535, F >= 1, P >= 1)", what, (long long)S, (long long)nx,
              (long long)ne, (long long)F, (long long)P);
  if (S == 0 || nx + ne == 0) return UDS_OK;
  UDS_REQUIRE(buf && off_x && off_e && (nx == 0 || (x && idx_x)) && (ne == 0 || (e && idx_e)), "%s: NULL argument", what);
  UDS_REQUIRE(nx + ne < INT32_MAX && P < INT32_MAX && F < INT32_MAX && (nx + ne) * F < (int64_t)INT32_MAX * 256, "%s: messages too large", what);
  const bool vec = F % 4 == 0 && aligned16(buf) && aligned16(x) && aligned16(e);
  uds::HaloAllArgs a{x, e, buf, idx_x, idx_e, off_x, off_e, n_x, n_e, (int)(nx + ne), (int)P, (int)F, (int)(vec ? F / 4 : F)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (op == HALO_PACK_CLEAR) return launched(what, uds::launch_halo_pack_clear_all(a, (int)S, vec, st));
  return launched(what, uds::launch_halo_rows_all(a, (int)S, op == HALO_PACK, vec, st));
}

int uds_halo_pack_all(const float *x, int64_t n_x, const float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx,
                      const int32_t *idx_e, int64_t ne, const int32_t *off_x, const int32_t *off_e, int64_t P, float *buf,
                      uds_stream_t stream) {
  return halo_rows_all("uds_halo_pack_all", HALO_PACK, const_cast<float *>(x), n_x, const_cast<float *>(e), n_e, S, F, idx_x, nx, idx_e, ne, off_x,
                       off_e, P, buf, stream);
}

int uds_halo_unpack_all(const float *buf, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx, const int32_t *idx_e, int64_t ne,
                        const int32_t *off_x, const int32_t *off_e, int64_t P, float *x, int64_t n_x, float *e, int64_t n_e,
                        uds_stream_t stream) {
  return halo_rows_all("uds_halo_unpack_all", HALO_UNPACK, x, n_x, e, n_e, S, F, idx_x, nx, idx_e, ne, off_x, off_e, P, const_cast<float *>(buf),
                       stream);
}

int uds_halo_pack_clear_all(float *x, int64_t n_x, float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx,
                            const int32_t *idx_e, int64_t ne, const int32_t *off_x, const int32_t *off_e, int64_t P, float *buf,
                            uds_stream_t stream) {
  return halo_rows_all("uds_halo_pack_clear_all", HALO_PACK_CLEAR, x, n_x, e, n_e, S, F, idx_x, nx, idx_e, ne, off_x, off_e, P, buf, stream);
}

int uds_halo_accumulate_all(const float *buf, int64_t S, int64_t F, const int32_t *off_x, const int32_t *off_e, int64_t P,
                            const int32_t *tgt_x, int64_t tx, const int32_t *tgt_e, int64_t te, const int32_t *ptr, const int32_t *src,
                            int64_t n_src, float *x, int64_t n_x, float *e, int64_t n_e, uds_stream_t stream) {
  const char *what = "uds_halo_accumulate_all";
  UDS_REQUIRE(S >= 0 && S <= 65535 && tx >= 0 && te >= 0 && n_src >= 0 && n_x >= 0 && n_e >= 0 && F >= 1 && P >= 1,
              "%s: bad sizes (S=%lld tx=%lld te=%lld n_src=%lld F=%lld P=%lld; needs S <= 65535, F >= 1, P >= 1)", what, (long long)S,
              (long long)tx, (long long)te, (long long)n_src, (long long)F, (long long)P);
  if (S == 0 || tx + te == 0) return UDS_OK;
  UDS_REQUIRE(off_x && off_e && ptr && (n_src == 0 || (buf && src)) && (tx == 0 || (x && tgt_x)) && (te == 0 || (e && tgt_e)),
              "%s: NULL argument", what);
  UDS_REQUIRE(tx + te < INT32_MAX && n_src < INT32_MAX && P < INT32_MAX && F < INT32_MAX && (tx + te) * F < (int64_t)INT32_MAX * 256,
              "%s: too many rows", what);
  const bool vec = F % 4 == 0 && aligned16(buf) && aligned16(x) && aligned16(e);
  uds::HaloAccArgs a{buf, x, e, off_x, off_e, tgt_x, tgt_e, ptr, src, n_x, n_e, (int)tx, (int)(tx + te), (int)P, (int)F, (int)(vec ? F / 4 : F)};
  return launched(what, uds::launch_halo_accumulate_all(a, (int)S, vec, static_cast<hipStream_t>(stream)));
}

int uds_roll_update(const uds_csr_t *inc_n, const float *sign, const float *span_e, const float *mini_e, const float *scale_in,
                    const float *scale_out, const float *y, int64_t cy, const float *ey, int64_t ce, const float *b, int64_t B, int64_t so,
                    int64_t T, int flood, float *x, float *ex, float *preds, uds_stream_t stream) {
  UDS_REQUIRE(inc_n && sign && span_e && mini_e && scale_in && scale_out && y && ey && b && x && ex && preds, "uds_roll_update: NULL argument");
  UDS_REQUIRE(B >= 0 && so >= 1 && T >= so && cy >= 1 && cy <= 8 && ce >= 1 && ce <= 8, "uds_roll_update: bad sizes B=%lld so=%lld T=%lld cy=%lld ce=%lld",
              (long long)B, (long long)so, (long long)T, (long long)cy, (long long)ce);
  UDS_REQUIRE(B * std::max(inc_n->n_rows, inc_n->n_cols) < INT32_MAX, "uds_roll_update: batch x rows exceeds the int32 index");
  if (B == 0) return UDS_OK;
  uds::RollArgs a{inc_n->d_rowptr, inc_n->d_col, sign, span_e, mini_e, scale_in, scale_out, y, ey, b, x, ex, preds,
                  (int)B, (int)so, (int)T, (int)inc_n->n_rows, (int)inc_n->n_cols, (int)cy, (int)ce, flood};
  return launched("uds_roll_update", uds::launch_roll_update(a, static_cast<hipStream_t>(stream)));
}

// ---- predict tail.  uds_predict_tail and uds_predict_tail_backward share tail_check: everything that needs no device first
// (inc_n is only looked into once the rest has passed).
static int tail_check(const char *what, const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey,
                      const float *a, const float *b_norm, const float *runoff, const float *h0, int64_t B, int64_t T,
                      std::initializer_list<const void *> more) {
  UDS_REQUIRE(inc_n && sign && p, "%s: NULL argument", what);
  UDS_REQUIRE(y && ey && b_norm && runoff && h0, "%s: NULL y/ey/b_norm/runoff/h0", what);
  UDS_REQUIRE(B >= 0 && T >= 1 && p->N >= 1 && p->E >= 1 && p->ce >= 2 && p->ce <= 8 && p->n_act >= 0 && p->b_channels >= 1,
              "%s: bad sizes B=%lld T=%lld N=%d E=%d ce=%d n_act=%d b_channels=%d (needs T >= 1, 2 <= ce <= 8)", what, (long long)B, (long long)T,
              p->N, p->E, p->ce, p->n_act, p->b_channels);
  const int want = (p->edge_fusion ? 1 : 3) + (p->if_flood ? 1 : 0);
  UDS_REQUIRE(p->cy == want, "%s: cy=%d does not go with edge_fusion=%d if_flood=%d (needs %d)", what, p->cy, p->edge_fusion, p->if_flood, want);
  UDS_REQUIRE(!p->act || (a && p->n_act >= 1), "%s: act needs the settings a and n_act >= 1", what);
  bool aligned = aligned16(y) && aligned16(ey) && aligned16(a) && aligned16(b_norm) && aligned16(runoff) && aligned16(h0);
  for (const void *q : more) aligned = aligned && aligned16(q);
  UDS_REQUIRE(aligned, "%s: tensors must be 16-byte aligned", what);
  UDS_REQUIRE(p->is_outfall && p->hmin && p->hmax && p->area_eps && p->ps && p->pump_in && p->pump_out && p->ny_in && p->ny_out && p->scale_in &&
                  p->scale_out && p->span_y && p->mini_y && p->offset && p->pump && p->pump_mask && p->pump_den && p->ehmax && p->from_ok &&
                  p->span_e && p->mini_e && p->from_node && p->link_node && p->link_sign,
              "%s: NULL table in uds_tail_t", what);
  UDS_REQUIRE(!p->act || (p->act_link && p->act_in && p->act_out && p->al_ptr && p->al_idx && p->ai_ptr && p->ai_idx && p->ao_ptr && p->ao_idx),
              "%s: act needs the action tables of uds_tail_t", what);
  UDS_REQUIRE(B * T * (int64_t)std::max(p->N, p->E) < INT32_MAX, "%s: batch x steps x rows exceeds the int32 index", what);
  UDS_REQUIRE(inc_n->n_rows == p->N && inc_n->n_cols == p->E, "%s: incidence pattern is %lld x %lld, uds_tail_t says N=%d E=%d", what,
              (long long)inc_n->n_rows, (long long)inc_n->n_cols, p->N, p->E);
  return UDS_OK;
}

int uds_predict_tail(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey, const float *a,
                     const float *b_norm, const float *runoff, const float *h0, int64_t B, int64_t T, float *out_y, float *out_ey,
                     uds_stream_t stream) {
  const char *what = "uds_predict_tail";
  UDS_REQUIRE(out_y && out_ey, "%s: NULL output", what);
  if (int rc = tail_check(what, inc_n, sign, p, y, ey, a, b_norm, runoff, h0, B, T, {out_y, out_ey})) return rc;
  if (B == 0) return UDS_OK;
  uds::TailArgs t{};
  t.p = *p;
  t.rowptr = inc_n->d_rowptr; t.col = inc_n->d_col; t.sign = sign;
  t.y = y; t.ey = ey; t.a = a; t.b_norm = b_norm; t.runoff = runoff; t.h0 = h0;
  t.out_y = out_y; t.out_ey = out_ey;
  t.B = (int)B; t.T = (int)T; t.C = 3 + (p->if_flood ? 1 : 0);
  return launched(what, uds::launch_tail_forward(t, static_cast<hipStream_t>(stream)));
}

int64_t uds_predict_tail_workspace_floats(int64_t N, int64_t E, int64_t B, int64_t T) {
  if (N < 0 || E < 0 || B < 0 || T < 0) return 0;
  return 3 * align4(B * T * N) + align4(B * T * E);
}

int uds_predict_tail_backward(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey, const float *a,
                              const float *b_norm, const float *runoff, const float *h0, int64_t B, int64_t T, const float *g_out_y,
                              const float *g_out_ey, float *dy, float *dey, float *da, float *dh0, float *workspace, uds_stream_t stream) {
  const char *what = "uds_predict_tail_backward";
  UDS_REQUIRE(g_out_y && g_out_ey && dy && dey && dh0 && workspace, "%s: NULL gradient / workspace", what);
  UDS_REQUIRE(!(p && p->act) || da, "%s: act needs da", what);
  if (int rc = tail_check(what, inc_n, sign, p, y, ey, a, b_norm, runoff, h0, B, T, {g_out_y, g_out_ey, dy, dey, da, dh0, workspace})) return rc;
  if (B == 0) return UDS_OK;
  uds::TailArgs t{};
  t.p = *p;
  t.rowptr = inc_n->d_rowptr; t.col = inc_n->d_col; t.sign = sign;
  t.y = y; t.ey = ey; t.a = a; t.b_norm = b_norm; t.runoff = runoff; t.h0 = h0;
  t.g_out_y = g_out_y; t.g_out_ey = g_out_ey; t.dy = dy; t.dey = dey; t.da = da; t.dh0 = dh0;
  const int64_t bn = align4(B * T * p->N);
  t.ws_qi = workspace; t.ws_qo = workspace + bn; t.ws_prev = workspace + 2 * bn; t.ws_set = workspace + 3 * bn;
  t.B = (int)B; t.T = (int)T; t.C = 3 + (p->if_flood ? 1 : 0);
  return launched(what, uds::launch_tail_backward(t, static_cast<hipStream_t>(stream)));
}

// ---- fit tail.  uds_fit_tail and uds_fit_tail_backward share fit_tail_check: tail_check (the fit tail has no runoff / previous
// depth operand: b_norm stands in for both) and the checks of the loss operands; it fills everything the two entries have in common.
int64_t uds_fit_tail_workspace_floats(int64_t N, int64_t E, int64_t B, int64_t T) {
  if (N < 0 || E < 0 || B < 0 || T < 0) return 0;
  return std::max<int64_t>(3 * uds::FIT_MAX_BLOCKS, 2 * align4(B * T * N));
}

static int fit_tail_check(const char *what, const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey,
                          const float *a, const float *b_norm, const float *y_true, const float *ey_true, const float *nwei, const float *poswei,
                          const float *ewei, const float *qw_den, const float *span_b, const float *mini_b, int64_t B, int64_t T, int64_t cyt,
                          int balance, const float *workspace, std::initializer_list<const void *> more, uds::FitTailArgs &f) {
  UDS_REQUIRE(y_true && ey_true && nwei && poswei && ewei && workspace, "%s: NULL y_true/ey_true/nwei/poswei/ewei/workspace", what);
  UDS_REQUIRE(balance == 0 || balance == 1, "%s: balance=%d (0 or 1)", what, balance);
  UDS_REQUIRE(!balance || (qw_den && span_b && mini_b), "%s: balance needs qw_den, span_b and mini_b", what);
  UDS_REQUIRE(cyt >= 3 && cyt <= 16, "%s: cyt=%lld (3 <= cyt <= 16)", what, (long long)cyt);
  UDS_REQUIRE(aligned16(y_true) && aligned16(ey_true) && aligned16(workspace), "%s: tensors must be 16-byte aligned", what);
  if (int rc = tail_check(what, inc_n, sign, p, y, ey, a, b_norm, b_norm, b_norm, B, T, more)) return rc;
  f.t.p = *p;
  f.t.rowptr = inc_n->d_rowptr; f.t.col = inc_n->d_col; f.t.sign = sign;
  f.t.y = y; f.t.ey = ey; f.t.a = a; f.t.b_norm = b_norm;
  f.t.B = (int)B; f.t.T = (int)T; f.t.C = 3 + (p->if_flood ? 1 : 0);
  f.y_true = y_true; f.ey_true = ey_true; f.nwei = nwei; f.poswei = poswei; f.ewei = ewei;
  f.qw_den = qw_den; f.span_b = span_b; f.mini_b = mini_b;
  f.cyt = (int)cyt; f.balance = balance;
  f.node_blocks = (int)uds::fit_blocks(B * T * p->N); f.link_blocks = (int)uds::fit_blocks(B * T * p->E);
  return UDS_OK;
}

int uds_fit_tail(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey, const float *a,
                 const float *b_norm, const float *y_true, const float *ey_true, const float *nwei, const float *poswei, const float *ewei,
                 const float *qw_den, const float *span_b, const float *mini_b, int64_t B, int64_t T, int64_t cyt, int balance, float *out_y,
                 float *out_ey, float *loss_sums, float *workspace, uds_stream_t stream) {
  const char *what = "uds_fit_tail";
  UDS_REQUIRE(out_y && out_ey && loss_sums, "%s: NULL output", what);
  uds::FitTailArgs f{};
  if (int rc = fit_tail_check(what, inc_n, sign, p, y, ey, a, b_norm, y_true, ey_true, nwei, poswei, ewei, qw_den, span_b, mini_b, B, T, cyt,
                              balance, workspace, {out_y, out_ey}, f))
    return rc;
  if (B == 0) return UDS_OK;
  f.t.out_y = out_y; f.t.out_ey = out_ey; f.loss_sums = loss_sums;
  f.part_node = workspace; f.part_flood = workspace + uds::FIT_MAX_BLOCKS; f.part_edge = workspace + 2 * uds::FIT_MAX_BLOCKS;
  return launched(what, uds::launch_fit_tail_forward(f, static_cast<hipStream_t>(stream)));
}

int uds_fit_tail_backward(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey, const float *a,
                          const float *b_norm, const float *y_true, const float *ey_true, const float *nwei, const float *poswei,
                          const float *ewei, const float *qw_den, const float *span_b, const float *mini_b, int64_t B, int64_t T, int64_t cyt,
                          int balance, const float *g_loss, const float *g_out_y, const float *g_out_ey, float *dy, float *dey,
                          float *workspace, uds_stream_t stream) {
  const char *what = "uds_fit_tail_backward";
  UDS_REQUIRE(g_loss && dy && dey, "%s: NULL g_loss / gradient output", what);
  uds::FitTailArgs f{};
  if (int rc = fit_tail_check(what, inc_n, sign, p, y, ey, a, b_norm, y_true, ey_true, nwei, poswei, ewei, qw_den, span_b, mini_b, B, T, cyt,
                              balance, workspace, {g_out_y, g_out_ey, dy, dey}, f))
    return rc;
  if (B == 0) return UDS_OK;
  f.g_loss = g_loss; f.t.g_out_y = g_out_y; f.t.g_out_ey = g_out_ey; f.t.dy = dy; f.t.dey = dey;
  f.t.ws_qi = workspace; f.t.ws_qo = workspace + align4(B * T * p->N);
  return launched(what, uds::launch_fit_tail_backward(f, static_cast<hipStream_t>(stream)));
}

int uds_csr_spmm(const uds_csr_t *csr, const float *val, const float *x, int64_t S, int64_t F, const float *bias,
                 int act, float *out, uds_stream_t stream) {
  UDS_REQUIRE(csr && x && out, "uds_csr_spmm: NULL csr/x/out");
  UDS_REQUIRE(S >= 0 && F > 0 && F % 4 == 0, "uds_csr_spmm: S=%lld F=%lld (F must be a positive multiple of 4)",
              (long long)S, (long long)F);
  UDS_REQUIRE(aligned16(x) && aligned16(out) && aligned16(bias), "uds_csr_spmm: x/out/bias must be 16-byte aligned");
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_csr_spmm: unknown activation %d", act);
  UDS_REQUIRE(S <= 65535, "uds_csr_spmm: S=%lld exceeds 65535 snapshots per call", (long long)S);
  if (S == 0 || csr->n_rows == 0) return UDS_OK;
  uds::SpmmArgs a{csr->d_rowptr, csr->d_col, csr->d_order, val, x, bias, out,
                  (int)csr->n_rows, (int)csr->n_cols, (int)(F / 4), act, (int)S};
  return launched("uds_csr_spmm", uds::launch_csr_spmm(a, static_cast<hipStream_t>(stream)));
}

int64_t uds_gat_workspace_floats(int64_t n, int64_t S, int64_t d) { return align4(S * n * (d + 2)); }

// ---- GATConv.  The forward aggregate entries share gat_aggregate_check, the backward entries gat_backward_check; `heads`
// selects the multi-head form of either (H checked, the per-head width called C instead of d).
static int gat_aggregate_check(const char *what, bool ptrs, const uds_csr_t *g, bool heads, int64_t H, int64_t d, int64_t S, int act,
                               const float *hx, const float *out, const float *bias) {
  UDS_REQUIRE(g && ptrs, "%s: NULL argument", what);
  UDS_REQUIRE(g->n_rows == g->n_cols, "%s: pattern must be square", what);
  if (heads) UDS_REQUIRE(H > 0 && H <= 64, "%s: H=%lld outside [1,64]", what, (long long)H);
  UDS_REQUIRE(d > 0 && d % 4 == 0 && d <= 256, "%s: %c=%lld must be a multiple of 4, at most 256", what, heads ? 'C' : 'd', (long long)d);
  UDS_REQUIRE(S >= 0 && S <= 65535, "%s: S=%lld outside [0,65535]", what, (long long)S);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "%s: unknown activation %d", what, act);
  UDS_REQUIRE(aligned16(hx) && aligned16(out) && aligned16(bias), "%s: hx/out/bias must be 16-byte aligned", what);
  return UDS_OK;
}

static int gat_backward_check(const char *what, bool ptrs, const uds_csr_t *g, const uds_csr_t *gt, bool heads, int64_t H, int64_t d, int64_t S,
                              const float *grad, const float *hx, const float *d_hx, const float *a_self, const float *a_nbr) {
  UDS_REQUIRE(g && gt && ptrs, "%s: NULL argument", what);
  UDS_REQUIRE(g->n_rows == g->n_cols && gt->n_rows == g->n_rows && gt->n_cols == g->n_cols && gt->nnz == g->nnz,
              "%s: the pattern and its transpose must be square with the same shape and entry count", what);
  if (heads) UDS_REQUIRE(H > 0 && H <= 64, "%s: H=%lld outside [1,64]", what, (long long)H);
  UDS_REQUIRE(d > 0 && d % 4 == 0 && d <= 256, "%s: %c=%lld must be a multiple of 4, at most 256", what, heads ? 'C' : 'd', (long long)d);
  UDS_REQUIRE(S >= 0 && S <= 65535, "%s: S=%lld outside [0,65535]", what, (long long)S);
  UDS_REQUIRE(aligned16(grad) && aligned16(hx) && aligned16(d_hx) && aligned16(a_self) && aligned16(a_nbr),
              "%s: grad/hx/d_hx/a_self/a_nbr must be 16-byte aligned", what);
  return UDS_OK;
}

// which single-head aggregate kernel an entry launches: each keeps its own (kernels_sparse.hpp)
enum GatKernel { GAT_PLAIN, GAT_COEF, GAT_MASKED, GAT_EX };

// the launch of the four single-head aggregate entries, and of uds_gat_forward after its projection
static int gat_aggregate_launch(const char *what, GatKernel k, const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr,
                                const float *bias, const float *edge_mask, const float *coef, int64_t S, int64_t d, int act, float *out,
                                uds_stream_t stream) {
  uds::GatArgs a{g->d_rowptr, g->d_col, g->d_order, hx, s_self, s_nbr, bias, out, (int)g->n_rows, (int)(d / 4), act, (int)S};
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
    case GAT_COEF: return launched(what, uds::launch_gat_aggregate_coef(a, coef, g->nnz, st));
    case GAT_MASKED: return launched(what, uds::launch_gat_aggregate_masked(a, edge_mask, g->nnz, st));
    case GAT_EX: return launched(what, uds::launch_gat_aggregate_ex(a, uds::GatEx{edge_mask, coef, g->nnz}, st));
    default: return launched(what, uds::launch_gat_aggregate(a, st));
  }
}

// uds_gat_aggregate, _coef (coef required), _masked (edge_mask required) and _ex (both optional)
static int gat_aggregate(const char *what, GatKernel k, const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr,
                         const float *bias, const float *edge_mask, const float *coef, int64_t S, int64_t d, int act, float *out,
                         uds_stream_t stream) {
  const bool ptrs = hx && s_self && s_nbr && out && (k != GAT_COEF || coef) && (k != GAT_MASKED || edge_mask);
  if (int rc = gat_aggregate_check(what, ptrs, g, false, 1, d, S, act, hx, out, bias)) return rc;
  if (S == 0 || g->n_rows == 0) return UDS_OK;
  return gat_aggregate_launch(what, k, g, hx, s_self, s_nbr, bias, edge_mask, coef, S, d, act, out, stream);
}

int uds_gat_forward(const uds_csr_t *g, const float *xa, int64_t fa, const float *xb, int64_t fb, int64_t S,
                    const float *W, const float *a_self, const float *a_nbr, const float *bias, int64_t d, int act,
                    float *ws, float *out, uds_stream_t stream) {
  UDS_REQUIRE(g && xa && W && a_self && a_nbr && ws && out, "uds_gat_forward: NULL argument");
  UDS_REQUIRE(g->n_rows == g->n_cols, "uds_gat_forward: pattern must be square (%lld x %lld)", (long long)g->n_rows,
              (long long)g->n_cols);
  UDS_REQUIRE(d > 0 && d % 4 == 0 && d <= 256, "uds_gat_forward: d=%lld must be a multiple of 4, at most 256", (long long)d);
  UDS_REQUIRE(S >= 0 && S <= 65535, "uds_gat_forward: S=%lld outside [0,65535]", (long long)S);
  UDS_REQUIRE(aligned16(ws) && aligned16(out) && aligned16(bias), "uds_gat_forward: workspace/out/bias must be 16-byte aligned");
  if (S == 0 || g->n_rows == 0) return UDS_OK;
  const int64_t n = g->n_rows;
  float *hx = ws;
  float *s_self = hx + S * n * d;
  float *s_nbr = s_self + S * n;
  int rc = uds_dense_act(xa, fa, xb, fb, S * n, W, nullptr, d, UDS_ACT_LINEAR, a_self, a_nbr, hx, s_self, s_nbr, stream);
  if (rc != UDS_OK) return rc;
  return gat_aggregate_launch("uds_gat_forward", GAT_PLAIN, g, hx, s_self, s_nbr, bias, nullptr, nullptr, S, d, act, out, stream);
}

int uds_gat_aggregate(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias, int64_t S,
                      int64_t d, int act, float *out, uds_stream_t stream) {
  return gat_aggregate("uds_gat_aggregate", GAT_PLAIN, g, hx, s_self, s_nbr, bias, nullptr, nullptr, S, d, act, out, stream);
}

int uds_gat_aggregate_coef(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                           const float *coef, int64_t S, int64_t d, int act, float *out, uds_stream_t stream) {
  return gat_aggregate("uds_gat_aggregate_coef", GAT_COEF, g, hx, s_self, s_nbr, bias, nullptr, coef, S, d, act, out, stream);
}

int uds_gat_aggregate_masked(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                             const float *edge_mask, int64_t S, int64_t d, int act, float *out, uds_stream_t stream) {
  return gat_aggregate("uds_gat_aggregate_masked", GAT_MASKED, g, hx, s_self, s_nbr, bias, edge_mask, nullptr, S, d, act, out, stream);
}

int uds_gat_aggregate_ex(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                         const float *edge_mask, const float *coef, int64_t S, int64_t d, int act, float *out, uds_stream_t stream) {
  return gat_aggregate("uds_gat_aggregate_ex", GAT_EX, g, hx, s_self, s_nbr, bias, edge_mask, coef, S, d, act, out, stream);
}

// uds_gat_backward_coef (what = "uds_gat_backward", the entry it grew out of) and uds_gat_backward_ex (ex: the row pass that
// takes the edge mask)
static int gat_backward(const char *what, bool ex, const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad,
                        const float *hx, const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr,
                        const float *edge_mask, const float *coef, int64_t S, int64_t d, float *alpha_ws, float *de_ws, float *d_hx,
                        float *ds_self, float *ds_nbr, uds_stream_t stream) {
  const bool ptrs = perm_t && grad && hx && s_self && s_nbr && a_self && a_nbr && alpha_ws && de_ws && d_hx && ds_self && ds_nbr;
  if (int rc = gat_backward_check(what, ptrs, g, gt, false, 1, d, S, grad, hx, d_hx, a_self, a_nbr)) return rc;
  if (S == 0 || g->n_rows == 0) return UDS_OK;
  const int d4 = (int)(d / 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uds::GatBwdRowsArgs ra{g->d_rowptr, g->d_col, grad, hx, s_self, s_nbr, alpha_ws, de_ws, ds_self,
                         (int)g->n_rows, d4, (int)S, uds::lanes_per_item(d4), g->nnz, coef, edge_mask};
  hipError_t e = ex ? uds::launch_gat_bwd_rows_ex(ra, st) : uds::launch_gat_bwd_rows(ra, st);
  if (e != hipSuccess) return fail(UDS_EHIP, "%s: row pass launch -> %s", what, hipGetErrorString(e));
  uds::GatBwdColsArgs ca{gt->d_rowptr, gt->d_col, perm_t, grad, alpha_ws, de_ws, ds_self, a_self, a_nbr, d_hx, ds_nbr,
                         (int)g->n_rows, d4, (int)S, g->nnz};
  e = uds::launch_gat_bwd_cols(ca, st);
  if (e != hipSuccess) return fail(UDS_EHIP, "%s: column pass launch -> %s", what, hipGetErrorString(e));
  return UDS_OK;
}

int uds_gat_backward(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                     const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr, int64_t S, int64_t d,
                     float *alpha_ws, float *de_ws, float *d_hx, float *ds_self, float *ds_nbr, uds_stream_t stream) {
  return uds_gat_backward_coef(g, gt, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, nullptr, S, d, alpha_ws, de_ws, d_hx, ds_self, ds_nbr, stream);
}

int uds_gat_backward_coef(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                          const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr, const float *coef, int64_t S,
                          int64_t d, float *alpha_ws, float *de_ws, float *d_hx, float *ds_self, float *ds_nbr, uds_stream_t stream) {
  return gat_backward("uds_gat_backward", false, g, gt, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, nullptr, coef, S, d, alpha_ws, de_ws, d_hx,
                      ds_self, ds_nbr, stream);
}

int uds_gat_backward_ex(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                        const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr, const float *edge_mask,
                        const float *coef, int64_t S, int64_t d, float *alpha_ws, float *de_ws, float *d_hx, float *ds_self,
                        float *ds_nbr, uds_stream_t stream) {
  return gat_backward("uds_gat_backward_ex", true, g, gt, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, edge_mask, coef, S, d, alpha_ws, de_ws,
                      d_hx, ds_self, ds_nbr, stream);
}

// workspace of uds_gat_backward_act: alpha | de (S * nnz each, rounded up to 4) | g (S * n * d) | the partials
static int64_t gat_act_parts(int64_t S, int64_t n) { return S * n < uds::GAT_ACT_WG_MAX ? S * n : uds::GAT_ACT_WG_MAX; }

int64_t uds_gat_backward_act_workspace_floats(int64_t S, int64_t n, int64_t nnz, int64_t d) {
  if (S <= 0 || n <= 0 || nnz < 0 || d <= 0) return 0;
  return 2 * align4(S * nnz) + S * n * d + 3 * d * gat_act_parts(S, n);
}

int uds_gat_backward_act(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *out, const float *gout, int act,
                         const float *hx, const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr,
                         const float *edge_mask, const float *coef, int64_t S, int64_t d, float *d_hx, float *ds_self, float *ds_nbr,
                         float *db, float *da, float *workspace, int64_t workspace_floats, uds_stream_t stream) {
  const char *what = "uds_gat_backward_act";
  const bool ptrs = perm_t && out && gout && hx && s_self && s_nbr && a_self && a_nbr && d_hx && ds_self && ds_nbr && workspace;
  if (int rc = gat_backward_check(what, ptrs, g, gt, false, 1, d, S, gout, hx, d_hx, a_self, a_nbr)) return rc;
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "%s: unknown activation %d", what, act);
  UDS_REQUIRE(aligned16(out) && aligned16(workspace), "%s: out/workspace must be 16-byte aligned", what);
  const int64_t n = g->n_rows, need = uds_gat_backward_act_workspace_floats(S, n, g->nnz, d);
  UDS_REQUIRE(workspace_floats >= need, "%s: workspace of %lld floats, %lld needed (uds_gat_backward_act_workspace_floats)", what,
              (long long)workspace_floats, (long long)need);
  if (S == 0 || n == 0) {       // nothing to walk: the parameter gradients are sums over no rows
    hipStream_t st0 = static_cast<hipStream_t>(stream);
    hipError_t e0 = db ? hipMemsetAsync(db, 0, sizeof(float) * d, st0) : hipSuccess;
    if (e0 == hipSuccess && da) e0 = hipMemsetAsync(da, 0, sizeof(float) * 2 * d, st0);
    if (e0 != hipSuccess) return fail(UDS_EHIP, "%s: memset -> %s", what, hipGetErrorString(e0));
    return UDS_OK;
  }
  const int d4 = (int)(d / 4);
  float *alpha_ws = workspace, *de_ws = alpha_ws + align4(S * g->nnz), *g_ws = de_ws + align4(S * g->nnz), *parts = g_ws + S * n * d;
  const bool linear = act == UDS_ACT_LINEAR;          // g = gout: nothing to store, the column pass gathers gout
  uds::GatBwdRowsActArgs ra;
  static_cast<uds::GatBwdRowsArgs &>(ra) = uds::GatBwdRowsArgs{g->d_rowptr, g->d_col, nullptr, hx, s_self, s_nbr, alpha_ws, de_ws, ds_self,
                                                               (int)n, d4, (int)S, uds::lanes_per_item(d4), g->nnz, coef, edge_mask};
  ra.out = out, ra.gout = gout, ra.gw = linear ? nullptr : g_ws, ra.bpart = nullptr, ra.act = act;
  uds::GatBwdColsActArgs ca;
  static_cast<uds::GatBwdColsArgs &>(ca) = uds::GatBwdColsArgs{gt->d_rowptr, gt->d_col, perm_t, linear ? gout : g_ws, alpha_ws, de_ws, ds_self,
                                                               a_self, a_nbr, d_hx, ds_nbr, (int)n, d4, (int)S, g->nnz};
  ca.hx = hx, ca.apart = nullptr;
  return launched(what, uds::launch_gat_bwd_act(ra, ca, db, da, parts, static_cast<hipStream_t>(stream)));
}

int uds_gat_aggregate_heads(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                            const float *edge_mask, const float *coef, int64_t S, int64_t H, int64_t C, int concat, int act,
                            float *out, float *alpha_out, uds_stream_t stream) {
  if (int rc = gat_aggregate_check("uds_gat_aggregate_heads", hx && s_self && s_nbr && out, g, true, H, C, S, act, hx, out, bias)) return rc;
  if (S == 0 || g->n_rows == 0) return UDS_OK;
  uds::GatHeadsArgs a{g->d_rowptr, g->d_col, g->d_order, hx, s_self, s_nbr, bias, edge_mask, coef, out, alpha_out,
                      (int)g->n_rows, (int)H, (int)(C / 4), act, (int)S, concat ? 0 : 1, g->nnz};
  return launched("uds_gat_aggregate_heads", uds::launch_gat_aggregate_heads(a, static_cast<hipStream_t>(stream)));
}

int uds_gat_backward_heads(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                           const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr,
                           const float *edge_mask, const float *coef, int64_t S, int64_t H, int64_t C, int concat,
                           float *alpha_ws, float *de_ws, float *d_hx, float *ds_self, float *ds_nbr, uds_stream_t stream) {
  const bool ptrs = perm_t && grad && hx && s_self && s_nbr && a_self && a_nbr && alpha_ws && de_ws && d_hx && ds_self && ds_nbr;
  if (int rc = gat_backward_check("uds_gat_backward_heads", ptrs, g, gt, true, H, C, S, grad, hx, d_hx, a_self, a_nbr)) return rc;
  if (S == 0 || g->n_rows == 0) return UDS_OK;
  const int c4 = (int)(C / 4);
  uds::GatBwdHeadsArgs a{g->d_rowptr, g->d_col, gt->d_rowptr, gt->d_col, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, edge_mask, coef,
                         alpha_ws, de_ws, d_hx, ds_self, ds_nbr, (int)g->n_rows, (int)H, c4, (int)S, uds::lanes_per_item(c4),
                         concat ? 0 : 1, g->nnz};
  return launched("uds_gat_backward_heads", uds::launch_gat_bwd_heads(a, static_cast<hipStream_t>(stream)));
}

int uds_csr_sddmm(const uds_csr_t *csr, const float *a, const float *b, int64_t S, int64_t F, float *out, uds_stream_t stream) {
  UDS_REQUIRE(csr && a && b && out, "uds_csr_sddmm: NULL argument");
  UDS_REQUIRE(S >= 0 && F > 0 && F % 4 == 0, "uds_csr_sddmm: S=%lld F=%lld (F must be a positive multiple of 4)", (long long)S,
              (long long)F);
  UDS_REQUIRE(aligned16(a) && aligned16(b), "uds_csr_sddmm: a/b must be 16-byte aligned");
  if (csr->nnz == 0) return UDS_OK;
  const int f4 = (int)(F / 4);
  uds::SddmmArgs sa{csr->d_rowidx, csr->d_col, a, b, out, (int)csr->n_rows, (int)csr->n_cols, f4, (int)S, uds::lanes_per_item(f4),
                    csr->nnz};
  return launched("uds_csr_sddmm", uds::launch_csr_sddmm(sa, static_cast<hipStream_t>(stream)));
}

int64_t uds_wgrad_workspace_floats(int64_t rows, int64_t F, int64_t H, int with_bias) {
  const int mt = uds::wgrad_mt((int)(F + (with_bias ? 1 : 0))), nt = uds::wgrad_nt((int)H);
  if (!mt || !nt || rows <= 0) return 0;
  return (int64_t)uds::wgrad_grid(rows) * mt * 16 * nt * 16;
}

int uds_wgrad(const float *a, const float *g, int64_t B, int64_t T, int64_t R, int64_t F, int64_t H, int64_t shift, int with_bias,
              float *workspace, float *d_kernel, float *d_bias, uds_stream_t stream) {
  UDS_REQUIRE(a && g && workspace && d_kernel, "uds_wgrad: NULL argument");
  UDS_REQUIRE(!with_bias || d_bias, "uds_wgrad: with_bias needs d_bias");
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0 && F > 0 && H > 0 && shift >= 0, "uds_wgrad: bad sizes");
  const int fr = (int)(F + (with_bias ? 1 : 0));
  const int mt = uds::wgrad_mt(fr), nt = uds::wgrad_nt((int)H);
  UDS_REQUIRE(mt && nt, "uds_wgrad: F=%lld (at most 128 rows incl. the bias row) or H=%lld (at most 64) not supported", (long long)F, (long long)H);
  UDS_REQUIRE(B * T * R < INT32_MAX, "uds_wgrad: %lld rows exceed the int32 row index", (long long)(B * T * R));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = B * T * R;
  if (rows == 0) {
    hipError_t e0 = hipMemsetAsync(d_kernel, 0, sizeof(float) * F * H, st);
    if (e0 == hipSuccess && with_bias) e0 = hipMemsetAsync(d_bias, 0, sizeof(float) * H, st);
    if (e0 != hipSuccess) return fail(UDS_EHIP, "uds_wgrad: memset -> %s", hipGetErrorString(e0));
    return UDS_OK;
  }
  const int grid = uds::wgrad_grid(rows);
  int64_t rpw = (rows + (int64_t)grid * 4 - 1) / ((int64_t)grid * 4);
  rpw = (rpw + 31) / 32 * 32;
  uds::WgradArgs wa{a, g, workspace, rows, (int)F, (int)H, with_bias ? (int)F : -1, (int)shift, (int)T, (int)R, (int)rpw};
  if (int rc = launched("uds_wgrad", uds::launch_wgrad(wa, mt, nt, grid, st))) return rc;
  hipLaunchKernelGGL(uds::k_wgrad_reduce, dim3((unsigned)((F * H + 15) / 16)), dim3(256), 0, st, workspace, grid, mt * 16, nt * 16,
                     (int)F, (int)H, d_kernel);
  if (with_bias)
    hipLaunchKernelGGL(uds::k_wgrad_reduce, dim3((unsigned)((H + 15) / 16)), dim3(256), 0, st, workspace + F * (nt * 16), grid,
                       mt * 16, nt * 16, 1, (int)H, d_bias);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UDS_EHIP, "uds_wgrad: reduce launch -> %s", hipGetErrorString(e));
  return UDS_OK;
}

int64_t uds_wgrad_wide_workspace_floats(int64_t rows, int64_t F, int64_t H, int with_bias) {
  (void)with_bias;                                             // the partial carries the bias row either way
  const uds::WgradWidePlan p = uds::wgrad_wide_plan(F, H);
  if (!p.ok || rows <= 0) return 0;
  return (int64_t)uds::wgrad_wide_grid(p, rows) * (p.ld_f + 1) * p.ld_n;
}

int uds_wgrad_wide(const float *a, const float *g, int64_t B, int64_t T, int64_t R, int64_t F, int64_t H, int64_t shift, int with_bias,
                   float *workspace, float *d_kernel, float *d_bias, uds_stream_t stream) {
  UDS_REQUIRE(a && g && workspace && d_kernel, "uds_wgrad_wide: NULL argument");
  UDS_REQUIRE(!with_bias || d_bias, "uds_wgrad_wide: with_bias needs d_bias");
  UDS_REQUIRE(B >= 0 && T > 0 && R > 0 && F > 0 && H > 0 && shift >= 0, "uds_wgrad_wide: bad sizes");
  const uds::WgradWidePlan p = uds::wgrad_wide_plan(F, H);
  UDS_REQUIRE(p.ok, "uds_wgrad_wide: F=%lld or H=%lld not supported (1 to 256 each)", (long long)F, (long long)H);
  UDS_REQUIRE(B * T * R < INT32_MAX, "uds_wgrad_wide: %lld rows exceed the int32 row index", (long long)(B * T * R));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = B * T * R;
  if (rows == 0) {
    hipError_t e0 = hipMemsetAsync(d_kernel, 0, sizeof(float) * F * H, st);
    if (e0 == hipSuccess && with_bias) e0 = hipMemsetAsync(d_bias, 0, sizeof(float) * H, st);
    if (e0 != hipSuccess) return fail(UDS_EHIP, "uds_wgrad_wide: memset -> %s", hipGetErrorString(e0));
    return UDS_OK;
  }
  const int grid = uds::wgrad_wide_grid(p, rows);
  int64_t rpw = (rows + (int64_t)grid * p.ks - 1) / ((int64_t)grid * p.ks);
  rpw = (rpw + 31) / 32 * 32;
  // T and R fit an int (rows does); a shift past T drops every term, as a shift of T does: clamp it before it is narrowed
  const int64_t sh = shift < T ? shift : T;
  uds::WgradWideArgs wa{a, g, workspace, rows, (int)F, (int)H, (int)sh, (int)T, (int)R, (int)rpw, p.rb, p.cb, p.ks};
  if (int rc = launched("uds_wgrad_wide", uds::launch_wgrad_wide(wa, p.mt, p.nt, grid, st))) return rc;
  hipLaunchKernelGGL(uds::k_wgrad_reduce, dim3((unsigned)((F * H + 15) / 16)), dim3(256), 0, st, workspace, grid, p.ld_f + 1, p.ld_n,
                     (int)F, (int)H, d_kernel);
  if (with_bias)
    hipLaunchKernelGGL(uds::k_wgrad_reduce, dim3((unsigned)((H + 15) / 16)), dim3(256), 0, st, workspace + (int64_t)p.ld_f * p.ld_n, grid,
                       p.ld_f + 1, p.ld_n, 1, (int)H, d_bias);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UDS_EHIP, "uds_wgrad_wide: reduce launch -> %s", hipGetErrorString(e));
  return UDS_OK;
}

// ---- d bias, d weight of a dense-parameter NodeEdge from g (S, R, h) and x (S, M, h) in their own layouts (kernels_node_edge_wgrad.hpp)
int uds_node_edge_wgrad_plan(int64_t R, int64_t M, int64_t S, int64_t h, int32_t *info4) {
  UDS_REQUIRE(info4 != nullptr, "uds_node_edge_wgrad_plan: info4 is NULL");
  const uds::NodeEdgeWgradPlan p = uds::node_edge_wgrad_plan(R, M, S, h);
  info4[0] = p.ks;
  info4[1] = p.pieces;
  info4[2] = p.spp;
  info4[3] = p.padded;
  return UDS_OK;
}

int64_t uds_node_edge_wgrad_workspace_bytes(int64_t R, int64_t M, int64_t S, int64_t h) {
  const uds::NodeEdgeWgradPlan p = uds::node_edge_wgrad_plan(R, M, S, h);
  return p.ks ? (int64_t)p.pieces * R * M * (int64_t)sizeof(float) : 0;
}

int uds_node_edge_wgrad(const float *g, const float *x, int64_t S, int64_t R, int64_t M, int64_t h, const float *inci, void *workspace,
                        float *d_bias, float *d_weight, uds_stream_t stream) {
  const uds::NodeEdgeWgradPlan p = uds::node_edge_wgrad_plan(R, M, S, h);
  UDS_REQUIRE(p.ks, "uds_node_edge_wgrad: S=%lld R=%lld M=%lld h=%lld not supported (h %% 4 == 0, 4 <= h <= 64, R, M >= 1, 0 <= S <= 2^24)",
              (long long)S, (long long)R, (long long)M, (long long)h);
  UDS_REQUIRE(d_bias != nullptr, "uds_node_edge_wgrad: d_bias is NULL");
  UDS_REQUIRE(!d_weight || inci, "uds_node_edge_wgrad: d_weight needs inci");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (S == 0) {
    hipError_t e0 = hipMemsetAsync(d_bias, 0, sizeof(float) * R * M, st);
    if (e0 == hipSuccess && d_weight) e0 = hipMemsetAsync(d_weight, 0, sizeof(float) * R * M, st);
    if (e0 != hipSuccess) return fail(UDS_EHIP, "uds_node_edge_wgrad: memset -> %s", hipGetErrorString(e0));
    return UDS_OK;
  }
  UDS_REQUIRE(g && x && workspace, "uds_node_edge_wgrad: NULL argument");
  UDS_REQUIRE(aligned16(g) && aligned16(x), "uds_node_edge_wgrad: g and x must be 16-byte aligned");
  uds::NodeEdgeWgradArgs a{g, x, static_cast<float *>(workspace), S, (int)R, (int)M, (int)h, p.spp, (int)p.tiles_m};
  if (int rc = launched("uds_node_edge_wgrad", uds::launch_node_edge_wgrad(a, p, st))) return rc;
  const int64_t n_out = R * M;
  hipLaunchKernelGGL(uds::k_node_edge_wgrad_reduce, dim3((unsigned)((n_out + 15) / 16)), dim3(256), 0, st, a.partial, p.pieces, n_out,
                     d_weight ? inci : nullptr, d_bias, d_weight);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UDS_EHIP, "uds_node_edge_wgrad: reduce launch -> %s", hipGetErrorString(e));
  return UDS_OK;
}

// Build (once) and upload the tile plan of kernel variant <fp, fs>.  A plan that does not fit the LDS leaves the slot
// !ok (the layer then runs unfused); only an allocation / copy failure is an error.
static int build_slot(uds_network *n, int fp, int fs) {
  uds_plan_slot &sl = n->slot[slot_index(fp, fs)];
  if (sl.built) return UDS_OK;
  sl.built = true;
  sl.fp = fp;
  sl.fs = fs;
  if ((fp == 128 || fs == 128) ? !plan_network128(n->adj->host, n->edge_adj->host, n->inc_n->host, n->inc_e->host, fp, fs, sl.plan, sl.lds_bytes)
                : !plan_network(n->adj->host, n->edge_adj->host, n->inc_n->host, n->inc_e->host, fp, fs, sl.plan, sl.lds_bytes, sl.blk_cap))
    return UDS_OK;
  hipError_t e;
  if ((e = hipMalloc(&sl.d_hdr, sizeof(int32_t) * sl.plan.hdr.size())) != hipSuccess ||
      (e = hipMalloc(&sl.d_pool, sizeof(int32_t) * sl.plan.pool.size())) != hipSuccess ||
      (e = hipMemcpy(sl.d_hdr, sl.plan.hdr.data(), sizeof(int32_t) * sl.plan.hdr.size(), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(sl.d_pool, sl.plan.pool.data(), sizeof(int32_t) * sl.plan.pool.size(), hipMemcpyHostToDevice)) != hipSuccess)
    return fail(UDS_ENOMEM, "tile plan upload -> %s", hipGetErrorString(e));
  auto upload_blocks = [&](const std::vector<int32_t> &hdr, int n_tiles, int32_t **dst) -> hipError_t {
    if (fp == 128 || fs == 128) return hipSuccess;
    std::vector<int32_t> bl;
    uds::build_ell_blocks(hdr, sl.plan.pool, n_tiles, sl.blk_cap, bl);
    hipError_t e2 = hipMalloc(dst, sizeof(int32_t) * bl.size());
    if (e2 != hipSuccess) return e2;
    return hipMemcpy(*dst, bl.data(), sizeof(int32_t) * bl.size(), hipMemcpyHostToDevice);
  };
  if ((e = upload_blocks(sl.plan.hdr, sl.plan.n_tiles, &sl.d_blocks)) != hipSuccess)
    return fail(UDS_ENOMEM, "tile block upload -> %s", hipGetErrorString(e));
  for (int side = 0; side < 2; ++side) {   // compact per-side header lists, in the merged (locality) order
    std::vector<int32_t> hs;
    for (int t = 0; t < sl.plan.n_tiles; ++t)
      if (sl.plan.hdr[(size_t)t * uds::TILE_HDR_INTS + 6] == side)
        hs.insert(hs.end(), sl.plan.hdr.begin() + (size_t)t * uds::TILE_HDR_INTS, sl.plan.hdr.begin() + (size_t)(t + 1) * uds::TILE_HDR_INTS);
    if ((e = hipMalloc(&sl.d_hdr_side[side], sizeof(int32_t) * std::max<size_t>(hs.size(), 1))) != hipSuccess ||
        (!hs.empty() && (e = hipMemcpy(sl.d_hdr_side[side], hs.data(), sizeof(int32_t) * hs.size(), hipMemcpyHostToDevice)) != hipSuccess))
      return fail(UDS_ENOMEM, "tile plan upload -> %s", hipGetErrorString(e));
    if ((e = upload_blocks(hs, (int)(hs.size() / uds::TILE_HDR_INTS), &sl.d_blocks_side[side])) != hipSuccess)
      return fail(UDS_ENOMEM, "tile block upload -> %s", hipGetErrorString(e));
  }
  sl.ok = true;
  return UDS_OK;
}

int uds_network_prepare(uds_network_t *net, int64_t fx, int64_t fe) {
  UDS_REQUIRE(net != nullptr, "uds_network_prepare: NULL network");
  if (net->adj->n_rows == 0 || net->edge_adj->n_rows == 0) return UDS_OK;
  if (fx == 128 && (fe == 128 || fe == 64)) {      // the d = 128 kernel: node tiles <fx, fe>, link tiles <fe, fx>
    int rc = build_slot(net, 128, (int)fe);
    if (rc == UDS_OK && fe == 64) rc = build_slot(net, 64, 128);
    return rc;
  }
  if (!((fx == 64 || fx == 96) && (fe == 64 || fe == 96))) return UDS_OK;
  int rc = build_slot(net, (int)fx, (int)fe);            // node tiles run <fx, fe>
  if (rc == UDS_OK) rc = build_slot(net, (int)fe, (int)fx);   // link tiles <fe, fx>
  return rc;
}

int uds_network_create(const uds_csr_t *adj, const uds_csr_t *edge_adj, const uds_csr_t *inc_n, const uds_csr_t *inc_e,
                       uds_network_t **out) {
  UDS_REQUIRE(out != nullptr, "uds_network_create: out is NULL");
  *out = nullptr;
  UDS_REQUIRE(adj && edge_adj && inc_n && inc_e, "uds_network_create: NULL pattern");
  const int64_t N = adj->n_rows, E = edge_adj->n_rows;
  UDS_REQUIRE(adj->n_cols == N && edge_adj->n_cols == E, "uds_network_create: adjacency patterns must be square");
  UDS_REQUIRE(inc_n->n_rows == N && inc_n->n_cols == E && inc_e->n_rows == E && inc_e->n_cols == N,
              "uds_network_create: incidence shapes (%lld x %lld), (%lld x %lld) do not match N=%lld E=%lld",
              (long long)inc_n->n_rows, (long long)inc_n->n_cols, (long long)inc_e->n_rows, (long long)inc_e->n_cols,
              (long long)N, (long long)E);
  uds_network *n = new (std::nothrow) uds_network;
  if (!n) return fail(UDS_ENOMEM, "uds_network_create: host allocation failed");
  n->adj = adj;
  n->edge_adj = edge_adj;
  n->inc_n = inc_n;
  n->inc_e = inc_e;
  // the tile plan of the 64-wide kernel variant is built now; 96-wide variants on request (uds_network_prepare)
  if (N > 0 && E > 0) {
    int rc = build_slot(n, 64, 64);
    if (rc != UDS_OK) {
      uds_network_destroy(n);
      return rc;
    }
  }
  *out = n;
  return UDS_OK;
}

int uds_network_destroy(uds_network_t *net) {
  if (!net) return UDS_OK;
  for (uds_plan_slot &sl : net->slot) {
    hipFree(sl.d_hdr);
    hipFree(sl.d_pool);
    hipFree(sl.d_hdr_side[0]);
    hipFree(sl.d_hdr_side[1]);
    hipFree(sl.d_blocks);
    hipFree(sl.d_blocks_side[0]);
    hipFree(sl.d_blocks_side[1]);
  }
  delete net;
  return UDS_OK;
}

int uds_network_plan_info(const uds_network_t *net, int32_t *info8) {
  UDS_REQUIRE(net && info8, "uds_network_plan_info: NULL argument");
  const uds_plan_slot &sl = net->slot[0];   // the plan for 64-float rows (d = 64 layers)
  info8[0] = (sl.ok ? 1 : 0) | ((net->slot[1].ok && net->slot[2].ok) ? 2 : 0) | (net->slot[3].ok ? 4 : 0) | (net->slot[4].ok ? 8 : 0) |
             ((net->slot[5].ok && net->slot[6].ok) ? 16 : 0) | ((sl.ok && ws_plan_ok(sl)) ? 32 : 0);
  info8[1] = sl.plan.side[0].n_tiles;
  info8[2] = sl.plan.side[1].n_tiles;
  info8[3] = sl.plan.p_cap;
  info8[4] = sl.plan.q_cap;
  info8[5] = sl.blk_cap ? sl.blk_cap : sl.plan.meta_cap;
  info8[6] = (int32_t)sl.lds_bytes;
  info8[7] = sl.plan.t_max[0] * 1000 + sl.plan.t_max[1];
  return UDS_OK;
}

int uds_fused_chunk(int64_t S, int64_t working_tiles, int64_t *chunk) {
  UDS_REQUIRE(chunk != nullptr, "uds_fused_chunk: NULL argument");
  UDS_REQUIRE(S >= 1 && working_tiles >= 1 && S < ((int64_t)1 << 31) && working_tiles < ((int64_t)1 << 31),
              "uds_fused_chunk: bad sizes S=%lld tiles=%lld (1 .. 2^31 - 1)", (long long)S, (long long)working_tiles);
  *chunk = pick_chunk(S, working_tiles);
  return UDS_OK;
}

int uds_network_fused_launches(const uds_network_t *net, int64_t fx, int64_t fe, int64_t d, int32_t *info11) {
  UDS_REQUIRE(net && info11, "uds_network_fused_launches: NULL argument");
  fused_launch l[2];
  const int n = fused_launches(net, fx, fe, d / 2, d, l);
  std::fill(info11, info11 + 11, 0);
  info11[0] = n;
  for (int i = 0; i < n; ++i) {
    int32_t *o = info11 + 1 + 5 * i;
    o[0] = l[i].kernel;
    o[1] = l[i].fp;
    o[2] = l[i].fs;
    o[3] = l[i].side_mask;
    o[4] = l[i].n_tiles;
  }
  return UDS_OK;
}

// ---- host-only tile planner access (integer bookkeeping, testable without a GPU) ----
int uds_tile_plan_create(const int32_t *adj_rowptr, const int32_t *adj_col, const int32_t *eadj_rowptr, const int32_t *eadj_col,
                         const int32_t *incn_rowptr, const int32_t *incn_col, const int32_t *ince_rowptr, const int32_t *ince_col,
                         int64_t n_node, int64_t n_edge, int32_t t_node, int32_t t_link, int32_t p_limit, int32_t q_limit,
                         uds_tile_plan_t **out) {
  UDS_REQUIRE(out != nullptr, "uds_tile_plan_create: out is NULL");
  *out = nullptr;
  UDS_REQUIRE(adj_rowptr && adj_col && eadj_rowptr && eadj_col && incn_rowptr && ince_rowptr, "uds_tile_plan_create: NULL array");
  UDS_REQUIRE(n_node > 0 && n_edge > 0 && t_node >= 1 && t_link >= 1, "uds_tile_plan_create: bad sizes");
  auto mk = [](const int32_t *rp, const int32_t *c, int64_t r, int64_t cc) {
    uds::HostCsr h;
    h.n_rows = r;
    h.n_cols = cc;
    h.rowptr.assign(rp, rp + r + 1);
    h.col.assign(c, c + rp[r]);
    return h;
  };
  uds_tile_plan *tp = new (std::nothrow) uds_tile_plan;
  if (!tp) return fail(UDS_ENOMEM, "uds_tile_plan_create: host allocation failed");
  tp->plan = uds::build_network_plan(mk(adj_rowptr, adj_col, n_node, n_node), mk(eadj_rowptr, eadj_col, n_edge, n_edge),
                                     mk(incn_rowptr, incn_col, n_node, n_edge), mk(ince_rowptr, ince_col, n_edge, n_node),
                                     t_node, t_link, p_limit, q_limit);
  *out = tp;
  return UDS_OK;
}

int uds_tile_plan_destroy(uds_tile_plan_t *tp) {
  delete tp;
  return UDS_OK;
}

int uds_tile_plan_sizes(const uds_tile_plan_t *tp, int64_t *n_tiles, int64_t *pool_len, int32_t *caps3) {
  UDS_REQUIRE(tp != nullptr, "uds_tile_plan_sizes: NULL plan");
  if (n_tiles) *n_tiles = tp->plan.n_tiles;
  if (pool_len) *pool_len = (int64_t)tp->plan.pool.size();
  if (caps3) {
    caps3[0] = tp->plan.p_cap;
    caps3[1] = tp->plan.q_cap;
    caps3[2] = tp->plan.meta_cap;
  }
  return UDS_OK;
}

int uds_tile_plan_refine_counts(const uds_tile_plan_t *tp, int64_t *counts3) {
  UDS_REQUIRE(tp && counts3, "uds_tile_plan_refine_counts: NULL argument");
  counts3[0] = tp->plan.side[0].n_fill + tp->plan.side[1].n_fill;
  counts3[1] = tp->plan.side[0].n_move + tp->plan.side[1].n_move;
  counts3[2] = tp->plan.side[0].n_dissolve + tp->plan.side[1].n_dissolve;
  return UDS_OK;
}

int uds_tile_plan_copy(const uds_tile_plan_t *tp, int32_t *hdr_out, int32_t *pool_out) {
  UDS_REQUIRE(tp && hdr_out && pool_out, "uds_tile_plan_copy: NULL argument");
  std::memcpy(hdr_out, tp->plan.hdr.data(), sizeof(int32_t) * tp->plan.hdr.size());
  std::memcpy(pool_out, tp->plan.pool.data(), sizeof(int32_t) * tp->plan.pool.size());
  return UDS_OK;
}

int uds_tile_plan_blocks(const uds_tile_plan_t *tp, int32_t *blocks_out, int64_t *stride_out) {
  UDS_REQUIRE(tp != nullptr, "uds_tile_plan_blocks: NULL plan");
  const int cap = uds::ell_block_cap(tp->plan.hdr, tp->plan.pool, tp->plan.n_tiles);
  UDS_REQUIRE(cap >= 0, "uds_tile_plan_blocks: a tile has more than 255 primary / 256 secondary rows (byte-wide local indices)");
  if (stride_out) *stride_out = cap;
  if (!blocks_out) return UDS_OK;
  std::vector<int32_t> bl;
  uds::build_ell_blocks(tp->plan.hdr, tp->plan.pool, tp->plan.n_tiles, cap, bl);
  std::memcpy(blocks_out, bl.data(), sizeof(int32_t) * (size_t)cap * tp->plan.n_tiles);
  return UDS_OK;
}

int64_t uds_spatial_workspace_floats(const uds_network_t *net, int64_t S, int64_t h, int64_t d) {
  if (!net) return 0;
  const int64_t N = net->adj->n_rows, E = net->edge_adj->n_rows;
  // packed weight fragments (fused path) + x_e (E,h) + e_x (N,h) + agg_n (N,h) + agg_e (E,h) + hx,s (N,d+2) + he,s (E,d+2)
  return PACKED_WEIGHT_FLOATS + S * 2 * (N + E) * h + align4(S * N * (d + 2)) + align4(S * E * (d + 2));
}


int64_t uds_spatial_packed_bytes(void) { return PACKED_WEIGHT_FLOATS * 4; }

int uds_spatial_pack_weights(const uds_spatial_params_t *p, int64_t fx, int64_t fe, int64_t h, int64_t d, void *packed_out,
                             uds_stream_t stream) {
  UDS_REQUIRE(p && packed_out && p->xe_k && p->ex_k && p->gx_k && p->ge_k, "uds_spatial_pack_weights: NULL argument");
  const bool wide = h == uds::F128_H && d == uds::F128_D && fx == 128 && (fe == 128 || fe == 64);
  UDS_REQUIRE(wide || (h == uds::FUSED_H && d == uds::FUSED_D && (fx == 64 || fx == 96) && (fe == 64 || fe == 96)),
              "uds_spatial_pack_weights: the fused kernels take h=32, d=64, fx, fe in {64, 96} or h=64, d=128, fx=128, fe in {64, 128} (got h=%lld d=%lld "
              "fx=%lld fe=%lld)", (long long)h, (long long)d, (long long)fx, (long long)fe);
  UDS_REQUIRE(aligned16(packed_out), "uds_spatial_pack_weights: output must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint4 *wq = reinterpret_cast<uint4 *>(packed_out);
  hipError_t he;
  // node side: secondary = links (xe_k on e), big = gx_k; link side: secondary = nodes (ex_k on x), big = ge_k
  const int o_small = wide ? 2048 : 768, o_big = wide ? 6144 : 2048;      // uint4 per packed kernel
  if ((he = pack_weights(p->xe_k, (int)fe, (int)h, wq, st)) != hipSuccess ||
      (he = pack_weights(p->gx_k, (int)(fx + h), (int)d, wq + o_small, st)) != hipSuccess ||
      (he = pack_weights(p->ex_k, (int)fx, (int)h, wq + o_small + o_big, st)) != hipSuccess ||
      (he = pack_weights(p->ge_k, (int)(fe + h), (int)d, wq + 2 * o_small + o_big, st)) != hipSuccess)
    return fail(UDS_EHIP, "uds_spatial_pack_weights: launch -> %s", hipGetErrorString(he));
  if (!wide && fx == 64 && fe == 64) {      // the wave-specialised kernel's P2 multiplies with 32x32x16 MFMAs: the big kernels in that fragment order too
    const int total = (int)((fx + h) / 16) * (int)(d / 32) * 64;
    hipLaunchKernelGGL(uds::k_pack_weight_frags32, dim3((total + 255) / 256), dim3(256), 0, st, p->gx_k, (int)(fx + h), (int)d, wq + WS_BIG32_OFF);
    hipLaunchKernelGGL(uds::k_pack_weight_frags32, dim3((total + 255) / 256), dim3(256), 0, st, p->ge_k, (int)(fe + h), (int)d, wq + WS_BIG32_OFF + WS_BIG32_LEN);
    const int ts = (int)(fe / 16) * (int)(h / 32) * 64;
    hipLaunchKernelGGL(uds::k_pack_weight_frags32, dim3((ts + 255) / 256), dim3(256), 0, st, p->xe_k, (int)fe, (int)h, wq + WS_SMALL32_OFF);
    hipLaunchKernelGGL(uds::k_pack_weight_frags32, dim3((ts + 255) / 256), dim3(256), 0, st, p->ex_k, (int)fx, (int)h, wq + WS_SMALL32_OFF + WS_SMALL32_LEN);
    return launched("uds_spatial_pack_weights", hipGetLastError());
  }
  return UDS_OK;
}

int uds_spatial_layer_forward(const uds_network_t *net, const uds_spatial_params_t *p, const float *x, int64_t fx,
                              const float *e, int64_t fe, int64_t S, int64_t h, int64_t d, int act, int flags, float *ws,
                              float *out_x, float *out_e, uds_stream_t stream) {
  return uds_spatial_layer_forward_split(net, p, x, fx, nullptr, 0, e, fe, nullptr, 0, S, h, d, act, flags, ws, out_x, out_e, stream);
}

static int spatial_forward_impl(const uds_network_t *net, const uds_spatial_params_t *p, const float *x, int64_t fxa,
                                const float *xb, int64_t fxb, const float *e, int64_t fea, const float *eb, int64_t feb,
                                const float *rem_x, const float *rem_e, int64_t S, int64_t h, int64_t d, int act, int flags,
                                float *ws, float *out_x, float *out_e, uds_stream_t stream);

int uds_spatial_layer_forward_split(const uds_network_t *net, const uds_spatial_params_t *p, const float *x, int64_t fxa,
                                    const float *xb, int64_t fxb, const float *e, int64_t fea, const float *eb, int64_t feb,
                                    int64_t S, int64_t h, int64_t d, int act, int flags, float *ws, float *out_x, float *out_e,
                                    uds_stream_t stream) {
  return spatial_forward_impl(net, p, x, fxa, xb, fxb, e, fea, eb, feb, nullptr, nullptr, S, h, d, act, flags, ws, out_x, out_e, stream);
}

int uds_spatial_layer_forward_rem(const uds_network_t *net, const uds_spatial_params_t *p, const float *x, int64_t fx,
                                  const float *e, int64_t fe, const float *rem_x, const float *rem_e, int64_t S, int64_t h,
                                  int64_t d, int act, int flags, float *ws, float *out_x, float *out_e, uds_stream_t stream) {
  UDS_REQUIRE(rem_x && rem_e, "uds_spatial_layer_forward_rem: NULL remainder");
  UDS_REQUIRE(aligned16(rem_x) && aligned16(rem_e), "uds_spatial_layer_forward_rem: rem_x / rem_e must be 16-byte aligned");
  return spatial_forward_impl(net, p, x, fx, nullptr, 0, e, fe, nullptr, 0, rem_x, rem_e, S, h, d, act, flags | UDS_FLAG_REQUIRE_FUSED, ws,
                              out_x, out_e, stream);
}

static int spatial_forward_impl(const uds_network_t *net, const uds_spatial_params_t *p, const float *x, int64_t fxa,
                                const float *xb, int64_t fxb, const float *e, int64_t fea, const float *eb, int64_t feb,
                                const float *rem_x, const float *rem_e, int64_t S, int64_t h, int64_t d, int act, int flags,
                                float *ws, float *out_x, float *out_e, uds_stream_t stream) {
  UDS_REQUIRE(net && p && x && e && ws && out_x && out_e, "uds_spatial_layer_forward: NULL argument");
  UDS_REQUIRE((xb != nullptr) == (fxb > 0) && (eb != nullptr) == (feb > 0), "uds_spatial_layer_forward_split: xb/fxb or eb/feb disagree");
  UDS_REQUIRE((!xb || (fxa == 64 && fxb == 32)) && (!eb || (fea == 64 && feb == 32)),
              "uds_spatial_layer_forward_split: a split input must be 64 + 32 columns (got %lld+%lld, %lld+%lld)", (long long)fxa,
              (long long)fxb, (long long)fea, (long long)feb);
  UDS_REQUIRE(aligned16(xb) && aligned16(eb), "uds_spatial_layer_forward_split: xb/eb must be 16-byte aligned");
  const int64_t fx = fxa + fxb, fe = fea + feb;
  if (xb || eb) flags |= UDS_FLAG_REQUIRE_FUSED;     // only the fused kernel reads split rows
  UDS_REQUIRE(p->xe_k && p->ex_k && p->ne_n_val && p->ne_e_val && p->gx_k && p->gx_as && p->gx_an && p->ge_k &&
                  p->ge_as && p->ge_an,
              "uds_spatial_layer_forward: NULL parameter tensor");
  UDS_REQUIRE(h > 0 && h % 4 == 0 && d > 0 && d % 4 == 0, "uds_spatial_layer_forward: h=%lld d=%lld must be multiples of 4",
              (long long)h, (long long)d);
  UDS_REQUIRE(act >= UDS_ACT_LINEAR && act <= UDS_ACT_HARD_SIGMOID, "uds_spatial_layer_forward: unknown activation %d", act);
  UDS_REQUIRE(out_x != x && out_e != e, "uds_spatial_layer_forward: outputs must not alias inputs");
  UDS_REQUIRE(aligned16(x) && aligned16(e) && aligned16(ws) && aligned16(out_x) && aligned16(out_e),
              "uds_spatial_layer_forward: x/e/workspace/outputs must be 16-byte aligned");
  const int64_t N = net->adj->n_rows, E = net->edge_adj->n_rows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (S == 0) return UDS_OK;

  // which kernels, on which tiles: decided in one place (fused_launches), which uds_network_fused_launches reports
  fused_launch launches[2];
  const int n_launch = (flags & UDS_FLAG_EXACT_FP32) ? 0 : fused_launches(net, fx, fe, h, d, launches);
  if (n_launch && launches[0].kernel == UDS_KERNEL_FUSED_CS) {
    // d = 128: the column-split fused kernel (kernels_fused128.hpp); 64-wide link rows -> one launch per side
    UDS_REQUIRE(aligned16(p->xe_b) && aligned16(p->ex_b) && aligned16(p->gx_as) && aligned16(p->gx_an) && aligned16(p->gx_b) &&
                    aligned16(p->ge_as) && aligned16(p->ge_an) && aligned16(p->ge_b),
                "uds_spatial_layer_forward: bias / attention vectors must be 16-byte aligned");
    const uint4 *wq = reinterpret_cast<const uint4 *>(p->packed);
    if (!wq) {
      int rc = uds_spatial_pack_weights(p, fx, fe, h, d, ws, stream);
      if (rc != UDS_OK) return rc;
      wq = reinterpret_cast<const uint4 *>(ws);
    } else {
      UDS_REQUIRE(aligned16(wq), "uds_spatial_layer_forward: packed weights must be 16-byte aligned");
    }
    uds::FusedArgs a;
    a.blocks = nullptr;
    a.side[0] = uds::FusedSide{x, e, nullptr, nullptr, out_x, wq, wq + 2048, nullptr, nullptr, p->xe_b, p->gx_as, p->gx_an, p->gx_b, p->ne_n_val, (int)N, (int)E, rem_x};
    a.side[1] = uds::FusedSide{e, x, nullptr, nullptr, out_e, wq + 8192, wq + 10240, nullptr, nullptr, p->ex_b, p->ge_as, p->ge_an, p->ge_b, p->ne_e_val, (int)E, (int)N, rem_e};
    a.S = (int)S;
    a.act = act;
    a.dbg = nullptr;
#ifdef UDS_PHASE_TIMING
    a.dbg = reinterpret_cast<unsigned long long *>(ws + PACKED_WEIGHT_FLOATS);
#endif
    auto launch_side = [&](const fused_launch &l) {       // l.side < 0: both sides in one launch
      const uds_plan_slot &u = net->slot[l.slot];
      a.hdr = l.side < 0 ? u.d_hdr : u.d_hdr_side[l.side];
      a.pool = u.d_pool;
      a.n_tiles = l.n_tiles;
      a.p_cap = u.plan.p_cap;
      a.q_cap = u.plan.q_cap;
      a.meta_cap = u.plan.meta_cap;
      a.side_mask = l.side_mask;
      if ((rem_x || rem_e) && a.p_cap > 64) return hipErrorInvalidValue;      // one P1.5 unit per wave (kernels_fused128.hpp)
      const int64_t chunk = pick_chunk(S, l.n_tiles);
      a.chunk = (int)chunk;
      const int grid = (int)(((S + chunk - 1) / chunk) * l.n_tiles);
      if (l.fp == 128) return l.fs == 128 ? launch_fused128<128, 128>(a, grid, u.lds_bytes, st) : launch_fused128<128, 64>(a, grid, u.lds_bytes, st);
      return launch_fused128<64, 128>(a, grid, u.lds_bytes, st);
    };
    hipError_t he = hipSuccess;
    for (int i = 0; i < n_launch && he == hipSuccess; ++i) he = launch_side(launches[i]);
    if (he != hipSuccess) return fail(UDS_EHIP, "uds_spatial_layer_forward: fused d=128 launch -> %s", hipGetErrorString(he));
    return UDS_OK;
  }
  UDS_REQUIRE((!rem_x && !rem_e) || (h == uds::FUSED_H && d == uds::FUSED_D && fxa == 64 && fea == 64),
              "uds_spatial_layer_forward_rem: the remainder goes into the d = 128 fused kernel or the 64-wide d = 64 one (fx=%lld fe=%lld h=%lld d=%lld, plan %d)",
              (long long)fxa, (long long)fea, (long long)h, (long long)d, (int)(net->slot[4].ok));
  if (flags & UDS_FLAG_REQUIRE_FUSED)
    UDS_REQUIRE(n_launch, "uds_spatial_layer_forward: fused kernel unavailable (plan %d, fx=%lld fe=%lld h=%lld d=%lld)",
                (int)net->slot[slot_index((int)fx, (int)fe)].ok, (long long)fx, (long long)fe, (long long)h, (long long)d);
  if (n_launch) {
    UDS_REQUIRE(aligned16(p->xe_b) && aligned16(p->ex_b) && aligned16(p->gx_as) && aligned16(p->gx_an) && aligned16(p->gx_b) &&
                    aligned16(p->ge_as) && aligned16(p->ge_an) && aligned16(p->ge_b),
                "uds_spatial_layer_forward: bias / attention vectors must be 16-byte aligned");
    hipError_t he;
    const uint4 *wq = reinterpret_cast<const uint4 *>(p->packed);
    if (!wq) {   // no pre-packed weights: split them now into the head of the workspace
      int rc = uds_spatial_pack_weights(p, fx, fe, h, d, ws, stream);
      if (rc != UDS_OK) return rc;
      wq = reinterpret_cast<const uint4 *>(ws);
    } else {
      UDS_REQUIRE(aligned16(wq), "uds_spatial_layer_forward: packed weights must be 16-byte aligned");
    }
    const uint4 *w_small_n = wq, *w_big_n = wq + 768, *w_small_e = wq + 768 + 2048, *w_big_e = wq + 2 * 768 + 2048;
    uds::FusedArgs a;
    a.blocks = nullptr;
    const bool has32 = fx == 64 && fe == 64;
    a.side[0] = uds::FusedSide{x, e, xb, eb, out_x, w_small_n, w_big_n, has32 ? wq + WS_BIG32_OFF : nullptr, has32 ? wq + WS_SMALL32_OFF : nullptr, p->xe_b, p->gx_as, p->gx_an, p->gx_b, p->ne_n_val, (int)N, (int)E, rem_x};
    a.side[1] = uds::FusedSide{e, x, eb, xb, out_e, w_small_e, w_big_e, has32 ? wq + WS_BIG32_OFF + WS_BIG32_LEN : nullptr, has32 ? wq + WS_SMALL32_OFF + WS_SMALL32_LEN : nullptr, p->ex_b, p->ge_as, p->ge_an, p->ge_b, p->ne_e_val, (int)E, (int)N, rem_e};
    int64_t lds_need = 0;
    auto use_plan = [&](const fused_launch &l) {     // l.side < 0: both sides (merged tile list), else that side's tiles only
      const uds_plan_slot &u = net->slot[l.slot];
      const int side = l.side;
      a.hdr = side < 0 ? u.d_hdr : u.d_hdr_side[side];
      a.pool = u.d_pool;
      a.n_tiles = l.n_tiles;
      a.p_cap = u.plan.p_cap;
      a.q_cap = u.plan.q_cap;
      a.meta_cap = u.blk_cap;      // LDS ints of the tile block (header + fixed-width index lists)
      a.blocks = side < 0 ? u.d_blocks : u.d_blocks_side[side];
      lds_need = u.lds_bytes;
    };
    a.S = (int)S;
    a.act = act;
    a.dbg = nullptr;
#ifdef UDS_PHASE_TIMING
    a.dbg = reinterpret_cast<unsigned long long *>(ws + PACKED_WEIGHT_FLOATS);   // diagnostic build: stamps go to the (otherwise unused) workspace
#endif
    auto set_chunk = [&](int64_t working_tiles) {     // (a launch for one side only skips the other side's tiles at once)
      int64_t chunk = pick_chunk(S, working_tiles);
#ifdef UDS_KNOBS
      if (const char *ov = std::getenv("UDS_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(S, std::atoll(ov)));   // experiment builds only (UDS_DEFINES=-DUDS_KNOBS)
#endif
      a.chunk = (int)chunk;
      return (int)(((S + chunk - 1) / chunk) * a.n_tiles);
    };
    he = hipSuccess;
    for (int i = 0; i < n_launch && he == hipSuccess; ++i) {      // one launch, or node tiles <fx, fe> then link tiles <fe, fx>
      const fused_launch &l = launches[i];
      use_plan(l);
      a.side_mask = l.side_mask;
      const int grid = set_chunk(l.n_tiles);
      const bool ws = l.kernel == UDS_KERNEL_FUSED_WS;
      const int64_t ws_lds = uds::fused_ws_lds_bytes(a.p_cap, a.q_cap, a.meta_cap);
      UDS_REQUIRE(ws || (!rem_x && !rem_e), "uds_spatial_layer_forward_rem: the wave-specialised d = 64 kernel cannot take this network's plan (p_cap %d, q_cap %d, %lld B of LDS)",
                  a.p_cap, a.q_cap, (long long)ws_lds);
      if (ws) he = launch_fused_ws(a, grid, ws_lds, st);
      else if (l.fp == l.fs) he = (l.fp == 64) ? launch_fused<64, 64>(a, grid, lds_need, st) : launch_fused<96, 96>(a, grid, lds_need, st);
      else he = (l.fp == 64) ? launch_fused<64, 96>(a, grid, lds_need, st) : launch_fused<96, 64>(a, grid, lds_need, st);
    }
    if (he != hipSuccess) return fail(UDS_EHIP, "uds_spatial_layer_forward: fused launch -> %s", hipGetErrorString(he));
    return UDS_OK;
  }

  float *base = ws + PACKED_WEIGHT_FLOATS;
  float *x_e = base;                  // (S,E,h)
  float *e_x = x_e + S * E * h;       // (S,N,h)
  float *agg_n = e_x + S * N * h;     // (S,N,h)
  float *agg_e = agg_n + S * N * h;   // (S,E,h)
  float *gat_ws_n = agg_e + S * E * h;        // S*N*(d+2)
  float *gat_ws_e = gat_ws_n + align4(S * N * (d + 2));
  int rc;
  if ((rc = uds_dense_act(e, fe, nullptr, 0, S * E, p->xe_k, p->xe_b, h, act, nullptr, nullptr, x_e, nullptr, nullptr, stream))) return rc;
  if ((rc = uds_dense_act(x, fx, nullptr, 0, S * N, p->ex_k, p->ex_b, h, act, nullptr, nullptr, e_x, nullptr, nullptr, stream))) return rc;
  if ((rc = uds_csr_spmm(net->inc_n, p->ne_n_val, x_e, S, h, nullptr, UDS_ACT_LINEAR, agg_n, stream))) return rc;
  if ((rc = uds_csr_spmm(net->inc_e, p->ne_e_val, e_x, S, h, nullptr, UDS_ACT_LINEAR, agg_e, stream))) return rc;
  if ((rc = uds_gat_forward(net->adj, x, fx, agg_n, h, S, p->gx_k, p->gx_as, p->gx_an, p->gx_b, d, act, gat_ws_n, out_x, stream))) return rc;
  if ((rc = uds_gat_forward(net->edge_adj, e, fe, agg_e, h, S, p->ge_k, p->ge_as, p->ge_an, p->ge_b, d, act, gat_ws_e, out_e, stream))) return rc;
  return UDS_OK;
}

}  // extern "C"
