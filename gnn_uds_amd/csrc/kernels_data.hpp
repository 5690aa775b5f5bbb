// Training-data kernels: the reference draws one random batch of sliding windows per epoch on the host (DataGenerator.prepare_batch,
// dataloader.py:106-143, windows cut as dataloader.py:93-95,144-169), normalises five tensors (main.py:219) and uploads them
// (main.py:209-232).  Here the event series stay on the device:
//
//   k_window_batch   ONE launch fills x, a, b, y, ex, ey of B windows from the time-major series, normalised or raw
//   k_window_draw    B window starts from a weighted table: Philox4x32-10 counter j = count + i, u = (r * total) >> 64, binary search
//   k_window_bump    one thread, after the draw on the same stream: count += B (no draw thread reads count after it moved)
//
// k_window_batch: workgroup (blockIdx.x = window * (seq_in + t_out) + row, blockIdx.y = chunk of 256 items of that row); the items
// of a row are its N nodes, then its E links, then (output rows only) its n_act settings.  A node thread reads its 16 bytes of
// `states` (float4) plus flood / tide, a link thread its 16 bytes of `edge_states`: consecutive threads read consecutive addresses.
// Every offset is 64-bit.  A window whose rows are not all inside [0, Ttot) reads nothing and has every output element set to NaN
// (window starts are device values the host cannot check; the NaN then fails fit_eval's finite test).  Normalisation is
// (v - min) / span with a correctly rounded division, the arithmetic of Emulator.normalize.  Plain vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_sparse.hpp"      // philox4x32_10

namespace uds {

constexpr int WINDOW_THREADS = 256;
constexpr int WINDOW_DRAW_MAX = 4096;

struct WindowBatchArgs {
  const float *states, *flood, *edge_states, *settings, *tide;      // settings / tide may be NULL
  const float *span_x, *min_x, *span_b, *min_b, *span_y, *min_y, *span_e, *min_e;      // (N, cx) (N, cb) (N, cx) (E, 4); a NULL span = raw
  const int32_t *starts;
  float *x, *a, *b, *y, *ex, *ey;
  int64_t Ttot;
  int N, E, n_act, seq_in, t_out, if_flood;
};

__device__ __forceinline__ float window_norm(float v, const float *span, const float *mini, int64_t i) {
  return span ? __fdiv_rn(v - mini[i], span[i]) : v;
}

__global__ __launch_bounds__(WINDOW_THREADS) void k_window_batch(WindowBatchArgs p) {
  const int rows = p.seq_in + p.t_out;
  const int64_t w = (int64_t)blockIdx.x / rows;
  const int row = (int)((int64_t)blockIdx.x - w * rows);
  const bool out_row = row >= p.seq_in;
  const int t = out_row ? row - p.seq_in : row;
  const int64_t item = (int64_t)blockIdx.y * WINDOW_THREADS + threadIdx.x;
  const int64_t s = p.starts[w];
  const bool valid = s >= 0 && s + rows <= p.Ttot;
  const int64_t g = s + row;                                      // the series row (used only when valid)
  const float nan = __uint_as_float(0x7FC00000u);
  const int cx = p.if_flood ? 5 : 4, cb = p.tide ? 2 : 1;
  if (item < p.N) {
    const int64_t n = item;
    float4 st = make_float4(nan, nan, nan, nan);
    float fl = nan, td = nan;
    if (valid) {
      st = reinterpret_cast<const float4 *>(p.states)[g * p.N + n];
      fl = p.flood[g * p.N + n];
      if (p.tide) td = p.tide[g * p.N + n];
    }
    const float bit = valid ? (fl > 0.f ? 1.f : 0.f) : nan;
    const float last = out_row ? fl : st.w;                       // X ends in r, Y in the flooding volume
    const float *span = out_row ? p.span_y : p.span_x, *mini = out_row ? p.min_y : p.min_x;
    float *dst = (out_row ? p.y + (w * p.t_out + t) * (int64_t)p.N * cx : p.x + (w * p.seq_in + t) * (int64_t)p.N * cx) + n * cx;
    const int64_t c0 = n * cx;
    int c = 0;
    dst[c] = window_norm(st.x, span, mini, c0 + c); ++c;
    dst[c] = window_norm(st.y - st.w, span, mini, c0 + c); ++c;
    dst[c] = window_norm(st.z, span, mini, c0 + c); ++c;
    if (p.if_flood) { dst[c] = window_norm(bit, span, mini, c0 + c); ++c; }
    dst[c] = window_norm(last, span, mini, c0 + c);
    if (out_row) {
      float *db = p.b + ((w * p.t_out + t) * (int64_t)p.N + n) * cb;
      db[0] = window_norm(st.w, p.span_b, p.min_b, n * cb);
      if (p.tide) db[1] = window_norm(td, p.span_b, p.min_b, n * cb + 1);
    }
  } else if (item < (int64_t)p.N + p.E) {
    const int64_t e = item - p.N;
    float4 es = make_float4(nan, nan, nan, nan);
    if (valid) es = reinterpret_cast<const float4 *>(p.edge_states)[g * p.E + e];
    const float v0 = window_norm(es.x, p.span_e, p.min_e, e * 4), v1 = window_norm(es.y, p.span_e, p.min_e, e * 4 + 1),
                v2 = window_norm(es.z, p.span_e, p.min_e, e * 4 + 2);
    if (out_row) {
      float *d = p.ey + ((w * p.t_out + t) * (int64_t)p.E + e) * 3;
      d[0] = v0; d[1] = v1; d[2] = v2;
    } else {
      const float v3 = window_norm(es.w, p.span_e, p.min_e, e * 4 + 3);
      reinterpret_cast<float4 *>(p.ex)[(w * p.seq_in + t) * (int64_t)p.E + e] = make_float4(v0, v1, v2, v3);
    }
  } else if (out_row && item < (int64_t)p.N + p.E + p.n_act) {
    const int64_t j = item - p.N - p.E;
    p.a[(w * p.t_out + t) * (int64_t)p.n_act + j] = valid ? p.settings[g * p.n_act + j] : nan;      // never normalised
  }
}

struct WindowDrawArgs {
  const int32_t *table;                 // (W) window starts
  const unsigned long long *cum;        // (W) inclusive prefix sums of the weights
  const unsigned long long *count;      // draws made so far
  int32_t *out;                         // (B)
  unsigned long long seed;
  int W, B;
};

__global__ __launch_bounds__(WINDOW_THREADS) void k_window_draw(WindowDrawArgs p) {
  const int i = blockIdx.x * WINDOW_THREADS + threadIdx.x;
  if (i >= p.B) return;
  unsigned r[4];
  philox4x32_10(*p.count + (unsigned long long)i, 0ull, p.seed, r);
  const unsigned long long u = __umul64hi(((unsigned long long)r[0] << 32) | r[1], p.cum[p.W - 1]);      // < total
  int lo = 0, hi = p.W - 1;                                         // the smallest k with cum[k] > u
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p.cum[mid] > u) hi = mid; else lo = mid + 1;
  }
  p.out[i] = p.table[lo];
}

__global__ void k_window_bump(unsigned long long *count, unsigned long long by) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *count = *count + by;
}

}  // namespace uds
