"""Row GEMM, streaming Conv1D, split-K weight gradient and the fp32 Dense kernels: the route mirror, the case tables and the fp64
references shared by tests/test_rowgemm_route_math.py (CPU: every case reaches the route it claims, every instantiation is
reached, the references carry signal) and tests/test_gpu_rowgemm_routes.py (GPU parity at every route).

The route mirror restates, in plain Python, the host-side `if`s that pick a template instantiation; each function cites the lines
it restates.  route(case) names the instantiation a case runs:
  ('small', MB, KT)                               k_rowgemm_small<MB, KT>
  ('persistent', MB, ring, stage, xcd)            k_rowgemm_mfma<MB, 4, ring, stage>, xcd = the seg > 0 row mapping
  ('stream', D, act_class, dir, n_seg, last_len)  k_conv3_stream<D, ACT>, act_class 'relu' / 'linear' / 'generic'
  ('wgrad', MT, NT, grid)                         k_wgrad_mfma<MT, NT> on `grid` workgroups
  ('embed', F) / ('tiled', CG)                    k_embed_act<F> / k_dense_act<CG> (kernels_dense.hpp)
"""
import numpy as np
import torch

from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from tests.util import f32_exact

ACTS = ('linear', 'relu', 'tanh', 'sigmoid', 'hard_sigmoid')
LDS_BYTES = 160 * 1024

# ---------------------------------------------------------------------------------------------------------------------------
# route mirror
# ---------------------------------------------------------------------------------------------------------------------------
ROWGEMM_SMALL_ROWS = 16 * 8 * 256            # kernels_rowgemm.hpp:350
ROWGEMM_SMALL_KT = (2, 3, 4, 6, 9, 12)       # kernels_rowgemm.hpp:397-404, the instantiated depths of launch_rowgemm_small
WAVE_TILE = 64                               # NB * 16 with NB = 4 (kernels_rowgemm.hpp:457-459, :425)
CS_WAVES = 8                                 # kernels_conv_stream.hpp:34-40


def rowgemm_mb(fo):
    """kernels_rowgemm.hpp:447."""
    return 1 if fo <= 16 else 2 if fo <= 32 else 4


def rowgemm_lds_bytes(K, MB, ring, stage=True):
    """kernels_rowgemm.hpp:408-411."""
    cg = 2 if MB >= 2 else 1
    return (K // 32) * MB * 2 * 1024 + 256 + 8 * ring * 2048 + (8 * 16 * (16 * cg + 4) * 4 if stage else 0)


def rowgemm_ring(K, MB):
    """kernels_rowgemm.hpp:413-419: 5, 3, -3 (ring 3 without the output tile), 2, or 0 when the weights do not fit."""
    if rowgemm_lds_bytes(K, MB, 5) <= LDS_BYTES:
        return 5
    if rowgemm_lds_bytes(K, MB, 3) <= LDS_BYTES:
        return 3
    if rowgemm_lds_bytes(K, MB, 3, False) <= LDS_BYTES:
        return -3
    if rowgemm_lds_bytes(K, MB, 2) <= LDS_BYTES:
        return 2
    return 0


def ring2_reachable(MB):
    """True when some K / 32 gives ring 2 for this MB.  The ring-2 layout keeps the output tile, the ring -3 layout drops it; for
    MB = 2 and 4 the tile (18 KiB) outweighs the third ring slot (16 KiB), so whatever fits ring 2 already fits ring -3."""
    return any(rowgemm_ring(32 * kt, MB) == 2 for kt in range(1, 129))


def rowgemm_is_small(rows, K):
    """launch_rowgemm_small, kernels_rowgemm.hpp:395-406."""
    return rows <= ROWGEMM_SMALL_ROWS and K // 32 in ROWGEMM_SMALL_KT


def rowgemm_xcd_seg(taps, R):
    """launch_rowgemm_r, kernels_rowgemm.hpp:429-433: the seg of the XCD-aware row mapping, 0 = consecutive wave-tiles."""
    if taps > 1 and R >= 64 * WAVE_TILE:
        return ((R + 7) // 8 + 15) // 16 * 16
    return 0


def conv_stream_supported(taps, F, fo, dil):
    """kernels_conv_stream.hpp:183-186."""
    return taps == 3 and F == 64 and fo == 64 and abs(dil) in (1, 2, 4)


def conv_stream_taken(B, R, taps, F, fo, dil, ldo):
    """uds_rowgemm_forward_cat, uds_hip.hip:612-614: the shape, at least 256 (batch element, 16-row block) streams, a plain
    output (ldo == f_out)."""
    return conv_stream_supported(taps, F, fo, dil) and B * ((R + 15) // 16) >= 256 and ldo == fo


def conv_stream_segments(B, R, T, d):
    """launch_conv_stream, kernels_conv_stream.hpp:188-196: (n_seg, seg_len, length of the last segment)."""
    streams = B * ((R + 15) // 16)
    n_seg = (256 * CS_WAVES) // streams
    n_seg = max(1, min(n_seg, T // (4 * d)))
    seg_len = (T + n_seg - 1) // n_seg
    n_seg = (T + seg_len - 1) // seg_len
    return n_seg, seg_len, T - (n_seg - 1) * seg_len


def stream_act_class(act):
    """launch_conv_stream_t, kernels_conv_stream.hpp:176-180."""
    return act if act in ('relu', 'linear') else 'generic'


def wgrad_mt(f_rows):
    """kernels_wgrad.hpp:137-143."""
    need = (f_rows + 15) // 16
    for have in (1, 2, 3, 5, 7, 8):
        if have >= need:
            return have
    return 0


def wgrad_nt(H):
    """kernels_wgrad.hpp:144."""
    return 1 if H <= 16 else 2 if H <= 32 else 4 if H <= 64 else 0


def wgrad_grid(rows):
    """kernels_wgrad.hpp:145."""
    return min(512, (rows + 127) // 128)


def wgrad_rows_per_wave(rows):
    """uds_wgrad, uds_hip.hip:1178-1180."""
    grid = wgrad_grid(rows)
    rpw = (rows + grid * 4 - 1) // (grid * 4)
    return (rpw + 31) // 32 * 32


def wgrad_empty_waves(rows):
    """Waves of the launch whose r_begin >= rows (kernels_wgrad.hpp:40-43)."""
    rpw = wgrad_rows_per_wave(rows)
    return sum(1 for w in range(wgrad_grid(rows) * 4) if w * rpw >= rows)


def dense_route(rows, fa, fo, taps):
    """launch_dense_act, kernels_dense.hpp:240-260."""
    if taps == 0 and fa <= 8 and fo % 4 == 0 and rows >= 64:
        return ('embed', fa)
    groups = (fo + 3) // 4
    for cg in (1, 2, 4, 8, 16, 32, 64):
        if groups <= cg:
            return ('tiled', cg)
    return ('tiled', 64)


def embed_blocks(rows, fo):
    """launch_embed_f, kernels_dense.hpp:229-235: the grid, a multiple of f4 / gcd(256, f4)."""
    f4 = fo // 4
    blocks = min((rows * f4 + 255) // 256, 256 * 16)
    g, x = f4, 256
    while x % 2 == 0 and g % 2 == 0:
        x //= 2
        g //= 2
    return max(g, blocks // g * g)


def route(c):
    kind = c['kind']
    if kind == 'rowgemm':
        B, T, R, taps, dil, fo = c['B'], c['T'], c['R'], c['taps'], c['dil'], c['fo']
        F = c['F'] + c['F2']
        rows, K = B * T * R, taps * F
        if conv_stream_taken(B, R, taps, F, fo, dil, c['ldo']):
            n_seg, _, last = conv_stream_segments(B, R, T, abs(dil))
            return ('stream', abs(dil), stream_act_class(c['act']), 1 if dil > 0 else -1, n_seg, last)
        MB = rowgemm_mb(fo)
        if rowgemm_is_small(rows, K):
            return ('small', MB, K // 32)
        ring = rowgemm_ring(K, MB)
        assert ring != 0, 'the entry refuses this shape'
        return ('persistent', MB, abs(ring), ring > 0, rowgemm_xcd_seg(taps, R) > 0)
    if kind == 'wgrad':
        return ('wgrad', wgrad_mt(c['F'] + (1 if c['bias'] else 0)), wgrad_nt(c['H']), wgrad_grid(c['B'] * c['T'] * c['R']))
    if kind == 'dense':
        return dense_route(c['B'] * c['T'] * c['R'], c['F'], c['fo'], c['taps'])
    raise ValueError(kind)


# every instantiation the launch code can select
ALL_SMALL = {('small', mb, kt) for mb in (1, 2, 4) for kt in ROWGEMM_SMALL_KT}
ALL_PERSISTENT = {(mb, ring, stage) for mb in (1, 2, 4) for ring, stage in ((5, True), (3, True), (3, False), (2, True))
                  if (ring, stage) != (2, True) or ring2_reachable(mb)}
ALL_STREAM = {(d, a, s) for d in (1, 2, 4) for a in ('relu', 'linear', 'generic') for s in (1, -1)}
ALL_WGRAD = {(mt, nt) for mt in (1, 2, 3, 5, 7, 8) for nt in (1, 2, 4)}
ALL_EMBED = {('embed', f) for f in range(1, 9)}
ALL_TILED = {('tiled', cg) for cg in (1, 2, 4, 8, 16, 32, 64)}


# ---------------------------------------------------------------------------------------------------------------------------
# case tables: every case carries the route it claims (tests/test_rowgemm_route_math.py holds them to route())
# ---------------------------------------------------------------------------------------------------------------------------
def _rg(B, T, R, F, taps, dil, fo, act, claims, bias=True, F2=0, ldo=None, col0=0, same_as=None):
    """x (B,T,R,F) [| x2 (B,T,R,F2)], kernel (taps, F + F2, fo); the output is the column block [col0, col0 + fo) of rows of ldo.
    same_as: the case whose data this one runs on (its first B batch elements)."""
    return dict(kind='rowgemm', B=B, T=T, R=R, F=F, taps=taps, dil=dil, fo=fo, act=act, bias=bias, F2=F2, ldo=fo if ldo is None else ldo,
                col0=col0, claims=claims, same_as=same_as)


# every (MB, KT), KT built from one wide tap and from several; f_out 1, 3, 16 | 17, 32 | 33, 50, 64; rows 1, 15, 16, 17;
# R = 5, T = 7, B = 2: a 16-row block spans four time steps, one of them (rows 32 .. 47) both batch elements
SMALL_CASES = [
    _rg(1, 1, 1, 64, 1, 1, 1, 'linear', ('small', 1, 2)),
    _rg(2, 7, 5, 32, 2, 1, 3, 'relu', ('small', 1, 2)),
    _rg(1, 1, 15, 96, 1, 1, 16, 'tanh', ('small', 1, 3)),
    _rg(2, 7, 5, 32, 3, -1, 1, 'sigmoid', ('small', 1, 3)),
    _rg(1, 1, 16, 128, 1, 1, 3, 'hard_sigmoid', ('small', 1, 4)),
    _rg(1, 3, 17, 32, 4, 2, 16, 'relu', ('small', 1, 4), bias=False),             # shifts 6, 4, 2, 0 against T = 3
    _rg(1, 1, 17, 192, 1, 1, 1, 'relu', ('small', 1, 6)),
    _rg(2, 7, 5, 64, 3, -2, 3, 'linear', ('small', 1, 6)),
    _rg(1, 1, 33, 288, 1, 1, 16, 'linear', ('small', 1, 9)),
    _rg(1, 5, 20, 96, 3, 4, 3, 'tanh', ('small', 1, 9)),                          # 2 * dil >= T
    _rg(1, 1, 100, 384, 1, 1, 1, 'sigmoid', ('small', 1, 12)),
    _rg(2, 4, 9, 128, 3, -4, 16, 'relu', ('small', 1, 12)),                       # |dil| >= T: only the last tap is live
    _rg(1, 1, 16, 64, 1, 1, 32, 'relu', ('small', 2, 2)),
    _rg(2, 7, 5, 32, 2, -1, 17, 'tanh', ('small', 2, 2)),
    _rg(1, 1, 17, 96, 1, 1, 17, 'linear', ('small', 2, 3)),
    _rg(2, 7, 5, 32, 3, 2, 32, 'hard_sigmoid', ('small', 2, 3)),
    _rg(1, 1, 1, 128, 1, 1, 32, 'sigmoid', ('small', 2, 4)),
    _rg(3, 5, 11, 64, 2, -2, 17, 'relu', ('small', 2, 4), bias=False),
    _rg(1, 1, 15, 192, 1, 1, 17, 'relu', ('small', 2, 6)),
    _rg(2, 7, 5, 96, 2, 4, 32, 'linear', ('small', 2, 6)),
    _rg(1, 1, 40, 288, 1, 1, 32, 'tanh', ('small', 2, 9)),
    _rg(2, 3, 7, 96, 3, -4, 17, 'sigmoid', ('small', 2, 9)),                      # |dil| > T
    _rg(1, 1, 16, 384, 1, 1, 17, 'hard_sigmoid', ('small', 2, 12)),
    _rg(1, 6, 30, 64, 6, 1, 32, 'relu', ('small', 2, 12)),
    _rg(1, 1, 17, 64, 1, 1, 64, 'relu', ('small', 4, 2)),
    _rg(2, 7, 5, 32, 2, 1, 33, 'linear', ('small', 4, 2)),
    _rg(1, 1, 1, 96, 1, 1, 50, 'tanh', ('small', 4, 3)),
    _rg(2, 7, 5, 32, 3, -1, 64, 'relu', ('small', 4, 3)),
    _rg(1, 1, 15, 128, 1, 1, 33, 'sigmoid', ('small', 4, 4)),
    _rg(2, 7, 5, 64, 2, 4, 50, 'hard_sigmoid', ('small', 4, 4)),
    _rg(1, 1, 16, 192, 1, 1, 64, 'linear', ('small', 4, 6), bias=False),
    _rg(2, 7, 5, 64, 3, -2, 64, 'tanh', ('small', 4, 6)),                         # the streaming shape, far too few streams
    _rg(1, 1, 17, 288, 1, 1, 50, 'relu', ('small', 4, 9)),
    _rg(1, 9, 23, 96, 3, 2, 33, 'relu', ('small', 4, 9)),
    _rg(1, 1, 300, 384, 1, 1, 64, 'relu', ('small', 4, 12)),
    _rg(2, 5, 13, 128, 3, -1, 64, 'relu', ('small', 4, 12)),
]

# K = 384 just over the small kernel's row limit: the 3 x 128 -> 64 Conv1D of a d = 128 emulator (kernels_rowgemm.hpp:135-136, :444).
# One batch element of it (16400 rows) is a k_rowgemm_small<4, 12> problem on the same rows.
K384_CASE = _rg(2, 5, 3280, 128, 3, 1, 64, 'relu', ('persistent', 4, 3, False, False))
K384_HEAD = _rg(1, 5, 3280, 128, 3, 1, 64, 'relu', ('small', 4, 12), same_as=K384_CASE)

# the 3 x 64 -> 64 shape into a column block (ldo = 128: not the streaming route; 36900 rows: not the small kernel) ...
XCD_BLOCK_CASES = [
    _rg(1, 9, 4100, 64, 3, 2, 64, 'relu', ('persistent', 4, 5, True, True), ldo=128, col0=64),
    _rg(1, 9, 4100, 64, 3, -1, 64, 'linear', ('persistent', 4, 5, True, True), ldo=128, col0=64),
]
# ... and the same data, plain output: 257 streams, k_conv3_stream
XCD_BLOCK_STREAM = [
    _rg(1, 9, 4100, 64, 3, 2, 64, 'relu', ('stream', 2, 'relu', 1, 1, 9), same_as=XCD_BLOCK_CASES[0]),
    _rg(1, 9, 4100, 64, 3, -1, 64, 'linear', ('stream', 1, 'linear', -1, 2, 4), same_as=XCD_BLOCK_CASES[1]),
]

# every reachable (MB, ring): the first and the last K / 32 of each ring; rows below, at and above one 64-row wave-tile
PERSISTENT_CASES = [
    _rg(1, 1, 63, 32, 1, 1, 64, 'relu', ('persistent', 4, 5, True, False)),
    _rg(1, 1, 300, 160, 1, 1, 50, 'tanh', ('persistent', 4, 5, True, False)),
    _rg(1, 1, 64, 224, 1, 1, 33, 'linear', ('persistent', 4, 5, True, False)),
    _rg(1, 1, 65, 256, 1, 1, 64, 'relu', ('persistent', 4, 3, True, False)),
    _rg(1, 1, 200, 352, 1, 1, 50, 'sigmoid', ('persistent', 4, 3, True, False), bias=False),
    _rg(1, 1, 129, 416, 1, 1, 64, 'hard_sigmoid', ('persistent', 4, 3, False, False)),
    K384_CASE,
    _rg(1, 1, 1, 480, 1, 1, 32, 'relu', ('persistent', 2, 5, True, False)),
    _rg(1, 1, 64, 512, 1, 1, 17, 'linear', ('persistent', 2, 3, True, False)),
    _rg(1, 1, 250, 736, 1, 1, 32, 'tanh', ('persistent', 2, 3, True, False)),
    _rg(1, 1, 65, 768, 1, 1, 32, 'relu', ('persistent', 2, 3, False, False)),
    _rg(1, 1, 130, 864, 1, 1, 17, 'sigmoid', ('persistent', 2, 3, False, False)),
    _rg(1, 1, 63, 1088, 1, 1, 16, 'relu', ('persistent', 1, 5, True, False)),
    _rg(1, 1, 64, 1120, 1, 1, 3, 'linear', ('persistent', 1, 3, True, False)),
    _rg(1, 1, 300, 1600, 1, 1, 16, 'hard_sigmoid', ('persistent', 1, 3, True, False)),
    _rg(1, 1, 65, 1632, 1, 1, 1, 'tanh', ('persistent', 1, 3, False, False)),
    _rg(1, 1, 200, 1760, 1, 1, 16, 'relu', ('persistent', 1, 3, False, False)),
    _rg(1, 1, 17, 1792, 1, 1, 3, 'sigmoid', ('persistent', 1, 2, True, False)),
    _rg(1, 1, 257, 1856, 1, 1, 16, 'relu', ('persistent', 1, 2, True, False)),
    # 258 wave-tiles on 256 workgroups: two waves of two workgroups get a tile, the rest one
    _rg(1, 1, 16500, 32, 1, 1, 64, 'relu', ('persistent', 4, 5, True, False)),
    # a two-tensor row [x (96) | x2 (64)]
    _rg(1, 1, 200, 96, 1, 1, 64, 'tanh', ('persistent', 4, 5, True, False), F2=64),
    # the XCD-aware mapping: R = 4100 gives seg = 528, the eighth range holds 404 rows, its last wave-tile 20
    _rg(1, 2, 4100, 32, 5, 1, 32, 'relu', ('persistent', 2, 5, True, True)),
    _rg(1, 2, 4100, 32, 5, -1, 64, 'linear', ('persistent', 4, 5, True, True)),
    _rg(1, 5, 4100, 32, 5, -2, 17, 'tanh', ('persistent', 2, 5, True, True)),
    _rg(1, 5, 4100, 32, 5, 1, 50, 'relu', ('persistent', 4, 5, True, True), bias=False),
] + XCD_BLOCK_CASES


def _cs(B, R, T, d, sign, act, n_seg, last, bias=True):
    return _rg(B, T, R, 64, 3, sign * d, 64, act, ('stream', d, stream_act_class(act), sign, n_seg, last), bias=bias)


# streams = 256 (16 x 16) or 258 (3 x 86, 86 x 3), the last 16-row block ragged (10, 10 and 1 rows); every multi-segment
# layout in both directions
STREAM_LAYOUTS = [            # (T, D, n_seg, last segment) at B = 16, R = 250
    (1, 1, 1, 1), (2, 2, 1, 2), (8, 1, 2, 4), (13, 1, 3, 3), (17, 1, 4, 2), (21, 1, 5, 1), (17, 2, 2, 8), (25, 2, 3, 7), (33, 4, 2, 16),
    (49, 4, 3, 15),
]
STREAM_CASES = [
    _cs(16, 250, 1, 1, 1, 'relu', 1, 1),
    _cs(16, 250, 2, 2, 1, 'linear', 1, 2),
    _cs(16, 250, 8, 1, 1, 'relu', 2, 4), _cs(16, 250, 8, 1, -1, 'linear', 2, 4),
    _cs(16, 250, 13, 1, 1, 'tanh', 3, 3), _cs(16, 250, 13, 1, -1, 'relu', 3, 3),
    _cs(16, 250, 17, 1, 1, 'linear', 4, 2), _cs(16, 250, 17, 1, -1, 'sigmoid', 4, 2),
    _cs(16, 250, 21, 1, 1, 'hard_sigmoid', 5, 1), _cs(16, 250, 21, 1, -1, 'tanh', 5, 1),
    _cs(16, 250, 17, 2, 1, 'relu', 2, 8), _cs(16, 250, 17, 2, -1, 'tanh', 2, 8),
    _cs(16, 250, 25, 2, 1, 'sigmoid', 3, 7), _cs(16, 250, 25, 2, -1, 'linear', 3, 7),
    _cs(16, 250, 33, 4, 1, 'relu', 2, 16), _cs(16, 250, 33, 4, -1, 'linear', 2, 16),
    _cs(16, 250, 49, 4, 1, 'tanh', 3, 15), _cs(16, 250, 49, 4, -1, 'hard_sigmoid', 3, 15),
    _cs(3, 1370, 9, 2, -1, 'relu', 1, 9),
    _cs(3, 1370, 5, 4, -1, 'relu', 1, 5, bias=False),           # T < 2 D + 1
    _cs(86, 33, 20, 4, 1, 'linear', 1, 20),
    _cs(86, 33, 9, 1, -1, 'relu', 2, 4),
] + XCD_BLOCK_STREAM

ROWGEMM_CASES = SMALL_CASES + [K384_HEAD] + PERSISTENT_CASES + STREAM_CASES


def _wg(B, T, R, F, H, shift, bias, claims):
    return dict(kind='wgrad', B=B, T=T, R=R, F=F, H=H, shift=shift, bias=bias, claims=('wgrad',) + claims)


# all 18 (MT, NT); F + bias on both sides of every tile edge: the bias row opens a tile of its own at F = 16, 48, 80, 112
WGRAD_CASES = [
    _wg(1, 1, 1, 1, 1, 0, True, (1, 1, 1)),
    _wg(1, 1, 31, 5, 16, 0, True, (1, 1, 1)),
    _wg(1, 1, 32, 15, 17, 0, True, (1, 2, 1)),
    _wg(1, 1, 33, 16, 33, 0, False, (1, 4, 1)),
    _wg(1, 1, 128, 16, 1, 0, True, (2, 1, 1)),
    _wg(1, 1, 129, 31, 32, 0, True, (2, 2, 2)),                 # grid 2, waves 5, 6, 7 empty
    _wg(2, 3, 33, 31, 64, 1, True, (2, 4, 2)),                  # wave ranges cut time steps; b = 1, t = 0 must not read b = 0, t = 2
    _wg(1, 5, 20, 32, 16, 4, True, (3, 1, 1)),                  # shift = T - 1
    _wg(1, 3, 11, 47, 17, 3, True, (3, 2, 1)),                  # shift = T: d_kernel exactly zero
    _wg(2, 3, 7, 48, 64, 4, False, (3, 4, 1)),                  # shift = T + 1
    _wg(1, 1, 200, 48, 16, 0, True, (5, 1, 2)),
    _wg(1, 2, 50, 79, 32, 1, True, (5, 2, 1)),
    _wg(1, 1, 100, 79, 33, 0, True, (5, 4, 1)),
    _wg(1, 1, 64, 80, 1, 0, True, (7, 1, 1)),
    _wg(1, 1, 150, 111, 17, 0, True, (7, 2, 2)),
    _wg(1, 4, 33, 80, 63, 2, True, (7, 4, 2)),
    _wg(1, 1, 90, 112, 16, 0, True, (8, 1, 1)),
    _wg(1, 1, 77, 127, 32, 0, True, (8, 2, 1)),
    _wg(1, 2, 40, 128, 64, 1, False, (8, 4, 1)),
    _wg(1, 1, 2049, 5, 16, 0, True, (1, 1, 17)),                # 17 partials: the reduce kernel's lanes take 2 or 1
    _wg(1, 1, 65409, 5, 3, 0, True, (1, 1, 512)),               # the last row count that reaches 512 workgroups uncapped
    _wg(2, 7, 5000, 8, 8, 1, True, (1, 1, 512)),                # 70000 rows: the cap; 64 rows per wave, 954 waves empty
]
WGRAD_REFUSED = [(128, 64, True), (64, 65, True), (129, 64, False), (64, 65, False)]      # (F, H, with_bias)


def _de(rows, F, fo, act, claims, bias=True):
    return dict(kind='dense', B=1, T=1, R=rows, F=F, taps=0, dil=1, fo=fo, act=act, bias=bias, claims=claims)


def _dc(B, T, R, F, taps, dil, fo, act, claims, bias=True):
    return dict(kind='dense', B=B, T=T, R=R, F=F, taps=taps, dil=dil, fo=fo, act=act, bias=bias, claims=claims)


# k_embed_act<1 .. 8>; f_out / 4 = 1, 3, 5, 7, 24, 64: grids rounded to multiples of 1, 3, 5, 7, 3, 1; rows at the threshold
DENSE_CASES = [
    _de(64, 1, 4, 'relu', ('embed', 1)),
    _de(65, 2, 12, 'tanh', ('embed', 2)),
    _de(4097, 3, 20, 'linear', ('embed', 3)),
    _de(64, 4, 28, 'sigmoid', ('embed', 4)),
    _de(65, 5, 96, 'relu', ('embed', 5), bias=False),
    _de(4097, 6, 256, 'hard_sigmoid', ('embed', 6)),
    _de(4097, 7, 12, 'relu', ('embed', 7)),
    _de(65, 8, 20, 'linear', ('embed', 8)),
    _de(4097, 1, 96, 'tanh', ('embed', 1)),
    _de(64, 3, 28, 'relu', ('embed', 3)),
    _de(63, 3, 12, 'relu', ('tiled', 4)),                       # one row short of the threshold
    _de(63, 6, 256, 'tanh', ('tiled', 64)),
    # uds_conv1d_causal with a negative dilation, once per CG class
    _dc(2, 5, 7, 6, 3, -1, 3, 'relu', ('tiled', 1)),
    _dc(2, 5, 7, 6, 3, -2, 8, 'linear', ('tiled', 2)),
    _dc(2, 5, 7, 5, 2, -4, 13, 'tanh', ('tiled', 4)),
    _dc(2, 5, 7, 6, 3, -1, 32, 'linear', ('tiled', 8), bias=False),
    _dc(2, 3, 7, 6, 3, -2, 50, 'sigmoid', ('tiled', 16)),
    _dc(2, 5, 7, 4, 3, -5, 100, 'relu', ('tiled', 32)),         # |dil| >= T
    _dc(2, 5, 9, 6, 3, -1, 256, 'hard_sigmoid', ('tiled', 64)),
]

ALL_CASES = ROWGEMM_CASES + WGRAD_CASES + DENSE_CASES


def case_id(c):
    if c['kind'] == 'wgrad':
        return 'B%dT%dR%d-F%d-H%d-s%d%s' % (c['B'], c['T'], c['R'], c['F'], c['H'], c['shift'], '' if c['bias'] else '-nobias')
    s = 'B%dT%dR%d-F%d' % (c['B'], c['T'], c['R'], c['F'])
    if c.get('F2'):
        s += '+%d' % c['F2']
    if c['taps']:
        s += '-taps%d-dil%d' % (c['taps'], c['dil'])
    s += '-fo%d-%s' % (c['fo'], c['act'])
    if c.get('ldo', c['fo']) != c['fo']:
        s += '-ldo%d+%d' % (c['ldo'], c['col0'])
    return s + ('' if c['bias'] else '-nobias')


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and fp64 references
# ---------------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return 5000 + next(i for i, k in enumerate(ALL_CASES) if k is c)


def _uni(rng, lim, *shape):
    return torch.from_numpy(f32_exact(rng.uniform(-lim, lim, shape)))


def rowgemm_inputs(c):
    """fp64 tensors of fp32 values: x (B,T,R,F) and x2 (B,T,R,F2) or None uniform in +-0.5, a Glorot kernel (taps, F + F2, fo), a
    bias uniform in +-0.1 (never zero) or None.  Cases that name the same data (XCD_BLOCK_*, K384_*) draw from one seed."""
    src = c.get('same_as') or c
    rng = np.random.default_rng(_seed(src))
    Fi = src['F'] + src.get('F2', 0)
    taps = max(src['taps'], 1)
    x = _uni(rng, 0.5, src['B'], src['T'], src['R'], src['F'])
    x2 = _uni(rng, 0.5, src['B'], src['T'], src['R'], src['F2']) if src.get('F2') else None
    lim = (6.0 / (taps * Fi + taps * src['fo'])) ** 0.5
    k = _uni(rng, lim, taps, Fi, src['fo'])
    b = _uni(rng, 0.1, src['fo'])
    b = torch.where(b == 0, torch.full_like(b, 0.05), b)
    if src is not c:
        x = x[:c['B']].contiguous()
    return dict(x=x, x2=x2, k=k, b=b if c['bias'] else None)


def wgrad_inputs(c):
    """a (B,T,R,F), g (B,T,R,H): fp64 tensors of fp32 values, uniform in +-0.5."""
    rng = np.random.default_rng(_seed(c))
    return dict(a=_uni(rng, 0.5, c['B'], c['T'], c['R'], c['F']), g=_uni(rng, 0.5, c['B'], c['T'], c['R'], c['H']))


def conv_ref(x, k, b, dil, act):
    """fp64 causal (dil > 0) or look-ahead (dil < 0) Conv1D along axis 1 of x (B,T,R,F), kernel (taps,F,H):
    out[t] = act(sum_j x[t - (taps-1-j) dil] k[j] + b), rows outside [0, T) zero.  dil > 0 is oracle.emulator_ref.conv1d_causal;
    dil < 0 is time-flip o conv1d_causal(|dil|) o time-flip (bias and activation are pointwise: they commute with the flip)."""
    B, T, R, F = x.shape
    bias = b if b is not None else torch.zeros(k.shape[-1], dtype=torch.float64)
    xs = x if dil > 0 else torch.flip(x, dims=(1,))
    y = OE.conv1d_causal(xs.permute(0, 2, 1, 3).reshape(B * R, T, F), k, bias, abs(dil), act).reshape(B, R, T, -1).permute(0, 2, 1, 3)
    return (y if dil > 0 else torch.flip(y, dims=(1,))).contiguous()


def rowgemm_ref(c, p):
    """fp64 reference of a rowgemm / dense case on rowgemm_inputs(c): (B, T, R, fo)."""
    x = p['x'] if p['x2'] is None else torch.cat([p['x'], p['x2']], dim=-1)
    if c['taps'] <= 1:
        return OD.dense(x, p['k'][0], p['b'], c['act'])
    return conv_ref(x, p['k'], p['b'], c['dil'], c['act'])


def wgrad_ref(a, g, shift):
    """(d_kernel (F,H), d_bias (H)) in fp64: a[:, :T - shift]^T @ g[:, shift:] summed over batch, time and rows, and the column
    sums of g over ALL rows (the bias of the layer sees every output row, whatever the tap)."""
    B, T, R, F = a.shape
    H = g.shape[-1]
    if shift >= T:
        dk = torch.zeros(F, H, dtype=torch.float64)
    else:
        dk = a[:, :T - shift].reshape(-1, F).t() @ g[:, shift:].reshape(-1, H)
    return dk, g.reshape(-1, H).sum(0)


def wgrad_tol(rows):
    """The project's bound (tests/test_gpu_train.py, test_wgrad_kernel: fp32 sums over the rows); the CPU signal checks use it,
    tests/test_gpu_rowgemm_routes.py asserts a tighter one."""
    return 4e-5 * max(1.0, (rows / 1000.0) ** 0.5)
