"""Cases, seeded inputs and fp64 references of the exact-fp32 Dense / Conv1D / cumsum family (uds_dense_act, uds_conv1d_causal,
uds_cumsum_act, uds_gat_forward), shared by tests/test_dense_route_math.py (CPU: the Python restatement of the route agrees with
uds_dense_route, every case lands on the kernel it names, the references carry signal) and tests/test_gpu_dense_routes.py (GPU
parity at every route).

The route (kernels_dense.hpp: dense_route, reported by uds_dense_route):
  k_embed_act<F>    fb = 0, taps = 0, no attention scalars, fa = F <= 8, f_out % 4 == 0, rows >= 64, W and bias 16-byte aligned.
                    One lane per float4 of the output; min(ceil(rows f4 / 256), 4096) workgroups of 256 lanes, rounded DOWN to a
                    multiple of g = f4 / gcd(256, f4) (at least g), f4 = f_out / 4: the grid stride keeps a lane on its column chunk
  k_dense_act<CG>   everything else; CG = the power of two >= ceil(f_out / 4), 1 .. 64; a workgroup owns TILE_ROWS[CG] rows
"""
import math
import zlib

import numpy as np
import torch

from oracle import emulator_ref as OE
from oracle import spektral_dense as OD

ACTS = ('linear', 'relu', 'tanh', 'sigmoid', 'hard_sigmoid')
TOL = 5e-6               # dense, conv and attention outputs (tests/test_gpu_parity.py: TOL; test_conv1d_causal)
TOL_CUMSUM = 1e-6        # tests/test_gpu_parity.py: test_cumsum_act_and_flow_balance
TILE_ROWS = {1: 128, 2: 128, 4: 128, 8: 128, 16: 64, 32: 32, 64: 16}      # rows of one k_dense_act<CG> workgroup
EMBED_CAP = 256 * 16     # workgroups of k_embed_act at most


# ---------------------------------------------------------------------------------------------------------------
# the route, restated
# ---------------------------------------------------------------------------------------------------------------
def tiled_cg(f_out):
    groups = (f_out + 3) // 4
    return next(c for c in (1, 2, 4, 8, 16, 32, 64) if groups <= c)


def embed_blocks(f_out, rows):
    f4 = f_out // 4
    g = f4 // math.gcd(256, f4)
    return max(g, min((rows * f4 + 255) // 256, EMBED_CAP) // g * g)


def route_py(fa, f_out, rows, fb=0, taps=0, attn=False, aligned=True):
    """What _lib.dense_route returns, from the rules above."""
    if fb == 0 and taps == 0 and not attn and fa <= 8 and f_out % 4 == 0 and rows >= 64 and aligned:
        blocks = embed_blocks(f_out, rows)
        return dict(kernel='embed', param=fa, rows_per_wg=0, workgroups=blocks, stride=256 * blocks)
    cg = tiled_cg(f_out)
    return dict(kernel='tiled', param=cg, rows_per_wg=TILE_ROWS[cg], workgroups=-(-rows // TILE_ROWS[cg]), stride=0)


# ---------------------------------------------------------------------------------------------------------------
# uds_dense_act cases.  kernel / param are written out per case (what the case is FOR); wgs is the workgroup count the route must
# report: from TILE_ROWS for the tiled kernel, embed_blocks for the stream (the two capped grids give theirs as literals)
# ---------------------------------------------------------------------------------------------------------------
def _dense(group, fa, fo, rows, kernel, param, fb=0, act='linear', bias=True, attn=False, scale=1.0, wgs=None):
    if wgs is None:
        wgs = -(-rows // TILE_ROWS[param]) if kernel == 'tiled' else embed_blocks(fo, rows)
    cid = '%s-fa%d%s-fo%d-r%d-%s%s%s' % (group, fa, '+%d' % fb if fb else '', fo, rows, act, '' if bias else '-nobias', '-attn' if attn else '')
    return dict(id=cid, group=group, fa=fa, fb=fb, fo=fo, rows=rows, act=act, bias=bias, attn=attn, scale=scale, kernel=kernel, param=param,
                wgs=wgs)


def _rot(i):
    return ACTS[i % len(ACTS)]


# (i) tiled widths: fa = 40, linear, bias, rows = 2 ROWS + 1 (three workgroups, the last holding one row).  f_out -> CG:
#   1, 2 <1> scalar store; 4 <1> float4 store; 6 <2> scalar; 8 <2> float4; 12 <4> one idle group; 20 <8> three idle groups;
#   36 <16> idle groups, 64 rows per workgroup; 64 <16>; 68, 128 <32>; 132 <64> idle groups; 250 <64> scalar store, the last group
#   holds 2 of 4 columns; 256 <64>
WIDTHS = [(1, 1), (2, 1), (4, 1), (6, 2), (8, 2), (12, 4), (20, 8), (36, 16), (64, 16), (68, 32), (128, 32), (132, 64), (250, 64), (256, 64)]
TILED_WIDTH_CASES = [_dense('width', 40, fo, 2 * TILE_ROWS[cg] + 1, 'tiled', cg) for fo, cg in WIDTHS]
TILED_WIDTH_CASES += [_dense('width', 40, fo, rows, 'tiled', cg) for fo, cg in ((4, 1), (64, 16), (256, 64))
                      for rows in (1, TILE_ROWS[cg] - 1, TILE_ROWS[cg])]

# (ii) K sweep: around the 32-wide K chunk at f_out = 64; narrow inputs that stay on the tiled kernel because rows < 64; the K limit
K_CASES = [_dense('k', fa, 64, 129, 'tiled', 16, act=_rot(i)) for i, fa in enumerate((9, 31, 32, 33, 96, 200))]
K_CASES += [_dense('k', fa, 64, 63, 'tiled', 16, act=_rot(i + 1)) for i, fa in enumerate((1, 5, 8))]
K_CASES += [_dense('k', 4096, 8, 70, 'tiled', 2)]

# (iii) concat: the xa | xb boundary on a chunk boundary (64, 32), inside a chunk (40, 24), (3, 2), (33, 200), in the first column (1, 70)
CONCAT_SHAPES = [(40, 24), (64, 32), (3, 2), (1, 70), (33, 200)]
CONCAT_CASES = [_dense('cat', fa, fo, 129, 'tiled', cg, fb=fb, act=_rot(i + j)) for i, (fa, fb) in enumerate(CONCAT_SHAPES)
                for j, (fo, cg) in enumerate(((64, 16), (7, 2)))]

# (iv) the narrow-input stream.  f_out = 12 and 252 give an odd lane count per row (g = 3, 63); 333 rows a ragged last workgroup
EMBED_CASES = [_dense('embed', F, 64, 200, 'embed', F, act=_rot(F)) for F in range(1, 9)]
EMBED_CASES += [_dense('embed', F, fo, rows, 'embed', F, act=_rot(F + i + rows)) for F in (1, 5, 8) for i, fo in enumerate((4, 12, 96, 252, 256))
                for rows in (64, 333)]
# capped grids: 16400 * 64 = 1049600 lanes over a stride of 4096 * 256 = 1048576: 1024 lanes make a second trip;
# 16700 * 63 = 1052100 lanes over 4095 * 256 = 1048320 (4096 rounded down to a multiple of 63): 3780 lanes make a second trip
CAPPED_CASES = [_dense('capped', 3, 256, 16400, 'embed', 3, act='relu', wgs=4096), _dense('capped', 2, 252, 16700, 'embed', 2, act='tanh', wgs=4095)]
CAPPED_SECOND_TRIP = {CAPPED_CASES[0]['id']: 1024, CAPPED_CASES[1]['id']: 3780}
EMBED_BITWISE_CASES = [c for c in EMBED_CASES if c['fa'] in (1, 5, 8)]      # rows 0 .. 62 alone run on the tiled kernel: the same bits
EMBED_BITWISE_ROWS = 63

# (v) activations x bias given / none; weights x 4: the pre-activations cross zero and pass both clamps of hard_sigmoid (|v| > 2.5)
ACT_CASES = [_dense('act', fa, fo, rows, kernel, param, act=act, bias=bias, scale=4.0)
             for fa, fo, rows, kernel, param in ((40, 7, 129, 'tiled', 2), (40, 64, 129, 'tiled', 16), (8, 64, 200, 'embed', 8))
             for act in ACTS for bias in (True, False)]

# (vi) attention scalars: every CG, idle column groups (12, 36, 132, 250: the xor-shuffle tree sums lanes that own no column), with and
# without xb; no bias, linear (the GAT linear map)
ATTN_WIDTHS = [(4, 1), (8, 2), (12, 4), (36, 16), (64, 16), (132, 64), (250, 64), (256, 64)]
ATTN_CASES = [_dense('attn', 40, fo, 2 * TILE_ROWS[cg] + 1, 'tiled', cg, fb=fb, bias=False, attn=True) for fo, cg in ATTN_WIDTHS for fb in (0, 24)]

# the alignment rule: W and bias offset by one float run on the tiled kernel, with the bits of the aligned (embed) call
MISALIGNED_CASE = _dense('misaligned', 5, 64, 200, 'embed', 5, act='tanh')

DENSE_CASES = TILED_WIDTH_CASES + K_CASES + CONCAT_CASES + EMBED_CASES + CAPPED_CASES + ACT_CASES + ATTN_CASES + [MISALIGNED_CASE]

# (x) row independence: (case, row slices); the slices of the embed case keep 64 rows, the fewest that stay on that kernel
ROW_SUBSETS = [(TILED_WIDTH_CASES[7], [(0, 64), (64, 128), (128, 129)]),
               (next(c for c in EMBED_CASES if (c['fa'], c['fo'], c['rows']) == (5, 96, 333)), [(0, 64), (64, 128), (256, 320), (269, 333)])]


def case_route(c, aligned=True):
    return dict(fa=c['fa'], f_out=c['fo'], rows=c['rows'], fb=c['fb'], attn=c['attn'], aligned=aligned)


def _gen(cid):
    return np.random.default_rng(zlib.crc32(cid.encode()))


def _u(rng, lim, *shape):
    """Uniform in +-lim, fp64 tensor of fp32 values: the device sees the same numbers."""
    return torch.from_numpy(rng.uniform(-lim, lim, shape).astype(np.float32).astype(np.float64))


def dense_inputs(c):
    """x (rows, fa), xb (rows, fb) or None, W (fa + fb, fo), b (fo) or None, a_self / a_nbr (fo) or None: signed, uniform in +-0.5
    (W in +-0.5 scale), fp64 tensors of fp32 values."""
    rng = _gen(c['id'])
    p = dict(x=_u(rng, 0.5, c['rows'], c['fa']), xb=_u(rng, 0.5, c['rows'], c['fb']) if c['fb'] else None,
             W=_u(rng, 0.5 * c['scale'], c['fa'] + c['fb'], c['fo']), b=_u(rng, 0.5, c['fo']) if c['bias'] else None, a_self=None, a_nbr=None)
    if c['attn']:
        p['a_self'], p['a_nbr'] = _u(rng, 0.5, c['fo']), _u(rng, 0.5, c['fo'])
    return p


def dense_pre(p):
    """fp64 pre-activation [x | xb] @ W + b."""
    x = p['x'] if p['xb'] is None else torch.cat([p['x'], p['xb']], -1)
    v = x @ p['W']
    return v if p['b'] is None else v + p['b']


def dense_ref(c, p, act=None):
    """fp64 (out, s_self, s_nbr); the attention scalars are those of the pre-activation rows, None without attn."""
    v = dense_pre(p)
    out = OD.activation(act or c['act'])(v)
    if not c['attn']:
        return out, None, None
    return out, v @ p['a_self'], v @ p['a_nbr']


# ---------------------------------------------------------------------------------------------------------------
# uds_conv1d_causal: (B, T, R, F, H, taps), |dil|; each runs at +dil and -dil.  B > 1 with T * R below the workgroup's row count is
# deliberate: a workgroup then straddles time steps and batch elements
# ---------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [((3, 5, 7, 10, 6, 3), 1), ((3, 5, 7, 10, 6, 3), 2), ((2, 13, 33, 64, 64, 3), 4), ((2, 4, 5, 64, 32, 2), 1),
               ((1, 1, 9, 12, 8, 3), 1),                 # T = 1
               ((2, 3, 5, 16, 12, 3), 7),                # every shifted tap falls outside [0, T)
               ((1, 6, 3, 64, 64, 16), 1),               # taps * F = 1024
               ((2, 5, 130, 8, 250, 3), 2)]
CONV_CASES = [dict(id='B%dT%dR%dF%dH%dk%d-dil%+d' % (shape + (sign * dil,)), shape=shape, dil=sign * dil, act=_rot(i + (sign < 0)), bias=(i + (sign > 0)) % 3 != 0)
              for i, (shape, dil) in enumerate(CONV_SHAPES) for sign in (1, -1)]
CONV_OUT_OF_RANGE = [c for c in CONV_CASES if c['shape'] == (2, 3, 5, 16, 12, 3)]
CONV_BATCH_SUBSET = [c for c in CONV_CASES if c['shape'] == (2, 13, 33, 64, 64, 3)]      # (x): one batch element alone


def conv_route(c):
    B, T, R, F, H, taps = c['shape']
    return dict(fa=F, f_out=H, rows=B * T * R, taps=taps)


def conv_inputs(c):
    """x (B, T, R, F), kernel (taps, F, H), b (H) or None: uniform in +-0.5, fp64 tensors of fp32 values."""
    B, T, R, F, H, taps = c['shape']
    rng = _gen(c['id'])
    return dict(x=_u(rng, 0.5, B, T, R, F), kernel=_u(rng, 0.5, taps, F, H), b=_u(rng, 0.5, H) if c['bias'] else None)


def conv_pre(x, kernel, dil):
    """fp64 loop: out[b, t, r] = sum_j x[b, t - (taps-1-j) dil, r] @ kernel[j], zero outside [0, T).  For dil < 0 tap j reads step
    t + (taps-1-j)|dil|: the look-ahead of the input gradient."""
    B, T, R, _ = x.shape
    taps, _, H = kernel.shape
    out = torch.zeros(B, T, R, H, dtype=torch.float64)
    for j in range(taps):
        s = (taps - 1 - j) * dil
        for t in range(T):
            if 0 <= t - s < T:
                out[:, t] += x[:, t - s] @ kernel[j]
    return out


def conv_ref(c, p):
    """fp64 reference: oracle.emulator_ref.conv1d_causal for dil > 0, the loop above for dil < 0."""
    B, T, R, F, H, taps = c['shape']
    if c['dil'] > 0:
        xm = p['x'].permute(0, 2, 1, 3).reshape(B * R, T, F)
        out = OE.conv1d_causal(xm, p['kernel'], 0.0 if p['b'] is None else p['b'], c['dil'], c['act'])
        return out.reshape(B, R, T, H).permute(0, 2, 1, 3).contiguous()
    v = conv_pre(p['x'], p['kernel'], c['dil'])
    return OD.activation(c['act'])(v if p['b'] is None else v + p['b'])


def conv_shifted_rows(x, taps, dil):
    """The convolution's GEMM operand built on the host: (B T R, taps F) rows [x(t - s_0) | .. | x(t - s_{taps-1})], s_j =
    (taps-1-j) dil, zeros outside [0, T).  uds_dense_act on it with kernel.view(taps F, H) runs the same ascending-k fmaf chain."""
    B, T, R, F = x.shape
    rows = torch.zeros(B, T, R, taps * F, dtype=x.dtype)
    for j in range(taps):
        s = (taps - 1 - j) * dil
        for t in range(T):
            if 0 <= t - s < T:
                rows[:, t, :, j * F:(j + 1) * F] = x[:, t - s]
    return rows.reshape(B * T * R, taps * F)


def conv_live_taps(c):
    """Taps that read inside [0, T) for at least one t."""
    _, T, _, _, _, taps = c['shape']
    return [j for j in range(taps) if abs((taps - 1 - j) * c['dil']) < T]


# ---------------------------------------------------------------------------------------------------------------
# uds_cumsum_act: (B, T, R, F) x five activations x res given / none.  (3, 7, 43, 12): 387 lanes, two workgroups, the second ragged,
# lanes of different b in one wave
# ---------------------------------------------------------------------------------------------------------------
CUMSUM_SHAPES = [(3, 7, 43, 12), (1, 1, 5, 4), (2, 13, 64, 64), (2, 60, 9, 8)]
CUMSUM_CASES = [dict(id='B%dT%dR%dF%d-%s%s' % (shape + (act, '-res' if res else '')), shape=shape, act=act, res=res)
                for shape in CUMSUM_SHAPES for act in ACTS for res in (True, False)]


def cumsum_inputs(c):
    B, T, R, F = c['shape']
    rng = _gen(c['id'])
    return dict(x=_u(rng, 0.5, B, T, R, F), res=_u(rng, 0.5, B, 1, R, F) if c['res'] else None)


def cumsum_ref(c, p):
    v = torch.cumsum(p['x'], 1)
    return OD.activation(c['act'])(v if p['res'] is None else v + p['res'])


# ---------------------------------------------------------------------------------------------------------------
# uds_gat_forward on tests.util.ladder(67): d, (fa, fb) = (40, 24), S = 3
# ---------------------------------------------------------------------------------------------------------------
GAT_WIDTHS = [(8, 2), (12, 4), (64, 16), (256, 64)]      # d -> CG of its projection (attention scalars: the tiled kernel)
GAT_N, GAT_S, GAT_FA, GAT_FB = 67, 3, 40, 24


def gat_inputs(d):
    rng = _gen('gat-d%d' % d)
    return dict(xa=_u(rng, 0.5, GAT_S, GAT_N, GAT_FA), xb=_u(rng, 0.5, GAT_S, GAT_N, GAT_FB), W=_u(rng, 0.5, GAT_FA + GAT_FB, d),
                a_self=_u(rng, 0.5, d), a_nbr=_u(rng, 0.5, d), bias=_u(rng, 0.5, d))
