"""uds_wgrad_wide (k_wgrad_wide<MT, NT> + k_wgrad_reduce): the Python restatement of the host routing, the case table and the
seeded inputs shared by tests/test_wgrad_wide_math.py (CPU: the restatement agrees with the library, every case reaches the
instantiation it claims, every instantiation is reached, the references carry signal) and tests/test_gpu_wgrad_wide.py (GPU
parity).  The fp64 reference and the project's bound are tests.rowgemm_util.wgrad_ref / wgrad_tol.

plan(F, H) restates wgrad_wide_plan (gnn_uds_amd/csrc/kernels_wgrad.hpp): the output is cut into rb x cb blocks of MT x NT MFMA
tiles, one wave of the workgroup per block and split:
  rb   row blocks: 1 up to 8 row tiles (F <= 128), else 2            MT  row tiles per block, instantiated 2, 4, 6, 8
  cb   column blocks of 64 columns: ceil(H / 64)                      NT  column tiles per block, 1 (H <= 16) or 4
  ks   waves per block: 4, 4, 2, 2, 1, 1 at rb * cb = 1, 2, 3, 4, 6, 8 (4, 8, 6, 8, 6, 8 waves per workgroup)
The bias gradient is one more row of the partial, so the partial is (rb MT 16 + 1) x (cb NT 16) whether or not it is wanted.
route(case) = ('wide', MT, NT, rb, cb, grid).
"""
import numpy as np
import torch

from tests.util import f32_exact

WIDE_MT = (2, 4, 6, 8)
WIDE_NT = (1, 4)
ALL_WIDE = {(mt, nt) for mt in WIDE_MT for nt in WIDE_NT}


def plan(F, H):
    """wgrad_wide_plan; None for the shapes the entry refuses."""
    if not (1 <= F <= 256 and 1 <= H <= 256):
        return None
    ft, ht = (F + 15) // 16, (H + 15) // 16
    rb = 2 if ft > 8 else 1
    need = (ft + rb - 1) // rb
    mt = next(m for m in WIDE_MT if m >= need)
    cb = (ht + 3) // 4
    nt = 1 if ht == 1 else 4
    nb = rb * cb
    ks = 4 if nb <= 2 else 2 if nb <= 4 else 1
    ld_f, ld_n = rb * mt * 16, cb * nt * 16
    unit = 32 * ks
    min_span = max(unit, (4 * (ld_f + 1) * ld_n // (F + H) + unit - 1) // unit * unit)
    return dict(mt=mt, nt=nt, rb=rb, cb=cb, nb=nb, ks=ks, waves=nb * ks, ld_f=ld_f, ld_n=ld_n, min_span=min_span,
                grid_cap=512 if nb * ks <= 4 else 256)


def grid(p, rows):
    """wgrad_wide_grid."""
    return max(1, min(p['grid_cap'], (rows + p['min_span'] - 1) // p['min_span']))


def rows_per_wave(p, rows):
    """uds_wgrad_wide: a workgroup's span is ks of these."""
    g = grid(p, rows)
    rpw = (rows + g * p['ks'] - 1) // (g * p['ks'])
    return (rpw + 31) // 32 * 32


def workspace_floats(rows, F, H):
    p = plan(F, H)
    if p is None or rows <= 0:
        return 0
    return grid(p, rows) * (p['ld_f'] + 1) * p['ld_n']


def empty_splits(p, rows):
    """(row splits with no rows, workgroups with no rows) of the launch."""
    g, rpw = grid(p, rows), rows_per_wave(p, rows)
    splits = sum(1 for w in range(g * p['ks']) if w * rpw >= rows)
    return splits, sum(1 for b in range(g) if b * p['ks'] * rpw >= rows)


def route(c):
    p = plan(c['F'], c['H'])
    return ('wide', p['mt'], p['nt'], p['rb'], p['cb'], grid(p, c['B'] * c['T'] * c['R']))


def _w(B, T, R, F, H, shift, bias, claims):
    return dict(kind='wgrad', B=B, T=T, R=R, F=F, H=H, shift=shift, bias=bias, claims=('wide',) + claims)


# claims = (MT, NT, rb, cb, grid)
EDGE_CASES = [
    # F + bias = 129, 130, 144, 145, 160, 193, 256, 257 with the bias row; H = 64 | 65, 80, 127, 128 | 129, 192 | 193, 255, 256;
    # rows 1, 31, 32, 33, 129
    _w(1, 1, 1, 128, 64, 0, True, (8, 4, 1, 1, 1)),              # one block, one row
    _w(1, 1, 31, 129, 65, 0, True, (6, 4, 2, 2, 1)),             # the 129th input row opens the second row block
    _w(1, 1, 32, 143, 80, 0, True, (6, 4, 2, 2, 1)),
    _w(1, 1, 33, 144, 127, 0, True, (6, 4, 2, 2, 1)),
    _w(1, 1, 129, 159, 128, 0, True, (6, 4, 2, 2, 1)),
    _w(1, 1, 200, 192, 129, 0, True, (6, 4, 2, 3, 1)),           # six blocks, six waves
    _w(1, 1, 150, 255, 192, 0, True, (8, 4, 2, 3, 1)),
    _w(1, 1, 300, 256, 256, 0, True, (8, 4, 2, 4, 1)),           # the full 257 x 256: eight blocks
    # the same sums without the bias row: F = 129 .. 256
    _w(1, 1, 64, 129, 255, 0, False, (6, 4, 2, 4, 1)),
    _w(1, 1, 77, 130, 64, 0, False, (6, 4, 2, 1, 1)),
    _w(1, 1, 90, 144, 16, 0, False, (6, 1, 2, 1, 1)),
    _w(1, 1, 120, 145, 3, 0, False, (6, 1, 2, 1, 1)),
    _w(1, 1, 70, 160, 65, 0, False, (6, 4, 2, 2, 1)),
    _w(1, 1, 80, 193, 64, 0, False, (8, 4, 2, 1, 1)),            # 13 row tiles: 7 per block
    _w(1, 1, 100, 256, 193, 0, False, (8, 4, 2, 4, 1)),
    _w(1, 1, 33, 128, 65, 0, False, (8, 4, 1, 2, 1)),            # F = 128 without the bias: still one row block
    # the narrow shapes uds_wgrad also takes, and the instantiations only they reach
    _w(1, 1, 40, 20, 16, 0, True, (2, 1, 1, 1, 1)),
    _w(1, 1, 45, 50, 10, 0, True, (4, 1, 1, 1, 1)),
    _w(1, 1, 129, 33, 17, 0, True, (4, 4, 1, 1, 1)),             # 64 rows per split: the fourth split is empty
    _w(1, 1, 240, 2, 128, 0, False, (2, 4, 1, 2, 1)),            # GatFn's da
    _w(1, 1, 130, 96, 1, 0, True, (6, 1, 1, 1, 2)),              # two workgroups; the second one's splits 1, 2, 3 are empty
    _w(1, 1, 60, 97, 64, 0, True, (8, 4, 1, 1, 1)),
]
SHIFT_CASES = [
    _w(2, 3, 33, 128, 64, 1, True, (8, 4, 1, 1, 1)),             # 64-row splits cut time steps; b = 1, t = 0 must not read b = 0, t = 2
    _w(2, 3, 33, 192, 128, 1, False, (6, 4, 2, 2, 1)),
    _w(1, 6, 29, 128, 64, 2, True, (8, 4, 1, 1, 1)),             # a dilation-2 tap
    _w(1, 5, 20, 192, 128, 4, False, (6, 4, 2, 2, 1)),           # shift = T - 1
    _w(1, 3, 11, 129, 65, 3, True, (6, 4, 2, 2, 1)),             # shift = T: d_kernel exactly zero, d_bias the full column sum
    _w(2, 3, 7, 64, 256, 4, True, (4, 4, 1, 4, 1)),              # shift = T + 1
]
# the weight gradients of a default-size model (embed_size 128, hidden_dim 64) that uds_wgrad refuses, at a few hundred rows
MODEL_SHAPES = [(128, 64, True), (192, 128, False), (64, 128, False), (64, 128, True), (128, 3, True), (128, 192, True), (64, 256, True)]
MODEL_CASES = [
    _w(1, 1, 300, 128, 64, 0, True, (8, 4, 1, 1, 2)),
    _w(1, 1, 300, 192, 128, 0, False, (6, 4, 2, 2, 1)),
    _w(1, 1, 300, 64, 128, 0, False, (4, 4, 1, 2, 2)),
    _w(1, 1, 300, 64, 128, 0, True, (4, 4, 1, 2, 2)),
    _w(1, 1, 300, 128, 3, 0, True, (8, 1, 1, 1, 3)),
    _w(1, 1, 300, 128, 192, 0, True, (8, 4, 1, 3, 1)),
    _w(1, 1, 300, 64, 256, 0, True, (4, 4, 1, 4, 2)),
]
# the grid at the narrowest wide shape (2 x 128: 256 rows per workgroup at least, 256 workgroups at most)
GRID_CASES = [
    _w(1, 1, 4353, 2, 128, 0, False, (2, 4, 1, 2, 18)),          # 18 partials: the reduce kernel's lanes take 2 or 1
    _w(1, 1, 65281, 2, 128, 0, False, (2, 4, 1, 2, 256)),        # the smallest count that reaches the cap
    _w(2, 7, 5000, 2, 128, 1, False, (2, 4, 1, 2, 256)),         # 70000 rows: beyond it; 96 rows per wave, workgroups 183 .. 255 empty
]
WIDE_CASES = EDGE_CASES + SHIFT_CASES + MODEL_CASES + GRID_CASES
WIDE_REFUSED = [(257, 64, True), (257, 64, False), (64, 257, True), (300, 300, False)]      # (F, H, with_bias)


def case_id(c):
    return 'B%dT%dR%d-F%d-H%d-s%d%s' % (c['B'], c['T'], c['R'], c['F'], c['H'], c['shift'], '' if c['bias'] else '-nobias')


def _seed(c):
    return 9100 + next(i for i, k in enumerate(WIDE_CASES) if k is c)


def _uni(rng, lim, *shape):
    return torch.from_numpy(f32_exact(rng.uniform(-lim, lim, shape)))


_INPUTS = {}


def wide_inputs(c):
    """a (B,T,R,F), g (B,T,R,H): fp64 tensors of fp32 values, uniform in +-0.5; computed once per case and left unchanged."""
    if id(c) not in _INPUTS:
        rng = np.random.default_rng(_seed(c))
        _INPUTS[id(c)] = dict(a=_uni(rng, 0.5, c['B'], c['T'], c['R'], c['F']), g=_uni(rng, 0.5, c['B'], c['T'], c['R'], c['H']))
    return _INPUTS[id(c)]
