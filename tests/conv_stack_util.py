"""uds_conv_stack_forward (k_conv3_stack<L, ACT>): the plan mirror, the case table and the fp64 reference shared by
tests/test_conv_stack_math.py (CPU: the planner equals its mirror, the cases reach every layout, the reference carries signal) and
tests/test_gpu_conv_stack.py (GPU: bit-identity with the layer chain, parity, memory discipline, the model wiring).

The mirror restates csrc/kernels_conv_stack.hpp (conv_stack_plan, conv_stack_halo, conv_stack_slots) and the forced-n_seg
arithmetic of uds_conv_stack_forward in plain Python.
"""
import functools

import numpy as np
import torch

from tests import rowgemm_util as RU
from tests.util import f32_exact

STACK_WAVES = 4                  # CK_WAVES: one wave per SIMD
SLOTS = 256 * STACK_WAVES        # conv_stack_slots(): resident waves of one launch
STREAM_MIN = 256                 # the stream count from which the layer chain runs k_conv3_stream (uds_rowgemm_forward_cat)


def halo(L):
    """conv_stack_halo: sum_i 2 D_i with D_i = 2^i."""
    return sum(2 * 2 ** i for i in range(L))


def streams(B, R):
    return B * ((R + 15) // 16)


def stack_plan(B, R, T, L):
    """conv_stack_plan: (n_seg, seg_len, halo) of n_seg = 0."""
    n_seg = max(1, min(SLOTS // max(1, streams(B, R)), T // (2 * halo(L))))
    seg_len = (T + n_seg - 1) // n_seg
    return (T + seg_len - 1) // seg_len, seg_len, halo(L)


def forced_plan(T, n_seg):
    """uds_conv_stack_forward with 1 <= n_seg <= T: (n_seg, seg_len) as launched."""
    seg_len = (T + n_seg - 1) // n_seg
    return (T + seg_len - 1) // seg_len, seg_len


def segments(c):
    """[(t_first, s0, s1)] of a case: the segment writes steps [s0, s1) and starts at t_first = max(0, s0 - halo)."""
    B, R, T, L = c['B'], c['R'], c['T'], c['L']
    n_seg, seg_len = forced_plan(T, c['n_seg']) if c['n_seg'] else stack_plan(B, R, T, L)[:2]
    return [(max(0, s * seg_len - halo(L)), s * seg_len, min(T, (s + 1) * seg_len)) for s in range(n_seg)]


def act_class(act):
    """launch_conv_stack_t: the compiled-in activations."""
    return act if act in ('relu', 'linear') else 'generic'


def _c(B, R, T, L, act, bias=True, n_seg=0):
    return dict(B=B, R=R, T=T, L=L, act=act, bias=bias, n_seg=n_seg)


# >= 256 streams: 256 (16 x 16) and 258 (3 x 86, 86 x 3), the last 16-row block of 10, 10 and 1 rows; T = 1, 2, 5, 9, 15, 29, 57
BIG_CASES = [
    _c(16, 250, 1, 2, 'relu'), _c(16, 250, 2, 3, 'linear'), _c(16, 250, 5, 2, 'tanh'), _c(16, 250, 9, 3, 'relu'),
    _c(16, 250, 15, 2, 'linear', bias=False), _c(16, 250, 29, 2, 'relu'), _c(16, 250, 57, 3, 'tanh'),
    _c(3, 1370, 1, 3, 'tanh'), _c(3, 1370, 2, 2, 'relu', bias=False), _c(3, 1370, 5, 3, 'relu'), _c(3, 1370, 9, 2, 'linear'),
    _c(3, 1370, 15, 3, 'linear'), _c(3, 1370, 29, 3, 'relu', bias=False), _c(3, 1370, 57, 2, 'relu'),
    _c(86, 33, 1, 2, 'linear'), _c(86, 33, 2, 3, 'relu'), _c(86, 33, 5, 2, 'sigmoid'), _c(86, 33, 9, 3, 'hard_sigmoid'),
    _c(86, 33, 15, 3, 'relu'), _c(86, 33, 29, 2, 'tanh'), _c(86, 33, 57, 3, 'relu'),
    # forced segmentations: s0 = 3 < halo (the start is clamped to 0); more units (1290) than resident waves, s0 = 12 < 14;
    # one step per segment
    _c(16, 250, 9, 2, 'relu', n_seg=3), _c(3, 1370, 57, 3, 'relu', n_seg=5), _c(86, 33, 15, 3, 'linear', n_seg=15),
]
REPEAT_CASE = BIG_CASES[-2]
# below the caller's threshold, for the entry called directly: one row, R < 16; two batch elements with a 1-row block; forced n_seg
SMALL_CASES = [
    _c(1, 1, 3, 2, 'relu'), _c(2, 17, 7, 3, 'tanh'), _c(1, 20, 40, 3, 'relu', n_seg=4), _c(1, 20, 40, 2, 'linear', bias=False, n_seg=3),
]
CASES = BIG_CASES + SMALL_CASES


def case_id(c):
    return 'B%dR%dT%d-L%d-%s%s%s' % (c['B'], c['R'], c['T'], c['L'], c['act'], '' if c['bias'] else '-nobias',
                                     '-seg%d' % c['n_seg'] if c['n_seg'] else '')


def _uni(rng, lim, *shape):
    return torch.from_numpy(f32_exact(rng.uniform(-lim, lim, shape)))


def stack_inputs(c):
    """As rowgemm_util.rowgemm_inputs makes them: fp64 tensors of fp32 values, x (B,T,R,64) uniform in +-0.5, per layer a Glorot
    kernel (3, 64, 64) and a bias uniform in +-0.1 (never zero) or None."""
    rng = np.random.default_rng(7000 + CASES.index(c))
    x = _uni(rng, 0.5, c['B'], c['T'], c['R'], 64)
    lim = (6.0 / (3 * 64 + 3 * 64)) ** 0.5
    ks, bs = [], []
    for _ in range(c['L']):
        ks.append(_uni(rng, lim, 3, 64, 64))
        b = _uni(rng, 0.1, 64)
        bs.append(torch.where(b == 0, torch.full_like(b, 0.05), b) if c['bias'] else None)
    return dict(x=x, k=ks, b=bs)


def stack_eval(x, ks, bs, act, dils=None, inner_act=True):
    """fp64: oracle.emulator_ref.conv1d_causal (through rowgemm_util.conv_ref) applied len(ks) times.  dils: the dilations, 2^i by
    default; inner_act False leaves the activation out between the layers (wrong on purpose)."""
    L = len(ks)
    dils = dils or [2 ** i for i in range(L)]
    for i in range(L):
        x = RU.conv_ref(x, ks[i], bs[i], dils[i], act if (inner_act or i == L - 1) else 'linear')
    return x


def stack_ref(c, p):
    """The reference of a case on stack_inputs(c): (B, T, R, 64) fp64."""
    return stack_eval(p['x'], p['k'], p['b'], c['act'])


def segmented_eval(x, ks, bs, act, s0, history):
    """Steps [s0, T) computed by a segment that starts `history` steps before s0 (clamped to 0) with empty rings: exact when
    history >= halo."""
    start = max(0, s0 - history)
    return stack_eval(x[:, start:], ks, bs, act)[:, s0 - start:]


@functools.lru_cache(maxsize=2)      # the largest reference is 117 MB: tests that share one run back to back
def _data(i):
    p = stack_inputs(CASES[i])
    return p, stack_ref(CASES[i], p)


def data(c):
    """(inputs, reference) of a case, computed once and shared (read only)."""
    return _data(CASES.index(c))
