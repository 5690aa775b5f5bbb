"""uds_conv_stack_plan / uds_conv_stack_forward without a device: the planner equals its Python mirror, the case table of
tests/conv_stack_util.py reaches every layout of k_conv3_stack, every argument check of the entry answers -22 with its name, and
the fp64 reference tells the right stack from four wrong ones.
"""
import ctypes

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from tests import conv_stack_util as CU
from tests.conv_stack_util import CASES, case_id

EINVAL = -22
_BUF = np.zeros(64, dtype=np.float32)
P = _BUF.ctypes.data - _BUF.ctypes.data % 16 + 16       # a 16-byte aligned address (never read)
FAR = P + (1 << 30)                                     # ... and one that no tensor of these checks reaches from P


# ---- the planner ----------------------------------------------------------------------------------------------------------
def _plan(B, T, R, L):
    return _lib.conv_stack_plan(B, T, R, L)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_plan_equals_its_mirror_on_every_case(case):
    assert _plan(case['B'], case['T'], case['R'], case['L']) == CU.stack_plan(case['B'], case['R'], case['T'], case['L'])


def test_plan_equals_its_mirror_on_a_sweep():
    for L in (2, 3):
        for B in (1, 2, 3, 16, 32, 86, 300):
            for R in (1, 15, 16, 17, 33, 250, 1370, 4096, 10000, 12000, 40000):
                for T in (1, 2, 5, 6, 11, 12, 13, 27, 28, 29, 56, 57, 60, 120, 500):
                    got = _plan(B, T, R, L)
                    assert got == CU.stack_plan(B, R, T, L), (B, R, T, L)
                    n_seg, seg_len, h = got
                    assert h == {2: 6, 3: 14}[L]
                    assert n_seg >= 1 and (n_seg - 1) * seg_len < T <= n_seg * seg_len
                    assert n_seg == 1 or seg_len >= 2 * h              # the halo a segment re-computes stays <= 50 % of it
                    assert n_seg == 1 or n_seg * CU.streams(B, R) <= CU.SLOTS      # one resident round


def test_plan_refuses_bad_arguments():
    lib = _lib.load()
    out = [ctypes.c_int64() for _ in range(3)]
    refs = [ctypes.byref(o) for o in out]
    for args in ((2, 5, 7, 1), (2, 5, 7, 4), (2, 0, 7, 2), (2, 5, 0, 3), (-1, 5, 7, 2)):
        B, T, R, L = args
        assert lib.uds_conv_stack_plan(B, T, R, L, *refs) == EINVAL
        assert lib.uds_last_error().decode().startswith('uds_conv_stack_plan:')
    assert lib.uds_conv_stack_plan(2, 5, 7, 2, None, refs[1], refs[2]) == EINVAL


# ---- the cases reach every layout -----------------------------------------------------------------------------------------
def _some(pred):
    return [case_id(c) for c in CASES if pred(c)]


def test_cases_reach_every_layout():
    segs = {case_id(c): CU.segments(c) for c in CASES}
    for c in CASES:      # the segments tile [0, T)
        s = segs[case_id(c)]
        assert s[0][1] == 0 and s[-1][2] == c['T'] and all(a[2] == b[1] for a, b in zip(s, s[1:])) and all(a[1] < a[2] for a in s)
    h = CU.halo
    last_rows = lambda c: c['R'] - (c['R'] - 1) // 16 * 16
    D_last = lambda c: 2 ** (c['L'] - 1)
    assert _some(lambda c: len(segs[case_id(c)]) == 1 and c['T'] > 1)
    short_last = lambda c: len(segs[case_id(c)]) >= 2 and segs[case_id(c)][-1][2] - segs[case_id(c)][-1][1] < segs[case_id(c)][0][2]
    assert _some(lambda c: short_last(c) and not c['n_seg']), 'the planner itself cuts a case into segments, the last one shorter'
    assert _some(lambda c: short_last(c) and c['n_seg'])
    assert _some(lambda c: any(0 < s0 < h(c['L']) and tf == 0 for tf, s0, _ in segs[case_id(c)])), 'a start clamped to 0'
    assert _some(lambda c: any(tf > 0 for tf, _, _ in segs[case_id(c)])), 'a start after step 0'
    assert _some(lambda c: len(segs[case_id(c)]) * CU.streams(c['B'], c['R']) > CU.SLOTS), 'more units than resident waves'
    for L in (2, 3):
        assert _some(lambda c: c['L'] == L and c['T'] == 1)
        assert _some(lambda c: c['L'] == L and 1 < c['T'] < 2 * D_last(c) + 1)
        assert _some(lambda c: c['L'] == L and 2 * D_last(c) + 1 <= c['T'] < h(L)) or L == 2      # L = 2: 2 D + 1 = 5, halo 6: T = 5 below
        assert _some(lambda c: c['L'] == L and c['T'] < h(L))
        assert _some(lambda c: c['L'] == L and len(segs[case_id(c)]) >= 2)
        for rows in (1, 10):
            assert _some(lambda c: c['L'] == L and last_rows(c) == rows and CU.streams(c['B'], c['R']) >= CU.STREAM_MIN)
        for cls in ('relu', 'linear', 'generic'):
            assert _some(lambda c: c['L'] == L and CU.act_class(c['act']) == cls)
        assert _some(lambda c: c['L'] == L and not c['bias']) and _some(lambda c: c['L'] == L and c['bias'])
    assert _some(lambda c: c['R'] < 16)
    assert _some(lambda c: CU.streams(c['B'], c['R']) == CU.STREAM_MIN) and _some(lambda c: CU.streams(c['B'], c['R']) < CU.STREAM_MIN)
    assert all(CU.streams(c['B'], c['R']) >= CU.STREAM_MIN for c in CU.BIG_CASES)
    assert not any(CU.streams(c['B'], c['R']) >= CU.STREAM_MIN for c in CU.SMALL_CASES)
    assert len({case_id(c) for c in CASES}) == len(CASES)


# ---- the entry's checks ---------------------------------------------------------------------------------------------------
def _stack(n_layers=3, act=1, packed=(P, P, P), bias=(None, None, None)):
    st = _lib._ConvStack()
    st.n_layers, st.act = n_layers, act
    for i in range(3):
        st.packed[i], st.bias[i] = packed[i], bias[i]
    return st


GOOD = dict(x=P, B=2, T=9, R=5, layers=None, n_seg=0, out=FAR)
CHECKS = [
    ('null-x', dict(x=None), {}, 'NULL x/out/layers'),
    ('null-out', dict(out=None), {}, 'NULL x/out/layers'),
    ('null-layers', dict(layers=0), {}, 'NULL x/out/layers'),
    ('null-packed-1', {}, dict(packed=(P, None, P)), 'layer 1 has no weights'),
    ('null-packed-2', {}, dict(packed=(P, P, None)), 'layer 2 has no weights'),
    ('one-layer', {}, dict(n_layers=1), 'stacks of 2 or 3 layers (got 1)'),
    ('four-layers', {}, dict(n_layers=4), 'stacks of 2 or 3 layers (got 4)'),
    ('T-zero', dict(T=0), {}, 'bad sizes B=2 T=0 R=5'),
    ('R-zero', dict(R=0), {}, 'bad sizes B=2 T=9 R=0'),
    ('B-negative', dict(B=-1), {}, 'bad sizes B=-1'),
    ('act-unknown', {}, dict(act=5), 'unknown activation 5'),
    ('act-negative', {}, dict(act=-1), 'unknown activation -1'),
    ('x-misaligned', dict(x=P + 4), {}, '16-byte aligned'),
    ('out-misaligned', dict(out=FAR + 8), {}, '16-byte aligned'),
    ('packed-misaligned', {}, dict(packed=(P, P + 4, P)), '16-byte aligned'),
    ('bias-misaligned', {}, dict(bias=(None, None, P + 4)), '16-byte aligned'),
    ('out-is-x', dict(out=P), {}, 'out overlaps x'),
    ('out-inside-x', dict(out=P + 2 * 9 * 5 * 256 - 16), {}, 'out overlaps x'),
    ('x-inside-out', dict(x=FAR + 256), {}, 'out overlaps x'),
    ('n_seg-negative', dict(n_seg=-1), {}, 'n_seg -1 outside [0, T = 9]'),
    ('n_seg-above-T', dict(n_seg=10), {}, 'n_seg 10 outside [0, T = 9]'),
    ('rows-int32', dict(B=1 << 11, T=1 << 10, R=1 << 10), {}, 'rows exceed the int32 row index'),
]


def _call(args, stack_kw):
    st = _stack(**stack_kw)
    a = dict(GOOD, **args)
    layers = ctypes.byref(st) if a['layers'] is None else None
    lib = _lib.load()
    rc = lib.uds_conv_stack_forward(a['x'], a['B'], a['T'], a['R'], layers, a['n_seg'], a['out'], None)
    return rc, (lib.uds_last_error() or b'').decode()


@pytest.mark.parametrize('name,args,stack_kw,text', CHECKS, ids=[c[0] for c in CHECKS])
def test_bad_argument_is_refused_with_the_entrys_name(name, args, stack_kw, text):
    rc, msg = _call(args, stack_kw)
    assert rc == EINVAL and msg.startswith('uds_conv_stack_forward: ') and text in msg, (rc, msg)


def test_empty_batch_is_ok_and_launches_nothing():
    for kw in ({}, dict(n_layers=2)):
        rc, msg = _call(dict(B=0), kw)       # no device on this path: a launch would fail
        assert rc == 0, msg
    rc, _ = _call(dict(B=0, T=0), {})        # the checks come first
    assert rc == EINVAL


def test_binding_refuses_what_is_not_a_stack_input():
    with pytest.raises(_lib.UdsError):
        _lib.conv_stack_forward(torch.zeros(2, 3, 5, 32), [(None, None)] * 2)
    with pytest.raises(_lib.UdsError):
        _lib.conv_stack_forward(torch.zeros(3, 5, 64), [(None, None)] * 2)


# ---- the reference carries signal -----------------------------------------------------------------------------------------
SIGNAL = 1e-2
# degenerate by construction, left out of the assertion below:
#   T = 1                                       one step has no history: every variant computes the same thing
#   'no-inner-act' with a linear stack          there is no activation to leave out
#   'short-halo' at T <= halo                   a segment that starts a full halo after step 0 does not exist: s0 - (halo - 1) <= 0 is
#                                               clamped to the true start
DEGENERATE_T1 = [case_id(c) for c in CASES if c['T'] == 1]
DEGENERATE_LINEAR = [case_id(c) for c in CASES if c['act'] == 'linear']
DEGENERATE_SHORT = [case_id(c) for c in CASES if c['T'] <= CU.halo(c['L'])]


@pytest.mark.parametrize('case', [c for c in CASES if c['T'] >= 2], ids=case_id)
def test_reference_tells_wrong_stacks_apart(case):
    """On the first batch element and at most 24 rows of the case's own inputs (rows are independent: the maximum over a subset is a
    lower bound of the maximum over the case)."""
    p = CU.stack_inputs(case)
    x, ks, bs, act, L, T = p['x'][:1, :, :24].contiguous(), p['k'], p['b'], case['act'], case['L'], case['T']
    ref = CU.stack_eval(x, ks, bs, act)
    assert float(ref.abs().max()) <= 1.6
    dist = lambda y, lo=0: float((y - ref[:, lo:]).abs().max())
    seen = {}
    if case_id(case) not in DEGENERATE_LINEAR:
        seen['no-inner-act'] = dist(CU.stack_eval(x, ks, bs, act, inner_act=False))
    seen['reversed-dilations'] = dist(CU.stack_eval(x, ks, bs, act, dils=[2 ** (L - 1 - i) for i in range(L)]))
    s0 = max(1, T // 2)
    assert dist(CU.segmented_eval(x, ks, bs, act, s0, CU.halo(L)), s0) <= 1e-12      # the full halo is exact (to fp64 rounding)
    seen['empty-history'] = dist(CU.segmented_eval(x, ks, bs, act, s0, 0), s0)
    if case_id(case) not in DEGENERATE_SHORT:
        h = CU.halo(L)
        assert dist(CU.segmented_eval(x, ks, bs, act, h, h), h) <= 1e-12
        seen['short-halo'] = dist(CU.segmented_eval(x, ks, bs, act, h, h - 1), h)
    print(case_id(case), ' '.join('%s %.3e' % kv for kv in seen.items()))
    assert all(v >= SIGNAL for v in seen.values()), seen
