"""CPU checks behind tests/test_gpu_recurrent_routes.py: every case of tests/recurrent_util.py reaches the kernel it claims and
every instantiation is reached, the route mirror agrees with the library wherever the library answers without a device, the fp64
references are the oracle's sequences and torch autograd's derivatives, the bounds of the GPU file hold with room for the reference
evaluated in the kernels' arithmetic alone, and a kernel that makes one of the classic mistakes moves every case it touches past
ten times its bound.

Bounds (tests/recurrent_util.py), all relative to max(1, max|ref|) except the backward one:
  exact fp32 forward     TOL_FP32 = 5e-6; plain fp32 evaluation of the reference must stay within a third of it
  one-launch forward     TOL_BF16X3 = 2e-5; the split-bf16 model must stay within a third of it
  backward               per output tensor, allowed = 3 x max|split-bf16 model - fp64 reference| of that case; asserted here to be
                         no looser than the project's 1e-3 * max|reference gradient|

MEASURED here (UDS_TOL_REPORT=1 prints every case), worst over the tables:
  fp32 evaluation / TOL_FP32       0.054  [GRU, H = 200, T = 9]; 0.051 at H = 256; 0.044 at H = 128, T = 96
  split-bf16 model / TOL_BF16X3    0.288  [GRU, F = 64]; 0.174 at F = 128 (inputs +-0.5: +-1 gave 0.39), 0.145 LSTM F = 64,
                                   0.129 / 0.048 at F = 0; at (3, 17) T = 9 -> 96 gives 0.222 -> 0.282 (F = 64), 0.113 -> 0.129
                                   (F = 0): the maximum over eleven times as many values, no growth along the time axis (asserted)
  backward, allowed / (1e-3 * max|ref grad|)
                                   0.0058 [bwd-GRU-B2T64R32-H64: model error 2.7e-6 (dxp), 1.9e-6 (darec)]
                                   0.0057 [bwd-GRU-B2T9R32-H48], 0.0054 [bwd-GRU-B3T9R17-H128]
                                   smallest 0.00016 [bwd-LSTM-B1T1R1-H64: model error 2.4e-8, fp32 rounding alone: one step from
                                   the zero state has no split-bf16 product]
"""
import os

import pytest
import torch

from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from tests import recurrent_util as RU
from tests.recurrent_util import GATES, bound, case_id, forward_ref, inputs, route

REPORT = bool(os.environ.get('UDS_TOL_REPORT'))
FORWARD_CASES = RU.EXACT_CASES + RU.FUSED_CASES
_TOL = {'exact': RU.TOL_FP32, 'fused': RU.TOL_BF16X3}


# ---- tables and routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RU.ALL_CASES, ids=case_id)
def test_case_reaches_the_route_it_claims(case):
    assert route(case) == case['claims']
    for c in ([RU.sat_bwd_case(case)] if case.get('sat') else []):
        assert route(c) == c['claims']


def test_case_ids_are_unique():
    ids = [case_id(c) for c in RU.ALL_CASES]
    assert len(ids) == len(set(ids))


def test_every_instantiation_is_reached():
    routes = {route(c) for c in RU.ALL_CASES}
    assert {r[:2] for r in routes if r[0] in ('lds', 'stream')} == {('lds', 3), ('lds', 4), ('stream', 3), ('stream', 4)}
    assert {r[1:] for r in routes if r[0] == 'mfma'} == {(3, 0), (3, 2), (3, 4), (4, 0), (4, 2)}
    assert {r[1] for r in routes if r[0] == 'bwd64'} == {3, 4}
    assert {r[1:3] for r in routes if r[0] == 'bwd_h'} == {(G, H) for G in (3, 4) for H in RU.TRAIN_WIDTHS if H != 64}
    assert {r[2] for r in routes if r[0] == 'bwd_h' and r[3]} == {16, 32, 48}      # the image staged in LDS / read in place
    sat = {route(c)[:2] for c in RU.SAT_CASES}
    assert sat == {('lds', 3), ('lds', 4), ('stream', 3), ('stream', 4), ('mfma', 3), ('mfma', 4)}
    assert all(route(c)[2] == 0 for c in RU.SAT_CASES if c['fam'] == 'fused')


def test_route_boundaries():
    """The LDS route ends at 116 (GRU) / 100 (LSTM) units, whatever the width below or above."""
    for kind, last in (('GRU', 116), ('LSTM', 100)):
        names = [RU.forward_route(kind, H)[0] for H in range(1, 257)]
        assert names == ['lds'] * last + ['stream'] * (256 - last)
        assert RU.FIRST_STREAMED[kind] == last + 1
        assert RU.recurrent_lds_bytes(GATES[kind], last) <= RU.LDS_BYTES < RU.recurrent_lds_bytes(GATES[kind], last + 1)
    # above the 64 KiB a kernel gets without raising its limit: a GRU from 74 units up, the two-device case among them
    assert RU.forward_route('GRU', 73)[0] == 'lds' and RU.recurrent_lds_bytes(3, 73) <= 64 * 1024 < RU.recurrent_lds_bytes(3, 74)
    assert RU.TWO_DEVICE_CASE['kind'] == 'GRU' and 64 * 1024 < RU.recurrent_lds_bytes(3, RU.TWO_DEVICE_CASE['H']) <= RU.LDS_BYTES


def test_tables_cover_the_edges_the_issue_lists():
    ex = RU.EXACT_CASES
    for kind in ('GRU', 'LSTM'):
        for bias in (True, False):
            got = {(c['B'], c['T'], c['R'], c['H']) for c in ex if c['kind'] == kind and c['bias'] == bias}
            want = {(2, 9, 37, H) for H in RU.EXACT_WIDTHS} | {(2, 96, 37, 64), (2, 96, 37, 128)}
            want |= {s + (H,) for s in ((1, 1, 1), (3, 2, 5)) for H in (20, RU.FIRST_STREAMED[kind])}
            assert got == want
    threads = {route(c)[3] for c in ex}
    assert {240, 202, 200} <= threads and any(t % 64 for t in threads)
    fu = RU.FUSED_CASES
    for kind, F in RU.FUSED_FORMS:
        for bias in ((True, False) if kind == 'GRU' else (False,)):
            got = {(c['B'], c['R'], c['T']) for c in fu if (c['kind'], c['F'], c['bias']) == (kind, F, bias)}
            assert got == {(B, R, T) for (B, R) in RU.FUSED_ROWS for T in (1, 2, 3, 9)} | {(3, 17, 96)}
    assert {c['R'] for c in fu} >= {1, 15, 16, 17}
    units = {RU.fused_units(B, R) for (B, R) in RU.FUSED_ROWS}
    assert units == {1, 2, 4, 6} and any(u % 4 for u in units)              # waves of the last workgroup return early
    bw = RU.BWD_CASES
    for kind in ('GRU', 'LSTM'):
        for H in _lib.RECURRENT_TRAIN_WIDTHS:
            got = {(c['B'], c['R'], c['T']) for c in bw if (c['kind'], c['H']) == (kind, H)}
            assert got == {(B, R, T) for (B, R) in RU.BWD_ROWS for T in (1, 2, 9) + ((64,) if H in (64, 128) else ())}
    assert {c['bias'] for c in bw if c['kind'] == 'LSTM'} == {True, False}
    big = max(RU.ALL_CASES, key=lambda c: c['B'] * c['T'] * c['R'] * c['H'])
    assert (big['B'], big['T'], big['R'], big['H']) == (2, 96, 37, 128)


# ---- the mirror against the library -----------------------------------------------------------------------------------------
def test_mirror_agrees_with_the_library():
    lib = _lib.load()
    assert RU.TRAIN_WIDTHS == _lib.RECURRENT_TRAIN_WIDTHS
    for k, kind in enumerate(('GRU', 'LSTM')):
        G = GATES[kind]
        for F in (0, 1, 32, 64, 96, 128, 160, 192, 256):
            assert bool(lib.uds_recurrent_fused_supported(F, k)) == RU.recurrent_mfma_supported(G, F) == _lib.recurrent_fused_supported(F, kind)
        for H in range(0, 161):
            want = RU.recurrent_bwd_packed_bytes(G, H)
            assert lib.uds_recurrent_bwd_packed_bytes(H, k) == want == _lib.recurrent_bwd_packed_bytes(H, G)
            assert (want > 0) == (_lib.recurrent_bwd_route(H) is not None)
    assert {(kind, F) for kind in ('GRU', 'LSTM') for F in (0, 64, 128) if RU.recurrent_mfma_supported(GATES[kind], F)} == set(RU.FUSED_FORMS)
    assert RU.recurrent_mfma_lds(3, 4) == 144 * 1024 and RU.recurrent_mfma_lds(4, 4) == 192 * 1024
    for c in RU.BWD_CASES:
        assert _lib.recurrent_bwd_route(c['H']) == ('uds_recurrent_backward' if c['claims'][0] == 'bwd64' else 'uds_recurrent_backward_h')


# ---- the references are the oracle's sequences and autograd's derivatives ----------------------------------------------------
def _flat(x):
    B, T, R, F = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * R, T, F)


def _unflat(y, B, R):
    return y.reshape(B, R, y.shape[1], y.shape[2]).permute(0, 2, 1, 3)


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
def test_references_equal_the_oracle_and_autograd(kind):
    g = torch.Generator().manual_seed(3)
    B, T, R, F, H, G = 2, 5, 3, 4, 6, GATES[kind]
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) - 0.5
    x, W, U, gh = rnd(B, T, R, F), rnd(F, G * H), rnd(H, G * H), rnd(B, T, R, H)
    bias = rnd(2, G * H) if kind == 'GRU' else rnd(G * H)
    seq = OE.gru_sequence if kind == 'GRU' else OE.lstm_sequence
    b_in, rb = (bias[0], bias[1]) if kind == 'GRU' else (bias, None)
    xp = x @ W + b_in
    h, c = RU.recurrence(kind, xp, U, rb)
    assert float((h - _unflat(seq(_flat(x), W, U, bias), B, R)).abs().max()) <= 1e-13
    if kind == 'LSTM':                                               # the cell states are the ones the oracle's h comes from
        o = torch.sigmoid((xp[:, 1:] + h[:, :-1] @ U)[..., 3 * H:])
        assert float((o * torch.tanh(c[:, 1:]) - h[:, 1:]).abs().max()) <= 1e-13
        assert RU.recurrence(kind, xp, U, torch.zeros(G * H, dtype=torch.float64))[1].equal(c)
    # derivatives: the oracle on the projection itself (identity kernel), its recurrent kernel and recurrent bias as leaves
    case = dict(kind=kind, H=H)
    dxp, darec = RU.backward_ref(case, dict(x=xp, U=U, rb=rb, gh=gh))
    xl, Ul = xp.clone().requires_grad_(True), U.clone().requires_grad_(True)
    zero = torch.zeros(G * H, dtype=torch.float64)
    bl = (torch.stack([zero, rb]) if kind == 'GRU' else zero).clone().requires_grad_(True)
    y = _unflat(seq(_flat(xl), torch.eye(G * H, dtype=torch.float64), Ul, bl), B, R)
    (y * gh).sum().backward()
    assert float((dxp - xl.grad).abs().max()) <= 1e-13
    da = darec.permute(1, 2, 3, 0, 4).reshape(B, T, R, G * H)       # (B,T,R,G H): the gradient of h[t-1] U + rb
    dU = torch.einsum('btrk,btrj->kj', h[:, :-1], da[:, 1:])
    assert float((dU - Ul.grad).abs().max()) <= 1e-13
    if kind == 'GRU':
        assert float((da.sum((0, 1, 2)) - bl.grad[1]).abs().max()) <= 1e-13
        assert float((da[..., :2 * H] - dxp[..., :2 * H]).abs().max()) == 0 and float((da[..., 2 * H:] - dxp[..., 2 * H:]).abs().max()) > 1e-3
    else:
        assert darec.permute(1, 2, 3, 0, 4).reshape(B, T, R, G * H).equal(dxp)


def test_split_model_is_the_three_product_scheme():
    """hi and lo are bf16 numbers, hi + lo restores an operand to 2^-16 relative; the three products miss a @ w by the lo * lo
    term and fp32 summation, one product alone has bf16's error."""
    g = torch.Generator().manual_seed(5)
    a, w = torch.rand(37, 64, generator=g) * 2 - 1, torch.rand(64, 192, generator=g) - 0.5
    (hi, lo), (wh, wl) = RU.split(a), RU.split(w)
    assert hi.bfloat16().float().equal(hi) and lo.bfloat16().float().equal(lo)
    assert float((hi + lo - a).abs().max()) <= 2.0 ** -16
    exact = a.double() @ w.double()
    dropped = (lo.double() @ wl.double()).abs().max()               # 2.2e-5 here: 64 terms of up to 2^-9 * 2^-10
    resid = ((a - hi - lo).abs().double() @ w.abs().double() + a.abs().double() @ (w - wh - wl).abs().double()).max()
    assert float((RU.mm3(a, w).double() - exact).abs().max()) <= float(dropped + resid) + 64 * 2.0 ** -24 * float(exact.abs().max())
    assert float(dropped) < 1e-4 < 1e-3 < float(((hi @ wh).double() - exact).abs().max())


# ---- the bounds hold for the reference alone --------------------------------------------------------------------------------
def _ratio(got, ref, tol):
    return float((got.double() - ref).abs().max()) / bound(ref, tol)


@pytest.mark.parametrize('case', RU.EXACT_CASES + [c for c in RU.SAT_CASES if c['fam'] == 'exact'], ids=case_id)
def test_fp32_evaluation_stays_within_a_third_of_the_bound(case):
    p = inputs(case)
    (h, c), (h32, c32) = forward_ref(case, p), forward_ref(case, p, dtype=torch.float32)
    assert bool(torch.isfinite(h32).all())
    ratio = max(_ratio(h32, h, RU.TOL_FP32), _ratio(c32, c, RU.TOL_FP32) if c is not None else 0.0)
    if REPORT:
        print('fp32 evaluation %-40s %.3f of TOL_FP32' % (case_id(case), ratio))
    assert ratio <= 1.0 / 3.0


@pytest.mark.parametrize('case', RU.FUSED_CASES + [c for c in RU.SAT_CASES if c['fam'] == 'fused'], ids=case_id)
def test_split_model_stays_within_a_third_of_the_bound(case):
    p = inputs(case)
    h, _ = forward_ref(case, p)
    m = RU.model_forward(case, p)
    assert bool(torch.isfinite(m).all())
    ratio = _ratio(m, h, RU.TOL_BF16X3)
    if REPORT:
        print('split-bf16 model %-40s %.3f of TOL_BF16X3' % (case_id(case), ratio))
    assert ratio <= 1.0 / 3.0


def test_split_model_error_does_not_grow_with_the_horizon():
    for kind, F in RU.FUSED_FORMS:
        long = next(c for c in RU.FUSED_CASES if (c['kind'], c['F'], c['T'], c['bias']) == (kind, F, 96, kind == 'GRU'))
        p = inputs(long)
        h, _ = forward_ref(long, p)
        err = (RU.model_forward(long, p).double() - h).abs().amax((0, 2, 3))      # per time step
        assert float(err[48:].max()) <= 1.5 * float(err[:48].max())


@pytest.mark.parametrize('case', RU.BWD_CASES + [RU.sat_bwd_case(c) for c in RU.SAT_CASES], ids=case_id)
def test_backward_bound_is_no_looser_than_the_projects(case):
    p = inputs(case)
    dxp, darec, a_dxp, a_darec, (e_dxp, e_darec) = RU.backward_bounds(case, p)
    s_dxp, s_darec = float(dxp.abs().max()), float(darec.abs().max())
    if REPORT:
        print('backward model %-36s dxp err %.3e (max %.3e) darec err %.3e (max %.3e) allowed / project %.5f'
              % (case_id(case), e_dxp, s_dxp, e_darec, s_darec, max(a_dxp / (RU.TOL_GRAD * s_dxp), a_darec / (RU.TOL_GRAD * s_darec))))
    assert 0 < a_dxp <= RU.TOL_GRAD * s_dxp and 0 < a_darec <= RU.TOL_GRAD * s_darec


# ---- the tests bite: a kernel with one of these mistakes moves every case it touches past ten times its bound -----------------
def _touched(c, wrong):
    gru, T = c['kind'] == 'GRU', c['T']
    return {'swap_zr': gru, 'reset_before': gru and (T > 1 or c['bias']), 'no_rb': c['bias'], 'state_t2': T > 1,
            'no_cell_carry': not gru and T > 1, 'last_row': c['R'] > 1}[wrong]


@pytest.mark.parametrize('wrong', RU.WRONG + ('last_row',))
def test_forward_bounds_bite(wrong):
    n = 0
    for c in FORWARD_CASES:
        if not _touched(c, wrong):
            continue
        p = inputs(c)
        h, cs = forward_ref(c, p)
        bad = RU.last_row_of_block_repeats(h) if wrong == 'last_row' else forward_ref(c, p, wrong=wrong)[0]
        assert float((bad - h).abs().max()) > 10 * bound(h, _TOL[c['fam']]), (case_id(c), wrong)
        n += 1
    assert n >= 40


_BOUNDS = {}


@pytest.mark.parametrize('wrong', RU.WRONG + ('last_row',))
def test_backward_bounds_bite(wrong):
    n = 0
    for c in RU.BWD_CASES:
        if not _touched(c, wrong):
            continue
        p = inputs(c)
        if case_id(c) not in _BOUNDS:                                 # one reference per case, shared by the six mistakes
            _BOUNDS[case_id(c)] = RU.backward_bounds(c, p)[:4]
        dxp, darec, a_dxp, a_darec = _BOUNDS[case_id(c)]
        if wrong == 'last_row':
            bad_x, bad_a = RU.last_row_of_block_repeats(dxp), RU.last_row_of_block_repeats(darec.flatten(0, 1)).reshape(darec.shape)
        else:
            bad_x, bad_a = RU.backward_ref(c, p, wrong=wrong)
        assert float((bad_x - dxp).abs().max()) > 10 * a_dxp and float((bad_a - darec).abs().max()) > 10 * a_darec, (case_id(c), wrong)
        n += 1
    assert n >= 40


# ---- saturated gates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RU.SAT_CASES, ids=case_id)
def test_saturated_cases_are_what_they_claim(case):
    c, p = case, inputs(case)
    H, G = c['H'], GATES[c['kind']]
    assert c['T'] == 5 and float(p['U'].abs().sum(0).max()) <= RU.SAT_HU
    x = p['x']
    hard = torch.arange(c['R']) % RU.SAT_MODERATE_EVERY != RU.SAT_MODERATE_EVERY - 1
    assert set(x[:, :, hard].unique().tolist()) == set(RU.SAT_VALUES) and float(x[:, :, ~hard].abs().max()) <= 1.0
    every_gate = (x[:, :, hard].reshape(c['B'], c['T'], -1, G, H).abs() >= 60).all(3)
    assert 0.2 < float(every_gate.double().mean()) < 0.6                      # (4 / 5) ** G of the elements: every gate saturated
    h, _ = forward_ref(c, p)
    h32, _ = forward_ref(c, p, dtype=torch.float32)
    assert float(h.abs().max()) <= 1.0 and float(((h[:, :-1] @ p['U']).abs()).max()) <= RU.SAT_HU
    if c['kind'] == 'GRU':
        carry, fresh, sign = RU.sat_gru_masks(c, p)
        # every feature of some series is carried through z = 1 and refreshed through z = 0 within the five steps
        assert bool((carry[:, 1:].any(1) & fresh.any(1)).any()) and int(carry.sum()) > 1000 and int(fresh.sum()) > 1000
        prev = torch.cat([torch.zeros_like(h[:, :1]), h[:, :-1]], dim=1)
        prev32 = torch.cat([torch.zeros_like(h32[:, :1]), h32[:, :-1]], dim=1)
        assert h[carry].equal(prev[carry]) and h32[carry].equal(prev32[carry])        # in fp64 as in fp32: bit for bit
        assert h[fresh].equal(sign[fresh]) and h32[fresh].double().equal(sign[fresh])
    # a sigmoid evaluated as 1 / (1 + exp(-v)) in fp32 meets exp(100) = inf there: the quotient must come out 0, not NaN
    assert float(torch.exp(torch.tensor(100.0))) == float('inf')
