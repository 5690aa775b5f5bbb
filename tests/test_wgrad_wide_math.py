"""CPU checks behind tests/test_gpu_wgrad_wide.py (the library loads without a device): the restatement of tests/wgrad_wide_util.py
agrees with uds_wgrad_wide_workspace_floats, the entry refuses what it must with the codes and messages of its contract, every
case reaches the instantiation it claims and every instantiation is reached, autograd.weight_grad_route sends every shape where
the routing rules say, and the references carry signal at the shapes the cases use."""
import ctypes

import pytest
import torch

from gnn_uds_amd import _lib, autograd
from tests import rowgemm_util as RU
from tests import wgrad_wide_util as WU
from tests.rowgemm_util import wgrad_ref, wgrad_tol
from tests.wgrad_wide_util import case_id, route


# ---- tables and routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WU.WIDE_CASES, ids=case_id)
def test_case_reaches_the_route_it_claims(case):
    assert route(case) == case['claims']


def test_case_ids_are_unique():
    ids = [case_id(c) for c in WU.WIDE_CASES]
    assert len(ids) == len(set(ids))


def test_every_instantiation_is_reached():
    assert len(WU.ALL_WIDE) == 8 and {route(c)[1:3] for c in WU.WIDE_CASES} == WU.ALL_WIDE
    blocks = {route(c)[3:5] for c in WU.WIDE_CASES}
    assert blocks == {(rb, cb) for rb in (1, 2) for cb in (1, 2, 3, 4)}          # every block grid, 4 to 8 waves


def test_table_covers_the_edges_the_issue_lists():
    cs = WU.WIDE_CASES
    assert {c['F'] + 1 for c in cs if c['bias']} >= {129, 130, 144, 145, 160, 193, 256, 257}
    assert {c['F'] for c in cs if not c['bias']} >= {129, 130, 144, 145, 160, 193, 256}
    assert {c['F'] for c in cs} >= {128, 129, 96, 97, 2}                         # this kernel's own edges: F, not F + 1
    assert {c['H'] for c in cs} >= {64, 65, 80, 127, 128, 129, 192, 193, 255, 256, 3, 16, 17}
    assert any((c['F'], c['H'], c['bias']) == (128, 64, True) and route(c)[3:5] == (1, 1) for c in cs)
    assert any((c['F'], c['H'], c['bias']) == (256, 256, True) and route(c)[3:5] == (2, 4) for c in cs)
    assert any((c['F'], c['H']) == (2, 128) for c in cs)
    rows = {c['B'] * c['T'] * c['R'] for c in cs}
    assert {1, 31, 32, 33, 129} <= rows and max(rows) == 70000
    assert all(c['F'] == 2 for c in cs if c['B'] * c['T'] * c['R'] > 5000)       # the long cases at the narrowest width only
    p = WU.plan(2, 128)
    assert p['min_span'] == 256 and p['grid_cap'] == 256
    assert WU.grid(p, 65280) == 255 and WU.grid(p, 65281) == 256 and WU.grid(p, 70000) == 256
    assert WU.rows_per_wave(p, 70000) == 96 and WU.empty_splits(p, 70000) == (294, 73)
    assert WU.empty_splits(WU.plan(96, 1), 130) == (3, 0) and WU.empty_splits(WU.plan(128, 64), 1) == (3, 0)
    sh = {(c['shift'], c['T']) for c in cs}
    assert any(s == T - 1 and s > 0 for s, T in sh) and any(s == T for s, T in sh) and any(s == T + 1 for s, T in sh)
    assert any(c['shift'] == 1 and c['R'] == 33 and c['B'] == 2 and WU.rows_per_wave(WU.plan(c['F'], c['H']), 198) % 33 for c in cs)
    for F, H, b in WU.MODEL_SHAPES:
        assert any((c['F'], c['H'], c['bias']) == (F, H, b) and 200 <= c['B'] * c['T'] * c['R'] <= 500 for c in cs), (F, H, b)


# ---- the restatement against the library ------------------------------------------------------------------------------------
def test_workspace_agrees_with_the_library():
    lib = _lib.load()
    widths = (1, 2, 15, 16, 17, 32, 33, 64, 65, 96, 97, 127, 128, 129, 144, 145, 160, 161, 192, 193, 208, 255, 256)
    for rows in (1, 127, 128, 129, 300, 4353, 65280, 65281, 70000, 600000, 10 ** 7):
        for F in widths:
            for H in widths:
                for wb in (0, 1):
                    assert lib.uds_wgrad_wide_workspace_floats(rows, F, H, wb) == WU.workspace_floats(rows, F, H), (rows, F, H, wb)
    for F, H in ((0, 64), (257, 64), (64, 0), (64, 257), (-1, 5), (1000, 1000)):
        for wb in (0, 1):
            assert lib.uds_wgrad_wide_workspace_floats(128, F, H, wb) == 0 and WU.plan(F, H) is None
    assert lib.uds_wgrad_wide_workspace_floats(0, 128, 64, 1) == 0
    for F in range(1, 257):
        for H in (1, 64, 256):
            assert _lib.wgrad_wide_supported(F, H, True) and _lib.wgrad_wide_supported(H, F, False)
    for F, H, wb in WU.WIDE_REFUSED:
        assert not _lib.wgrad_wide_supported(F, H, wb)


def test_partials_stay_small_and_fit():
    """A partial is (ld_f + 1) x ld_n floats; a workgroup's rows hold 4 times as many or more, and a block's LDS tile is 32 KiB + a
    bias row at most."""
    for F in range(1, 257):
        for H in range(1, 257, 5):
            p = WU.plan(F, H)
            assert p['ld_f'] >= F and p['ld_n'] >= H and p['waves'] in (4, 6, 8) and p['nb'] * p['ks'] == p['waves']
            # (the quotient is taken rounded down before it is rounded up to whole k-steps of every split: hence the + 1)
            assert (p['min_span'] + 1) * (F + H) > 4 * (p['ld_f'] + 1) * p['ld_n'] and p['min_span'] % (32 * p['ks']) == 0
            assert (p['mt'] * 16 * p['nt'] * 16 + p['nt'] * 16) * 4 <= 33 * 1024


def test_refusals():
    """-22 and a message that starts with the entry's name; nothing is launched (the checks come before any device call)."""
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    call = lambda a=p, g=p, B=1, T=1, R=4, F=128, H=64, shift=0, wb=1, ws=p, dk=p, db=p: lib.uds_wgrad_wide(a, g, B, T, R, F, H, shift, wb,
                                                                                                          ws, dk, db, None)
    msg = lambda: lib.uds_last_error().decode()
    for kw in (dict(a=None), dict(g=None), dict(ws=None), dict(dk=None)):
        assert call(**kw) == -22 and msg() == 'uds_wgrad_wide: NULL argument'
    assert call(db=None) == -22 and msg() == 'uds_wgrad_wide: with_bias needs d_bias'
    for kw in (dict(B=-1), dict(T=0), dict(R=0), dict(F=0), dict(H=0), dict(shift=-1)):
        assert call(**kw) == -22 and msg() == 'uds_wgrad_wide: bad sizes'
    for F, H, wb in WU.WIDE_REFUSED:
        assert call(F=F, H=H, wb=int(wb)) == -22 and msg().startswith('uds_wgrad_wide: F=%d or H=%d' % (F, H))
    assert call(B=1 << 16, T=1 << 10, R=1 << 5) == -22 and msg().startswith('uds_wgrad_wide: %d rows exceed' % (1 << 31))
    with pytest.raises(_lib.UdsError):
        _lib.wgrad_wide(torch.zeros(1, 1, 4, 257), torch.zeros(1, 1, 4, 64))
    with pytest.raises(_lib.UdsError):
        _lib.wgrad_wide(torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 5, 64))


# ---- autograd.weight_grad_route ---------------------------------------------------------------------------------------------
def test_route_keeps_uds_wgrad_shapes():
    for c in RU.WGRAD_CASES:
        assert autograd.weight_grad_route(c['F'], c['H'], c['bias'], 'bf16x3') == 'wgrad', RU.case_id(c)


def test_route_of_the_default_model_shapes():
    assert autograd.WIDE_WGRAD is True
    for F, H, b in WU.MODEL_SHAPES + [(2, 128, False), (128, 128, False), (128, 256, True), (64, 192, True)]:
        assert not _lib.wgrad_supported(F, H, b)
        assert autograd.weight_grad_route(F, H, b, 'bf16x3') == 'wgrad_wide', (F, H, b)
        assert autograd.weight_grad_route(F, H, b, 'fp32') == 'library'
    assert autograd.weight_grad_route(64, 257, True, 'bf16x3') == 'library'
    assert autograd.weight_grad_route(257, 64, False, 'bf16x3') == 'library'
    assert autograd.weight_grad_route(64, 64, True, 'fp32') == 'library'


def test_route_with_the_switch_off(monkeypatch):
    monkeypatch.setattr(autograd, 'WIDE_WGRAD', False)
    for F, H, b in WU.MODEL_SHAPES:
        assert autograd.weight_grad_route(F, H, b, 'bf16x3') == 'library'
    for c in RU.WGRAD_CASES:
        assert autograd.weight_grad_route(c['F'], c['H'], c['bias'], 'bf16x3') == 'wgrad'


def test_route_counts_is_a_plain_dict():
    assert set(autograd.ROUTE_COUNTS) == {'wgrad', 'wgrad_wide', 'library'}


# ---- signal: a kernel with the same mistake cannot pass -------------------------------------------------------------------
def _moved(wrong, ref, tol):
    return float((wrong - ref).abs().max()) > tol * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('case', [c for c in WU.WIDE_CASES if c['B'] * c['T'] * c['R'] <= 5000], ids=case_id)
def test_signal(case):
    """A shift one off, the last input column or the last output column dropped, the last row dropped, the bias row read one row
    off, the shift applied to flat rows across the batch boundary: each moves the result by more than the bound."""
    c = case
    p = WU.wide_inputs(c)
    rows, F, H = c['B'] * c['T'] * c['R'], c['F'], c['H']
    tol = wgrad_tol(rows)
    dk, db = wgrad_ref(p['a'], p['g'], c['shift'])
    if c['shift'] < c['T']:
        assert _moved(wgrad_ref(p['a'], p['g'], c['shift'] + 1)[0], dk, tol)
        if F > 1:                                                    # the last column left out of the sum: a zero row of d_kernel
            a2 = p['a'].clone()
            a2[..., -1] = 0
            assert _moved(wgrad_ref(a2, p['g'], c['shift'])[0], dk, tol)
        g2 = p['g'].clone()
        g2[..., -1] = 0
        assert _moved(wgrad_ref(p['a'], g2, c['shift'])[0], dk, tol)
    else:
        assert not dk.any()
    if c['bias']:
        assert _moved(dk[F - 1], db, tol) and _moved(torch.zeros_like(db), db, tol)
    if c['shift'] == 0 and rows > 1:
        assert _moved(p['a'].reshape(-1, F)[:-1].t() @ p['g'].reshape(-1, H)[:-1], dk, tol)
    if 0 < c['shift'] < c['T'] and c['B'] > 1:
        s = c['shift'] * c['R']
        assert _moved(p['a'].reshape(-1, F)[:-s].t() @ p['g'].reshape(-1, H)[s:], dk, tol)
