"""CPU side of tests/test_gpu_dense_routes.py: the route of the exact-fp32 Dense family restated in Python and checked against
uds_dense_route (host only), the case tables of tests/dense_util.py landing on the kernels they name, the fp64 references carrying
signal, and the out= / s_out= checks of the wrappers.  No GPU needed."""
import itertools

import pytest
import torch

from gnn_uds_amd import _lib
from tests import dense_util as D


def test_route_restatement_agrees_with_the_entry():
    """f_out = 1 .. 256 x fa in {1, 8, 9} x rows in {1, 63, 64, 10^6} x (xb, taps, attention scalars, alignment)."""
    flags = [dict(), dict(fb=3), dict(taps=2), dict(attn=True), dict(aligned=False), dict(fb=3, attn=True)]
    n_embed = 0
    for fo, fa, rows, fl in itertools.product(range(1, 257), (1, 8, 9), (1, 63, 64, 10 ** 6), flags):
        got, want = _lib.dense_route(fa, fo, rows, **fl), D.route_py(fa, fo, rows, **fl)
        assert got == want, (fa, fo, rows, fl, got, want)
        n_embed += got['kernel'] == 'embed'
        if got['kernel'] == 'embed':
            assert not fl and fa <= 8 and fo % 4 == 0 and rows >= 64
            assert got['stride'] % (fo // 4) == 0 and got['stride'] == 256 * got['workgroups'] and 1 <= got['workgroups'] <= D.EMBED_CAP
        else:
            assert got['rows_per_wg'] * got['param'] in (128, 256, 512, 1024) and got['rows_per_wg'] == D.TILE_ROWS[got['param']]
            assert (got['workgroups'] - 1) * got['rows_per_wg'] < rows <= got['workgroups'] * got['rows_per_wg']
            assert 4 * got['param'] >= fo and (got['param'] == 1 or 2 * got['param'] < fo)
    assert n_embed == 64 * 2 * 2


def test_embed_stride_keeps_a_lane_on_its_chunk():
    """Every f_out the stream takes, at row counts around the cap: the stride is a multiple of the lanes of a row, the grid covers
    the lanes in at most ceil(total / stride) trips, and never launches more than the cap."""
    for fo in range(4, 257, 4):
        f4 = fo // 4
        for rows in (64, 65, 333, 4096, 16383, 16384, 16400, 16700, 10 ** 6, 1 << 40):
            r = _lib.dense_route(8, fo, rows)
            assert r == D.route_py(8, fo, rows) and r['kernel'] == 'embed'
            assert r['stride'] % f4 == 0 and r['workgroups'] <= D.EMBED_CAP
            if rows * f4 <= r['stride']:                   # one trip: at most g - 1 surplus workgroups short of covering every lane
                assert rows * f4 > r['stride'] - 256 * (f4 // D.math.gcd(256, f4)) or r['workgroups'] == f4 // D.math.gcd(256, f4)


def test_refused_shapes():
    for kw in (dict(fa=0, f_out=8, rows=3), dict(fa=8, f_out=257, rows=3), dict(fa=4000, fb=97, f_out=8, rows=3), dict(fa=8, f_out=8, rows=-1),
               dict(fa=8, f_out=8, rows=3, taps=17), dict(fa=8, f_out=8, rows=3, taps=2, fb=1), dict(fa=257, f_out=8, rows=3, taps=16)):
        with pytest.raises(_lib.UdsError, match='uds_dense_route'):
            _lib.dense_route(**kw)


def test_every_case_lands_on_its_kernel():
    ids = [c['id'] for c in D.DENSE_CASES]
    assert len(set(ids)) == len(ids)
    reached = set()
    for c in D.DENSE_CASES:
        r = _lib.dense_route(**D.case_route(c))
        assert (r['kernel'], r['param'], r['workgroups']) == (c['kernel'], c['param'], c['wgs']), (c['id'], r)
        reached.add((r['kernel'], r['param']))
    for c in D.CONV_CASES:
        r = _lib.dense_route(**D.conv_route(c))
        assert r['kernel'] == 'tiled' and r['param'] == D.tiled_cg(c['shape'][4])
        reached.add((r['kernel'], r['param']))
    assert reached == {('embed', F) for F in range(1, 9)} | {('tiled', cg) for cg in D.TILE_ROWS}


def test_case_tables_are_what_they_claim():
    for c in D.TILED_WIDTH_CASES[:len(D.WIDTHS)] + D.ATTN_CASES:              # three workgroups, the last holding one row
        assert c['wgs'] == 3 and c['rows'] % D.TILE_ROWS[c['param']] == 1
    assert sorted({c['param'] for c in D.ATTN_CASES}) == [1, 2, 4, 16, 64]
    assert [c['rows'] for c in D.TILED_WIDTH_CASES[len(D.WIDTHS):]] == [1, 127, 128, 1, 63, 64, 1, 15, 16]
    assert all(c['rows'] < 64 and c['kernel'] == 'tiled' for c in D.K_CASES if c['fa'] <= 8)
    for c in D.CAPPED_CASES:                                                    # the grid-stride loop makes a full second trip
        r = _lib.dense_route(**D.case_route(c))
        lanes = c['rows'] * c['fo'] // 4
        assert lanes > r['stride'] and lanes - r['stride'] == D.CAPPED_SECOND_TRIP[c['id']]
        assert c['rows'] * c['fo'] * 4 < 20e6
    assert [c['wgs'] for c in D.CAPPED_CASES] == [4096, 4095]
    # the sub-call of the bitwise comparison runs on the tiled kernel; odd lane counts per row are in the table
    for c in D.EMBED_BITWISE_CASES:
        assert _lib.dense_route(c['fa'], c['fo'], D.EMBED_BITWISE_ROWS)['kernel'] == 'tiled'
    assert {c['fo'] // 4 for c in D.EMBED_CASES} >= {1, 3, 63, 64}
    assert len(D.EMBED_BITWISE_CASES) == 3 + 3 * 5 * 2
    # the misaligned call goes to the tiled kernel, the aligned one to the stream
    assert _lib.dense_route(**D.case_route(D.MISALIGNED_CASE, aligned=False))['kernel'] == 'tiled'
    # row subsets stay on the batch call's kernel
    for c, slices in D.ROW_SUBSETS:
        for lo, hi in slices:
            r = _lib.dense_route(c['fa'], c['fo'], hi - lo)
            assert (r['kernel'], r['param']) == (c['kernel'], c['param']) and 0 <= lo < hi <= c['rows']
    # conv: a workgroup straddles time steps and batch elements wherever B > 1 and T R is below its rows
    straddle = [c for c in D.CONV_CASES if c['shape'][0] > 1 and c['shape'][1] * c['shape'][2] < D.TILE_ROWS[D.tiled_cg(c['shape'][4])]]
    assert len(straddle) >= 6
    assert {c['dil'] for c in D.CONV_CASES} == {1, -1, 2, -2, 4, -4, 7, -7}
    B, T, R, F = D.CUMSUM_SHAPES[0]
    assert B * R * F // 4 == 387


def test_activation_cases_carry_signal():
    """The pre-activations cross zero and pass both clamps of hard_sigmoid."""
    for c in D.ACT_CASES:
        v = D.dense_pre(D.dense_inputs(c))
        assert float(v.min()) < -2.5 and float(v.max()) > 2.5, (c['id'], float(v.min()), float(v.max()))
        assert 0.2 < float((v > 0).double().mean()) < 0.8
        out = D.dense_ref(c, D.dense_inputs(c))[0]
        if c['act'] == 'hard_sigmoid':
            assert bool((out == 0).any()) and bool((out == 1).any()) and bool(((out > 0) & (out < 1)).any())
        if c['act'] == 'relu':
            assert bool((out == 0).any()) and bool((out > 0).any())


def test_inputs_are_signed_and_f32_exact():
    for c in D.DENSE_CASES[::7] + [D.CAPPED_CASES[0]]:
        for t in D.dense_inputs(c).values():
            if t is not None:
                assert bool((t.float().double() == t).all()) and (t.numel() < 8 or float(t.min()) < 0 < float(t.max()))
    c = D.ATTN_CASES[5]
    p = D.dense_inputs(c)
    out, ss, sn = D.dense_ref(c, p)
    assert ss.shape == (c['rows'],) and float(ss.abs().max()) > 0.5 and not torch.equal(ss, sn)


@pytest.mark.parametrize('c', D.CONV_CASES, ids=[c['id'] for c in D.CONV_CASES])
def test_conv_reference(c):
    """The loop agrees with the oracle for dil > 0; the shifted rows times the flat kernel give the convolution; the dil < 0
    reference is the adjoint of the dil > 0 one: <conv(x; W, d), g> = <x, conv(g; W^T per tap, -d)>."""
    B, T, R, F, H, taps = c['shape']
    p = D.conv_inputs(c)
    pre = D.conv_pre(p['x'], p['kernel'], c['dil'])
    lin = dict(c, act='linear')
    ref = D.conv_ref(lin, dict(p, b=None))
    assert float((ref - pre).abs().max()) <= 1e-13 * max(1.0, float(pre.abs().max()))
    rows = D.conv_shifted_rows(p['x'], taps, c['dil'])
    assert rows.shape == (B * T * R, taps * F)
    gemm = (rows @ p['kernel'].reshape(taps * F, H)).reshape(B, T, R, H)
    assert float((gemm - pre).abs().max()) <= 1e-13 * max(1.0, float(pre.abs().max()))
    g = torch.from_numpy(D._gen(c['id'] + '-g').uniform(-0.5, 0.5, (B, T, R, H)))
    adj = D.conv_pre(g, p['kernel'].transpose(1, 2).contiguous(), -c['dil'])
    lhs, rhs = float((pre * g).sum()), float((p['x'] * adj).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)) and abs(lhs) > 1e-3
    assert float(D.conv_ref(c, p).abs().max()) > 0.1


def test_conv_out_of_range_case_has_one_live_tap():
    assert len(D.CONV_OUT_OF_RANGE) == 2
    for c in D.CONV_OUT_OF_RANGE:
        assert D.conv_live_taps(c) == [c['shape'][5] - 1]
        p = D.conv_inputs(c)
        pre = D.conv_pre(p['x'], p['kernel'], c['dil'])
        assert torch.equal(pre, p['x'] @ p['kernel'][-1])
    for c in D.CONV_CASES:
        if c not in D.CONV_OUT_OF_RANGE and c['shape'][1] > 1:
            assert len(D.conv_live_taps(c)) > 1


def test_cumsum_reference():
    for c in D.CUMSUM_CASES:
        p = D.cumsum_inputs(c)
        ref = D.cumsum_ref(c, p)
        assert ref.shape == c['shape'] and bool(torch.isfinite(ref).all())
    c = next(c for c in D.CUMSUM_CASES if c['shape'] == (2, 60, 9, 8) and c['act'] == 'linear' and c['res'])
    p = D.cumsum_inputs(c)
    ref = D.cumsum_ref(c, p)
    assert torch.allclose(ref[:, 59], p['x'].sum(1) + p['res'][:, 0], rtol=0, atol=1e-12) and float(ref.abs().max()) > 2


def test_out_arguments_are_checked_without_a_device():
    """Host tensors only, so this runs anywhere: a wrong shape of out= / s_out= is refused before anything else is looked at, a
    host tensor (of any dtype) as out= by the device check.  tests/test_gpu_dense_routes.py repeats the dtype case on the device."""
    x, k = torch.zeros(5, 4), torch.zeros(4, 8)
    with pytest.raises(_lib.UdsError, match=r'out must be \(5, 8\)'):
        _lib.dense_act(x, k, out=torch.zeros(5, 4))
    with pytest.raises(_lib.UdsError, match=r's_self must be \(5,\)'):
        _lib.dense_act(x, k, attn=(torch.zeros(8), torch.zeros(8)), s_out=(torch.zeros(4), torch.zeros(5)))
    with pytest.raises(_lib.UdsError, match='s_out is given without attn'):
        _lib.dense_act(x, k, s_out=(torch.zeros(5), torch.zeros(5)))
    with pytest.raises(_lib.UdsError, match=r'out must be \(1, 2, 3, 8\)'):
        _lib.conv1d_causal(torch.zeros(1, 2, 3, 4), torch.zeros(2, 4, 8), out=torch.zeros(1, 2, 3, 4))
    with pytest.raises(_lib.UdsError, match=r'out must be \(1, 2, 3, 4\)'):
        _lib.cumsum_act(torch.zeros(1, 2, 3, 4), out=torch.zeros(1, 2, 3, 8))
    with pytest.raises(_lib.UdsError, match='out is on cpu'):
        _lib.cumsum_act(torch.zeros(1, 2, 3, 4), out=torch.zeros(1, 2, 3, 4, dtype=torch.float64))
    with pytest.raises(_lib.UdsError, match='out is on cpu'):
        _lib.dense_act(x, k, out=torch.zeros(5, 8))
