"""CPU checks behind tests/test_gpu_rowgemm_routes.py: every case of tests/rowgemm_util.py reaches the instantiation it claims,
every instantiation the launch code can select is reached, the route mirror agrees with the library wherever the library answers
without a device, the fp64 references are the derivatives they stand for, and a kernel that makes one of the classic boundary
mistakes moves the result by more than the GPU tolerance at the shapes the cases use."""
import pytest
import torch

from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from tests import rowgemm_util as RU
from tests.rowgemm_util import case_id, conv_ref, route, wgrad_ref

TOL_ROWGEMM = 1e-4      # the bound of tests/test_gpu_emulator.py; the GPU file's own bounds are no larger


# ---- tables and routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RU.ALL_CASES, ids=case_id)
def test_case_reaches_the_route_it_claims(case):
    assert route(case) == case['claims']


def test_case_ids_are_unique():
    ids = [case_id(c) for c in RU.ALL_CASES]
    assert len(ids) == len(set(ids))


def test_every_instantiation_is_reached():
    routes = [route(c) for c in RU.ALL_CASES]
    assert len(RU.ALL_SMALL) == 18 and {r for r in routes if r[0] == 'small'} == RU.ALL_SMALL
    pers = [r for r in routes if r[0] == 'persistent']
    assert len(RU.ALL_PERSISTENT) == 10 and {r[1:4] for r in pers} == RU.ALL_PERSISTENT
    assert {r[4] for r in pers} == {False, True}
    assert {r[1] for r in pers if r[4]} == {2, 4}                    # the XCD mapping with both store paths of the epilogue
    stream = [r for r in routes if r[0] == 'stream']
    assert len(RU.ALL_STREAM) == 18 and {r[1:4] for r in stream} == RU.ALL_STREAM
    assert len(RU.ALL_WGRAD) == 18 and {r[1:3] for r in routes if r[0] == 'wgrad'} == RU.ALL_WGRAD
    assert len(RU.ALL_EMBED) == 8 and {r for r in routes if r[0] == 'embed'} == RU.ALL_EMBED
    assert {r for r in routes if r[0] == 'tiled'} == RU.ALL_TILED
    conv_tiled = {route(c) for c in RU.DENSE_CASES if c['taps'] and c['dil'] < 0}
    assert conv_tiled == RU.ALL_TILED                                # a negative dilation once per CG class


def test_ring_2_is_reachable_at_one_block_column_only():
    """Nobody needs to look for a ring-2 case at MB = 2 or 4: whatever fits ring 2 there already fits ring 3 without the tile."""
    assert RU.ring2_reachable(1) and not RU.ring2_reachable(2) and not RU.ring2_reachable(4)
    assert [kt for kt in range(1, 65) if RU.rowgemm_ring(32 * kt, 1) == 2] == [56, 57, 58]
    # the ranges the persistent cases sit at the ends of
    rings = lambda mb: {r: [kt for kt in range(1, 65) if RU.rowgemm_ring(32 * kt, mb) == r] for r in (5, 3, -3)}
    ends = lambda mb: {r: (v[0], v[-1]) for r, v in rings(mb).items()}
    assert ends(4) == {5: (1, 7), 3: (8, 11), -3: (12, 13)}
    assert ends(2) == {5: (1, 15), 3: (16, 23), -3: (24, 27)}
    assert ends(1) == {5: (1, 34), 3: (35, 50), -3: (51, 55)}


def test_small_table_covers_the_edges_the_issue_lists():
    cs = RU.SMALL_CASES
    rows = {c['B'] * c['T'] * c['R'] for c in cs}
    assert {1, 15, 16, 17} <= rows
    assert {c['fo'] for c in cs} >= {1, 3, 17, 33, 50, 16, 32, 64}
    assert {c['dil'] for c in cs if c['taps'] > 1} >= {1, 2, 4, -1, -2, -4}
    assert any(c['taps'] > 1 and abs(c['dil']) >= c['T'] for c in cs)
    assert any((c['B'], c['T'], c['R']) == (2, 7, 5) for c in cs)
    assert any(not c['bias'] for c in cs) and {c['act'] for c in cs} == set(RU.ACTS)
    for mb in (1, 2, 4):                                             # every depth from one wide tap and from several
        for kt in RU.ROWGEMM_SMALL_KT:
            taps = {c['taps'] > 1 for c in cs if c['claims'] == ('small', mb, kt)}
            assert taps == {False, True}, (mb, kt)


def test_persistent_table_rows_and_grid():
    cs = RU.PERSISTENT_CASES
    rows = {c['B'] * c['T'] * c['R'] for c in cs}
    assert {63, 64, 65} <= rows and min(rows) == 1
    assert any(r > 256 * RU.WAVE_TILE and r <= RU.ROWGEMM_SMALL_ROWS for r in rows)       # more wave-tiles than workgroups
    assert any(c['F2'] for c in cs)
    x = [c for c in cs if route(c)[4]]
    assert {c['T'] for c in x} >= {2, 5, 9} and {c['dil'] > 0 for c in x} == {False, True}
    seg = RU.rowgemm_xcd_seg(5, 4100)
    assert seg == 528 and 4100 - 7 * seg == 404 and 404 % RU.WAVE_TILE == 20
    assert route(RU.K384_CASE) == ('persistent', 4, 3, False, False) and route(RU.K384_HEAD) == ('small', 4, 12)
    assert RU.K384_CASE['B'] * RU.K384_CASE['T'] * RU.K384_CASE['R'] > RU.ROWGEMM_SMALL_ROWS


def test_stream_layouts():
    for T, D, n_seg, last in RU.STREAM_LAYOUTS:
        got = RU.conv_stream_segments(16, 250, T, D)
        assert (got[0], got[2]) == (n_seg, last), (T, D, got)
        both = {c['dil'] > 0 for c in RU.STREAM_CASES if (c['B'], c['R'], c['T'], abs(c['dil'])) == (16, 250, T, D)}
        assert both == ({False, True} if n_seg > 1 else {True}), (T, D)
    assert any(last < 2 * D + 1 and n_seg > 1 for T, D, n_seg, last in RU.STREAM_LAYOUTS)     # shorter than the accumulator ring
    streams = {c['B'] * ((c['R'] + 15) // 16) for c in RU.STREAM_CASES if c['same_as'] is None}
    assert streams == {256, 258}
    assert all(c['R'] % 16 for c in RU.STREAM_CASES)
    assert {c['act'] for c in RU.STREAM_CASES} == set(RU.ACTS)
    assert sum(not c['bias'] for c in RU.STREAM_CASES) == 1


def test_wgrad_table_covers_the_edges_the_issue_lists():
    cs = RU.WGRAD_CASES
    assert {c['F'] for c in cs if c['bias']} >= {15, 16, 31, 32, 47, 48, 79, 80, 111, 112, 127, 1, 5}
    assert {c['F'] for c in cs if not c['bias']} >= {16, 48, 128}
    assert {c['H'] for c in cs} >= {1, 16, 17, 32, 33, 63, 64}
    assert {c['B'] * c['T'] * c['R'] for c in cs} >= {1, 31, 32, 33, 128, 129, 2049, 65409, 70000}
    assert RU.wgrad_grid(129) == 2 and RU.wgrad_empty_waves(129) == 3
    assert RU.wgrad_grid(2049) == 17 and RU.wgrad_grid(65409) == 512 and (70000 + 127) // 128 > 512
    assert RU.wgrad_rows_per_wave(70000) == 64 and RU.wgrad_empty_waves(70000) == 954
    sh = {(c['shift'], c['T']) for c in cs}
    assert any(s == 0 for s, _ in sh) and any(s == T - 1 and s > 0 for s, T in sh) and any(s == T for s, T in sh) and any(s == T + 1 for s, T in sh)
    assert any(c['shift'] == 1 and c['R'] == 33 and c['B'] == 2 for c in cs)


# ---- the mirror against the library -----------------------------------------------------------------------------------------
def test_mirror_agrees_with_the_library():
    lib = _lib.load()
    for rows in (1, 127, 128, 129, 2049, 65408, 65409, 65537, 70000, 10 ** 7):
        for F in (1, 15, 16, 17, 47, 48, 49, 80, 81, 112, 113, 127, 128, 129):
            for H in (1, 16, 17, 32, 33, 64, 65):
                for wb in (0, 1):
                    mt, nt = RU.wgrad_mt(F + wb), RU.wgrad_nt(H)
                    want = RU.wgrad_grid(rows) * mt * 16 * nt * 16
                    assert lib.uds_wgrad_workspace_floats(rows, F, H, wb) == want, (rows, F, H, wb)
    for fo in range(1, 65):
        for kt in (1, 2, 13, 58):
            assert lib.uds_rowgemm_packed_bytes(32 * kt, fo) == kt * RU.rowgemm_mb(fo) * 2 * 64 * 16
    assert lib.uds_rowgemm_packed_bytes(64, 65) == 0 and lib.uds_rowgemm_packed_bytes(48, 16) == 0
    for fo in (1, 16, 17, 32, 33, 64):
        for kt in range(1, 65):
            assert _lib.rowgemm_supported(32 * kt, 32, fo) == (RU.rowgemm_ring(32 * kt, RU.rowgemm_mb(fo)) != 0), (kt, fo)


def test_wgrad_supported_agrees_with_the_refusals():
    for F, H, wb in RU.WGRAD_REFUSED:
        assert not _lib.wgrad_supported(F, H, wb)
        assert RU.wgrad_mt(F + int(wb)) == 0 or RU.wgrad_nt(H) == 0
    assert _lib.wgrad_supported(127, 64, True) and _lib.wgrad_supported(128, 64, False)
    for c in RU.WGRAD_CASES:
        assert _lib.wgrad_supported(c['F'], c['H'], c['bias'])


# ---- the references are the derivatives they stand for ----------------------------------------------------------------------
def _flat(x):
    B, T, R, F = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * R, T, F)


@pytest.mark.parametrize('taps,dil,T', [(3, 1, 7), (3, 2, 5), (2, 4, 6), (3, 4, 3), (4, 1, 5)])
def test_references_equal_autograd(taps, dil, T):
    """conv_ref with a negative dilation on the transposed taps (as autograd.Conv1DFn forms them) is the input gradient of
    conv1d_causal; wgrad_ref with shift (taps - 1 - j) dil is the gradient of tap j; its column sums are the bias gradient."""
    g = torch.Generator().manual_seed(taps * 100 + dil * 10 + T)
    B, R, F, H = 2, 5, 6, 4
    x = (torch.rand(B, T, R, F, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    k = (torch.rand(taps, F, H, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    b = (torch.rand(H, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    gz = torch.rand(B, T, R, H, generator=g, dtype=torch.float64) - 0.5
    y = OE.conv1d_causal(_flat(x), k, b, dil, 'linear')
    dx, dk, db = torch.autograd.grad((y * _flat(gz)).sum(), (x, k, b))
    kt = k.detach().transpose(1, 2).contiguous()
    assert float((conv_ref(gz, kt, None, -dil, 'linear') - dx).abs().max()) <= 1e-12
    for j in range(taps):
        wk, wb = wgrad_ref(x.detach(), gz, (taps - 1 - j) * dil)
        assert float((wk - dk[j]).abs().max()) <= 1e-12
        assert float((wb - db).abs().max()) <= 1e-12


# ---- signal: a kernel with the same mistake cannot pass -------------------------------------------------------------------
def _moved(wrong, ref, tol):
    return float((wrong - ref).abs().max()) > tol * max(1.0, float(ref.abs().max()))


def test_signal_row_gemm_boundaries():
    """Small and persistent kernels: a ragged block whose last row repeats the row before it (the clamp of the loads leaking into
    the stores), a dilation taken one step off, a look-ahead window read as a causal one."""
    for c in (RU.SMALL_CASES[1], RU.SMALL_CASES[7], RU.SMALL_CASES[27], RU.PERSISTENT_CASES[21], RU.PERSISTENT_CASES[23]):
        p = RU.rowgemm_inputs(c)
        ref = RU.rowgemm_ref(c, p)
        flat = ref.reshape(-1, c['fo']).clone()
        flat[-1] = flat[-2]
        assert _moved(flat.reshape(ref.shape), ref, TOL_ROWGEMM), case_id(c)
        off = conv_ref(p['x'], p['k'], p['b'], c['dil'] + (1 if c['dil'] > 0 else -1), c['act'])
        assert _moved(off, ref, TOL_ROWGEMM), case_id(c)
        assert _moved(conv_ref(p['x'], p['k'], p['b'], -c['dil'], c['act']), ref, TOL_ROWGEMM), case_id(c)
    c = RU.PERSISTENT_CASES[1]                                       # Dense: a dropped last k-step
    p = RU.rowgemm_inputs(c)
    ref = RU.rowgemm_ref(c, p)
    q = dict(p, k=p['k'].clone())
    q['k'][0, -32:] = 0
    assert _moved(RU.rowgemm_ref(c, q), ref, TOL_ROWGEMM)


def test_signal_stream_halo():
    """Streaming kernel: a segment that re-reads 2 D - 1 halo steps instead of 2 D loses x[s0 - 2 D] W_0 in out[s0]."""
    for c in (RU.STREAM_CASES[6], RU.STREAM_CASES[11], RU.STREAM_CASES[17]):
        assert route(c)[4] > 1
        p = RU.rowgemm_inputs(c)
        ref = RU.rowgemm_ref(c, p)
        D, T = abs(c['dil']), c['T']
        _, seg_len, _ = RU.conv_stream_segments(c['B'], c['R'], T, D)
        xs = p['x'] if c['dil'] > 0 else torch.flip(p['x'], dims=(1,))      # logical time
        pre = torch.zeros_like(ref)
        s0 = seg_len
        pre[:, s0] = xs[:, s0 - 2 * D] @ p['k'][0]
        pre = pre if c['dil'] > 0 else torch.flip(pre, dims=(1,))
        # remove the lost contribution before the activation: recompute from the pre-activation
        lin = conv_ref(p['x'], p['k'], p['b'], c['dil'], 'linear')
        wrong = OD.activation(c['act'])(lin - pre)
        assert _moved(wrong, ref, TOL_ROWGEMM), case_id(c)


def test_signal_wgrad_boundaries():
    """Weight gradient: a shift one off, the last row of the last 32-row step dropped, the bias row read one row off, the second
    batch element's first time steps reading the first's last."""
    for c in RU.WGRAD_CASES:
        p = RU.wgrad_inputs(c)
        rows = c['B'] * c['T'] * c['R']
        tol = RU.wgrad_tol(rows)
        dk, db = wgrad_ref(p['a'], p['g'], c['shift'])
        if c['shift'] < c['T']:                                      # at shift = T - 1 the next shift gives zero
            assert _moved(wgrad_ref(p['a'], p['g'], c['shift'] + 1)[0], dk, tol), case_id(c)
        if c['bias']:                                                # row F of the partial is d_bias: rows F - 1 and F + 1 are not
            assert _moved(dk[c['F'] - 1], db, tol) and _moved(torch.zeros_like(db), db, tol), case_id(c)
        if c['shift'] == 0 and rows > 1:
            a2, g2 = p['a'].reshape(-1, c['F'])[:-1], p['g'].reshape(-1, c['H'])[:-1]
            assert _moved(a2.t() @ g2, dk, tol), case_id(c)
        if 0 < c['shift'] < c['T'] and c['B'] > 1:                   # the shift applied to flat rows, across the batch boundary
            F, H, s = c['F'], c['H'], c['shift'] * c['R']
            a2, g2 = p['a'].reshape(-1, F), p['g'].reshape(-1, H)
            assert _moved(a2[:-s].t() @ g2[s:], dk, tol), case_id(c)


def test_signal_fp32_kernels():
    """k_embed_act / k_dense_act: a lane that keeps the wrong column chunk (a grid stride that is no multiple of f_out / 4), a
    missing last row."""
    for c in RU.DENSE_CASES:
        p = RU.rowgemm_inputs(c)
        ref = RU.rowgemm_ref(c, p)
        if c['fo'] >= 8:
            assert _moved(torch.roll(ref, 4, dims=-1), ref, 5e-6), case_id(c)
        flat = ref.reshape(-1, c['fo']).clone()
        flat[-1] = flat[-2]
        assert _moved(flat.reshape(ref.shape), ref, 5e-6), case_id(c)
