"""Direct fp64 parity of the C entries that run in every inference forward and every rollout step and were reached only through
whole-`Emulator` tests: uds_dense_cumsum_heads, uds_rowgemm_forward_pair, uds_rowgemm_forward_cat with a column block,
uds_roll_update, plus the small shapes of uds_dense_cumsum.  References: oracle/tail_ref.py (pinned on the CPU by
tests/test_tail_ref_math.py), oracle.emulator_ref.conv1d_causal and oracle.spektral_dense.dense, all in fp64.

Every output (and the in-place windows of uds_roll_update) is a contiguous view inside a larger tensor filled with a sentinel
bit pattern that must survive on both sides; every input is a view inside a NaN-filled tensor and every output element must be
finite.  Plain allocations: nothing here is meant to fault.

Tolerances (relative to max(1, max|ref|), tests.util.close; UDS_TOL_REPORT=1 prints observed / allowed):
  uds_dense_cumsum_heads   tests.util.heads_tol -- see HEADS TOLERANCE below
  pair / cat / dense_cumsum   the project's TOL_ROWGEMM = 1e-4 (x sqrt(T) for the prefix sum), as tests/test_gpu_emulator.py
  uds_roll_update          q_in / q_out 1e-6 (the uds_flow_balance tolerance); everything else is a copy: torch.equal

HEADS TOLERANCE (measured, not assumed: UDS_TOL_REPORT=1 on an MI355X, fp64 reference oracle.tail_ref.dense_cumsum_heads_ref)
  Observed max|out - ref| over the 24 cases: 5.5e-8 .. 1.86e-5; relative to max(1, max|ref|) the largest is 1.70e-5
  (B2R33T1, n_hidden 2, linear hidden and output activations), then 1.43e-5 (B3R17T2, n_hidden 2) and 1.41e-5 (B1R70T4,
  n_hidden 4); by depth the worst case is n_hidden 0: 9.9e-6, 1: 9.1e-6, 2: 1.7e-5, 3: 1.1e-5, 4: 1.4e-5, 5: 1.1e-5; by
  length T = 1: 1.7e-5, 2: 1.4e-5, 3: 1.2e-5, 4: 1.4e-5, 7: 1.1e-5.  Bounded activations shrink the error, linear / relu chains
  do not; neither T nor the number of chained split-bf16 layers shows a trend, so the file uses one constant,
  tests.util.HEADS_TOL = 8e-5 = 4.7 x the largest observed (the project keeps tolerances 3-6 x above what it measures).

Which case reaches which code (uds_rowgemm_forward_pair): PAIR_CASES below names the instantiation of every case.
"""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from oracle.tail_ref import roll_update_ref
from tests.util import HEADS_CASES, SENTINEL, Guarded, close, heads_case_id, heads_inputs, heads_ref, heads_tol, nan_in

pytestmark = pytest.mark.gpu

TOL_ROWGEMM = 1e-4
TOL_FLOW = 1e-6


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def pack(kernel2d, dev):
    return nan_in(_lib.rowgemm_pack(kernel2d.float().to(dev).contiguous()), dev)


def r32(t):
    return t.float().double()


def rnd(g, *shape):
    """Uniform in +-0.5, fp64 values exactly representable in fp32."""
    return r32(torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5)


# ---- uds_dense_cumsum_heads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', HEADS_CASES, ids=heads_case_id)
def test_dense_cumsum_heads(dev, case):
    p = heads_inputs(case)
    ref = heads_ref(case, p)
    f = lambda t: nan_in(t, dev)
    out = Guarded(ref.shape, dev)
    head_f = (pack(p['Fk'], dev), f(p['f_bias']), case['act_f'], case['act_h']) if case['n_hidden'] else None
    got = _lib.dense_cumsum_heads(f(p['x']), pack(p['W'], dev), f(p['b']), f(p['res']), case['act'],
                                  (pack(p['A'], dev), f(p['a_bias']), case['n_a'], case['act_a']),
                                  [(pack(H, dev), f(hb)) for H, hb in p['hidden']], head_f, out=out.view)
    assert got is out.view
    torch.cuda.synchronize()
    out.check('out')
    tol = heads_tol(case)
    d = (got.double().cpu() - ref).abs()
    print('heads %-70s err a %.3e  f %.3e  allowed %.3e' % (heads_case_id(case), float(d[..., :case['n_a']].max()),
                                                          float(d[..., case['n_a']:].max()) if case['n_hidden'] else 0.0,
                                                          tol * max(1.0, float(ref.abs().max()))))
    close(got, ref, tol)


# ---- uds_rowgemm_forward_pair -----------------------------------------------------------------------------------------------
# (B, T, R0, R1, F, taps, dil, f_out), what it reaches
PAIR_CASES = [
    ((1, 1, 1, 1, 64, 1, 1, 64), 'k_rowgemm_small_pair<4, 2>: a single row each'),
    ((2, 5, 7, 40, 64, 3, 1, 64), 'k_rowgemm_small_pair<4, 6>: 70 against 400 rows'),
    ((1, 4, 300, 3, 64, 3, 2, 32), 'k_rowgemm_small_pair<2, 6>: the first problem much larger'),
    # the grid comes from the larger problem whichever it is: 38 sixteen-row blocks next to 1 (a grid sized from the first
    # problem alone would hold 8 of them)
    ((1, 2, 3, 300, 64, 3, 1, 64), 'k_rowgemm_small_pair<4, 6>: the second problem much larger'),
    ((3, 3, 17, 16, 64, 1, 1, 16), 'k_rowgemm_small_pair<1, 2>'),
    ((2, 6, 33, 5, 64, 3, 4, 3), 'k_rowgemm_small_pair<1, 6>: f_out no multiple of 4, a dilation past T'),
    ((1, 5, 20, 9, 32, 2, 1, 32), 'k_rowgemm_small_pair<2, 2>: two taps of one k-step each'),
    ((2, 4, 10, 12, 96, 2, 1, 64), 'k_rowgemm_small_pair<4, 6>: three k-steps per tap'),
    ((1, 1, 50, 70, 192, 1, 1, 48), 'k_rowgemm_small_pair<4, 6>: Dense with f_out < 64, the other epilogue branch'),
    ((1, 1, 16384, 16384, 64, 1, 1, 64), 'k_rowgemm_small_pair<4, 2> exactly at its row limit'),
    ((1, 1, 16400, 8, 64, 1, 1, 64), 'fall-back, one problem over the row limit: two launches'),
    ((1, 3, 9, 9, 32, 3, 1, 32), 'fall-back, K / 32 = 3: two launches'),
]
ACTS = ['relu', 'tanh', 'linear', 'sigmoid', 'hard_sigmoid']


def rowgemm_ref(x, k, b, taps, dil, act):
    B, T, R, F = x.shape
    if taps == 1:
        return OD.dense(x, k[0], b, act)
    bias = b if b is not None else torch.zeros(k.shape[-1], dtype=torch.float64)
    return OE.conv1d_causal(x.permute(0, 2, 1, 3).reshape(B * R, T, F), k, bias, dil, act).reshape(B, R, T, -1).permute(0, 2, 1, 3)


@pytest.mark.parametrize('shape,what', PAIR_CASES, ids=['B%dT%d-R%d-R%d-F%d-taps%d-dil%d-fo%d' % c for c, _ in PAIR_CASES])
def test_rowgemm_forward_pair(dev, shape, what):
    B, T, R0, R1, F, taps, dil, fo = shape
    i = [c for c, _ in PAIR_CASES].index(shape)
    act = ACTS[i % 5]
    g = torch.Generator().manual_seed(200 + i)
    xs = [rnd(g, B, T, R, F) for R in (R0, R1)]
    ks = [rnd(g, taps, F, fo) for _ in range(2)]
    bs = [rnd(g, fo), rnd(g, fo)]
    bs[i % 2] = None                                     # one problem without a bias
    xd = [nan_in(x, dev) for x in xs]
    pk = [pack(k.reshape(taps * F, fo), dev) for k in ks]
    bd = [nan_in(b, dev) for b in bs]
    outs = [Guarded((B, T, R, fo), dev) for R in (R0, R1)]
    got = _lib.rowgemm_forward_pair(xd[0], pk[0], bd[0], xd[1], pk[1], bd[1], fo, act, taps=taps, dilation=dil, out=(outs[0].view, outs[1].view))
    torch.cuda.synchronize()
    for j in range(2):
        assert got[j] is outs[j].view
        outs[j].check('out%d' % j)
        err = close(got[j], rowgemm_ref(xs[j], ks[j], bs[j], taps, dil, act), TOL_ROWGEMM)
        print('pair %s out%d err %.3e' % (what, j, err))
        single = _lib.rowgemm_forward(xd[j], pk[j], bd[j], fo, act, taps=taps, dilation=dil)
        assert torch.equal(got[j].reshape(single.shape), single), 'problem %d differs from uds_rowgemm_forward' % j


# ---- uds_rowgemm_forward_cat into a column block ----------------------------------------------------------------------------
def check_block(out, col0, fo, ref, what):
    """`out` (rows, ldo), sentinel-filled before the call: columns [col0, col0 + fo) hold the result, the rest is untouched."""
    bits = out.view.view(torch.int32)
    assert bool((bits[:, :col0] == SENTINEL).all()) and bool((bits[:, col0 + fo:] == SENTINEL).all()), '%s: wrote outside its columns' % what
    out.check(what)
    return close(out.view[:, col0:col0 + fo], ref, TOL_ROWGEMM)


@pytest.mark.parametrize('with_x2', [False, True])
@pytest.mark.parametrize('col0,fo', [(0, 64), (0, 28), (64, 64), (64, 28), (100, 28)])
def test_rowgemm_cat_column_block(dev, col0, fo, with_x2):
    ldo = 128
    for rows in (1, 17, 100):
        g = torch.Generator().manual_seed(rows + col0 + fo)
        x, x2 = rnd(g, rows, 64), rnd(g, rows, 32) if with_x2 else None
        k, b = rnd(g, 96 if with_x2 else 64, fo), rnd(g, fo)
        out = Guarded((rows, ldo), dev)
        got = _lib.rowgemm_cat(nan_in(x, dev), nan_in(x2, dev), pack(k, dev), nan_in(b, dev), fo, 'tanh', out=out.view, col0=col0)
        assert got is out.view
        torch.cuda.synchronize()
        ref = OD.dense(torch.cat([x, x2], dim=-1) if with_x2 else x, k, b, 'tanh')
        check_block(out, col0, fo, ref, 'rows %d' % rows)


def test_rowgemm_cat_conv_into_a_column_block(dev):
    """taps > 1 with a column block: the C entry allows it, no wrapper reaches it."""
    B, T, R, F, taps, dil, fo, ldo, col0 = 2, 5, 9, 64, 3, 2, 32, 64, 32
    g = torch.Generator().manual_seed(7)
    x, k, b = rnd(g, B, T, R, F), rnd(g, taps, F, fo), rnd(g, fo)
    xd, pk, bd = nan_in(x, dev), pack(k.reshape(taps * F, fo), dev), nan_in(b, dev)
    out = Guarded((B * T * R, ldo), dev)
    rc = _lib.load().uds_rowgemm_forward_cat(xd.data_ptr(), F, None, 0, B, T, R, pk.data_ptr(), bd.data_ptr(), taps, dil, fo, _lib.ACT['relu'],
                                             out.view.data_ptr(), ldo, col0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().uds_last_error()
    torch.cuda.synchronize()
    check_block(out, col0, fo, rowgemm_ref(x, k, b, taps, dil, 'relu').reshape(B * T * R, fo), 'conv block')


# ---- uds_dense_cumsum: small and ragged shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,R,act', [(3, 5, 17, 'relu'), (1, 4, 1, 'tanh'), (1, 6, 15, 'linear'), (2, 11, 33, 'relu')])
def test_dense_cumsum_small_shapes(dev, B, T, R, act):
    """B > 2, T round the input ring of 5, R < 16, an odd number of 16-row units (the last workgroup half empty); the reference
    and the tolerance TOL_ROWGEMM * sqrt(T) of test_dense_cumsum_stream."""
    g = torch.Generator().manual_seed(T + R)
    x, k, b, res = rnd(g, B, T, R, 64), rnd(g, 64, 64), rnd(g, 64), rnd(g, B, 1, R, 64)
    ref = OD.activation(act)(torch.cumsum(x @ k + b, dim=1) + res)
    out = Guarded(ref.shape, dev)
    got = _lib.dense_cumsum(nan_in(x, dev), pack(k, dev), nan_in(b, dev), nan_in(res, dev), act, out=out.view)
    assert got is out.view
    torch.cuda.synchronize()
    out.check('out')
    close(got, ref, TOL_ROWGEMM * max(1.0, T ** 0.5))
    out2 = Guarded(ref.shape, dev)
    _lib.dense_cumsum(nan_in(x, dev), pack(k, dev), None, None, 'linear', out=out2.view)
    torch.cuda.synchronize()
    out2.check('out (no bias, no residual)')
    close(out2.view, torch.cumsum(x @ k, dim=1), TOL_ROWGEMM * max(1.0, T ** 0.5))


# ---- uds_roll_update --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def roll_graph(dev):
    """About 100 nodes: a synthetic drainage network, one hub (node 100, 14 links of both directions) and one node without a
    link (node 101: an empty incidence row)."""
    edges = np.asarray(U.synthetic_drainage_network(100, 120, seed=3), dtype=np.int64)
    hub = np.array([[100, 7 * j + 1] if j % 2 else [7 * j + 1, 100] for j in range(14)], dtype=np.int64)
    gph = U.DrainageGraph.from_edges(np.concatenate([edges, hub]), 102)
    deg = np.diff(np.asarray(gph.inc_n.rowptr))
    assert deg[101] == 0 and deg[100] == 14 and gph.n_node == 102
    handle = _lib.CsrHandle(gph.inc_n)
    sign = torch.as_tensor(gph.inc_n.val, dtype=torch.float32, device=dev)
    return gph, handle, sign, torch.from_numpy(gph.inc_n.to_dense())


@pytest.mark.parametrize('cy,ce,flood', [(1, 3, 0), (2, 3, 1), (5, 1, 1), (8, 8, 0), (2, 8, 1)])
@pytest.mark.parametrize('so,T', [(1, 5), (2, 4), (3, 3), (1, 1)])
def test_roll_update(dev, roll_graph, so, T, cy, ce, flood):
    gph, handle, sign, inc = roll_graph
    B, N, E = 3, gph.n_node, gph.n_edge                   # B * N = 306 threads: more than one 256-thread block
    g = torch.Generator().manual_seed(100 * so + 10 * T + cy + ce)
    u = lambda *s: r32(torch.rand(*s, generator=g, dtype=torch.float64))
    span, mini = 0.5 + u(E), r32((u(E) - 0.5) * 0.6 + 0.05)
    s_in, s_out = 0.5 + 1.5 * u(N), 0.5 + 1.5 * u(N)
    s_in[[2, 50, 100]] = 0.0
    s_out[[9, 50]] = 0.0
    assert bool((mini != 0).all())
    y, ey, b = u(B, so, N, cy), u(B, so, E, ce) * 2 - 1, u(B, so, N, 1)
    x, ex = u(B, T, N, cy + 3), u(B, T, E, ce + 1)
    if flood:                                             # exactly at, just above and just below the threshold
        half = np.float32(0.5)
        y[0, 0, :3, cy - 1] = torch.tensor([0.5, float(np.nextafter(half, np.float32(1))), float(np.nextafter(half, np.float32(0)))], dtype=torch.float64)
        y[2, so - 1, N - 3:, cy - 1] = y[0, 0, :3, cy - 1]
    flow = ey[..., -1] * span + mini
    assert bool((flow > 0).any()) and bool((flow < 0).any())
    ref_p, ref_x, ref_ex = roll_update_ref(inc, span, mini, s_in, s_out, y, ey, b, x, ex, flood)

    f = lambda t: nan_in(t, dev)
    xw, exw, preds = Guarded(x.shape, dev, x), Guarded(ex.shape, dev, ex), Guarded(ref_p.shape, dev)
    got = _lib.roll_update(handle, sign, f(span), f(mini), f(s_in), f(s_out), f(y), f(ey), f(b), xw.view, exw.view, flood, preds=preds.view)
    assert got is preds.view
    torch.cuda.synchronize()
    for t, name in ((xw, 'x'), (exw, 'ex'), (preds, 'preds')):
        t.check(name)
    P, X, EX = preds.view.cpu(), xw.view.cpu(), exw.view.cpu()
    copies = [0] + list(range(3, cy + 2))                 # channels of preds that are copies of y
    assert torch.equal(P[..., copies], ref_p[..., copies].float())
    close(P[..., 1:3], ref_p[..., 1:3], TOL_FLOW)
    assert torch.equal(EX, ref_ex.float())                # shifted rows, ey and the constant 1
    keep = T - so
    assert torch.equal(X[:, :keep], ref_x[:, :keep].float())        # the shifted window rows, every channel
    fed = copies + [cy + 2]                               # y channels (the thresholded bit among them) and b
    assert torch.equal(X[:, keep:][..., fed], ref_x[:, keep:][..., fed].float())
    close(X[:, keep:, :, 1:3], ref_x[:, keep:, :, 1:3], TOL_FLOW)
    assert torch.equal(X[:, keep:, :, 1:3], P[..., 1:3])   # what is fed back is what is returned
    if flood:
        assert X[0, keep, :3, cy + 1].tolist() == [0.0, 1.0, 0.0]
    assert float(P[:, :, 101, 1:3].abs().max()) == 0.0      # the node without links
