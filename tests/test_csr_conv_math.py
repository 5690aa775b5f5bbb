"""GCN and Diffusion from a CSR graph, on the CPU: the raw adjacency matrices a `DrainageGraph` keeps, the filters normalised
on their CSR pattern against the dense calls, the moment form of DiffusionConv (what uds_diffusion_forward_m /
uds_diffusion_backward_m compute) against the collapsed formulas of tests/test_diffusion_grad_math.py, and the models built from
`args.graph`.  With K = K1 - 1, M_0[s, i] = tot[s], M_m[s, i] = sum_{p in row i} a_p^m r[s, col p], gz = act'(y) gy and
G_m[s, i] = sum_q theta[q][K-m] gz[s, i, q]:

    out[s, i, q] = act( sum_{m=0..K} theta[q][K-m] M_m[s, i] )
    dr[s, j]     = sum_i G_0[s, i] + sum_{p : col p = j} sum_{m=1..K} a_p^m G_m[s, row p]
    dtheta[q, k] = sum_{s, i} gz[s, i, q] M_{K-k}[s, i]

`moment_forward` / `moment_grads` evaluate them in a given dtype in the kernels' order (powers by running product, entries in
row order, m upwards); tests/test_gpu_csr_convs.py imports them and the filters below.

Bounds: fp64 against the collapsed formulas and autograd of the dense call 1e-12; the fp32 evaluation a tenth of the operator
bounds of tests/test_gpu_diffusion_train.py (5e-6 forward and dr, 2e-6 dtheta).  Worst fp32 ratio to those bounds measured
here: forward 0.014, dr 0.0004, dtheta 0.064.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd.graph import CSR
from oracle import graphs as OG
from oracle import spektral_dense as OD
from tests.test_diffusion_grad_math import act_from_pre, act_grad_from_out, collapsed_forward, collapsed_grads, csr_of, nonsymmetric_filter
from tests.util import emulator_args, f32_exact, ladder, thick

THETA_SCALE = 0.002       # as tests/test_gpu_diffusion_train.py: glorot-sized coefficients saturate the activation
OP_FWD, OP_DR, OP_DTHETA = 5e-6, 5e-6, 2e-6
# networks on which the reference's networkx calls are defined, as tests/test_graph.py
DEFINED = {'RedChicoSur': (False, True), 'astlingen': (False, True), 'hague': (False, True), 'chaohu': (), 'shunqing': (False,)}


# ------------------------------------------------------------------------------------------------------------------
# the moment form in the kernels' order
# ------------------------------------------------------------------------------------------------------------------
def row_moments(rowptr, col, aval, r, K1, dtype):
    """M (S, n_rows, K1) in `dtype`: M_0 = tot, M_m by running product, the entries of a row in order."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    a, r = np.asarray(aval).astype(dtype), np.asarray(r).astype(dtype)
    S, n_rows = r.shape[0], len(rowptr) - 1
    M = np.zeros((S, n_rows, K1), dtype=dtype)
    M[:, :, 0] = r.sum(axis=-1, dtype=dtype)[:, None]
    for i in range(n_rows):
        for p in range(rowptr[i], rowptr[i + 1]):
            pw = r[:, col[p]].copy()
            for m in range(1, K1):
                pw = pw * a[p]
                M[:, i, m] += pw
    return M


def moment_forward(rowptr, col, aval, theta, r, act, dtype=np.float64):
    theta = np.asarray(theta).astype(dtype)
    K1 = theta.shape[1]
    M = row_moments(rowptr, col, aval, r, K1, dtype)
    z = theta[:, K1 - 1] * M[:, :, 0, None]
    for m in range(1, K1):
        z = z + theta[:, K1 - 1 - m] * M[:, :, m, None]
    return act_from_pre(z, act).astype(dtype)


def moment_grads(rowptr, col, aval, theta, r, y, gy, act, dtype=np.float64):
    """(dr, dtheta) in `dtype` by the moment formulas: G_m per row, then the column walk in row order, g0 added last."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    theta, a = np.asarray(theta).astype(dtype), np.asarray(aval).astype(dtype)
    y, gy = np.asarray(y).astype(dtype), np.asarray(gy).astype(dtype)
    K1 = theta.shape[1]
    S, n_cols = np.asarray(r).shape
    M = row_moments(rowptr, col, aval, r, K1, dtype)
    gz = act_grad_from_out(y, gy, act).astype(dtype)
    G = (gz @ theta[:, ::-1]).astype(dtype)                       # G[s, i, m] = sum_q theta[q][K - m] gz[s, i, q]
    acc = np.zeros((S, n_cols), dtype=dtype)
    for i in range(len(rowptr) - 1):
        for p in range(rowptr[i], rowptr[i + 1]):
            pw = np.ones((), dtype=dtype)
            for m in range(1, K1):
                pw = pw * a[p]
                acc[:, col[p]] += pw * G[:, i, m]
    dr = G[:, :, 0].sum(axis=1, dtype=dtype)[:, None] + acc
    # dtheta[q, k] = sum_{s, i} gz M_{K-k}: the row pass (shared with the table form) sums a row's snapshots in order, then the
    # rows by a balanced tree (xor shuffles, LDS, the reduce kernel) -- restated as such, not as one running sum
    t = np.zeros((len(rowptr) - 1, theta.shape[0], K1), dtype=dtype)
    for s in range(S):
        t += gz[s][:, :, None] * M[s][:, None, :]
    n = 1
    while n < t.shape[0]:
        n *= 2
    t = np.concatenate([t, np.zeros((n - t.shape[0],) + t.shape[1:], dtype=dtype)])
    while t.shape[0] > 1:
        t = t[:t.shape[0] // 2] + t[t.shape[0] // 2:]
    return dr, np.ascontiguousarray(t[0][:, ::-1])


# ------------------------------------------------------------------------------------------------------------------
# filters shared with the GPU tests: (rowptr, col, values) with fp32-exact values
# ------------------------------------------------------------------------------------------------------------------
def valued(csr, seed=0):
    """A pattern with seeded positive values, normalised like DiffusionConv.preprocess, rounded to fp32 numbers."""
    rng = np.random.default_rng(seed)
    c = U.DiffusionConv.preprocess(CSR(csr.rowptr, csr.col, csr.n_rows, csr.n_cols, 0.5 + rng.random(csr.nnz)))
    return CSR(c.rowptr, c.col, c.n_rows, c.n_cols, f32_exact(c.val))


def nonsym_csr():
    ah = f32_exact(nonsymmetric_filter(40, seed=5))
    rowptr, col, val = csr_of(ah)
    return CSR(rowptr.astype(np.int32), col.astype(np.int32), 40, 40, val)


def zero_one_csr():
    """A 12-node directed ring-with-chords filter that stores an explicit 0 and an exact 1 on its support."""
    n = 12
    rng = np.random.default_rng(9)
    pairs = sorted({(i, (i + k) % n) for i in range(n) for k in (1, 3, 4)})
    rc = np.array(pairs)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rc[:, 0], minlength=n))]).astype(np.int32)
    val = f32_exact(0.1 + 0.6 * rng.random(len(pairs)))
    val[5], val[20] = 0.0, 1.0
    return CSR(rowptr, rc[:, 1].astype(np.int32), n, n, val)


FILTERS = {'nonsym': nonsym_csr, 'zero-one': zero_one_csr, 'thick': lambda: valued(thick(67), 1), 'ladder': lambda: valued(ladder(67), 2)}


def problem(csr, C, K1, S, seed, scale=THETA_SCALE):
    """fp32-exact theta (C, K1), r (S, n_cols), gy (S, n_rows, C) in fp64."""
    rng = np.random.default_rng(seed)
    lim = np.sqrt(6.0 / (2 * K1))
    theta = f32_exact((rng.random((C, K1)) * 2 - 1) * lim * scale)
    r = f32_exact(rng.random((S, csr.n_cols)) * 3 - 0.9)
    gy = f32_exact(rng.random((S, csr.n_rows, C)) - 0.5)
    return theta, r, gy


# ------------------------------------------------------------------------------------------------------------------
# graph and filter equivalence
# ------------------------------------------------------------------------------------------------------------------
def _options(net):
    opts = [dict(order=1, directed=False), dict(order=2, directed=False), dict(order=1, directed=True), dict(order=2, directed=True)]
    if net.get('lengths') is not None:
        opts += [dict(order=1, directed=False, length=120.0, lengths=np.array(net['lengths'])),
                 dict(order=1, directed=True, length=120.0, lengths=np.array(net['lengths']))]
    return opts


def _same(got, ref, exact):
    assert np.array_equal(got != 0, ref != 0)
    if exact:
        assert np.array_equal(got, ref)
    else:
        assert np.allclose(got, ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize('name', sorted(DEFINED))
def test_raw_matrices_and_filters_equal_the_dense_calls(networks, name):
    net = networks[name]
    e, n = np.array(net['edges']), net['n_node']
    for o in _options(net):
        kw = dict(directed=o['directed'], order=o['order'], length=o.get('length', 0), lengths=o.get('lengths'))
        exact = not kw['length']
        g = U.DrainageGraph.from_edges(e, n, **kw)
        adj = OG.adjacency(e, **kw)
        # the line graph: the networkx oracle where the reference is defined, the product's own dense view elsewhere
        eadj = OG.edge_adjacency(e, **kw) if o['directed'] in DEFINED[name] else U.graph.get_edge_adj(e, **kw)
        assert g.raw_adj.val is not None and g.raw_edge_adj.val is not None
        _same(g.raw_adj.to_dense(), adj, exact)
        _same(g.raw_edge_adj.to_dense(), eadj, exact)
        gd = U.DrainageGraph.from_dense(adj, eadj, OG.node_edge_incidence(n, e), e)
        _same(gd.raw_adj.to_dense(), adj, True)
        _same(gd.raw_edge_adj.to_dense(), eadj, True)
        for raw, dense in ((g.raw_adj, adj), (g.raw_edge_adj, eadj)):
            for cls in (U.GCNConv, U.DiffusionConv):
                f = cls.preprocess(raw)
                assert isinstance(f, CSR) and f.val is not None and f.col.dtype == np.int32
                _same(f.to_dense(), cls.preprocess(dense), exact)
    r2 = g.replicated(2)
    assert r2.raw_adj.nnz == 2 * g.raw_adj.nnz and np.array_equal(r2.raw_adj.to_dense()[n:, n:], g.raw_adj.to_dense())
    assert r2.raw_edge_adj.n_rows == 2 * g.n_edge


@pytest.mark.parametrize('name', sorted(DEFINED))
def test_graph_base_filters_equal_the_dense_calls(networks, name):
    """The combined (N+E) x (N+E) matrices of graph_base 1 / 2, all five networks, every option of _options.  The dense matrix
    is the networkx oracle's; chaohu's parallel link makes networkx raise in the edge-based builder (as in get_edge_adj,
    tests/test_graph.py), so there the dense matrix is the product's own dense view of the same CSR."""
    net = networks[name]
    e = np.array(net['edges'])
    for build, ref in ((U.graph.node_based_adj_csr, OG.node_based_adjacency), (U.graph.edge_based_adj_csr, OG.edge_based_adjacency)):
        for kw in _options(net):
            c = build(e, None, **kw)                        # no values (length = 0): preprocess counts them as ones
            if name == 'chaohu' and ref is OG.edge_based_adjacency:
                with pytest.raises(Exception):
                    ref(e, **kw)
                dense = c.to_dense()
            else:
                dense = ref(e, **kw)
                _same(c.to_dense(), dense, not kw.get('length'))
            for cls in (U.GCNConv, U.DiffusionConv):
                _same(cls.preprocess(c).to_dense(), cls.preprocess(dense), not kw.get('length'))


def test_gcn_preprocess_adds_a_missing_diagonal_and_keeps_an_isolated_row():
    a = np.array([[0, 2.0, 0, 0], [0.5, 1.0, 0, 0], [0, 0, 0, 0], [0, 3.0, 0, 0]])
    rowptr, col, val = csr_of(a)
    f = U.GCNConv.preprocess(CSR(rowptr.astype(np.int32), col.astype(np.int32), 4, 4, val))
    assert np.allclose(f.to_dense(), U.GCNConv.preprocess(a), rtol=1e-15, atol=0)
    assert f.to_dense()[2, 2] == 1.0 and f.nnz == 7


# ------------------------------------------------------------------------------------------------------------------
# moment-form math
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def references():
    """(filter, K1, act) -> everything the checks below share, computed once."""
    out = {}
    for fname in ('nonsym', 'zero-one', 'thick'):
        csr = FILTERS[fname]()
        rowptr, col = csr.rowptr.astype(np.int64), csr.col.astype(np.int64)
        for K1 in (1, 2, 7, 16):
            for act in ('tanh', 'relu', 'linear', 'sigmoid') if K1 == 7 else ('tanh',):
                theta, r, gy = problem(csr, 8, K1, 3, seed=K1 + len(fname))
                y = collapsed_forward(rowptr, col, csr.val, theta, r, act)
                dr, dth = collapsed_grads(rowptr, col, csr.val, theta, r, y, gy, act)
                out[fname, K1, act] = (csr, rowptr, col, theta, r, gy, y, dr, dth)
    return out


def _cases():
    return [(f, K1, act) for f in ('nonsym', 'zero-one', 'thick') for K1 in (1, 2, 7, 16)
            for act in (('tanh', 'relu', 'linear', 'sigmoid') if K1 == 7 else ('tanh',))]


def test_the_filters_are_what_they_claim():
    ns = nonsym_csr().to_dense()
    assert not ns[4].any() and not ns[:, 4].any() and not np.allclose(ns, ns.T)
    zo = zero_one_csr()
    assert (zo.val == 0.0).sum() == 1 and (zo.val == 1.0).sum() == 1 and zo.nnz == 36
    assert thick(67).degrees().min() == 33


@pytest.mark.parametrize('fname,K1,act', _cases())
def test_moment_form_equals_the_collapsed_formulas_in_fp64(references, fname, K1, act):
    csr, rowptr, col, theta, r, gy, y, dr, dth = references[fname, K1, act]
    ym = moment_forward(rowptr, col, csr.val, theta, r, act)
    assert np.abs(ym - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    drm, dthm = moment_grads(rowptr, col, csr.val, theta, r, y, gy, act)
    assert np.abs(drm - dr).max() <= 1e-12 * max(1.0, np.abs(dr).max())
    assert np.abs(dthm - dth).max() <= 1e-12 * max(1.0, np.abs(dth).max())
    assert np.abs(dth).max() > 1e-3                                           # the references carry signal
    if act in ('tanh', 'sigmoid'):
        lo, hi = (-0.9, 0.9) if act == 'tanh' else (0.1, 0.9)
        assert np.mean((y > lo) & (y < hi)) > 0.9                             # unsaturated
    # autograd of the dense call (an explicit 0 on the support is a zero entry of the dense array: both take c0)
    x = torch.from_numpy(np.stack([r * 0.25, r * 0.75], axis=-1)).requires_grad_(True)       # x.sum(-1) = r
    th = torch.from_numpy(theta).requires_grad_(True)
    yd = OD.diffusion_conv_dense(x, torch.from_numpy(csr.to_dense()), th, act)
    (yd * torch.from_numpy(gy)).sum().backward()
    assert np.abs(ym - yd.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(y).max())
    drm, dthm = moment_grads(rowptr, col, csr.val, theta, r, yd.detach().numpy(), gy, act)
    assert np.abs(drm - x.grad[..., 0].numpy()).max() <= 1e-12 * max(1.0, np.abs(dr).max())
    assert np.abs(dthm - th.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dth).max())


@pytest.mark.parametrize('fname,K1,act', _cases())
def test_fp32_in_the_kernels_order_stays_within_a_tenth_of_the_operator_bounds(references, fname, K1, act):
    csr, rowptr, col, theta, r, gy, y, dr, dth = references[fname, K1, act]
    y32 = moment_forward(rowptr, col, csr.val, theta, r, act, np.float32)
    assert y32.dtype == np.float32
    dr32, dth32 = moment_grads(rowptr, col, csr.val, theta, r, y32, gy, act, np.float32)
    # the gradients of the fp64 reference at the fp32 output would mix two errors: compare at the same y, as the GPU test does
    dr_ref, dth_ref = collapsed_grads(rowptr, col, csr.val, theta, r, y32.astype(np.float64), gy, act)
    ratios = (np.abs(y32 - y).max() / (OP_FWD * max(1.0, np.abs(y).max())),
              np.abs(dr32 - dr_ref).max() / (OP_DR * max(1.0, np.abs(dr_ref).max())),
              np.abs(dth32 - dth_ref).max() / (OP_DTHETA * max(1.0, np.abs(dth_ref).max())))
    print('fp32 / bound: forward %.4f dr %.4f dtheta %.4f' % ratios)
    assert max(ratios) <= 0.1, ratios


# ------------------------------------------------------------------------------------------------------------------
# models from args.graph
# ------------------------------------------------------------------------------------------------------------------
def _shapes(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


@pytest.mark.parametrize('graph_base', [0, 1])
@pytest.mark.parametrize('conv', ['GCN', 'Diffusion'])
def test_models_build_from_args_graph(networks, conv, graph_base):
    """Emulator and ConvNet from `args.graph` (no dense matrix in args): same parameters, names and shapes, and the same initial
    values from the same generator, as the dense-built model; Diffusion layers take the table-free form."""
    net = networks['astlingen']
    e, n = np.array(net['edges']), net['n_node']
    over = dict(conv=conv, n_sp_layer=2, graph_base=graph_base)
    dense_args = emulator_args(e, n, **over)
    g_args = SimpleNamespace(**{k: v for k, v in vars(dense_args).items() if k not in ('adj', 'edge_adj', 'node_edge')})
    g_args.graph = U.DrainageGraph.from_edges(e, n)
    for make in (lambda a: U.Emulator(a.conv, a.resnet, a.recurrent, a, generator=torch.Generator().manual_seed(5)),
                 lambda a: U.agent.ConvNet(SimpleNamespace(**dict(vars(a), conv_dim=64)), conv, generator=torch.Generator().manual_seed(5))):
        md, mg = make(dense_args), make(g_args)
        assert _shapes(md) == _shapes(mg) and len(_shapes(mg)) > 0
        for (k, a), (_, b) in zip(md.state_dict().items(), mg.state_dict().items()):
            assert torch.equal(a, b), k
        convs = [m for m in mg.modules() if isinstance(m, (U.DiffusionConv, U.GCNConv))]
        assert len(convs) == (2 if graph_base else 4) * (2 if isinstance(mg, U.Emulator) else 1)
        if conv == 'Diffusion':
            assert all(m.moments for m in convs) and not any(m.moments for m in md.modules() if isinstance(m, U.DiffusionConv))
        filt = mg._base_filter if isinstance(mg, U.Emulator) and graph_base else None
        if filt is not None:
            assert isinstance(filt, CSR) and np.allclose(filt.to_dense(), md._base_filter, rtol=1e-12, atol=0)


@pytest.mark.parametrize('graph_base', [1, 2])
def test_convnet_gat_graph_base_from_args_graph(networks, graph_base):
    """ConvNet(conv='GAT', graph_base) from `args.graph`: the combined pattern built in CSR is the dense-built model's."""
    net = networks['astlingen']
    e, n = np.array(net['edges']), net['n_node']
    dense_args = emulator_args(e, n, n_sp_layer=2, graph_base=graph_base, conv_dim=64)
    g_args = SimpleNamespace(**{k: v for k, v in vars(dense_args).items() if k not in ('adj', 'edge_adj', 'node_edge')})
    g_args.graph = U.DrainageGraph.from_edges(e, n)
    md = U.ConvNet(dense_args, 'GAT', generator=torch.Generator().manual_seed(5))
    mg = U.ConvNet(g_args, 'GAT', generator=torch.Generator().manual_seed(5))
    assert _shapes(md) == _shapes(mg)
    assert all(torch.equal(a, b) for a, b in zip(md.state_dict().values(), mg.state_dict().values()))
    assert np.array_equal(md.block.filt.rowptr, mg.block.filt.rowptr) and np.array_equal(md.block.filt.col, mg.block.filt.col)


def test_a_graph_without_raw_matrices_is_refused(networks):
    net = networks['astlingen']
    e, n = np.array(net['edges']), net['n_node']
    g = U.DrainageGraph.from_edges(e, n)
    bare = U.DrainageGraph(g.n_node, g.n_edge, g.edges, g.adj, g.edge_adj, g.inc_n, g.inc_e)
    assert bare.raw_adj is None and bare.raw_edge_adj is None
    args = emulator_args(e, n, conv='GCN')
    args.graph = bare
    with pytest.raises(ValueError, match='from_edges'):
        U.Emulator(args.conv, args.resnet, args.recurrent, args)
    with pytest.raises(ValueError, match='from_dense'):
        U.agent.ConvNet(args, 'Diffusion')
