"""GCN and Diffusion models built from a CSR graph (`args.graph`), and the table-free DiffusionConv kernels
(uds_diffusion_forward_m / uds_diffusion_backward_m), on the GPU against the fp64 CPU references.

Entries: guarded outputs, NaN-surrounded inputs, against the collapsed formulas of tests/test_diffusion_grad_math.py.  Layer and
models: autograd of the fp64 oracle fed the DENSE matrices, while the device model sees the CSR graph only.

Bounds (all existing ones, relative to max(1, max|reference|) unless said otherwise):
  operator forward / dr 5e-6, dtheta 2e-6                     tests/test_gpu_diffusion_train.py
  at size (N = 50 000, C = 128, S = 4)  out 5e-6, dr 2e-6, dkernel 5e-6      its at-size bounds
  whole forward / predict_tf  TOL_FWD['bf16x3'] = 2e-5 at the default precision, TOL_FWD['fp32'] = 5e-6 at precision='fp32'      tests/test_gpu_emulator.py
  whole-model gradients  GRAD_TOL['GCN'] = 5e-3 / DIFF_GRAD_TOL = 2e-3 of the tensor's largest gradient + 1e-7 of the largest of all
  GCN conv at size: 5e-6, the exact-fp32 operator bound
Networks: the forward / predict_tf and the gradient tests run astlingen and hague; the fit_eval, MPC, graph_base and ConvNet tests
run astlingen (30 nodes: seconds each), as the existing tests they restate do.
Worst observed / allowed on an MI355X (UDS_TOL_REPORT=1; also DESIGN.md 7.0b):
  test_entries_against_the_collapsed_formulas   forward 0.013, dr 0.004, dtheta 0.158 (thick, C = 4)
  test_moment_layer_under_autograd              0.071 (astlingen-node, C = 64, dkernel)
  test_moment_layer_at_size                     out 0.021, dr 0.086, dkernel 0.103
  test_emulator_forward_and_predict_tf          0.556 (default precision, one layer per block: hague Diffusion, link outputs); 0.38 (precision='fp32', two layers: hague
                                                Diffusion, link outputs)
  test_emulator_gradients                       0.364 (hague Diffusion, embed_e.kernel)
  test_mpc_objective_and_gradient_on_the_diffusion_model 0.279; test_graph_base_diffusion_from_the_graph 0.278
  test_gcn_spatial_layer_at_size                0.042
"""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd.graph import CSR, csr_from_dense
from oracle import emulator_ref as OE
from oracle import graphs as OG
from oracle import spektral_dense as OD
from oracle import train_ref as OT
from tests import test_gpu_convnet_train as CT
from tests.test_csr_conv_math import FILTERS, problem
from tests.test_diffusion_grad_math import collapsed_forward, collapsed_grads, nonsymmetric_filter
from tests.test_gpu_diffusion_train import DIFF_GRAD_TOL, THETA_SCALE
from tests.test_gpu_emulator import OUTLIERS_ALLOWED, TOL_FWD
from tests.test_gpu_train import GRAD_TOL
from tests.util import (OBSERVED, PAD, SENTINEL, Guarded, close, emulator_args, emulator_norms, emulator_param_pairs, ladder_rect, load_emulator,
                        nan_in)

pytestmark = pytest.mark.gpu
TOL = {'GCN': GRAD_TOL['GCN'], 'Diffusion': DIFF_GRAD_TOL}
ACTS = ('tanh', 'relu', 'linear', 'sigmoid')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def pats():
    return {k: (FILTERS[k](), ) for k in ('ladder', 'thick', 'nonsym')}


def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def f32(t, dev):
    return torch.as_tensor(np.asarray(t), dtype=torch.float32).to(dev).contiguous()


def entry_forward(h, a, theta, r, act, dev):
    S, C = r.shape[0], theta.shape[0]
    out = Guarded((S, h.n_rows, C), dev)
    rd = nan_in(f32(r, dev), dev)
    got = _lib.diffusion_forward_m(h, nan_in(f32(a, dev), dev), nan_in(f32(theta, dev), dev), rd, nan_in(rd.sum(-1), dev), act, out=out.view)
    torch.cuda.synchronize()
    out.check('out')
    return got


def entry_backward(h, a, theta, r, y, gy, act, dev):
    S, (C, K1) = r.shape[0], theta.shape
    dr, dth = Guarded((S, h.n_cols), dev), Guarded((C, K1), dev)
    nws = int(_lib.load().uds_diffusion_backward_m_workspace_floats(h.n_rows, S, C, K1))
    ws = Guarded((max(nws, 4),), dev, torch.full((max(nws, 4),), float('nan')))
    rd = nan_in(f32(r, dev), dev)
    _lib.diffusion_backward_m(h, nan_in(f32(a, dev), dev), nan_in(f32(theta, dev), dev), rd, nan_in(rd.sum(-1), dev), nan_in(y, dev),
                              nan_in(f32(gy, dev), dev), act, out=(dr.view, dth.view), workspace=ws.view)
    torch.cuda.synchronize()
    dr.check('dr'), dth.check('dtheta')
    bits = ws.buf.view(torch.int32)
    assert bool((bits[:PAD] == SENTINEL).all()) and bool((bits[PAD + ws.n:] == SENTINEL).all()), 'workspace overrun'      # (its up4 padding stays NaN: no Guarded.check)
    return dr.view, dth.view


# ---- the two entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 8, 12, 64, 128, 256])
@pytest.mark.parametrize('pattern', ['ladder', 'thick', 'nonsym'])
def test_entries_against_the_collapsed_formulas(dev, pats, pattern, C):
    """Both entries at every K1 in {1, 2, 7, 16}, S in {1, 3} and activation; dtheta bit-equal to the table entry's (the row
    pass and the reduction are shared)."""
    csr = pats[pattern][0]
    h = _lib.CsrHandle(csr)
    rowptr, col = csr.rowptr.astype(np.int64), csr.col.astype(np.int64)
    worst = [0.0, 0.0, 0.0]
    for K1 in (1, 2, 7, 16):
        for S in (1, 3):
            theta, r, gy = problem(csr, C, K1, S, seed=C + K1 + S)
            for act in ACTS:
                y_ref = collapsed_forward(rowptr, col, csr.val, theta, r, act)
                y = entry_forward(h, csr.val, theta, r, act, dev)
                e0 = close(y, torch.from_numpy(y_ref), 5e-6)
                dr_ref, dth_ref = collapsed_grads(rowptr, col, csr.val, theta, r, y.double().cpu().numpy(), gy, act)
                dr, dth = entry_backward(h, csr.val, theta, r, y, gy, act, dev)
                e1 = close(dr, torch.from_numpy(dr_ref), 5e-6)
                e2 = close(dth, torch.from_numpy(dth_ref), 2e-6)
                if K1 > 1 and S == 3:
                    assert np.abs(dth_ref).max() > 1e-3
                sc = lambda ref: max(1.0, float(np.abs(ref).max()))
                worst = [max(w, e / (t * sc(ref))) for w, e, t, ref in zip(worst, (e0, e1, e2), (5e-6, 5e-6, 2e-6), (y_ref, dr_ref, dth_ref))]
                if act == 'tanh':          # the table entry on the same inputs: the shared launches give the same dtheta bits
                    th = torch.from_numpy(theta)
                    av = torch.from_numpy(csr.val)[:, None]
                    v = th[:, 0].expand(av.shape[0], -1)
                    for k in range(1, K1):
                        v = v * av + th[:, k]
                    vals, c0 = (v - th[:, -1]).float().contiguous().to(dev), th[:, -1].float().contiguous().to(dev)
                    rd = f32(r, dev)
                    _, dth_t = _lib.diffusion_backward(h, f32(csr.val, dev), vals, c0, rd, rd.sum(-1), y.contiguous(), f32(gy, dev), K1, act)
                    assert torch.equal(dth_t, dth)
    print('%s C=%d: worst / allowed forward %.3f dr %.3f dtheta %.3f' % (pattern, C, *worst))


@pytest.mark.parametrize('C,K1', [(12, 7), (64, 7), (128, 16)])
def test_batch_is_its_snapshots_and_backward_is_repeatable(dev, pats, C, K1):
    csr = pats['ladder'][0]
    h = _lib.CsrHandle(csr)
    theta, r, gy = problem(csr, C, K1, 3, seed=3)
    y = entry_forward(h, csr.val, theta, r, 'tanh', dev).clone()
    dr, dth = (t.clone() for t in entry_backward(h, csr.val, theta, r, y, gy, 'tanh', dev))
    dr2, dth2 = entry_backward(h, csr.val, theta, r, y, gy, 'tanh', dev)
    assert torch.equal(dr, dr2) and torch.equal(dth, dth2)
    for s in range(3):
        ys = entry_forward(h, csr.val, theta, r[s:s + 1], 'tanh', dev)
        assert torch.equal(ys[0], y[s])
        drs, _ = entry_backward(h, csr.val, theta, r[s:s + 1], ys, gy[s:s + 1], 'tanh', dev)
        assert torch.equal(drs[0], dr[s])


def test_refusals_are_uds_errors(dev, pats):
    csr = pats['ladder'][0]
    h = _lib.CsrHandle(csr)
    a = f32(csr.val, dev)
    r = torch.rand(2, csr.n_cols, device=dev)
    tot = r.sum(-1)
    for C, K1 in ((6, 7), (8, 17), (260, 7), (8, 0)):
        theta = torch.zeros(C, K1, device=dev)
        with pytest.raises(_lib.UdsError):
            _lib.diffusion_forward_m(h, a, theta, r, tot)
        y = torch.zeros(2, csr.n_rows, C, device=dev)
        with pytest.raises(_lib.UdsError):
            _lib.diffusion_backward_m(h, a, theta, r, tot, y, y)
    # a csr_t that is not the transpose (67 x 41 against a 67 x 67 pattern): the C entry itself refuses
    lib, C, K1 = _lib.load(), 8, 7
    wrong = _lib.CsrHandle(ladder_rect())
    theta, y = torch.zeros(C, K1, device=dev), torch.zeros(2, csr.n_rows, C, device=dev)
    _, perm = h.transposed(dev)
    ws = torch.empty(int(lib.uds_diffusion_backward_m_workspace_floats(csr.n_rows, 2, C, K1)), device=dev)
    dr, dth = torch.empty(2, csr.n_cols, device=dev), torch.empty(C, K1, device=dev)
    with pytest.raises(_lib.UdsError, match='transpose'):
        _lib._check(lib.uds_diffusion_backward_m(h.ptr, wrong.ptr, perm.data_ptr(), a.data_ptr(), theta.data_ptr(), r.data_ptr(), tot.data_ptr(),
                                                 y.data_ptr(), y.data_ptr(), 2, C, K1, 2, ws.data_ptr(), dr.data_ptr(), dth.data_ptr(),
                                                 _lib._stream()), 'uds_diffusion_backward_m')
    with pytest.raises(ValueError, match='values'):
        U.GCNConv(8, in_channels=4).to(dev)([torch.zeros(1, csr.n_rows, 4, device=dev), CSR(csr.rowptr, csr.col, csr.n_rows, csr.n_cols)])


# ---- the layer ------------------------------------------------------------------------------------------------------------------
def _filter(networks, which):
    if which == 'nonsym':
        return nonsymmetric_filter(40, seed=5)
    name, kind = which.split('-')
    edges = np.array(networks[name]['edges'])
    adj = {'node': lambda: OG.adjacency(edges), 'link': lambda: OG.edge_adjacency(edges), 'base': lambda: OG.node_based_adjacency(edges)}[kind]()
    return U.DiffusionConv.preprocess(adj)


@pytest.mark.parametrize('C', [16, 64])
@pytest.mark.parametrize('which', ['astlingen-node', 'astlingen-link', 'astlingen-base', 'nonsym'])
def test_moment_layer_under_autograd(dev, networks, which, C):
    """tests/test_gpu_diffusion_train.py::test_operator_gradients for DiffusionConv(moments=True) on a CSR filter."""
    ah = _filter(networks, which)
    filt = csr_from_dense(ah, keep_values=True)
    for act in ACTS:
        g = torch.Generator().manual_seed(C + len(which))
        S, N, F = 3, ah.shape[0], 6
        layer = U.DiffusionConv(C, activation=act, generator=g, moments=True).to(dev).requires_grad_(True)
        with torch.no_grad():
            layer.kernel.mul_(THETA_SCALE)
        x, gy = rnd(g, S, N, F), rnd(g, S, N, C) - 0.5
        xr, kr = x.clone().requires_grad_(True), layer.kernel.detach().double().cpu().requires_grad_(True)
        ref = OD.diffusion_conv_dense(xr, torch.from_numpy(ah), kr, act)
        (ref * gy).sum().backward()
        if act in ('tanh', 'sigmoid'):
            lo, hi = (-0.9, 0.9) if act == 'tanh' else (0.1, 0.9)
            assert float(((ref > lo) & (ref < hi)).double().mean()) > 0.9
        xd = x.float().to(dev).requires_grad_(True)
        with torch.no_grad():
            y0 = layer([xd.detach(), filt])
        out = layer([xd, filt])
        assert torch.equal(out.detach(), y0) and layer._packs.peek('table') is None          # no table was built
        close(out, ref.detach(), 5e-6)
        (out * gy.float().to(dev)).sum().backward()
        close(xd.grad, xr.grad, 5e-6)
        close(layer.kernel.grad, kr.grad, 2e-6)
        assert float(kr.grad.abs().max()) > 1e-3


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _shrink(params):
    for blk in ('block1', 'block2'):
        for q in params[blk]:
            for conv in (q['gat'],) if 'gat' in q else (q['gat_x'], q['gat_e']):
                if 'theta' in conv:
                    conv['theta'] *= THETA_SCALE
    return params


def graph_args(args):
    """The same args without any dense matrix: `graph` instead of adj / edge_adj / node_edge."""
    g = SimpleNamespace(**{k: v for k, v in vars(args).items() if k not in ('adj', 'edge_adj', 'node_edge')})
    g.graph = U.DrainageGraph.from_edges(np.asarray(args.edges), args.state_shape[0])
    return g


def _problem(networks, name, conv, dev, seed=3, B=2, build=True, precision='bf16x3', **over):
    net = networks[name]
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, conv=conv, **over)                       # dense: what the oracle reads
    norms = emulator_norms(args)
    params = _shrink(OE.init_params(args, seed=1))
    c = OE.config(args)
    g = torch.Generator().manual_seed(seed)
    T_out = c.seq_out * max(c.roll, 1)
    x, b, ex = rnd(g, B, c.seq_in, n, c.n_in), rnd(g, B, T_out, n, c.b_in) * 0.1, rnd(g, B, c.seq_in, len(edges), c.e_in)
    a = rnd(g, B, T_out, len(args.act_edges)) if c.act else None
    y = rnd(g, B, T_out, n, 5)
    y[..., -2] = (y[..., -2] > 0.7).double()
    ey = rnd(g, B, T_out, len(edges), 3)
    emul = None
    if build:
        ga = graph_args(args)
        emul = U.Emulator(ga.conv, ga.resnet, ga.recurrent, ga, precision=precision)      # CSR: what the device model reads
        assert emul.filter is None or isinstance(emul.filter, CSR)
        load_emulator(emul, params, dev)
        emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    t32 = lambda t: None if t is None else t.float().to(dev)
    return args, norms, params, emul, (x, a, b, y, ex, ey), tuple(t32(t) for t in (x, a, b, y, ex, ey))


def _pairs(emul, flat):
    return emulator_param_pairs(emul, {(k[:-len('theta')] + 'kernel' if k.endswith('.theta') else k): v for k, v in flat.items()})


def _outliers(out, ref, tol):
    d = (out.double().cpu() - ref).abs()
    return int((d > tol * max(1.0, float(ref.abs().max()))).sum())


@pytest.mark.parametrize('precision,layers', [('bf16x3', 1), ('fp32', 2)])
@pytest.mark.parametrize('conv', ['GCN', 'Diffusion'])
@pytest.mark.parametrize('name', ['astlingen', 'hague'])
def test_emulator_forward_and_predict_tf(dev, networks, name, conv, precision, layers):
    """The two-graph model built from the graph: network outputs and predict_tf against the oracle fed the dense matrices.
    Default precision (split-bf16 Dense / Conv1D layers), one spatial layer per block as the existing Diffusion model tests run,
    at TOL_FWD['bf16x3']; and two layers per block at precision='fp32' at TOL_FWD['fp32'] = 5e-6: what a graph-built model adds
    to a dense-built one -- the filters normalised on the CSR pattern, csr_spmm on them, the table-free Diffusion kernels -- is
    exact fp32, so there the whole forward is held to the exact-fp32 bound."""
    tol = TOL_FWD[precision]
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, name, conv, dev, n_sp_layer=layers, precision=precision)
    x, a, b, y, ex, ey = cpu_in
    xd, ad, bd, yd, exd, eyd = dev_in
    c = OE.config(args)
    ry, rey = OE.forward(args, params, x, b, ex, OE.get_edge_action(c, a))
    with torch.no_grad():
        oy, oey = emul(xd, bd, exd, emul.get_edge_action(ad))
        py, pey = emul.predict_tf(xd, bd, ad, exd)
    close(oy, ry, tol)
    close(oey, rey, tol)
    qy, qey = OE.predict(args, params, norms, x, b, a, ex)
    assert tuple(py.shape) == tuple(qy.shape)
    assert _outliers(py, qy, tol) <= OUTLIERS_ALLOWED and _outliers(pey, qey, tol) <= OUTLIERS_ALLOWED
    if conv == 'Diffusion':
        assert all(m.moments and m._packs.peek('table') is None for m in emul.modules() if isinstance(m, U.DiffusionConv))


def reference_moves_by(args, params, norms, cpu_in, tol, rel=1e-6, probes=2):
    """tests/test_gpu_gat_heads_model.py's pre-check in units of THIS conv's bound: how far the fp64 reference gradients move when
    every parameter is perturbed by `rel` relative Gaussian noise.  Oracle only."""
    x, a, b, y, ex, ey = cpu_in
    _, g0 = OT.grads(args, params, norms, x, a, b, y, ex, ey)
    gmax = max(float(t.abs().max()) for t in g0.values())
    worst = 0.0
    for k in range(probes):
        gn = torch.Generator().manual_seed(k)
        q = copy.deepcopy(params)
        for _, t in OT.tree_leaves(q):
            t.data = t.data * (1 + rel * torch.randn(t.shape, generator=gn, dtype=torch.float64))
        _, g1 = OT.grads(args, q, norms, x, a, b, y, ex, ey)
        worst = max(worst, max(float((g0[n] - g1[n]).abs().max()) / (tol * float(g0[n].abs().max()) + 1e-7 * gmax) for n in g0))
    return worst


# seed of the input draw per case: the first from 3 upwards whose fp64 reference gradients move by less than a tenth of the bound
# under 1e-6 relative parameter noise (a property of the reference alone, asserted before anything is compared).  Measured on
# the CPU: astlingen GCN 0.001, Diffusion 0.008; hague GCN 0.023; hague Diffusion 0.61 at seed 3 (a relu kink), 0.051 at seed 4
GRAD_SEEDS = {('astlingen', 'GCN'): 3, ('astlingen', 'Diffusion'): 3, ('hague', 'GCN'): 3, ('hague', 'Diffusion'): 4}


@pytest.mark.parametrize('name,conv', sorted(GRAD_SEEDS))
def test_emulator_gradients(dev, networks, name, conv):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, name, conv, dev, seed=GRAD_SEEDS[name, conv], n_sp_layer=1)
    x, a, b, y, ex, ey = cpu_in
    assert reference_moves_by(args, params, norms, cpu_in, TOL[conv]) < 0.1
    ref_losses, ref_grads = OT.grads(args, params, norms, x, a, b, y, ex, ey)
    emul.requires_grad_(True)
    xd, ad, bd, yd, exd, eyd = dev_in
    ae = emul.get_edge_action(ad, True) if emul.act else None
    preds, edge_preds = emul._model(xd, ad, bd, exd, ae, None, True)
    lw = emul._loss_setup(dev)
    ls = [emul.get_node_loss(yd, bd, preds)] + ([emul.get_flood_loss(yd, preds)] if emul.if_flood else []) + [emul._mse(eyd, edge_preds, lw['ewei'])]
    for got, ref in zip(ls, ref_losses):
        close(got, ref, 2e-5)
    sum(ls).backward()
    gmax = max(float(t.abs().max()) for t in ref_grads.values())
    n_checked = 0
    for pname, p, ref in _pairs(emul, ref_grads):
        got = p.grad.detach().double().cpu() if p.grad is not None else torch.zeros_like(ref)
        assert got.numel() == ref.numel()
        ref = ref.reshape(got.shape)
        scale, err = float(ref.abs().max()), float((got - ref).abs().max())
        if os.environ.get('UDS_TOL_REPORT'):
            OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0] + ':' + pname, 0, err, TOL[conv] * scale + 1e-7 * gmax))
        assert err <= TOL[conv] * scale + 1e-7 * gmax, '%s: grad err %.3e vs max|grad| %.3e' % (pname, err, scale)
        n_checked += 1
    assert n_checked == len(list(emul.parameters()))


@pytest.mark.parametrize('conv', ['GCN', 'Diffusion'])
def test_fit_eval_steps_match_oracle_adam(dev, networks, conv):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', conv, dev, embed_size=64, n_sp_layer=1, learning_rate=1e-3)
    x, a, b, y, ex, ey = cpu_in
    opt = OT.Adam(lr=1e-3)
    leaves = list(OT.tree_leaves(params))
    ref_hist = []
    for _ in range(3):
        ls, gr = OT.grads(args, params, norms, x, a, b, y, ex, ey)
        ref_hist.append([float(l) for l in ls])
        opt.step(leaves, gr)
    hist = [[float(l) for l in emul.fit_eval(*dev_in)] for _ in range(3)]
    for h, r in zip(hist, ref_hist):
        assert np.allclose(h, r, rtol=2e-3, atol=1e-5), (hist, ref_hist)
    for pname, p, ref in _pairs(emul, dict(OT.tree_leaves(params))):
        err = float((p.detach().double().cpu() - ref.reshape(p.shape)).abs().max())
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)


def test_mpc_objective_and_gradient_on_the_diffusion_model(dev, networks):
    """tests/test_gpu_diffusion_train.py::test_mpc_objective_and_gradient with the model built from the graph."""
    from gnn_uds_amd import mpc as M
    net = networks['astlingen']
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, conv='Diffusion', seq_in=4, seq_out=2, n_sp_layer=1, if_flood=1, epsilon=0.0)
    norms = emulator_norms(args)
    params = _shrink(OE.init_params(args, seed=3))
    c = OE.config(args)
    g = torch.Generator().manual_seed(11)
    T, n_step = c.seq_out, 1
    state, runoff, edge_state = rnd(g, c.seq_in, n, 5), rnd(g, T, n, 1) * 0.05, rnd(g, c.seq_in, len(edges), 4)
    state[..., 3] = (state[..., 3] > 0.8).double()
    pop, n_act, r_step = 3, len(args.act_edges), 2
    y = 0.2 + 0.6 * rnd(g, pop, n_step * n_act)
    tg = dict(flood_idx=torch.tensor([3, 7, 11]), flood_w=torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64),
              outflow_idx=torch.tensor([0]), outflow_w=torch.tensor([0.3], dtype=torch.float64),
              smooth_idx=torch.tensor([5, 9]), smooth_w=torch.tensor([0.7, 0.2], dtype=torch.float64))
    gamma = torch.tensor([1.0, 0.9][:T], dtype=torch.float64)
    yy = y.clone().requires_grad_(True)
    ref = OE.mpc_objective(args, params, norms, yy, state, runoff, edge_state, n_step, n_act, r_step, tg, gamma)
    gref = torch.autograd.grad(ref.sum(), yy)[0]
    ga = graph_args(args)
    emul = load_emulator(U.Emulator(ga.conv, ga.resnet, ga.recurrent, ga), params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    f = lambda t: t.float().to(dev)
    tgd = {k: (v.to(dev) if v.dtype == torch.int64 else f(v)) for k, v in tg.items()}
    obj, grad = M.objective_and_gradient(emul, f(y), f(state), f(runoff), f(edge_state), n_step, n_act, r_step, tgd, f(gamma))
    close(obj, ref.detach(), 2e-5)
    gmax = float(gref.abs().max())
    assert gmax > 0
    err = float((grad.double().cpu() - gref).abs().max())
    assert err <= 2e-3 * gmax, 'gradient err %.3e vs max|grad| %.3e' % (err, gmax)


@pytest.mark.parametrize('graph_base', [0, 1])
def test_gcn_from_the_graph_is_bit_equal_to_the_dense_built_model(dev, networks, graph_base):
    net = networks['astlingen']
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, conv='GCN', n_sp_layer=2, graph_base=graph_base)
    ga = graph_args(args)
    md = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(5)).to(dev)
    mg = U.Emulator(ga.conv, ga.resnet, ga.recurrent, ga, generator=torch.Generator().manual_seed(5)).to(dev)
    norms = emulator_norms(args)
    for m in (md, mg):
        m.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    g = torch.Generator().manual_seed(2)
    c = OE.config(args)
    x, b, ex = rnd(g, 2, c.seq_in, n, c.n_in), rnd(g, 2, c.seq_out, n, c.b_in) * 0.1, rnd(g, 2, c.seq_in, len(edges), c.e_in)
    a = rnd(g, 2, c.seq_out, len(args.act_edges))
    f = lambda t: t.float().to(dev)
    with torch.no_grad():
        yd, eyd = md(f(x), f(b), f(ex), md.get_edge_action(f(a)))
        yg, eyg = mg(f(x), f(b), f(ex), mg.get_edge_action(f(a)))
    assert torch.equal(yd, yg) and torch.equal(eyd, eyg) and bool(torch.isfinite(yg).all()) and float(yg.abs().max()) > 0


def test_graph_base_diffusion_from_the_graph(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', 'Diffusion', dev, graph_base=1, n_sp_layer=1)
    assert isinstance(emul._base_filter, CSR) and all(m.moments for m in emul.block1.layers)
    x, a, b, y, ex, ey = cpu_in
    xd, ad, bd, yd, exd, eyd = dev_in
    c = OE.config(args)
    ry, rey = OE.forward(args, params, x, b, ex, OE.get_edge_action(c, a))
    with torch.no_grad():
        oy, oey = emul(xd, bd, exd, emul.get_edge_action(ad))
    close(oy, ry, TOL_FWD['bf16x3']); close(oey, rey, TOL_FWD['bf16x3'])


@pytest.mark.parametrize('conv,graph_base', [('GCN', 0), ('Diffusion', 0), ('Diffusion', 1)])
def test_convnet_from_the_graph_gradients(dev, networks, conv, graph_base):
    """tests/test_gpu_convnet_train.py::test_convnet_gradients with the encoder built from `args.graph` (its seed 7, whose
    reference stability is asserted first)."""
    tol = TOL[conv]
    args, params, X, E, W = CT.problem(networks, 'astlingen', conv, 1, graph_base, 7)
    m = U.ConvNet(graph_args(args), conv).to(dev)
    pairs = CT.load(m, params, conv, dev)
    names = sorted(pairs) + ['X', 'E']
    assert CT.reference_moves_by(args, params, X, E, W, tol, names) < 0.1
    ref_out, ref = CT.reference_grads(args, params, X, E, W)
    m.requires_grad_(True)
    Xd, Ed = X.float().to(dev).requires_grad_(True), E.float().to(dev).requires_grad_(True)
    out = m(Xd, Ed)
    close(out, ref_out, TOL_FWD['bf16x3'])
    (out * W.float().to(dev)).sum().backward()
    got = {k: p.grad for k, p in pairs.items()}
    got.update(X=Xd.grad, E=Ed.grad)
    gmax = max(float(ref[k].abs().max()) for k in names)
    for k in names:
        assert got[k] is not None, k
        gk = got[k].detach().double().cpu()
        rk = ref[k].reshape(gk.shape)
        err, lim = float((gk - rk).abs().max()), CT.bound(tol, rk, gmax)
        if os.environ.get('UDS_TOL_REPORT'):
            OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0] + ':' + k, 0, err, lim))
        assert err <= lim, '%s: grad err %.3e vs max|grad| %.3e (bound %.3e)' % (k, err, float(rk.abs().max()), lim)


@pytest.mark.parametrize('conv', ['GCN', 'GAT'])
def test_convnet_graph_base_from_the_graph_is_bit_equal(dev, networks, conv):
    """The oracle's graph_base encoder restates GAT only: the GCN one from the graph against the dense-built model, bit for bit;
    and the GAT one, whose combined pattern `args.graph` now builds in CSR too (it used to need the dense `args.adj`)."""
    args = CT.problem(networks, 'astlingen', conv, 1, 1, 7)[0]
    md = U.ConvNet(args, conv, generator=torch.Generator().manual_seed(3)).to(dev)
    mg = U.ConvNet(graph_args(args), conv, generator=torch.Generator().manual_seed(3)).to(dev)
    g = torch.Generator().manual_seed(4)
    X, E = torch.rand(6, args.state_shape[0], 4, generator=g).to(dev), torch.rand(6, args.edge_state_shape[0], 3, generator=g).to(dev)
    with torch.no_grad():
        out = mg(X, E)
        assert torch.equal(md(X, E), out) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


# ---- at size --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    return U.DrainageGraph.from_edges(U.synthetic_drainage_network(50000, 65000, 0))


def _collapsed_forward_rows(rowptr, col, aval, theta, r, act):
    """collapsed_forward for a pattern without empty rows: the row sums by np.add.reduceat (np.add.at takes seconds here)."""
    from tests.test_diffusion_grad_math import _support, act_from_pre
    _, v = _support(rowptr, col, aval, theta)
    assert (np.diff(rowptr) > 0).all()
    z = np.stack([np.add.reduceat(v * r[s, col][:, None], rowptr[:-1], axis=0) + theta[:, -1] * r[s].sum() for s in range(r.shape[0])])
    return act_from_pre(z, act)


def test_moment_layer_at_size(dev, big):
    """N = 50 000, C = 128, S = 4 (BASELINE C3's node graph): forward, dr and dkernel against the collapsed fp64 formulas, and
    the memory an inference forward takes: less than the (nnz, C) table alone."""
    ah = U.DiffusionConv.preprocess(big.raw_adj)
    g = torch.Generator().manual_seed(4)
    S, F, C = 4, 8, 128
    layer = U.DiffusionConv(C, generator=g, moments=True).to(dev).requires_grad_(True)
    with torch.no_grad():
        layer.kernel.mul_(THETA_SCALE)
    x, gy = rnd(g, S, big.n_node, F) - 0.5, rnd(g, S, big.n_node, C) - 0.5
    r = x.float().sum(-1).double().numpy()       # the fp32 feature sums the layer uses: this check isolates the sparse part
    theta = layer.kernel.detach().double().cpu().numpy()
    rowptr, col, aval = ah.rowptr.astype(np.int64), ah.col.astype(np.int64), ah.val.astype(np.float32).astype(np.float64)
    small = FILTERS['ladder']()
    th8, r8, _ = problem(small, 8, 7, 2, seed=1)
    sp = (small.rowptr.astype(np.int64), small.col.astype(np.int64), small.val)
    assert np.abs(_collapsed_forward_rows(*sp, th8, r8, 'tanh') - collapsed_forward(*sp, th8, r8, 'tanh')).max() < 1e-14
    y = _collapsed_forward_rows(rowptr, col, aval, theta, r, 'tanh')
    assert float(np.mean(np.abs(y) < 0.9)) > 0.9
    dr, dtheta = collapsed_grads(rowptr, col, aval, theta, r, y, gy.numpy(), 'tanh')
    xd = x.float().to(dev).requires_grad_(True)
    out = layer([xd, ah])
    close(out, torch.from_numpy(y), 5e-6)
    (out * gy.float().to(dev)).sum().backward()
    assert torch.isfinite(xd.grad).all() and torch.isfinite(layer.kernel.grad).all()
    close(xd.grad[..., 0], torch.from_numpy(dr), 2e-6)
    close(layer.kernel.grad, torch.from_numpy(dtheta), 5e-6)
    assert float(np.abs(dtheta).max()) > 1e-3
    del out, xd
    x1 = x[:1].float().to(dev)
    with torch.no_grad():
        layer([x1, ah])                                    # handle, support values: resident before the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        y1 = layer([x1, ah])
        torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print('inference forward at S = 1: %d bytes, the table alone %d' % (grew, ah.nnz * C * 4))
    assert y1.shape == (1, big.n_node, C) and grew < ah.nnz * C * 4 and layer._packs.peek('table') is None


def test_gcn_spatial_layer_at_size(dev, big):
    """A GCN SpatialLayer from CSR filters at N = 50 000 / E = 65 000, S = 2: finite, repeatable, snapshot-independent, and
    sampled rows of both convs against an fp64 CSR evaluation from the layer's own fp32 inputs."""
    d = 64
    filters = (U.GCNConv.preprocess(big.raw_adj), U.GCNConv.preprocess(big.raw_edge_adj))
    layer = U.SpatialLayer(big, d, 'relu', conv='GCN', filters=filters, generator=torch.Generator().manual_seed(1)).to(dev)
    assert layer.node_edge_n.sparse
    g = torch.Generator().manual_seed(2)
    x1, e1 = torch.rand(1, big.n_node, d, generator=g) - 0.5, torch.rand(1, big.n_edge, d, generator=g) - 0.5
    x, e = torch.cat([x1, x1]).to(dev), torch.cat([e1, e1]).to(dev)
    with torch.no_grad():
        ox, oe = layer(x, e)
        ox2, oe2 = layer(x, e)
        cx = torch.cat([x, layer.node_edge_n(layer.dense_xe(e))], dim=-1)
        ce = torch.cat([e, layer.node_edge_e(layer.dense_ex(x))], dim=-1)
    assert torch.equal(ox, ox2) and torch.equal(oe, oe2) and torch.equal(ox[0], ox[1]) and torch.equal(oe[0], oe[1])
    assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oe).all()) and float(ox.abs().max()) > 0 and float(oe.abs().max()) > 0
    rng = np.random.default_rng(0)
    for out, cat, filt, conv in ((ox, cx, filters[0], layer.gcn_x), (oe, ce, filters[1], layer.gcn_e)):
        rows = np.concatenate([[0, filt.n_rows - 1], rng.choice(filt.n_rows, 200, replace=False)])
        hx = cat[0].double().cpu() @ conv.kernel.detach().double().cpu()
        val32 = torch.from_numpy(filt.val.astype(np.float32).astype(np.float64))
        ref = torch.stack([(val32[filt.rowptr[i]:filt.rowptr[i + 1], None] * hx[filt.col[filt.rowptr[i]:filt.rowptr[i + 1]].astype(np.int64)]).sum(0)
                           for i in rows]) + conv.bias.detach().double().cpu()
        close(out[0][torch.from_numpy(rows).to(dev)], torch.relu(ref), 5e-6)
