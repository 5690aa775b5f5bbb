"""fp64 parity of uds_node_edge_wgrad (k_node_edge_wgrad<1 | 2> + k_node_edge_wgrad_reduce), of autograd.NodeEdgeDenseFn on its
own, and of an Emulator that trains its dense-parameter NodeEdge layers through them (Emulator.dense_node_edge_train).
tests/node_edge_wgrad_util.py holds the cases, the Python restatement of the plan and the seeded inputs;
tests/test_node_edge_wgrad_math.py checks on the CPU that the cases reach what they claim.

Every input of the entry is a view inside a NaN-filled allocation; the workspace, d_bias and d_weight are views inside
sentinel-guarded allocations, pre-filled with NaN, checked on both sides and for finiteness (the WHOLE workspace: an element of
a partial the kernel does not write shows).  Plain allocations, valid shapes: nothing here is meant to fault; refusals are
return codes.

Tolerances, relative to max(1, max|ref|) through tests.util.close, the measure always the fp64 reference:
  uds_node_edge_wgrad, d_bias          3e-5 * max(1, sqrt(K / 1000)), K = S * h the reduction length: the weight-gradient bound of
                                       tests/test_gpu_wgrad_wide.py (the same three bf16 products, fp32 sums in a fixed order)
  d_weight                             bitwise d_bias * inci (one fp32 multiply)
  NodeEdgeDenseFn                      out, d xs: 1e-5 (TOL_GEMM / TOL_DXS of tests/test_gpu_remainder_routes.py); d weight, d bias:
                                       the bound above
  the model                            the construction and bounds of tests/test_gpu_train.py: losses 2e-5, every gradient
                                       GRAD_TOL['GAT'] = 1e-3 of the tensor's largest gradient + 1e-7 of the model's largest;
                                       three fit_eval steps rtol 2e-3 / atol 1e-5 on the losses, 3e-4 on the parameters
Every call of the entry is repeated: torch.equal.

MEASURED on an MI355X (UDS_TOL_REPORT=1), worst observed / allowed per test over all its cases [case]:
  test_entry_against_the_fp64_product, d_bias       0.102  [R443-M444-S2-h32]        err 2.91e-5; the long reductions sit lower:
                                                    0.020 [R449-M449-S65-h32], 0.034 [R65-M33-S17-h64]
  test_binding_returns_the_entry_s_results          0.089
  test_node_edge_dense_fn                           out 0.715 [astlingen-h32] (err 1.38e-5 of 1.93e-5), d xs 0.670 [astlingen-h32];
                                                    d weight 0.069, d bias 0.102 [padded-h20]
  test_module_takes_the_route_only_where_it_may     0.017 (flag on against flag off)
  test_emulator_gradients_on_the_dense_route        losses 0.014; gradients 0.086 [embed 64, block1.0.dense_xe.bias], 0.011 [embed 128,
                                                    out.kernel]
  test_fit_eval_steps_on_the_dense_route            worst parameter difference after 3 steps 5.3e-6 of 3e-4
No bound was raised.
"""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import autograd as AG
from gnn_uds_amd.layers import NodeEdge
from oracle import train_ref as OT
from tests import node_edge_wgrad_util as NU
from tests.test_gpu_train import GRAD_TOL, _problem
from tests.util import SENTINEL, Guarded, close, emulator_param_pairs, nan_in

pytestmark = pytest.mark.gpu

TOL_GEMM = TOL_DXS = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_entry(dev, case, g, x, inci):
    """One call of the C entry in guarded memory -> (d_bias, d_weight or None)."""
    R, M, S, h = case
    lib = _lib.load()
    n_ws = lib.uds_node_edge_wgrad_workspace_bytes(R, M, S, h) // 4
    assert n_ws == NU.plan(*case)['pieces'] * R * M > 0
    nan = lambda *shape: torch.full(shape, float('nan'), device=dev)
    ws, db = Guarded((n_ws,), dev, nan(n_ws)), Guarded((R, M), dev, nan(R, M))
    dw = Guarded((R, M), dev, nan(R, M)) if inci is not None else None
    rc = lib.uds_node_edge_wgrad(g.data_ptr(), x.data_ptr(), S, R, M, h, inci.data_ptr() if inci is not None else None, ws.view.data_ptr(),
                                 db.view.data_ptr(), dw.view.data_ptr() if dw else None, _stream())
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    ws.check('workspace')
    db.check('d_bias')
    if dw:
        dw.check('d_weight')
    return db.view, dw.view if dw else None


# ---- the C entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', NU.CASES, ids=NU.case_id)
def test_entry_against_the_fp64_product(dev, case):
    R, M, S, h = case
    p = NU.inputs(case)
    g, x, inci = nan_in(p['g'], dev), nan_in(p['x'], dev), nan_in(p['inci'], dev)
    db, dw = run_entry(dev, case, g, x, inci)
    tol = NU.wtol(S * h)
    err = float((db.double().cpu() - p['ref']).abs().max())
    print('node_edge_wgrad %-22s %s d_bias err %.3e allowed %.3e' % (NU.case_id(case), NU.plan(*case), err, tol * max(1.0, float(p['ref'].abs().max()))))
    close(db, p['ref'], tol)
    assert torch.equal(dw, db * inci)                          # one fp32 multiply per element
    db2, dw2 = run_entry(dev, case, g, x, inci)
    assert torch.equal(db, db2) and torch.equal(dw, dw2)       # no atomics: the same bits
    # without inci and d_weight only d_bias is written, and it is the same d_bias
    db3, none = run_entry(dev, case, g, x, None)
    assert none is None and torch.equal(db, db3)


def test_binding_returns_the_entry_s_results(dev):
    case = NU.CASES[3]
    p = NU.inputs(case)
    g, x, inci = (p[k].float().to(dev) for k in ('g', 'x', 'inci'))
    db, dw = _lib.node_edge_wgrad(g, x, inci)
    close(db, p['ref'], NU.wtol(case[2] * case[3]))
    assert torch.equal(dw, db * inci)
    db1, none = _lib.node_edge_wgrad(g, x)
    assert none is None and torch.equal(db, db1)


def test_zero_snapshots_give_zeros(dev):
    R, M, h = 37, 21, 32
    lib = _lib.load()
    assert lib.uds_node_edge_wgrad_workspace_bytes(R, M, 0, h) == 0
    nan = torch.full((R, M), float('nan'), device=dev)
    db, dw, inci = Guarded((R, M), dev, nan), Guarded((R, M), dev, nan), torch.ones(R, M, device=dev)
    rc = lib.uds_node_edge_wgrad(None, None, 0, R, M, h, inci.data_ptr(), None, db.view.data_ptr(), dw.view.data_ptr(), _stream())
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    db.check('d_bias')
    dw.check('d_weight')
    assert not db.view.any() and not dw.view.any()
    z, zw = _lib.node_edge_wgrad(torch.zeros(0, R, h, device=dev), torch.zeros(0, M, h, device=dev), inci)
    assert not z.any() and not zw.any() and z.shape == (R, M)


@pytest.mark.parametrize('case', NU.REFUSALS, ids=NU.case_id)
def test_refusals_launch_nothing(dev, case):
    R, M, S, h = case
    lib = _lib.load()
    rows, hh = max(R, 1), max(h, 4)
    g, x, inci = torch.zeros(S, rows, hh, device=dev), torch.zeros(S, M, hh, device=dev), torch.ones(rows, M, device=dev)
    nan = torch.full((rows, M), float('nan'), device=dev)
    ws, db, dw = Guarded((4096,), dev), Guarded((rows, M), dev, nan), Guarded((rows, M), dev, nan)
    rc = lib.uds_node_edge_wgrad(g.data_ptr(), x.data_ptr(), S, R, M, h, inci.data_ptr(), ws.view.data_ptr(), db.view.data_ptr(),
                                 dw.view.data_ptr(), _stream())
    assert rc == -22 and lib.uds_last_error().startswith(b'uds_node_edge_wgrad:')
    torch.cuda.synchronize()
    assert bool((ws.buf.view(torch.int32) == SENTINEL).all())
    for t in (db, dw):                                         # the NaN prefill is intact, and so are the guards
        assert bool(torch.isnan(t.view).all())
        bits = t.buf.view(torch.int32)
        assert bool((bits[:1024] == SENTINEL).all()) and bool((bits[1024 + t.n:] == SENTINEL).all())
    if R > 0:
        with pytest.raises(_lib.UdsError):
            _lib.node_edge_wgrad(g, x)


def test_d_weight_without_inci_is_refused(dev):
    lib = _lib.load()
    g, x = torch.zeros(1, 4, 32, device=dev), torch.zeros(1, 5, 32, device=dev)
    nan = torch.full((4, 5), float('nan'), device=dev)
    ws, db, dw = Guarded((64,), dev), Guarded((4, 5), dev, nan), Guarded((4, 5), dev, nan)
    rc = lib.uds_node_edge_wgrad(g.data_ptr(), x.data_ptr(), 1, 4, 5, 32, None, ws.view.data_ptr(), db.view.data_ptr(), dw.view.data_ptr(), _stream())
    assert rc == -22
    torch.cuda.synchronize()
    assert bool(torch.isnan(db.view).all()) and bool(torch.isnan(dw.view).all())


# ---- NodeEdgeDenseFn on its own -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,M,S,h', [(30, 29, 5, 32), (131, 113, 9, 64), (70, 50, 3, 20)], ids=['astlingen-h32', 'shunqing-h64-split', 'padded-h20'])
def test_node_edge_dense_fn(dev, R, M, S, h):
    """out, d weight, d bias and d xs against fp64 autograd of (W o inci + B) @ xs: an incidence with values other than 0 / 1, a
    bias that is non-zero everywhere, a non-contiguous upstream gradient."""
    gen = torch.Generator().manual_seed(R + M + S + h)
    u = lambda *shape: (torch.rand(*shape, generator=gen, dtype=torch.float64) - 0.25).float().double()
    inci = NU.incidence(R, M)
    W, B, xs = u(R, M), u(R, M) * 0.2, u(S, M, h)
    gy = u(S, h, R).transpose(1, 2)                            # (S, R, h), h not contiguous
    assert not gy.is_contiguous()
    Wr, Br, xr = (t.clone().requires_grad_(True) for t in (W, B, xs))
    ref = torch.matmul(Wr * inci + Br, xr)
    (ref * gy).sum().backward()

    mod = NodeEdge(inci.numpy()).to(dev)
    assert torch.equal(mod.dense_incidence().cpu().double(), inci)
    assert '_inci_dense' not in mod.state_dict()
    Wd, Bd, xd = (t.float().to(dev).requires_grad_(True) for t in (W, B, xs))
    out = AG.NodeEdgeDenseFn.apply(Wd, Bd, xd, mod)
    close(out, ref.detach(), TOL_GEMM)
    gyd = gy.float().to(dev)
    assert not gyd.is_contiguous()
    (out * gyd).sum().backward()
    tol = NU.wtol(S * h)
    for name, got, want, t in (('d weight', Wd.grad, Wr.grad, tol), ('d bias', Bd.grad, Br.grad, tol), ('d xs', xd.grad, xr.grad, TOL_DXS)):
        err = float((got.double().cpu() - want).abs().max())
        print('NodeEdgeDenseFn %dx%d S%d h%d %-8s err %.3e allowed %.3e' % (R, M, S, h, name, err, t * max(1.0, float(want.abs().max()))))
        close(got, want, t)
    assert torch.equal(Wd.grad, Bd.grad * mod.dense_incidence())


def test_module_takes_the_route_only_where_it_may(dev):
    R, M, S, h = 30, 29, 3, 32
    inci = NU.incidence(R, M).numpy()
    x = torch.rand(S, M, h, device=dev)

    def run(mod, x=x, **attr):
        mod.to(dev).requires_grad_(True)
        for k, v in attr.items():
            setattr(mod, k, v)
        mod(x).sum().backward()
        return mod.last_train_path

    assert NodeEdge.dense_train is False
    assert run(NodeEdge(inci)) == 'support+remainder'
    assert run(NodeEdge(inci), dense_train=True) == 'dense'
    assert run(NodeEdge(inci, sparse=True), dense_train=True) == 'support+remainder'
    assert run(NodeEdge(inci), dense_train=True, precision='fp32') == 'support+remainder'
    assert run(NodeEdge(inci), x=torch.rand(S, M, 68, device=dev), dense_train=True) == 'support+remainder'      # h above the gate
    frozen = NodeEdge(inci)
    frozen.to(dev).requires_grad_(True)
    frozen.bias.requires_grad_(False)
    frozen.dense_train = True
    frozen(x).sum().backward()
    assert frozen.last_train_path == 'support+remainder'
    # flag on and off give the same layer within the GEMM's bound
    a, b = NodeEdge(inci), NodeEdge(inci)
    b.load_state_dict(a.state_dict())
    run(a), run(b, dense_train=True)
    close(b.weight.grad, a.weight.grad.double().cpu(), NU.wtol(S * h))
    close(b.bias.grad, a.bias.grad.double().cpu(), NU.wtol(S * h))


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _node_edges(emul):
    return [m for m in emul.modules() if isinstance(m, NodeEdge)]


@pytest.mark.parametrize('embed', [64, 128])
def test_emulator_gradients_on_the_dense_route(dev, networks, embed):
    """tests/test_gpu_train.py::test_emulator_gradients with the flag on: a dense-parameter GAT Emulator on astlingen."""
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, embed_size=embed, n_sp_layer=1, n_tp_layer=1)
    assert emul.dense_node_edge_train is False
    emul.dense_node_edge_train = True
    assert all(m.dense_train for m in _node_edges(emul)) and len(_node_edges(emul)) == 4
    x, a, b, y, ex, ey = cpu_in
    ref_losses, ref_grads = OT.grads(args, params, norms, x, a, b, y, ex, ey)
    emul.requires_grad_(True)
    xd, ad, bd, yd, exd, eyd = dev_in
    ae = emul.get_edge_action(ad, True)
    preds, edge_preds = emul._model(xd, ad, bd, exd, ae, None, True)
    assert [m.last_train_path for m in _node_edges(emul)] == ['dense'] * 4
    lw = emul._loss_setup(dev)
    ls = [emul.get_node_loss(yd, bd, preds), emul.get_flood_loss(yd, preds), emul._mse(eyd, edge_preds, lw['ewei'])]
    for got, ref in zip(ls, ref_losses):
        close(got, ref, 2e-5)
    sum(ls).backward()
    gmax = max(float(t.abs().max()) for t in ref_grads.values())
    n_checked, worst = 0, (0.0, '')
    for pname, p, ref in emulator_param_pairs(emul, ref_grads):
        got = p.grad.detach().double().cpu() if p.grad is not None else torch.zeros_like(ref)
        ref = ref.reshape(got.shape)
        scale, err = float(ref.abs().max()), float((got - ref).abs().max())
        worst = max(worst, (err / (GRAD_TOL['GAT'] * scale + 1e-7 * gmax), pname))
        assert err <= GRAD_TOL['GAT'] * scale + 1e-7 * gmax, '%s: grad err %.3e vs max|grad| %.3e' % (pname, err, scale)
        n_checked += 1
    print('embed %d: worst observed / allowed %.3f [%s]' % (embed, worst[0], worst[1]))
    assert n_checked == len(list(emul.parameters()))
    # the flag off again: the existing path
    emul.dense_node_edge_train = False
    emul.zero_grad(set_to_none=True)
    emul._model(xd, ad, bd, exd, ae, None, True)
    assert [m.last_train_path for m in _node_edges(emul)] == ['support+remainder'] * 4


def test_fit_eval_steps_on_the_dense_route(dev, networks):
    """tests/test_gpu_train.py::test_fit_eval_steps_match_oracle_adam with the flag on."""
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, embed_size=64, n_sp_layer=1, learning_rate=1e-3)
    emul.dense_node_edge_train = True
    x, a, b, y, ex, ey = cpu_in
    opt = OT.Adam(lr=1e-3)
    leaves = list(OT.tree_leaves(params))
    ref_hist = []
    for _ in range(3):
        ls, gr = OT.grads(args, params, norms, x, a, b, y, ex, ey)
        ref_hist.append([float(l) for l in ls])
        opt.step(leaves, gr)
    hist = [[float(l) for l in emul.fit_eval(*dev_in)] for _ in range(3)]
    assert all(m.last_train_path == 'dense' for m in _node_edges(emul))
    for h, r in zip(hist, ref_hist):
        assert np.allclose(h, r, rtol=2e-3, atol=1e-5), (hist, ref_hist)
    worst = 0.0
    for pname, p, ref in emulator_param_pairs(emul, dict(OT.tree_leaves(params))):
        err = float((p.detach().double().cpu() - ref).abs().max())
        worst = max(worst, err)
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)
    print('fit_eval x 3: worst parameter difference %.3e of 3e-4' % worst)


@pytest.mark.parametrize('over', [dict(precision='fp32'), dict(sparse=True)], ids=['fp32', 'sparse'])
def test_flag_leaves_fp32_and_sparse_models_on_the_existing_path(dev, networks, over):
    net = networks['astlingen']
    from tests.util import emulator_args, emulator_norms
    args = emulator_args(np.array(net['edges']), net['n_node'], n_sp_layer=1, n_tp_layer=1)
    if over.get('sparse'):
        args.sparse_params = True
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, precision=over.get('precision', 'bf16x3')).to(dev)
    if over.get('sparse'):
        assert all(m.sparse for m in _node_edges(emul))
    norms = emulator_norms(args)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    emul.dense_node_edge_train = True
    emul.requires_grad_(True)
    g = torch.Generator().manual_seed(5)
    n, e, T = net['n_node'], len(net['edges']), args.seq_in
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    x, b, ex, a = r(2, T, n, 5), r(2, T, n, 1) * 0.1, r(2, T, e, 4), r(2, T, 2)
    ae = emul.get_edge_action(a, True)
    preds, edge_preds = emul._model(x, a, b, ex, ae, None, True)
    (preds.sum() + edge_preds.sum()).backward()
    assert [m.last_train_path for m in _node_edges(emul)] == ['support+remainder'] * 4
