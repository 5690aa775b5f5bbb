"""The predict tail as one HIP operator (uds_predict_tail / uds_predict_tail_backward, autograd.PredictTailFn) and the route
`Emulator.predict_tf` / `predict` / `simulate` take through it.

Reference: `oracle.emulator_ref.predict` / `predict_np` in fp64 with `forward` patched to return the chosen network outputs
(tests/predict_tail_util.py) -- exactly the tail; gradients by torch.autograd through the same call.  Configurations: see
predict_tail_util.configs; tests/test_predict_tail_math.py shows on the CPU that none of them has a gate within fp32 rounding of
its threshold, so ZERO entries may miss the tolerance here.

  direct entry     _lib.predict_tail in guarded, NaN-surrounded memory; y within T * 1e-6, ey within 1e-6 (TOL_FLOW) of
                   max(1, max|ref|); sentinels intact
  route identity   predict_tf / predict / simulate with fused_tail on are torch.equal to the same call with it off
  backward         per gradient tensor (y, ey, a, X[:, -1, :, 0]): fused vs fp64 <= max(3 x (tensor route vs fp64), 1e-7 max|ref|),
                   after the tensor route itself is shown to be within 1e-4 max|ref| (the inputs sit on no kink flip)
  planted ties     previous depth exactly hmin / hmax on pumped-storage nodes, q_us + r - q_ds exactly 0, link depth exactly 0
  end to end       mpc.objective_and_gradient, fused_tail on and off
  fallbacks        the cases that stay on the tensor route say so and still answer

The backward comparison leaves out `synth300` and uses `synth300_noloop`: with a link from a node to itself the TENSOR route's
backward is not the adjoint of its forward (autograd.FlowBalanceFn reads the link's ends from the link list, the forward from
the incidence pattern, where such a link is absent), so it fails its own 1e-4 gate there; the fused backward gathers through the
incidence entries and is checked against fp64 on that graph by itself.

The end-to-end case runs the pumps + offset model WITHOUT tide over two chunks: mpc.predict_horizon feeds the whole boundary
tensor back into the next chunk's state, which with tide (two boundary channels) is one channel wider than the model's input, on
either route.  The tide is covered end to end on one chunk.

Observed on an MI355X (UDS_TOL_REPORT=1):
  direct entry     out_y  1.2e-7 .. 7.4e-7 (allowed 2.8e-6 .. 1.7e-5), largest observed / allowed 0.075 (T1)
                   out_ey 5.6e-8 .. 1.2e-7 (allowed 1.4e-6 .. 1.5e-6), largest observed / allowed 0.082 (synth300, predict)
  backward         max|ref grad| 0.14 .. 4.8; tensor route vs fp64 0 .. 3.8e-7, fused vs fp64 0 .. 3.8e-7 -- equal to the tensor
                   route's error on most tensors; largest observed / allowed 0.58 (ef_act da: 4.05e-8 against 3 x 2.33e-8),
                   then 0.43 (ef_act dey: 2.10e-7 against 3 x 1.61e-7); dh0 without pumps is exactly 0 on both routes
  planted ties     depth ties: dy 2.98e-8, dey 3.00e-7 (tensor route 2.35e-7), da 3.5e-8, dh0 1.86e-8 (= the tensor route's);
                   q_w tie: dy 7.3e-8, dey 2.9e-8, both equal to the tensor route's
  self-loop graph  fused vs fp64: dy 2.97e-8, dey 3.75e-7, da 4.0e-8, dh0 2.98e-8 (allowed 1e-6 x max|ref| = 6.2e-7 .. 4.7e-6)
  end to end       objectives equal bit for bit; gradient error 1.95e-7 (two chunks) and 1.43e-7 (one chunk, tide) on
                   max|grad| 1.55 / 1.73, the same on both routes
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import dist as D
from gnn_uds_amd import mpc as M
from oracle import emulator_ref as OE
from tests import predict_tail_util as PT
from tests.util import Guarded, close, emulator_args, emulator_norms, load_emulator, nan_in

pytestmark = pytest.mark.gpu

ALL = ['ef_act', 'ef_pumps_offset_tide', 'ef_all_pumps', 'node_gates', 'eps0', 'plain', 'T1', 'synth300']
BWD = ['ef_act', 'ef_pumps_offset_tide', 'ef_all_pumps', 'node_gates', 'eps0', 'plain', 'T1', 'synth300_noloop']
REPORT = bool(os.environ.get('UDS_TOL_REPORT'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def built(networks, dev):
    """name -> the configuration's args, norms, inputs and its Emulator on the device (built once per module)."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = PT.configs(networks)[name]
            args, norms = PT.setup(cfg, networks)
            emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), OE.init_params(args, seed=3), dev)
            emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
            cache[name] = SimpleNamespace(cfg=cfg, args=args, norms=norms, inp=PT.inputs(args, cfg['seed']), emul=emul)
        return cache[name]
    return get


def f32(t, dev):
    return None if t is None else t.float().to(dev)


# ---- direct entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('np_form', [False, True], ids=['predict_tf', 'predict'])
@pytest.mark.parametrize('name', ALL)
def test_direct_entry(dev, built, name, np_form):
    c = built(name)
    emul, inp = c.emul, c.inp
    ry, rey = PT.reference(c.args, c.norms, inp, np_form)
    spec = emul._tail_spec(dev, 2 if emul.act else 0, inp.b.shape[-1], 3)
    handle = _lib.CsrHandle(emul.graph.inc_n)
    f = lambda t: None if t is None else nan_in(t.float(), dev)
    out_y, out_ey = Guarded(ry.shape, dev), Guarded(rey.shape, dev)
    override = emul.act and (emul._has_link_pump if np_form else emul._has_pump)
    gy, gey = _lib.predict_tail(handle, emul._inc_sign, spec, f(inp.y), f(inp.ey), f(inp.a), nan_in(emul.normalize(f32(inp.b, dev), 'b'), dev),
                                f(inp.b[..., 0]), f(inp.X[:, -1, :, 0]), 0.01 if np_form else 0.0, override, out_y=out_y.view, out_ey=out_ey.view)
    assert gy is out_y.view and gey is out_ey.view
    torch.cuda.synchronize()
    out_y.check('out_y')
    out_ey.check('out_ey')
    if REPORT:
        for what, got, ref, tol in (('y', gy, ry, PT.tol_y(c.cfg['T'])), ('ey', gey, rey, PT.TOL_FLOW)):
            print('tail %-22s %-10s %-2s observed %.3e allowed %.3e' % (name, 'predict' if np_form else 'predict_tf', what,
                                                                     float((got.double().cpu() - ref).abs().max()), tol * max(1.0, float(ref.abs().max()))))
    close(gy, ry, PT.tol_y(c.cfg['T']))          # max error within the tolerance: zero outliers
    close(gey, rey, PT.TOL_FLOW)


# ---- route identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_route_identity(dev, built, name):
    c = built(name)
    emul, inp = c.emul, c.inp
    X, b, a, Ex = f32(inp.X, dev), f32(inp.b, dev), f32(inp.a, dev), f32(inp.Ex, dev)
    try:
        with torch.no_grad():
            for fn in (emul.predict_tf, emul.predict, emul.simulate):
                emul.fused_tail = True
                y1, e1 = fn(X, b, a, Ex)
                assert emul.last_tail_path == 'hip', (fn.__name__, emul.last_tail_path)
                emul.fused_tail = False
                y0, e0 = fn(X, b, a, Ex)
                assert emul.last_tail_path == 'torch', (fn.__name__, emul.last_tail_path)
                assert torch.equal(y1, y0) and torch.equal(e1, e0), (name, fn.__name__, float((y1 - y0).abs().max()), float((e1 - e0).abs().max()))
                assert bool(torch.isfinite(y1).all())
    finally:
        emul.fused_tail = True


# ---- backward ---------------------------------------------------------------------------------------------------------------
def route_grads(emul, inp, X, gy, gey, dev, fused):
    """Gradients of sum(out_y gy) + sum(out_ey gey) through emul.predict_tf with the network forward replaced by the case's
    (y, ey): the tail alone, on the fused or the tensor route."""
    leaf = lambda t: None if t is None else f32(t, dev).requires_grad_(True)
    y, ey, a, Xd = leaf(inp.y), leaf(inp.ey), leaf(inp.a), leaf(X)
    emul.forward = lambda *args, **kw: (y, ey)
    emul.fused_tail = fused
    try:
        oy, oey = emul.predict_tf(Xd, f32(inp.b, dev), a, f32(inp.Ex, dev))
        path = emul.last_tail_path
    finally:
        del emul.forward
        emul.fused_tail = True
    ((oy * f32(gy, dev)).sum() + (oey * f32(gey, dev)).sum()).backward()
    g = lambda t: None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad).double().cpu()
    return dict(y=g(y), ey=g(ey), a=g(a), h0=g(Xd)[:, -1, :, 0]), path


def check_backward(name, emul, args, norms, inp, X, dev, seed):
    gy, gey = PT.upstream(inp, args, seed)
    ref = PT.reference_grads(args, norms, inp, gy, gey, X)
    tensor, p0 = route_grads(emul, inp, X, gy, gey, dev, False)
    fused, p1 = route_grads(emul, inp, X, gy, gey, dev, True)
    assert (p0, p1) == ('torch', 'hip-train')
    for k in ('y', 'ey', 'a', 'h0'):
        if ref[k] is None:
            continue
        gmax = float(ref[k].abs().max())
        err_t, err_f = float((tensor[k] - ref[k]).abs().max()), float((fused[k] - ref[k]).abs().max())
        allowed = max(PT.BWD_MARGIN * err_t, PT.BWD_FLOOR * gmax)
        if REPORT:
            print('tail-bwd %-22s d%-2s max|ref| %.3e tensor route %.3e fused observed %.3e allowed %.3e' % (name, k, gmax, err_t, err_f, allowed))
        assert err_t <= PT.TENSOR_ROUTE_GATE * gmax, (name, k, 'the tensor route itself misses fp64: the input sits on a kink', err_t, gmax)
        assert err_f <= allowed, (name, k, err_f, allowed, err_t, gmax)
    return ref


@pytest.mark.parametrize('name', BWD)
def test_backward(dev, built, name):
    c = built(name)
    ref = check_backward(name, c.emul, c.args, c.norms, c.inp, c.inp.X, dev, c.cfg['seed'])
    assert float(ref['y'].abs().max()) > 0 and float(ref['ey'].abs().max()) > 0
    if c.emul._has_any_pump and c.cfg['T'] > 1:
        assert float(ref['h0'].abs().max()) > 0          # the previous depth reaches the outputs through the depth recurrence


def test_backward_self_loop_graph_against_fp64(dev, built):
    """synth300 (a link from a node to itself): the fused backward alone against fp64, 1e-6 of max|ref| per tensor (a dozen fp32
    roundings per chain; observed: see the header)."""
    c = built('synth300')
    gy, gey = PT.upstream(c.inp, c.args, 8)
    ref = PT.reference_grads(c.args, c.norms, c.inp, gy, gey)
    fused, path = route_grads(c.emul, c.inp, c.inp.X, gy, gey, dev, True)
    assert path == 'hip-train'
    for k in ('y', 'ey', 'a', 'h0'):
        gmax = float(ref[k].abs().max())
        err = float((fused[k] - ref[k]).abs().max())
        if REPORT:
            print('tail-bwd synth300 d%-2s observed %.3e allowed %.3e' % (k, err, 1e-6 * gmax))
        assert err <= 1e-6 * gmax, (k, err, gmax)


def test_planted_ties(dev, built):
    """Ties are the normal case in MPC (a depth fed back from an earlier clamp sits exactly on hmin / hmax): maximum / minimum
    split evenly, clamp(min=0) passes at the bound -- as torch does in the fp64 reference."""
    # previous depth exactly hmin / hmax on pumped-storage nodes, link depth exactly 0 before the ehmax clamp
    c = built('ef_pumps_offset_tide')
    cfg = OE.config(c.args)
    ps = np.nonzero((cfg.area * (np.clip(cfg.node_edge, 0, 1) @ cfg.pump)) > 0)[0]
    assert len(ps) >= 4
    inp = SimpleNamespace(**{k: (None if v is None else v.clone()) for k, v in vars(c.inp).items()})
    X = inp.X.clone()
    X[:, -1, ps[::2], 0] = torch.as_tensor(cfg.hmin[ps[::2]])
    X[:, -1, ps[1::2], 0] = torch.as_tensor(cfg.hmax[ps[1::2]])
    inp.ey[:, :, ::3, 0] = 0.0
    ref = check_backward('ties:depth', c.emul, c.args, c.norms, inp, X, dev, 21)
    assert float(ref['h0'][:, ps].abs().max()) > 0
    # q_us + r - q_ds exactly 0: q_us = 0, q_ds = 0.5 * span (exact in fp32 and fp64), r = q_ds
    c = built('plain')
    inp = SimpleNamespace(**{k: (None if v is None else v.clone()) for k, v in vars(c.inp).items()})
    nodes = [3, 7, 11]
    span = c.norms['y'][0, nodes, 2] - c.norms['y'][1, nodes, 2]
    inp.y[:, :, nodes, 1], inp.y[:, :, nodes, 2] = 0.0, 0.5
    inp.b[:, :, nodes, 0] = 0.5 * span
    inp.ey[:, :, 1::3, 0] = 0.0
    ry, _ = PT.reference(c.args, c.norms, inp, False)
    assert float(ry[:, :, nodes, -1].abs().max()) == 0.0
    gy, _ = PT.upstream(inp, c.args, 22)
    ref = check_backward('ties:q_w', c.emul, c.args, c.norms, inp, inp.X, dev, 22)
    span1 = c.norms['y'][0, nodes, 1] - c.norms['y'][1, nodes, 1]
    assert float((ref['y'][:, :, nodes, 1] - (gy[:, :, nodes, 1] + gy[:, :, nodes, -1]) * span1).abs().max()) < 1e-12      # the bound passes


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunks,tide', [(2, False), (1, True)], ids=['two_chunks', 'one_chunk_tide'])
def test_mpc_objective_and_gradient(dev, networks, chunks, tide):
    """mpc.objective_and_gradient on the node-gates model with pumps and offsets: the objectives of the two routes are equal bit
    for bit, the gradients obey the backward rule against fp64 autograd over the oracle.  The tensor route's own error is that
    of the whole network's reverse mode here, so its gate is the one of tests/test_gpu_train.py::test_mpc_objective_and_gradient
    (2e-3 max|grad|)."""
    net = networks['astlingen']
    edges, n = np.array(net['edges']), net['n_node']
    rng = np.random.default_rng(5)
    e = len(edges)
    args = emulator_args(edges, n, seq_in=4, seq_out=2, n_sp_layer=1, if_flood=1, epsilon=0.1, edge_fusion=False, tide=tide,
                         pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
                         offset=rng.random(e) * (rng.random(e) > 0.5), area=0.2 + rng.random(n))
    norms = emulator_norms(args)
    params = OE.init_params(args, seed=3)
    c = OE.config(args)
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    T = c.seq_out * chunks
    state, runoff, edge_state = rnd(c.seq_in, n, 5), rnd(T, n, c.b_in) * 0.05, rnd(c.seq_in, e, 4)
    state[..., 3] = (state[..., 3] > 0.8).double()
    pop, n_step, n_act, r_step = 3, chunks, len(args.act_edges), 2
    y = 0.2 + 0.6 * rnd(pop, n_step * n_act)
    tg = dict(flood_idx=torch.tensor([3, 7, 11]), flood_w=torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64),
              outflow_idx=torch.tensor([0]), outflow_w=torch.tensor([0.3], dtype=torch.float64),
              smooth_idx=torch.tensor([5, 9]), smooth_w=torch.tensor([0.7, 0.2], dtype=torch.float64))
    gamma = torch.tensor([1.0, 0.9, 0.8, 0.7][:T], dtype=torch.float64)
    yr = y.clone().requires_grad_(True)
    ref = OE.mpc_objective(args, params, norms, yr, state, runoff, edge_state, n_step, n_act, r_step, tg, gamma)
    (gref,) = torch.autograd.grad(ref.sum(), yr)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args, precision='fp32'), params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    f = lambda t: t.float().to(dev)
    tgd = {k: (v.to(dev) if v.dtype == torch.int64 else f(v)) for k, v in tg.items()}
    run = lambda: M.objective_and_gradient(emul, f(y), f(state), f(runoff), f(edge_state), n_step, n_act, r_step, tgd, f(gamma))
    obj1, grad1 = run()
    assert emul.last_tail_path == 'hip-train'
    emul.fused_tail = False
    obj0, grad0 = run()
    assert emul.last_tail_path == 'torch'
    assert torch.equal(obj1, obj0)
    gmax = float(gref.abs().max())
    assert gmax > 0
    err_t, err_f = float((grad0.double().cpu() - gref).abs().max()), float((grad1.double().cpu() - gref).abs().max())
    allowed = max(PT.BWD_MARGIN * err_t, PT.BWD_FLOOR * gmax)
    if REPORT:
        print('tail-mpc chunks %d tide %d max|grad| %.3e tensor route %.3e fused observed %.3e allowed %.3e' % (chunks, tide, gmax, err_t, err_f, allowed))
    assert err_t <= 2e-3 * gmax, (err_t, gmax)
    assert err_f <= allowed, (err_f, allowed)


# ---- fallbacks --------------------------------------------------------------------------------------------------------------
def test_fallback_mlp_with_other_channel_counts(dev, networks):
    """conv='False' with a five-channel state: the network then emits one node channel more than the tail's row has."""
    net = networks['astlingen']
    n, e = net['n_node'], len(net['edges'])
    args = emulator_args(net['edges'], n, conv='False', state_shape=(n, 5), edge_fusion=True, act=True)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), OE.init_params(args, seed=3), dev)
    emul.set_norm(*(v.numpy() for v in (emulator_norms(args)[k] for k in 'xbyre')))
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    with torch.no_grad():
        y, ey = emul.predict_tf(r(2, 5, n, 6), r(2, 5, n, 1) * 0.1, r(2, 5, 2), r(2, 5, e, 4))
    assert emul.last_tail_path == 'torch'
    assert y.shape[:3] == (2, 5, n) and tuple(ey.shape) == (2, 5, e, 3) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(ey).all())


def test_fallback_shard_local(dev, built):
    """The local model of shard_emulator keeps the tensor route (its gated flows cross the cut before the balance): on the CPU,
    as built, and on the device, where the one-part shard still equals the unsharded model bit for bit."""
    c = built('ef_act')
    emul, inp = c.emul, c.inp
    prob = D.build_partition_plan(emul.graph, 1)[0]
    cpu = D.shard_emulator(emul, prob, 'cpu')
    assert hasattr(cpu.local, '_flow_exchange') and cpu.local.fused_tail
    t32 = lambda t: t.float()
    assert cpu.local._predict_tail_hip(t32(inp.y), t32(inp.ey), t32(inp.a), t32(inp.b), t32(inp.b), t32(inp.X), False) is None
    sh = D.shard_emulator(emul, prob, dev)
    X, b, a, Ex = f32(inp.X, dev), f32(inp.b, dev), f32(inp.a, dev), f32(inp.Ex, dev)
    with torch.no_grad():
        qy, qey = sh.predict_tf(X, b, a, Ex)
        assert sh.local.last_tail_path == 'torch'
        py, pey = emul.predict_tf(X, b, a, Ex)
        assert emul.last_tail_path == 'hip'
    assert torch.equal(qy, py) and torch.equal(qey, pey)


def test_fallback_numpy_mode_under_autograd(dev, built):
    c = built('node_gates')
    emul, inp = c.emul, c.inp
    X, b, Ex = f32(inp.X, dev), f32(inp.b, dev), f32(inp.Ex, dev)
    a = f32(inp.a, dev).requires_grad_(True)
    y, ey = emul.predict(X, b, a, Ex)
    assert emul.last_tail_path == 'torch' and bool(torch.isfinite(y).all())
    y.sum().backward()
    assert a.grad is not None and bool(torch.isfinite(a.grad).all())
    y2, _ = emul.predict_tf(X, b, f32(inp.a, dev).requires_grad_(True), Ex)
    assert emul.last_tail_path == 'hip-train' and y2.requires_grad
