"""The training tail as one HIP operator (uds_fit_tail / uds_fit_tail_backward, autograd.FitTailFn) and the route
`Emulator.fit_eval` / `fit_grad_norm` take through it (`emul.fused_fit_tail`, `emul.last_fit_tail_path`).

Reference: `oracle.train_ref.losses` in fp64 with `oracle.emulator_ref.forward` patched to return the chosen network outputs
(tests/fit_tail_util.py) -- exactly the tail; gradients by torch.autograd through the same call.  Cases: fit_tail_util.CASES;
tests/test_fit_tail_math.py shows on the CPU that their seeds put no gate, clamp or clip within fp32 rounding of its threshold.

  outputs          out_y / out_ey (written into guarded, sentinel-surrounded memory) are torch.equal to `post_proc_tf` on the same
                   device tensors
  losses           each loss against fp64: relative error <= (log2(n) + 8) 2^-24, n = the per-sample terms summed (the terms are
                   non-negative, the reduction is a tree, a term carries a few roundings); the tensor route's error is printed
                   beside it, not asserted
  backward         dy / dey for random g_loss (and random gradients at out_y / out_ey in the roll case): HIP route vs fp64 <=
                   max(BWD_MARGIN x (tensor route vs fp64), BWD_FLOOR max|ref|), after the tensor route is shown to be within
                   TENSOR_ROUTE_GATE max|ref| (the inputs sit on no kink)
  repeatability    losses, outputs and gradients equal bit for bit over two calls; the backward twice on one forward
  whole model      fit_eval for 3 Adam steps, fit_grad_norm, roll = 2: last_fit_tail_path == 'hip', losses and parameters against
                   oracle.train_ref at the bounds of tests/test_gpu_train.py
  guards           bad shapes / dtype, empty batch, a NaN row, the non-finite-loss error
  fallbacks        a local model of shard_emulator, a setting that needs a gradient, a model without norms and one with other
                   channel counts report 'torch'

As in tests/test_gpu_predict_tail.py the comparison with the tensor route's backward leaves out `synth300` (a link from a node to
itself: autograd.FlowBalanceFn, the TENSOR route's backward, is not the adjoint of its forward there and fails its own gate) and
uses `synth300_noloop`; on `synth300` the HIP backward is held to fp64 alone, 1e-6 of max|ref|.

The tensor route's flood loss misses the loss bound on every case with a flood channel, by 2e-3 .. 4e-3 relative: fp32 `clamp(1e-7,
1 - 1e-7)` clips a saturated probability at fl(1 - 1e-7) = 1 - 2^-23 and takes log(1.19e-7) where the definition has log(1e-7)
(tests/test_fit_tail_math.py prints the same figures for the fp32 oracle on the CPU).  The operator clips p and 1 - p apart and is
held to the bound.  Observed on an MI355X: see DESIGN.md 5.4c.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import autograd as AG
from gnn_uds_amd import dist as D
from oracle import emulator_ref as OE
from oracle import train_ref as OT
from tests import fit_tail_util as FT
from tests.util import Guarded, emulator_args, emulator_norms, emulator_param_pairs, load_emulator

pytestmark = pytest.mark.gpu

BWD = [n for n in FT.CASES if n != 'synth300']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def built(networks, dev):
    """name -> the case's args, norms, inputs (fp64 on the CPU: inp, fp32 on the device: d) and its Emulator (built once)."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = FT.case_configs(networks)[name]
            args, norms = FT.setup(cfg, networks)
            emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), OE.init_params(args, seed=3), dev)
            emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
            inp = FT.case_inputs(args, cfg['seed'])
            d = SimpleNamespace(**{k: (None if v is None else v.float().to(dev)) for k, v in vars(inp).items()})
            cache[name] = SimpleNamespace(name=name, cfg=cfg, args=args, norms=norms, inp=inp, d=d, emul=emul, ref_losses=FT.reference_losses(args, norms, inp))
        return cache[name]
    return get


def operands(c):
    """(spec, ops, handle, override) of the case's model: what `_fit_losses` hands to autograd.FitTailFn."""
    emul, d = c.emul, c.d
    emul.fused_fit_tail = True
    fused = emul._fit_tail_spec(d.X, d.a, d.b, d.y_true, d.ey_true)
    assert fused is not None
    return fused[0], fused[1], emul._inc_handle, emul.act and emul._has_pump


def hip_tail(c, y, ey):
    """(out_y, out_ey, loss_sums) of the operator on the case's whole time axis (it is pointwise in time: the chunks of a rollout
    in one call)."""
    spec, ops, handle, override = operands(c)
    return AG.FitTailFn.apply(y, ey, c.d.a if c.emul.act else None, c.d.b, c.d.y_true, c.d.ey_true, handle, spec, ops, override)


def tensor_tail(c, y, ey):
    """The same three from the tensor code: post_proc_tf, clamp, get_node_loss, get_flood_loss, _mse, times their sample counts."""
    emul, d = c.emul, c.d
    out_y, out_ey = emul.post_proc_tf((y, ey), d.a, d.b)
    preds = out_y.clamp(0, 1)
    node = emul.get_node_loss(d.y_true, d.b, preds)
    flood = emul.get_flood_loss(d.y_true, preds) if emul.if_flood and not emul.balance else torch.zeros((), device=y.device)
    edge = emul._mse(d.ey_true, out_ey, emul._loss_setup(y.device)['ewei'])
    n = FT.counts(c.args, c.inp)
    return out_y, out_ey, torch.stack([node * n[0], flood * n[1], edge * n[2]])


# ---- outputs, losses, repeatability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FT.CASES)
def test_outputs_and_losses(dev, built, name):
    c = built(name)
    emul, d = c.emul, c.d
    spec, ops, handle, override = operands(c)
    with torch.no_grad():
        ty, tey, tsums = tensor_tail(c, d.y, d.ey)
        gy, gey = Guarded(ty.shape, dev), Guarded(tey.shape, dev)
        oy, oey, sums = _lib.fit_tail(handle, spec, d.y, d.ey, d.a if emul.act else None, d.b, d.y_true, d.ey_true, ops, override, out_y=gy.view, out_ey=gey.view)
        torch.cuda.synchronize()
        gy.check('out_y')
        gey.check('out_ey')
        assert oy is gy.view and torch.equal(oy, ty) and torch.equal(oey, tey), (name, float((oy - ty).abs().max()), float((oey - tey).abs().max()))
        oy2, oey2, sums2 = hip_tail(c, d.y, d.ey)
        assert torch.equal(oy2, oy) and torch.equal(oey2, oey) and torch.equal(sums2, sums)
    counts = FT.counts(c.args, c.inp)
    for k, what in enumerate(('node', 'flood', 'edge')):
        ref = float(c.ref_losses[k])
        if ref == 0:
            assert float(sums[k]) == 0, (name, what, float(sums[k]))
            continue
        err_h = abs(float(sums[k].double()) / counts[k] - ref) / ref
        err_t = abs(float(tsums[k].double()) / counts[k] - ref) / ref
        print('fit-tail %-22s %-5s n %6d fp64 %.9e rel err hip %.3e tensor route %.3e bound %.3e' % (name, what, counts[k], ref, err_h, err_t, FT.loss_bound(counts[k])))
        assert err_h <= FT.loss_bound(counts[k]), (name, what, err_h, FT.loss_bound(counts[k]), err_t)


def fit_losses(c, fused, y, ey):
    """emul._fit_losses with the network forward replaced by the case's (y, ey), chunk after chunk."""
    emul, d = c.emul, c.d
    calls = iter(range(max(emul.roll, 1)))
    so = emul.seq_out

    def forward(*args, **kw):
        i = next(calls)
        return y[:, i * so:(i + 1) * so], ey[:, i * so:(i + 1) * so]
    emul.forward = forward
    emul.fused_fit_tail = fused
    try:
        ae = emul.get_edge_action(d.a, True) if emul.act else None
        out = emul._fit_losses(d.X, d.a, d.b, d.y_true, d.Ex, d.ey_true, ae, False)
        return out, emul.last_fit_tail_path
    finally:
        del emul.forward
        emul.fused_fit_tail = True


@pytest.mark.parametrize('name', [FT.ROLL, 'node_gates', 'plain_balance'])
def test_losses_through_the_emulator(dev, built, name):
    """`_fit_losses` (what fit_eval and fit_grad_norm call): one operator call per chunk, sums added, then the division."""
    c = built(name)
    with torch.no_grad():
        hip, p1 = fit_losses(c, True, c.d.y, c.d.ey)
        ten, p0 = fit_losses(c, False, c.d.y, c.d.ey)
    assert (p1, p0) == ('hip', 'torch')
    assert (hip[1] is None) == (ten[1] is None) == (not (c.emul.if_flood and not c.emul.balance))
    counts = FT.counts(c.args, c.inp)
    for k, what in enumerate(('node', 'flood', 'edge')):
        if hip[k] is None:
            continue
        ref = float(c.ref_losses[k])
        err_h, err_t = abs(float(hip[k]) - ref) / ref, abs(float(ten[k]) - ref) / ref
        print('fit-tail/emulator %-16s %-5s rel err hip %.3e tensor route %.3e bound %.3e' % (name, what, err_h, err_t, FT.loss_bound(counts[k])))
        # one more rounding than the sums: the division (and, with roll, the addition of the chunks' sums)
        assert err_h <= FT.loss_bound(counts[k]) + 2.0 ** -23, (name, what, err_h)


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def route_grads(c, tail, g_loss, gy, gey, dev):
    y, ey = c.d.y.clone().requires_grad_(True), c.d.ey.clone().requires_grad_(True)
    oy, oey, sums = tail(c, y, ey)
    total = (sums * g_loss.float().to(dev)).sum()
    if gy is not None:
        total = total + (oy * gy.float().to(dev)).sum() + (oey * gey.float().to(dev)).sum()
    total.backward()
    return dict(y=y.grad.double().cpu(), ey=ey.grad.double().cpu())


@pytest.mark.parametrize('name', BWD)
def test_backward(dev, built, name):
    c = built(name)
    g_loss, gy, gey = FT.upstream(c.args, c.inp, c.cfg['seed'], name == FT.ROLL)
    ref = FT.reference_grads(c.args, c.norms, c.inp, g_loss, gy, gey)
    tensor = route_grads(c, tensor_tail, g_loss, gy, gey, dev)
    fused = route_grads(c, hip_tail, g_loss, gy, gey, dev)
    again = route_grads(c, hip_tail, g_loss, gy, gey, dev)
    for k in ('y', 'ey'):
        gmax = float(ref[k].abs().max())
        err_t, err_f = float((tensor[k] - ref[k]).abs().max()), float((fused[k] - ref[k]).abs().max())
        allowed = max(FT.BWD_MARGIN * err_t, FT.BWD_FLOOR * gmax)
        print('fit-tail-bwd %-22s d%-2s max|ref| %.3e tensor route %.3e hip %.3e allowed %.3e' % (name, k, gmax, err_t, err_f, allowed))
        assert gmax > 0
        assert err_t <= FT.TENSOR_ROUTE_GATE * gmax, (name, k, 'the tensor route itself misses fp64: the input sits on a kink', err_t, gmax)
        assert err_f <= allowed, (name, k, err_f, allowed, err_t, gmax)
        assert torch.equal(fused[k], again[k])


def test_backward_self_loop_graph_against_fp64(dev, built):
    """synth300 (a link from a node to itself): the HIP backward alone against fp64, 1e-6 of max|ref| per tensor (a dozen fp32
    roundings per chain), as tests/test_gpu_predict_tail.py holds the predict tail on this graph."""
    c = built('synth300')
    g_loss, gy, gey = FT.upstream(c.args, c.inp, 8, True)
    ref = FT.reference_grads(c.args, c.norms, c.inp, g_loss, gy, gey)
    fused = route_grads(c, hip_tail, g_loss, gy, gey, dev)
    for k in ('y', 'ey'):
        gmax, err = float(ref[k].abs().max()), float((fused[k] - ref[k]).abs().max())
        print('fit-tail-bwd synth300 d%-2s max|ref| %.3e hip %.3e allowed %.3e' % (k, gmax, err, 1e-6 * gmax))
        assert err <= 1e-6 * gmax, (k, err, gmax)


def test_backward_twice_on_one_forward(dev, built):
    """fit_grad_norm takes two gradients of one forward (retain_graph): the second call sees nothing of the first."""
    c = built('node_gates')
    y, ey = c.d.y.clone().requires_grad_(True), c.d.ey.clone().requires_grad_(True)
    _, _, sums = hip_tail(c, y, ey)
    reg, cls = sums[0] + sums[2], sums[1]
    g_reg = torch.autograd.grad(reg, (y, ey), retain_graph=True)
    g_cls = torch.autograd.grad(cls, (y, ey), retain_graph=True)
    g_reg2 = torch.autograd.grad(reg, (y, ey))
    y2, ey2 = c.d.y.clone().requires_grad_(True), c.d.ey.clone().requires_grad_(True)
    g_cls_fresh = torch.autograd.grad(hip_tail(c, y2, ey2)[2][1], (y2, ey2))
    assert all(torch.equal(p, q) for p, q in zip(g_reg, g_reg2)) and all(torch.equal(p, q) for p, q in zip(g_cls, g_cls_fresh))
    assert float(g_cls[0][..., :3].abs().max()) == 0 < float(g_cls[0][..., 3].abs().max())      # the flood loss reaches the flood channel alone
    assert float(g_cls[1].abs().max()) == 0 < float(g_reg[1].abs().max())


# ---- whole model ------------------------------------------------------------------------------------------------------------------
def problem(networks, dev, seed=3, batch=2, **over):
    """A small GAT + Conv1D emulator on astlingen with its oracle twin: the set-up of tests/test_gpu_train.py."""
    net = networks['astlingen']
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, embed_size=64, n_sp_layer=1, **over)
    norms = emulator_norms(args)
    params = OE.init_params(args, seed=1)
    c = OE.config(args)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    T = c.seq_out * max(c.roll, 1)
    x, b, ex = rnd(batch, c.seq_in, n, c.n_in), rnd(batch, T, n, c.b_in) * 0.1, rnd(batch, c.seq_in, len(edges), c.e_in)
    a = rnd(batch, T, len(args.act_edges))
    y = rnd(batch, T, n, 5)
    y[..., -2] = (y[..., -2] > 0.7).double()
    ey = rnd(batch, T, len(edges), 3)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    emul.fused_fit_tail = True
    return args, norms, params, emul, (x, a, b, y, ex, ey), tuple(t.float().to(dev) for t in (x, a, b, y, ex, ey))


@pytest.mark.parametrize('over', [dict(), dict(roll=2, seq_out=2)], ids=['one_chunk', 'roll2'])
def test_fit_eval_steps_match_oracle_adam(dev, networks, over):
    """3 Adam steps through the fused tail against oracle.train_ref: the bounds of
    tests/test_gpu_train.py::test_fit_eval_steps_match_oracle_adam."""
    args, norms, params, emul, cpu_in, dev_in = problem(networks, dev, learning_rate=1e-3, **over)
    opt = OT.Adam(lr=1e-3)
    leaves = list(OT.tree_leaves(params))
    ref_hist = []
    for _ in range(3):
        ls, gr = OT.grads(args, params, norms, *cpu_in)
        ref_hist.append([float(l) for l in ls])
        opt.step(leaves, gr)
    hist = []
    for _ in range(3):
        hist.append([float(l) for l in emul.fit_eval(*dev_in)])
        assert emul.last_fit_tail_path == 'hip'
    for h, r in zip(hist, ref_hist):
        assert np.allclose(h, r, rtol=2e-3, atol=1e-5), (hist, ref_hist)
    for pname, p, ref in emulator_param_pairs(emul, dict(OT.tree_leaves(params))):
        err = float((p.detach().double().cpu() - ref).abs().max())
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)
    ev = emul.fit_eval(*dev_in, fit=False)
    assert emul.last_fit_tail_path == 'hip' and len(ev) == 3 and all(np.isfinite(float(v)) for v in ev)


def test_grad_norm_task_weights_match_the_oracle(dev, networks):
    """fit_grad_norm through the fused tail (two gradients of one forward): the bounds of
    tests/test_gpu_train.py::test_grad_norm_task_weights_match_the_oracle."""
    args, norms, params, emul, cpu_in, dev_in = problem(networks, dev, gradnorm=True)
    ini_ref = [float(l) for l in OT.losses(args, params, norms, *cpu_in)]
    ini = [float(l) for l in emul.fit_eval(*dev_in, fit=False)]
    assert emul.last_fit_tail_path == 'hip' and np.allclose(ini, ini_ref, rtol=2e-3, atol=1e-6)
    alpha = torch.ones(2, dtype=torch.float64)
    opt = OT.Adam(lr=1e-4, clipnorm=None)
    for _ in range(2):
        ref_loss = OT.grad_norm_step(args, params, norms, *cpu_in, ini_ref, alpha, opt)
        got_loss = emul.fit_grad_norm(*dev_in, ini_ref)
        assert emul.last_fit_tail_path == 'hip'
        assert abs(float(got_loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)) + 1e-9
        got = emul._alphas(dev).detach().double().cpu()
        assert abs(float(got.sum()) - 2.0) < 1e-6 and torch.allclose(got, alpha, rtol=0, atol=2e-6), (got, alpha)
    ls = emul.fit_eval(*dev_in)
    assert emul.last_fit_tail_path == 'hip' and len(ls) == 3 and all(np.isfinite(float(v)) for v in ls)


# ---- guards -----------------------------------------------------------------------------------------------------------------------
def test_bad_operands_are_refused(dev, built):
    c = built('node_gates')
    emul, d = c.emul, c.d
    spec, ops, handle, override = operands(c)
    call = lambda **kw: _lib.fit_tail(handle, spec, *[kw.get(k, getattr(d, k)) for k in ('y', 'ey', 'a', 'b', 'y_true', 'ey_true')], kw.get('ops', ops), override)
    for kw, text in ((dict(y=d.y[:, :, :-1].contiguous()), 'fit_tail: y must be'), (dict(ey_true=d.ey_true[..., :2].contiguous()), 'fit_tail: ey_true must be'),
                     (dict(y=d.y.double()), 'fit_tail: y must be float32'), (dict(y_true=d.y_true[..., :2].contiguous()), 'fit_tail: y_true needs at least 3 channels'),
                     (dict(ops=dict(ops, nwei=ops['nwei'][:, :2].contiguous())), 'fit_tail: nwei must be')):
        with pytest.raises(_lib.UdsError, match=text):
            call(**kw)
    with pytest.raises(_lib.UdsError, match='fit_tail_backward: g_loss must be'):
        _lib.fit_tail_backward(handle, spec, d.y, d.ey, d.a, d.b, d.y_true, d.ey_true, ops, torch.ones(2, device=dev))
    # behind the binding: the entry itself, with device pointers and one bad number
    lib, p = _lib.load(), spec.struct(0.0, override)
    out_y, out_ey, sums, ws = torch.empty(d.y.shape, device=dev), torch.empty_like(d.ey), torch.empty(3, device=dev), torch.empty(4096, device=dev)
    ptr = lambda t: t.data_ptr()
    lead = [handle.ptr, ptr(ops['sign']), ctypes.addressof(p), ptr(d.y), ptr(d.ey), ptr(d.a), ptr(d.b), ptr(d.y_true), ptr(d.ey_true), ptr(ops['nwei']),
            ptr(ops['poswei']), ptr(ops['ewei']), None, None, None, d.y.shape[0], d.y.shape[1]]
    rc = lib.uds_fit_tail(*lead, 2, 0, ptr(out_y), ptr(out_ey), ptr(sums), ptr(ws), None)
    assert rc == -22 and lib.uds_last_error().decode().startswith('uds_fit_tail: cyt=2')
    rc = lib.uds_fit_tail_backward(*lead, 5, 1, ptr(sums), None, None, ptr(out_y), ptr(out_ey), ptr(ws), None)
    assert rc == -22 and lib.uds_last_error().decode().startswith('uds_fit_tail_backward: balance needs')


def test_empty_batch_launches_nothing(dev, built):
    c = built('ef_act')
    emul, d = c.emul, c.d
    spec, ops, handle, override = operands(c)
    e = lambda t: t[:0].contiguous()
    oy, oey, sums = _lib.fit_tail(handle, spec, e(d.y), e(d.ey), e(d.a), e(d.b), e(d.y_true), e(d.ey_true), ops, override)
    assert oy.shape[0] == 0 and oey.shape[0] == 0 and sums.tolist() == [0.0, 0.0, 0.0]
    dy, dey = _lib.fit_tail_backward(handle, spec, e(d.y), e(d.ey), e(d.a), e(d.b), e(d.y_true), e(d.ey_true), ops, torch.ones(3, device=dev))
    assert dy.shape == e(d.y).shape and dey.shape == e(d.ey).shape


def test_nan_row_stays_in_its_row_and_fit_eval_raises(dev, built):
    c = built('node_gates')
    emul, d = c.emul, c.d
    y = d.y.clone()
    y[1, 2, 7, :] = float('nan')
    yl, eyl = y.clone().requires_grad_(True), d.ey.clone().requires_grad_(True)
    _, _, sums = hip_tail(c, yl, eyl)
    assert bool(torch.isnan(sums[0])) and bool(torch.isnan(sums[1])) and bool(torch.isfinite(sums[2]))
    sums.sum().backward()
    row = torch.zeros(y.shape[:3], dtype=torch.bool, device=dev)
    row[1, 2, 7] = True
    assert bool(torch.isfinite(yl.grad[~row]).all()) and bool(torch.isfinite(eyl.grad).all()) and float(yl.grad[~row].abs().max()) > 0
    for fused in (True, False):
        emul.forward = lambda *args, **kw: (y, d.ey)
        emul.fused_fit_tail = fused
        try:
            with pytest.raises(FloatingPointError):
                emul.fit_eval(d.X, d.a, d.b, d.y_true, d.Ex, d.ey_true)
            assert emul.last_fit_tail_path == ('hip' if fused else 'torch')
        finally:
            del emul.forward
            emul.fused_fit_tail = True


def test_if_flood_with_balance_is_refused_as_before(dev, built):
    c = built('node_gates_balance')
    emul, d = c.emul, c.d
    for fused in (True, False):
        emul.forward = lambda *args, **kw: (d.y, d.ey)
        emul.fused_fit_tail = fused
        try:
            with pytest.raises(NotImplementedError):
                emul.fit_eval(d.X, d.a, d.b, d.y_true, d.Ex, d.ey_true)
            assert len(emul.fit_eval(d.X, d.a, d.b, d.y_true, d.Ex, d.ey_true, fit=False)) == 2
            assert emul.last_fit_tail_path == ('hip' if fused else 'torch')
        finally:
            del emul.forward
            emul.fused_fit_tail = True


# ---- fallbacks --------------------------------------------------------------------------------------------------------------------
def test_fallback_setting_that_needs_a_gradient(dev, built):
    c = built('ef_act')
    a = c.d.a.clone().requires_grad_(True)
    d = SimpleNamespace(**dict(vars(c.d), a=a))
    c2 = SimpleNamespace(**dict(vars(c), d=d))
    with torch.enable_grad():
        (node, fl, edge), path = fit_losses(c2, True, c.d.y, c.d.ey)
        assert path == 'torch'
        (node + fl + edge).backward()
    assert a.grad is not None and bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().max()) > 0
    with torch.no_grad():                    # no tape: nothing needs a gradient
        _, path = fit_losses(c2, True, c.d.y, c.d.ey)
    assert path == 'hip'


def test_fallback_shard_local(dev, built):
    """The local model of shard_emulator keeps the tensor route (its gated flows cross the cut before the balance)."""
    c = built('ef_act')
    prob = D.build_partition_plan(c.emul.graph, 1)[0]
    sh = D.shard_emulator(c.emul, prob, dev)
    local, d = sh.local, c.d
    assert hasattr(local, '_flow_exchange') and local.fused_fit_tail
    assert local._fit_tail_spec(d.X, d.a, d.b, d.y_true, d.ey_true) is None
    c2 = SimpleNamespace(**dict(vars(c), emul=local))
    with torch.no_grad():
        got, path = fit_losses(c2, True, d.y, d.ey)
        want, _ = fit_losses(c, False, d.y, d.ey)
    assert path == 'torch' and all(torch.equal(p, q) for p, q in zip(got, want))


def test_fallback_model_without_norms(dev, networks):
    """A plain model (no settings, no edge fusion, no offsets) trains on normalised tensors without `set_norm`: its tensor code
    never asks for a norm, the kernels would."""
    net = networks['astlingen']
    n, e = net['n_node'], len(net['edges'])
    args = emulator_args(net['edges'], n, embed_size=64, n_sp_layer=1, edge_fusion=False, act=False, if_flood=0)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), OE.init_params(args, seed=3), dev)
    emul.fused_fit_tail = True
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    ls = emul.fit_eval(r(2, 5, n, 4), None, r(2, 5, n, 1) * 0.1, r(2, 5, n, 4), r(2, 5, e, 4), r(2, 5, e, 3), fit=False)
    assert emul.last_fit_tail_path == 'torch' and len(ls) == 2 and all(np.isfinite(float(v)) for v in ls)


def test_fallback_mlp_with_other_channel_counts(dev, networks):
    """conv='False' with a five-channel state: the network emits one node channel more than the tail's row has."""
    net = networks['astlingen']
    n, e = net['n_node'], len(net['edges'])
    args = emulator_args(net['edges'], n, conv='False', state_shape=(n, 5), edge_fusion=True, act=True)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), OE.init_params(args, seed=3), dev)
    emul.set_norm(*(v.numpy() for v in (emulator_norms(args)[k] for k in 'xbyre')))
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)
    assert emul.fused_fit_tail is not None
    emul.fused_fit_tail = True
    assert emul._fit_tail_spec(r(2, 5, n, 6), r(2, 5, 2), r(2, 5, n, 1), r(2, 5, n, 6), r(2, 5, e, 3)) is None
