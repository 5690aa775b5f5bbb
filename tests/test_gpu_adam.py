"""uds_adam_step / `HipKerasAdam` on the MI355X against the fp64 restatement of tests/adam_util.py (which tests/test_adam_math.py
holds `KerasAdam` to): the shapes and gradient scales of that file, one tensor of three workgroup spans + 1 elements and a list
one tensor longer than a launch's table, every operand in guarded memory.

Bounds.  Parameters, per tensor: the larger of 4 x the error `KerasAdam` (the optimizer of every earlier step) shows against the
same restatement on the same inputs on this device, and 2 ulp of max|p| (three steps of half an ulp each for the final rounding,
the rest for the update's own roundings; |p| >= 0.5 in these cases).  Slots: the larger of 4 x KerasAdam's error and, per step, five
ulp of the slot's largest element (three roundings per step and the clipped gradient's own, as in tests/test_adam_math.py).
UDS_TOL_REPORT=1 prints observed and allowed."""
import os

import pytest
import torch

from gnn_uds_amd import _lib
from gnn_uds_amd.emulator import HipKerasAdam, KerasAdam
from tests import adam_util as AU
from tests import util
from tests.util import Guarded

pytestmark = pytest.mark.gpu

SPAN3 = (3 * _lib.ADAM_SPAN + 1,)
FILL = _lib.ADAM_TABLE + 1 - len(AU.SHAPES) - 1             # small tensors up to one more than a launch's table holds
SHAPES = AU.SHAPES + [SPAN3] + [(7,)] * FILL
SCALES = AU.SCALES + [1.0] + [0.5 if k % 2 else 1e-2 for k in range(FILL)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def case(dev):
    """Inputs, the restatement, and KerasAdam's errors against it on this device: computed once, never written to."""
    assert len(SHAPES) == _lib.ADAM_TABLE + 1
    p0, grads = AU.make_inputs(SHAPES, SCALES, seed=3)
    return dict(p0=p0, grads=grads, ref=AU.restate(p0, grads), keras=AU.keras_errors(KerasAdam, p0, grads, dev))


def _guarded_optimizer(p0, dev, shift=0):
    """HipKerasAdam whose p, m, v live in guarded views (shift = 1: one float past a 16-byte boundary) -> (opt, guards)."""
    guards = {k: [Guarded((t.numel() + shift,), dev) for t in p0] for k in 'pmvg'}
    view = lambda k, i: guards[k][i].view[shift:].view(p0[i].shape)
    for k in 'pmvg':
        for g in guards[k]:
            g.view.zero_()
    ps = []
    for i, t in enumerate(p0):
        view('p', i).copy_(t)
        ps.append(torch.nn.Parameter(view('p', i)))
        assert ps[-1].data_ptr() == view('p', i).data_ptr()
    opt = HipKerasAdam(ps, AU.LR, AU.B1, AU.B2, AU.EPS, clipnorm=AU.CLIP)
    opt.m = [view('m', i) for i in range(len(p0))]
    opt.v = [view('v', i) for i in range(len(p0))]
    return opt, guards, view


def _run(opt, view, grads, loss=None):
    for gs in grads:
        for i, (p, g) in enumerate(zip(opt.params, gs)):
            view('g', i).copy_(g)
            p.grad = view('g', i)
        opt.step(loss)


def _check_guards(guards, shift):
    for k, gl in guards.items():
        for i, g in enumerate(gl):
            g.check('%s[%d]' % (k, i))
            if shift:
                assert float(g.view[0]) == 0.0, '%s[%d]: the float before the tensor was written' % (k, i)


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'one-float-off'])
def test_three_steps_against_the_restatement(case, dev, shift):
    opt, guards, view = _guarded_optimizer(case['p0'], dev, shift)
    _run(opt, view, case['grads'])
    torch.cuda.synchronize()
    _check_guards(guards, shift)
    assert opt.t == AU.STEPS and int(opt.state[1]) == 0
    rp, rm, rv = case['ref']
    kp, km, kv, kt = case['keras']
    assert kt == AU.STEPS
    report = os.environ.get('UDS_TOL_REPORT')
    for i, s in enumerate(SHAPES):
        for what, out, ref, kerr, floor in (('p', opt.params[i], rp[i], kp[i], 2 * AU.ulp32(rp[i].abs().max())),
                                            ('m', opt.m[i], rm[i], km[i], AU.STEPS * 5 * AU.ulp32(rm[i].abs().max())),
                                            ('v', opt.v[i], rv[i], kv[i], AU.STEPS * 5 * AU.ulp32(rv[i].abs().max()))):
            err, lim = AU.max_err(out, ref), max(4 * kerr, floor)
            if report:
                print('adam %s[%d] %r scale %g: observed %.3e allowed %.3e (KerasAdam %.3e)' % (what, i, s, SCALES[i], err, lim, kerr))
                util.OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', 'adam').split(' ')[0], i, err, max(lim, 1e-300)))
            assert err <= lim, (what, i, s, err, lim, kerr)
    # the zero gradient moved nothing
    z = SCALES.index(0.0)
    assert torch.equal(opt.params[z].detach().cpu(), case['p0'][z])


def test_two_runs_give_the_same_bits(case, dev):
    outs = []
    for _ in range(2):
        opt, guards, view = _guarded_optimizer(case['p0'], dev)
        _run(opt, view, case['grads'])
        outs.append([t.detach().clone() for t in list(opt.params) + opt.m + opt.v])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def _snapshot(opt):
    return [t.detach().clone() for t in list(opt.params) + opt.m + opt.v] + [opt.state[:1].clone()]


def test_a_nan_gradient_changes_nothing_and_sets_bit_1(case, dev):
    opt, guards, view = _guarded_optimizer(case['p0'], dev)
    _run(opt, view, case['grads'][:1])
    before = _snapshot(opt)
    bad = [g.clone() for g in case['grads'][1]]
    bad[SHAPES.index(SPAN3)][2 * _lib.ADAM_SPAN + 5] = float('nan')          # in the third span of the split tensor
    _run(opt, view, [bad])
    assert int(opt.state[1]) == 2
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(opt))) and opt.t == 1
    with pytest.raises(FloatingPointError, match='grads contain NaN/Inf!'):
        opt.raise_if_not_finite()
    bad = [g.clone() for g in case['grads'][1]]
    bad[-1][0] = float('inf')                                                # in the last tensor: the second launch of a pass
    _run(opt, view, [bad])
    assert int(opt.state[1]) == 2 and all(torch.equal(a, b) for a, b in zip(before, _snapshot(opt)))
    # the next good step goes through: status cleared, the same bits as a run that never saw the bad gradients
    _run(opt, view, case['grads'][1:2])
    assert int(opt.state[1]) == 0 and opt.t == 2
    opt.raise_if_not_finite()
    clean, _, cview = _guarded_optimizer(case['p0'], dev)
    _run(clean, cview, case['grads'][:2])
    assert all(torch.equal(a, b) for a, b in zip(_snapshot(clean), _snapshot(opt)))
    _check_guards(guards, 0)


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')])
def test_a_non_finite_loss_changes_nothing_and_sets_bit_0(case, dev, value):
    opt, guards, view = _guarded_optimizer(case['p0'], dev)
    before = _snapshot(opt)
    _run(opt, view, case['grads'][:1], loss=torch.tensor(value, device=dev))
    assert int(opt.state[1]) == 1 and all(torch.equal(a, b) for a, b in zip(before, _snapshot(opt)))
    with pytest.raises(FloatingPointError, match='Loss contains NaN or Inf values.'):
        opt.raise_if_not_finite()
    _run(opt, view, case['grads'][:1], loss=torch.tensor(0.25, device=dev))
    assert int(opt.state[1]) == 0 and opt.t == 1


def test_one_captured_step_replayed_three_times_equals_three_eager_calls(case, dev):
    eager, _, eview = _guarded_optimizer(case['p0'], dev)
    _run(eager, eview, case['grads'])
    opt, guards, view = _guarded_optimizer(case['p0'], dev)
    for i, p in enumerate(opt.params):
        p.grad = view('g', i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert opt.t == 0                                                        # capture runs nothing
    for gs in case['grads']:
        for i, g in enumerate(gs):
            view('g', i).copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert opt.t == AU.STEPS
    assert all(torch.equal(a, b) for a, b in zip(_snapshot(eager), _snapshot(opt)))
    _check_guards(guards, 0)


def test_state_dict_round_trip_with_keras_adam(case, dev):
    p0, grads = case['p0'][:8], [gs[:8] for gs in case['grads']]

    def run(cls_a, cls_b):
        """two steps with cls_a, its state_dict into cls_b, the third step there -> parameters, slots, t"""
        ps = [torch.nn.Parameter(t.clone().to(dev)) for t in p0]
        a = cls_a(ps, AU.LR, AU.B1, AU.B2, AU.EPS, clipnorm=AU.CLIP)
        for gs in grads[:2]:
            for p, g in zip(ps, gs):
                p.grad = g.clone().to(dev)
            a.step()
        sd = a.state_dict()
        assert sd['t'] == 2 and isinstance(sd['t'], int) and all(t.device.type == 'cpu' for t in sd['m'] + sd['v'])
        b = cls_b(ps, AU.LR, AU.B1, AU.B2, AU.EPS, clipnorm=AU.CLIP)
        b.load_state_dict(sd)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(b.m + b.v, sd['m'] + sd['v'])) and b.t == 2
        for p, g in zip(ps, grads[2]):
            p.grad = g.clone().to(dev)
        b.step()
        assert b.t == 3
        return ps

    rp, _, _ = AU.restate(p0, grads)
    for cls_a, cls_b in ((KerasAdam, HipKerasAdam), (HipKerasAdam, KerasAdam)):
        for p, r in zip(run(cls_a, cls_b), rp):
            assert AU.max_err(p, r) <= AU.STEPS * (0.5 * AU.ulp32(r.abs().max()) + 8 * 2.0 ** -24 * AU.LR)
    with pytest.raises(ValueError, match='does not match'):
        HipKerasAdam([torch.nn.Parameter(torch.zeros(3, device=dev))]).load_state_dict({'t': 1, 'm': [torch.zeros(4)], 'v': [torch.zeros(4)]})


def test_entry_refuses_what_it_cannot_run(dev):
    p = torch.zeros(8, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.UdsError, match='workspace'):
        _lib.adam_step([p], [p.clone()], [p.clone()], [p.clone()], state, torch.zeros(1, device=dev))
    with pytest.raises(_lib.UdsError, match='beta_1'):
        _lib.adam_step([p], [p.clone()], [p.clone()], [p.clone()], state, torch.zeros(2, device=dev), beta_1=1.5)
    with pytest.raises(_lib.UdsError, match='gradient'):
        _lib.adam_step([p], [torch.zeros(7, device=dev)], [p.clone()], [p.clone()], state, torch.zeros(2, device=dev))
    assert _lib.adam_workspace_floats([1, _lib.ADAM_SPAN, _lib.ADAM_SPAN + 1, 0]) == 2 * 4
    # no tensor has a gradient: the step still counts (KerasAdam.step)
    opt = HipKerasAdam([torch.nn.Parameter(p)])
    opt.step()
    assert opt.t == 1 and not bool(p.any())
