"""uds_mpc_objective / uds_mpc_objective_backward on the MI355X against the fp64 restatement of tests/mpc_util.py (which
tests/test_mpc_solver_math.py holds to `mpc.objective_pred`).

Bounds, from the kernels' stated order (csrc/kernels_mpc.hpp), not from what they return: the objective sums in fp64 and rounds
once, D = 2: |obj - ref| <= 2 * 2^-24 * sum|term| per candidate; an element of d_preds is its contributions summed in fp64 and
rounded once, held here to the 4 * 2^-24 * sum|contribution| the interface promises, and exactly 0 where no weight reaches.
Every input value is an fp32 number; operands and outputs sit in NaN-filled buffers whose guards must survive, and every output
element must have been written.  Shapes: pop 1, 3, 257 (more workgroups than a wave has lanes), T 1, 2, 7, N 30 (under one
stride of 256 threads) and 443 (a ragged second stride), C 2 (q_w and q_in are ONE channel) and 5."""
import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from gnn_uds_amd import autograd as AG
from tests import mpc_util as MU
from tests.window_util import guards_intact, nan_view

pytestmark = pytest.mark.gpu
D = 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _inputs(pop, T, N, C):
    rng = np.random.default_rng(1000 * pop + 100 * T + N + C)
    preds = MU.f32_exact(rng.uniform(-1, 1, (pop, T, N, C)))
    q0 = MU.f32_exact(rng.uniform(-1, 1, (pop, N)))
    w = {}
    for k, name in enumerate(('flood', 'out', 'smooth')):
        idx = rng.choice(N, 9, replace=True)                      # a few nodes, some twice, node 5 in every list
        w[name] = MU.f32_exact(MU.dense_weights(N, np.concatenate([idx, [5]]), rng.uniform(0.1, 2.0, 10)))
    smooth_nodes = np.nonzero(w['smooth'])[0]
    if T > 1:
        preds[:, 1, smooth_nodes[0], 1] = preds[:, 0, smooth_nodes[0], 1]      # q_in[t] == q_in[t-1]: the sub-gradient is 0
    preds[0, 0, smooth_nodes[-1], 1] = q0[0, smooth_nodes[-1]]                  # ... and against the history step
    gamma = MU.f32_exact(0.95 ** np.arange(T))
    g = MU.f32_exact(rng.uniform(0.5, 1.5, pop))
    return preds, q0, w, gamma, g


@pytest.mark.parametrize('C', [2, 5])
@pytest.mark.parametrize('N', [30, 443])
@pytest.mark.parametrize('T', [1, 2, 7])
@pytest.mark.parametrize('pop', [1, 3, 257])
def test_objective_and_backward(dev, pop, T, N, C):
    preds, q0, w, gamma, g = _inputs(pop, T, N, C)
    up = lambda a: None if a is None else nan_view(torch.as_tensor(a, dtype=torch.float32), dev)[0]
    preds_d, g_d = up(preds), up(g)
    worst = [0.0, 0.0]
    for batched in (False, True):
        q0_case = q0 if batched else q0[0]
        q0_d = up(q0_case)
        for absent in ((None, 'smooth') if batched else (None, 'flood', 'out', 'smooth', 'gamma')):
            wf, wo, ws = (None if absent == k else w[k] for k in ('flood', 'out', 'smooth'))
            gam = None if absent == 'gamma' else gamma
            ops = [up(wf), up(wo), up(ws), up(gam)]
            ref, mag = MU.objective_ref(preds, q0_case, wf, wo, ws, gam)
            dref, dmag = MU.objective_grad_ref(preds, q0_case, g, wf, wo, ws, gam)
            nan = float('nan')
            obj, obj_parent = nan_view(torch.full((pop,), nan, device=dev))
            dp, dp_parent = nan_view(torch.full(preds.shape, nan, device=dev))
            _lib.mpc_objective(preds_d, q0_d, *ops, out=obj)
            _lib.mpc_objective_backward(preds_d, q0_d, g_d, *ops, out=dp)
            tag = (batched, absent)
            assert guards_intact(obj_parent, pop) and guards_intact(dp_parent, dp.numel()), tag
            assert bool(torch.isfinite(obj).all()) and bool(torch.isfinite(dp).all()), tag      # every element written, nothing read outside
            err = np.abs(obj.double().cpu().numpy() - ref)
            assert (err <= D * MU.U24 * mag).all(), (tag, float((err / (MU.U24 * mag)).max()))
            derr = np.abs(dp.double().cpu().numpy() - dref)
            assert (derr <= 4 * MU.U24 * dmag).all(), (tag, float(derr.max()))
            assert (dp.cpu().numpy()[dmag == 0] == 0).all(), tag                                # exactly 0 where no weight reaches
            worst = [max(worst[0], float((err / (MU.U24 * mag)).max())), max(worst[1], float((derr / np.maximum(MU.U24 * dmag, 1e-300)).max()))]
            again, dagain = _lib.mpc_objective(preds_d, q0_d, *ops), _lib.mpc_objective_backward(preds_d, q0_d, g_d, *ops)
            assert torch.equal(again, obj) and torch.equal(dagain, dp), tag                     # a second call: the same bits
    print('pop %d T %d N %d C %d: objective error %.3f, gradient error %.3f (units of 2^-24 of the magnitude sums)' % (pop, T, N, C, *worst))


def test_function_differentiates_in_preds_only(dev):
    preds, q0, w, gamma, g = _inputs(3, 2, 30, 5)
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=dev)
    p = t(preds).requires_grad_(True)
    obj = AG.MpcObjectiveFn.apply(p, t(q0[0]), t(w['flood']), t(w['out']), t(w['smooth']), t(gamma))
    (grad,) = torch.autograd.grad((obj * t(g)).sum(), p)
    dref, dmag = MU.objective_grad_ref(preds, q0[0], g, w['flood'], w['out'], w['smooth'], gamma)
    assert (np.abs(grad.double().cpu().numpy() - dref) <= 4 * MU.U24 * dmag).all()
    assert torch.equal(obj, _lib.mpc_objective(t(preds), t(q0[0]), t(w['flood']), t(w['out']), t(w['smooth']), t(gamma)))


def test_empty_population_launches_nothing(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    assert tuple(_lib.mpc_objective(z(0, 2, 30, 5), z(30), z(30)).shape) == (0,)
    assert tuple(_lib.mpc_objective_backward(z(0, 2, 30, 5), z(30), z(0), z(30)).shape) == (0, 2, 30, 5)
