"""`mpc.Problem` on the MI355X, on the model of tests/test_gpu_train.py::test_mpc_objective_and_gradient (astlingen, seq_in 4,
seq_out 2, one spatial layer, if_flood 1; one and two chunks, and the use_adj variant of tests/test_gpu_use_adj_train.py):
the shared-history evaluation against autograd over the fp64 oracle with that test's own bounds (objective 2e-5 relative to
max(1, max|ref|), gradient 2e-3 max|grad|), `predict` against `predict_horizon` on replicated inputs, the route records, and the
two solvers against their restated rules (tests/mpc_util.py)."""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import mpc as M
from oracle import emulator_ref as OE
from tests import mpc_util as MU
from tests.util import close, emulator_args, emulator_norms, load_emulator

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


class Case:
    """Model, inputs, oracle objective and gradient of one variant, computed once and left unchanged."""

    def __init__(self, networks, dev, chunks, use_adj):
        net = networks['astlingen']
        edges, n = np.array(net['edges']), net['n_node']
        over = dict(use_adj=True, act_edges=edges[::2]) if use_adj else {}
        self.args = args = emulator_args(edges, n, seq_in=4, seq_out=2, n_sp_layer=1, if_flood=1, epsilon=0.0, **over)
        self.norms = norms = emulator_norms(args)
        self.params = params = OE.init_params(args, seed=3)
        c = OE.config(args)
        g = torch.Generator().manual_seed(11)
        T = c.seq_out * chunks
        state, runoff, edge_state = rnd(g, c.seq_in, n, 5), rnd(g, T, n, 1) * 0.05, rnd(g, c.seq_in, len(edges), 4)
        state[..., 3] = (state[..., 3] > 0.8).double()
        self.pop, self.n_step, self.n_act, self.r_step = 3, chunks, len(args.act_edges), 2
        if use_adj:                            # decision values on both sides of 1, none within 1e-3 of an integer (the adjacency flips there)
            y = 0.3 + 1.2 * rnd(g, self.pop, self.n_step * self.n_act)
            y = torch.where((y - y.round()).abs() < 1e-3, y + 3e-3, y)
        else:
            y = 0.2 + 0.6 * rnd(g, self.pop, self.n_step * self.n_act)
        tg = dict(flood_idx=torch.tensor([3, 7, 11]), flood_w=torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64),
                  outflow_idx=torch.tensor([0]), outflow_w=torch.tensor([0.3], dtype=torch.float64),
                  smooth_idx=torch.tensor([5, 9]), smooth_w=torch.tensor([0.7, 0.2], dtype=torch.float64))
        gamma = torch.tensor([1.0, 0.9, 0.8, 0.7][:T], dtype=torch.float64)
        fwd = OE.forward
        if use_adj:
            idx = torch.as_tensor(OE._act_edge_index(c))

            def forward_with_adj(args_, params_, X, B, E, AE=None, ADJ=None):
                # the settings are the actuated links' column of the edge action; ADJ is piecewise constant in them (no gradient)
                return fwd(args_, params_, X, B, E, AE, OE.get_adj_action(c, AE[..., idx, 0].detach()) if ADJ is None else ADJ)
            OE.forward = forward_with_adj
        try:
            yr = y.clone().requires_grad_(True)
            self.ref = OE.mpc_objective(args, params, norms, yr, state, runoff, edge_state, self.n_step, self.n_act, self.r_step, tg, gamma)
            (self.gref,) = torch.autograd.grad(self.ref.sum(), yr)
            self.ref = self.ref.detach()
        finally:
            OE.forward = fwd
        self.emul = emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), params, dev)
        emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
        f = self.f = lambda t: t.float().to(dev)
        self.y, self.state, self.runoff, self.edge_state, self.gamma = f(y), f(state), f(runoff), f(edge_state), f(gamma)
        self.targets = {k: (v.to(dev) if v.dtype == torch.int64 else f(v)) for k, v in tg.items()}

    def problem(self, **kw):
        return U.Problem(self.emul, self.state, self.runoff, self.edge_state, self.n_step, self.n_act, self.r_step, self.targets, self.gamma, **kw)


VARIANTS = {'one-chunk': (1, False), 'two-chunks': (2, False), 'use-adj': (1, True)}
_CASES = {}


@pytest.fixture(params=sorted(VARIANTS))
def case(request, networks, dev):
    if request.param not in _CASES:
        _CASES[request.param] = Case(networks, dev, *VARIANTS[request.param])
    return _CASES[request.param]


def test_objective_and_gradient_against_the_oracle(case):
    p = case.problem()
    obj, grad = p.objective_and_gradient(case.y)
    assert p.last_paths == {'prefix': 'shared', 'objective': 'hip'} and case.emul.last_prefix_batch == 1
    assert tuple(obj.shape) == (case.pop,) and tuple(grad.shape) == tuple(case.y.shape)
    print('objective error %.3e' % close(obj, case.ref, 2e-5))
    gmax = float(case.gref.abs().max())
    assert gmax > 0
    err = float((grad.double().cpu() - case.gref).abs().max())
    print('gradient error %.3e of max|grad| %.3e' % (err, gmax))
    assert err <= 2e-3 * gmax, 'gradient err %.3e vs max|grad| %.3e' % (err, gmax)
    close(p.objective(case.y), case.ref, 2e-5)                                     # the no-grad evaluation
    # every switch off: the replicated prefix and the tensor objective, the same numbers to the same bounds
    q = case.problem(shared_history=False, fused_objective=False)
    obj2, grad2 = q.objective_and_gradient(case.y)
    assert q.last_paths == {'prefix': 'replicated', 'objective': 'torch'} and case.emul.last_prefix_batch == case.pop
    close(obj2, case.ref, 2e-5)
    assert float((grad2.double().cpu() - case.gref).abs().max()) <= 2e-3 * gmax


def test_predict_against_the_replicated_path(case):
    p = case.problem()
    with torch.no_grad():
        preds, edge_preds = p.predict(case.y)
        settings = M.expand_settings(case.y, case.n_step, case.n_act, case.r_step, case.runoff.shape[0])
        rep = lambda t: t.unsqueeze(0).expand((case.pop,) + tuple(t.shape)).contiguous()
        want, edge_want = M.predict_horizon(case.emul, settings, rep(case.state), rep(case.runoff), rep(case.edge_state))
    assert p.last_paths['prefix'] == 'shared'
    close(preds, want.double().cpu(), 2e-5)
    close(edge_preds, edge_want.double().cpu(), 2e-5)


def test_predict_tf_shared_is_predict_tf_on_replicated_inputs(case):
    em, so = case.emul, case.emul.seq_out
    settings = M.expand_settings(case.y, case.n_step, case.n_act, case.r_step, case.runoff.shape[0])[:, :so]
    rep = lambda t: t.unsqueeze(0).expand((case.pop,) + tuple(t.shape)).contiguous()
    with torch.no_grad():
        y1, e1 = em.predict_tf_shared(case.state, case.runoff[:so], settings, case.edge_state)
        assert em.last_prefix_batch == 1 and em.last_tail_path == 'hip'
        y2, e2 = em.predict_tf(rep(case.state), rep(case.runoff[:so]), settings, rep(case.edge_state))
        assert em.last_prefix_batch == case.pop
        # the two halves compose to the forward, bit for bit at one batch size
        X, E = em.normalize(rep(case.state), 'x'), em.normalize(rep(case.edge_state), 'e')
        B, AE = em.normalize(rep(case.runoff[:so]), 'b'), em.get_edge_action(settings, True)
        ADJ = em.get_adj_action(settings, True) if em.use_adj else None
        whole = em.forward(X, B, E, AE, ADJ)
        halves = em.decode(em.encode_history(X, E), B, AE, ADJ)
    close(y1, y2.double().cpu(), 2e-5)
    close(e1, e2.double().cpu(), 2e-5)
    assert torch.equal(whole[0], halves[0]) and torch.equal(whole[1], halves[1])


def test_solve_ce(case):
    p = case.problem()
    a = p.solve_ce(pop=16, iters=4, n_elite=4, seed=5)
    b = p.solve_ce(pop=16, iters=4, n_elite=4, seed=5)
    assert all(torch.equal(s, t) for s, t in zip(a, b))                            # the same seed: the same bits
    assert p.last_paths == {'prefix': 'shared', 'objective': 'hip'}
    h = a.history.cpu().numpy()
    assert h.shape == (4,) and (np.diff(h) <= 0).all() and float(a.obj) == h[-1]
    assert tuple(a.y.shape) == (p.n_var,) and 0 <= float(a.y.min()) and float(a.y.max()) <= 1
    close(p.objective(a.y[None]), a.obj.double().cpu(), 2e-5)                      # best_y is the candidate best_obj belongs to
    # iteration 1, restated: the drawn population, its objectives as the device computed them, the update rule
    mean0, std0 = torch.full((p.n_var,), 0.5, device=a.y.device), torch.full((p.n_var,), 0.3, device=a.y.device)
    first = _lib.ce_draw(mean0, std0, 5, torch.zeros(1, dtype=torch.int64, device=a.y.device), 16)
    ref_y, _ = MU.ce_draw_ref(mean0.cpu().numpy(), std0.cpu().numpy(), 5, 0, 16)
    assert np.abs(first.double().cpu().numpy() - ref_y).max() <= 1e-5
    obj = p.objective(first)
    assert float(obj.min()) == h[0]
    one = p.solve_ce(pop=16, iters=1, n_elite=4, seed=5)
    mean, std = (t.double().cpu().numpy() for t in p.ce_state)
    ref = MU.ce_update_ref(first.double().cpu().numpy(), obj.double().cpu().numpy(), 4, 0.3, 1e-3, mean0.cpu().numpy(), std0.cpu().numpy(),
                           np.zeros(p.n_var), float('inf'))
    assert np.abs(mean - ref['mean']).max() <= MU.CE_MEAN_BOUND
    assert (np.abs(std - ref['std']) <= MU.ce_std_bound(first.double().cpu().numpy(), ref['elites'])).all()
    assert float(one.obj) == ref['best_obj'] and (one.y.double().cpu().numpy() == ref['best_y']).all()


def test_solve_gr(case):
    p = case.problem()
    y0 = case.y.clamp(0.05, 0.95)
    obj0, g = p.objective_and_gradient(y0)
    lr, b1, b2, eps = 0.05, 0.9, 0.999, 1e-7
    one = p.solve_gr(y0, 1, lr=lr)
    m, v = (1 - b1) * g.double(), (1 - b2) * g.double() ** 2
    want = (y0.double() - lr * (1 - b2) ** 0.5 / (1 - b1) * m / (v.sqrt() + eps)).clamp(0, 1)
    close(one.y, want.cpu(), 1e-6)                                                 # the Adam formula on objective_and_gradient(y0)
    assert float(one.history[0]) == float(obj0.min()) and tuple(one.obj.shape) == (case.pop,)
    res = p.solve_gr(y0, 5, lr=0.3)                                                # large steps: the projection is what keeps y in the box
    assert 0 <= float(res.y.min()) and float(res.y.max()) <= 1 and bool(torch.isfinite(res.obj).all())
    h = res.history.cpu().numpy()
    assert h.shape == (5,) and (np.diff(h) <= 0).all() and h[0] == float(obj0.min())
