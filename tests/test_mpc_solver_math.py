"""`mpc.Problem` without a device: the fp64 restatements of tests/mpc_util.py (the objective, the cross-entropy draw and update,
which the GPU tests hold the kernels to) against what they restate -- `mpc.objective_pred` with autograd on fp64 CPU tensors --
and against known answers; `Problem`'s export, its dense weights, its torch routes on CPU tensors and its argument errors."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import mpc as M
from tests import mpc_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the objective -----------------------------------------------------------------------------------------------------------
def _objective_case(seed, pop=3, T=4, N=12, C=5, q0_batched=False):
    rng = np.random.default_rng(seed)
    preds = rng.uniform(-1, 1, (pop, T, N, C))
    preds[:, 2, 5, 1] = preds[:, 1, 5, 1]                      # a step with q_in[t] == q_in[t-1] at a smoothed node
    q0 = rng.uniform(-1, 1, (pop, N) if q0_batched else (N,))
    preds[0, 0, 7, 1] = q0[0, 7] if q0_batched else q0[7]      # ... and one against the history step
    return preds, q0


TARGET_CASES = {
    'all-three-lists': dict(flood_idx=[3, 7, 11], flood_w=[1.0, 2.0, 0.5], outflow_idx=[0], outflow_w=[0.3], smooth_idx=[5, 7], smooth_w=[0.7, 0.2]),
    'duplicate-indices': dict(flood_idx=[3, 3, 11, 3], flood_w=[1.0, 2.0, 0.5, -0.25], outflow_idx=[0, 0], outflow_w=[0.3, 0.1], smooth_idx=[5, 5, 7],
                              smooth_w=[0.7, 0.2, 0.4]),
    'one-node-in-all-lists': dict(flood_idx=[5, 2], flood_w=[1.5, 1.0], outflow_idx=[5], outflow_w=[0.3], smooth_idx=[5, 7], smooth_w=[0.7, 0.1]),
    'no-outflow': dict(flood_idx=[3, 7], flood_w=[1.0, 2.0], outflow_idx=[], outflow_w=[], smooth_idx=[5, 7], smooth_w=[0.7, 0.2]),
    'no-smooth': dict(flood_idx=[3, 7], flood_w=[1.0, 2.0], outflow_idx=[0], outflow_w=[0.3], smooth_idx=None, smooth_w=None),
    'flood-only': dict(flood_idx=[3, 7], flood_w=[1.0, 2.0]),
}


@pytest.mark.parametrize('gamma', [None, [1.0, 0.9, 0.8, 0.7]], ids=['no-gamma', 'gamma'])
@pytest.mark.parametrize('q0_batched', [False, True], ids=['q0-shared', 'q0-per-candidate'])
@pytest.mark.parametrize('name', sorted(TARGET_CASES))
def test_objective_restatement_is_objective_pred(name, q0_batched, gamma):
    tg = TARGET_CASES[name]
    preds, q0 = _objective_case(1, q0_batched=q0_batched)
    pop, T, N, C = preds.shape
    w = {k: MU.dense_weights(N, tg.get(k + '_idx'), tg.get(k + '_w')) for k in ('flood', 'outflow', 'smooth')}
    obj, mag = MU.objective_ref(preds, q0, w['flood'], w['outflow'], w['smooth'], gamma)
    g = np.linspace(0.5, 1.5, pop)
    d, dmag = MU.objective_grad_ref(preds, q0, g, w['flood'], w['outflow'], w['smooth'], gamma)
    # what it restates: objective_pred on fp64 tensors; q_in0 is channel 1 of the last history step
    pt = torch.tensor(preds, requires_grad=True)
    state = torch.zeros(pop, 2, N, C, dtype=torch.float64)
    state[:, -1, :, 1] = torch.as_tensor(q0)
    tt = {k: (None if v is None else torch.tensor(v, dtype=torch.int64 if k.endswith('idx') else torch.float64)) for k, v in tg.items()}
    ref = M.objective_pred(pt, state, gamma=None if gamma is None else torch.tensor(gamma, dtype=torch.float64), **tt)
    (gref,) = torch.autograd.grad((ref * torch.as_tensor(g)).sum(), pt)
    assert np.abs(obj - ref.detach().numpy()).max() <= 1e-13 * max(1.0, mag.max())
    assert np.abs(d - gref.numpy()).max() <= 1e-13 * max(1.0, dmag.max())
    assert (mag >= np.abs(obj) - 1e-12).all() and (dmag >= np.abs(d) - 1e-12).all()
    # no weight reaches: exactly zero, and the tie steps carry no smooth gradient of their own
    reached = np.zeros((N, C), dtype=bool)
    for key, ch in (('flood', C - 1), ('outflow', 1), ('smooth', 1)):
        if w[key] is not None:
            reached[w[key] != 0, ch] = True
    assert (d[:, :, ~reached] == 0).all() and (dmag[:, :, ~reached] == 0).all()


def test_subgradient_of_the_smooth_term_is_zero_at_a_tie():
    preds = np.zeros((1, 2, 3, 2))
    preds[0, :, 1, 1] = [0.25, 0.25]                             # q_in[0] == q_in0, q_in[1] == q_in[0]
    q0 = np.array([0.0, 0.25, 0.0])
    ws = np.array([0.0, 2.0, 0.0])
    obj, _ = MU.objective_ref(preds, q0, None, None, ws, None)
    d, _ = MU.objective_grad_ref(preds, q0, np.ones(1), None, None, ws, None)
    assert obj[0] == 0.0 and (d == 0).all()
    preds[0, 1, 1, 1] = 0.75                                     # one rising step: +w at t = 1, -w at t = 0
    d, mag = MU.objective_grad_ref(preds, q0, np.ones(1), None, None, ws, None)
    assert d[0, 1, 1, 1] == 2.0 and d[0, 0, 1, 1] == -2.0 and mag[0, 0, 1, 1] == 2.0


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def test_draw_restatement_is_a_stream_of_standard_normals():
    z = MU.ce_normals(seed=0x1234567890ABCDEF, j0=0, pop=512, n_var=64)
    assert np.isfinite(z).all() and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    # candidate j is a function of (seed, j) alone: two halves equal the whole, another seed differs
    a, b = MU.ce_normals(7, 0, 8, 5), MU.ce_normals(7, 8, 8, 5)
    assert (np.concatenate([a, b]) == MU.ce_normals(7, 0, 16, 5)).all()
    assert (MU.ce_normals(8, 0, 8, 5) != a).any()
    # the variable is the second counter word: columns of one candidate differ
    assert len(set(a[0].tolist())) == 5
    out, raw = MU.ce_draw_ref(np.array([0.02, 0.5, 0.98]), np.array([0.3, 0.0, 0.3]), 3, 0, 64)
    assert (out[:, 1] == 0.5).all() and (out[raw <= 0] == 0).all() and (out[raw >= 1] == 1).all()
    assert (raw[:, 0] < 0).any() and (raw[:, 2] > 1).any()


def test_uniforms_above_two_to_the_23_round_to_even():
    """k + 0.5 needs 25 bits from k = 2^23 on: fp32 rounds it to even, so u may reach 1 (z = 0) and never 0."""
    k = np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 1], dtype=np.uint32)
    u = (k.astype(np.float32) + np.float32(0.5)).astype(np.float64) * MU.U24
    assert u.tolist() == [0.5 * MU.U24, 1.5 * MU.U24, 0.5 - 0.5 * MU.U24, 0.5, 0.5 + 2 * MU.U24, 1.0]


# ---- ranking and update ------------------------------------------------------------------------------------------------------
NAN, INF = float('nan'), float('inf')


def test_ranking_known_answers():
    assert MU.ce_ranks([3.0, 1.0, 2.0]) == [2, 0, 1]
    assert MU.ce_ranks([1.0, 1.0, 0.5, 1.0]) == [1, 2, 0, 3]                      # ties: the lower index first
    assert MU.ce_ranks([0.0, -0.0, -1.0]) == [1, 2, 0]                            # -0 == +0: a tie
    assert MU.ce_ranks([NAN, 2.0, INF, -INF, 1.0]) == [2, 1, 3, 4, 0]             # every non-finite value is +inf, tied by index
    assert MU.ce_elites([NAN, 2.0, INF, -INF, 1.0], 5) == [4, 1]                  # rank < n_elite AND finite
    assert MU.ce_elites([NAN, 2.0, INF, -INF, 1.0], 1) == [4]
    assert MU.ce_elites([3.0, 1.0, 2.0], 3) == [1, 2, 0]                          # n_elite = pop
    assert MU.ce_elites([NAN, INF, -INF], 2) == []                                # K = 0


def test_update_known_answers():
    y = np.array([[0.0, 1.0], [0.5, 0.5], [1.0, 0.0], [0.25, 0.75]])
    obj = np.array([4.0, 1.0, NAN, 2.0])
    mean, std = np.array([0.5, 0.5]), np.array([0.3, 0.3])
    out = MU.ce_update_ref(y, obj, 2, 0.0, 1e-3, mean, std, np.zeros(2), INF)
    assert out['elites'] == [1, 3] and out['status'] == 0
    assert np.allclose(out['mean'], [0.375, 0.625]) and np.allclose(out['std'], [0.125, 0.125])      # ddof 0
    assert out['best_obj'] == 1.0 and out['best_y'].tolist() == [0.5, 0.5]
    keep = MU.ce_update_ref(y, obj, 2, 0.0, 1e-3, mean, std, np.array([0.1, 0.2]), 1.0)              # not STRICTLY lower: best stays
    assert keep['best_obj'] == 1.0 and keep['best_y'].tolist() == [0.1, 0.2]
    one = MU.ce_update_ref(y, obj, 1, 0.5, 0.2, mean, std, np.zeros(2), INF)                         # K = 1: s = 0, the floor holds
    assert np.allclose(one['mean'], [0.5, 0.5]) and np.allclose(one['std'], [0.2, 0.2])
    none = MU.ce_update_ref(y, np.array([NAN, INF, -INF, NAN]), 4, 0.3, 1e-3, mean, std, np.array([0.1, 0.2]), 7.0)
    assert none['status'] == 1 and none['elites'] == [] and none['best_obj'] == 7.0
    assert (none['mean'] == mean).all() and (none['std'] == std).all() and none['best_y'].tolist() == [0.1, 0.2]


def test_update_bounds_stay_below_the_limit():
    assert MU.CE_MEAN_BOUND <= 1e-5 and MU.CE_STD_BOUND <= 1e-5


# ---- Problem -----------------------------------------------------------------------------------------------------------------
def _model(**over):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))['astlingen']
    edges, n = np.asarray(net['edges']), net['n_node']
    e = len(edges)
    args = SimpleNamespace(state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=4, seq_out=2, embed_size=64, hidden_dim=64, n_sp_layer=1,
                           n_tp_layer=2, if_flood=1, edges=edges, graph=U.DrainageGraph.from_edges(edges, n), act=True, act_edges=edges[[1, 4]],
                           conv='GAT', resnet=True, recurrent='Conv1D')
    for k, v in over.items():
        setattr(args, k, v)
    return U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)), n, e


def _problem_args(n, e, T=4):
    g = torch.Generator().manual_seed(5)
    tg = dict(flood_idx=torch.tensor([3, 7, 3]), flood_w=torch.tensor([1.0, 2.0, 0.5]), outflow_idx=torch.tensor([0]), outflow_w=torch.tensor([0.3]),
              smooth_idx=torch.tensor([], dtype=torch.int64), smooth_w=torch.tensor([]))
    return dict(state=torch.rand(4, n, 5, generator=g), runoff=torch.rand(T, n, 1, generator=g), edge_state=torch.rand(4, e, 4, generator=g),
                n_step=2, n_act=2, r_step=2, targets=tg)


def test_problem_is_exported_and_builds_its_dense_weights_once():
    assert U.Problem is M.Problem and M.Result._fields == ('y', 'obj', 'history')
    emul, n, e = _model()
    p = U.Problem(emul, gamma=torch.tensor([1.0, 0.9, 0.8, 0.7]), **_problem_args(n, e))
    assert p.n_var == 4 and p.shared_history and p.fused_objective and p.last_paths == {'prefix': None, 'objective': None}
    want = np.zeros(n)
    want[3], want[7] = 1.5, 2.0                                   # the duplicate index summed
    assert p.weights['flood'].tolist() == want.tolist() and float(p.weights['outflow'][0]) == pytest.approx(0.3)
    assert p.weights['smooth'] is None                            # an empty list is an absent term
    for name in ('predict', 'objective', 'objective_and_gradient', 'solve_ce', 'solve_gr'):
        assert callable(getattr(p, name))
    for name in ('encode_history', 'decode', 'predict_tf_shared'):
        assert callable(getattr(emul, name))


def test_problem_refuses_bad_arguments_without_a_device():
    emul, n, e = _model()
    good = _problem_args(n, e)
    bad = lambda **over: U.Problem(emul, **dict(good, **over))
    with pytest.raises(ValueError, match='unbatched 3-d'):
        bad(state=good['state'].unsqueeze(0))
    with pytest.raises(ValueError, match='one network and one history'):
        bad(runoff=torch.rand(4, n + 1, 1))
    with pytest.raises(ValueError, match='one network and one history'):
        bad(edge_state=torch.rand(3, e, 4))
    with pytest.raises(ValueError, match='multiple of seq_out = 2'):
        bad(runoff=torch.rand(3, n, 1))
    for name in ('n_step', 'n_act', 'r_step'):
        with pytest.raises(ValueError, match=name):
            bad(**{name: 0})
    with pytest.raises(ValueError, match=r'gamma must be \(4,\)'):
        bad(gamma=torch.ones(3))
    with pytest.raises(ValueError, match="needs 'flood_idx'"):
        bad(targets={})
    with pytest.raises(ValueError, match='flood_idx and flood_w'):
        bad(targets=dict(flood_idx=torch.tensor([1, 2]), flood_w=torch.tensor([1.0])))
    with pytest.raises(ValueError, match=r'outflow_idx outside \[0, %d\)' % n):
        bad(targets=dict(good['targets'], outflow_idx=torch.tensor([n])))
    with pytest.raises(ValueError, match='flood_idx is empty'):
        bad(targets=dict(flood_idx=torch.tensor([], dtype=torch.int64), flood_w=torch.tensor([])))
    p = bad()
    with pytest.raises(ValueError, match=r'y must be \(pop, n_step \* n_act = 4\)'):
        p.predict(torch.rand(3, 5))
    with pytest.raises(ValueError, match='solve_ce: pop=1'):
        p.solve_ce(1, 2, 1)
    with pytest.raises(ValueError, match='n_elite=9'):
        p.solve_ce(8, 2, 9)
    with pytest.raises(ValueError, match='iters=0'):
        p.solve_ce(8, 0, 2)
    with pytest.raises(_lib.UdsError, match='device only'):
        p.solve_ce(8, 2, 2)                                       # a CPU problem: no solver without the device
    with pytest.raises(ValueError, match='iters=0'):
        p.solve_gr(torch.rand(3, 4), 0)


def test_the_split_forward_refuses_the_mlp_model():
    emul, n, e = _model(conv=False, seq_in=2, seq_out=2)
    with pytest.raises(NotImplementedError):
        emul.encode_history(torch.zeros(1, 2, n, 5), torch.zeros(1, 2, e, 4))
    with pytest.raises(NotImplementedError):
        emul.predict_tf_shared(torch.zeros(2, n, 5), torch.zeros(2, n, 1), torch.zeros(3, 2, 2), torch.zeros(2, e, 4))
