"""`Emulator.graphed_fit`: a `fit_eval` step as ONE replay of a captured HIP graph (forward, tail, backward, `HipKerasAdam`) against
the eager step with the same optimizer class, on astlingen (tests/golden/networks.json) built as tools/fit_tail_time.py builds it:
actuated GAT, rated pumps, node pumps, offsets, tide, flood channel; embed 64, 2 + 2 spatial layers, T = 5, batch 2.

The graph launches the kernels the eager step launches, in the same order, on the same operands: losses, EVERY parameter, both
optimizer slots and the step count are compared with torch.equal -- no tensor is excepted (the library GEMM of the 'library'
weight-gradient route picks the same kernel under capture on this stack)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd.emulator import HipKerasAdam, KerasAdam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def build(dev, recurrent='Conv1D', conv='GAT', **over):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))['astlingen']
    edges, n, outfall = np.asarray(net['edges']), net['n_node'], np.asarray(net['is_outfall'], dtype=float)
    e = len(edges)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv=conv, resnet=True, recurrent=recurrent, roll=0, model_dir=None, tide=True,
        is_outfall=outfall, hmax=1.0 + rng.random(n), hmin=np.zeros(n), area=0.2 + rng.random(n), learning_rate=1e-3,
        pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
        offset=rng.random(e) * (rng.random(e) > 0.5), ehmax=0.3 + rng.random(e))
    for k, v in over.items():
        setattr(args, k, v)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, 4))
    return emul, n, e


def batch(emul, n, e, dev, seed, B=2):
    """(x, a, b, y, ex, ey) of one step: seq_in steps in, seq_out * max(roll, 1) steps out."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    To = T * max(emul.roll, 1)
    x, a, b, ex = r(B, T, n, 5), 0.1 + 0.9 * r(B, To, 2), r(B, To, n, emul.b_in) * 0.1, r(B, T, e, 4)
    y, ey = r(B, To, n, 5), r(B, To, e, 3)
    y[..., -2] = (y[..., -2] > 0.7).float()
    return x, a, b, y, ex, ey


def pair(dev, flags=(), scale=None, **over):
    """(graphed model, eager model with a HipKerasAdam of its own, n, e): same seed, same parameters (times `scale`)."""
    g, n, e = build(dev, **over)
    r, _, _ = build(dev, **over)
    for m in (g, r):
        for f in flags:
            setattr(m, f, True)
        if scale is not None:
            with torch.no_grad():
                for p in m.parameters():
                    p.mul_(scale)
    g.graphed_fit = True
    r._optimizer = HipKerasAdam([p for p in r.parameters()], r.learning_rate, clipnorm=1.0)
    assert all(torch.equal(a, b) for a, b in zip(g.parameters(), r.parameters()))
    return g, r, n, e


def same_model(g, r):
    for (name, a), b in zip(g.named_parameters(), r.parameters()):
        assert torch.equal(a, b), name
    og, orr = g._optimizer, r._optimizer
    assert isinstance(og, HipKerasAdam) and og.t == orr.t
    for k, (a, b) in enumerate(zip(og.m + og.v, orr.m + orr.v)):
        assert torch.equal(a, b), 'slot %d' % k


def same_losses(a, b):
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b)), (a, b)


VARIANTS = {
    'conv1d': dict(),
    'gru': dict(recurrent='GRU'),
    'gcn': dict(conv='GCN'),
    # (DiffusionConv sums its input channels: at the initialisers' scale every head of this model saturates and all gradients are 0)
    'diffusion': dict(conv='Diffusion', scale=0.1),
    'use_adj': dict(use_adj=True),
    'roll2': dict(roll=2, tide=False),                 # (the fed-back window holds one boundary channel: no tide)
    'gradnorm': dict(gradnorm=True),
    'dense_node_edge': dict(flags=('dense_node_edge_train',)),
}


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_three_graphed_steps_and_an_evaluation_equal_eager(dev, variant):
    g, r, n, e = pair(dev, **VARIANTS[variant])
    paths, ini = [], None
    start = [p.detach().clone() for p in g.parameters()]
    for step in range(3):
        bt = batch(g, n, e, dev, 10 + step)
        lg, lr = g.fit_eval(*bt), r.fit_eval(*bt)
        paths.append(g.last_fit_path)
        same_losses(lg, lr)
        assert r.last_fit_path == 'eager' and g.last_fit_refusal is None
        if variant == 'gradnorm':                      # the task weights move between steps: the graph reads their storage
            ini = ini or [float(v) for v in lr]
            same_losses([g.fit_grad_norm(*bt, ini)], [r.fit_grad_norm(*bt, ini)])
            assert torch.equal(g._alpha, r._alpha) and not torch.equal(g._alpha, torch.ones_like(g._alpha))
    assert paths == ['graph-capture', 'graph', 'graph']
    same_model(g, r)
    moved = max(float((p - q).abs().max()) for p, q in zip(g.parameters(), start))
    assert moved > 1e-3                                # three Adam steps of 1e-3 each did happen
    before = [p.detach().clone() for p in g.parameters()]
    bt = batch(g, n, e, dev, 20)
    same_losses(g.fit_eval(*bt, fit=False), r.fit_eval(*bt, fit=False))
    assert g.last_fit_path == 'graph-capture'
    same_losses(g.fit_eval(*bt, fit=False), r.fit_eval(*bt, fit=False))
    assert g.last_fit_path == 'graph'
    assert all(torch.equal(a, b) for a, b in zip(before, g.parameters())) and g._optimizer.t == 3
    same_model(g, r)


def test_eager_inference_after_graphed_training_packs_the_new_weights(dev):
    g, r, n, e = pair(dev)
    bt = batch(g, n, e, dev, 30)
    with torch.no_grad():
        g.forward(bt[0], bt[2], bt[4], g.get_edge_action(bt[1], True))      # packs of the initial weights are cached
    for step in range(2):
        g.fit_eval(*batch(g, n, e, dev, 31 + step))
    fresh, _, _ = build(dev)
    fresh.load_state_dict(g.state_dict())
    x, a, b, _, ex, _ = bt
    with torch.no_grad():
        for u, v in zip(g.forward(x, b, ex, g.get_edge_action(a, True)), fresh.forward(x, b, ex, fresh.get_edge_action(a, True))):
            assert torch.equal(u, v)
        for u, v in zip(g.predict_tf(x, b, a, ex), fresh.predict_tf(x, b, a, ex)):
            assert torch.equal(u, v)


def test_shape_changes_reuse_and_eviction(dev):
    g, r, n, e = pair(dev)
    paths = []
    for k, B in enumerate((2, 3, 2)):
        bt = batch(g, n, e, dev, 40 + k, B)
        same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
        paths.append(g.last_fit_path)
    assert paths == ['graph-capture', 'graph-capture', 'graph'] and len(g._fit_graphs) == 2
    for k, B in enumerate((2, 3)):                     # keys three and four: the evaluation graphs
        bt = batch(g, n, e, dev, 50 + k, B)
        same_losses(g.fit_eval(*bt, fit=False), r.fit_eval(*bt, fit=False))
        assert g.last_fit_path == 'graph-capture'
    assert len(g._fit_graphs) == g.FIT_GRAPHS == 4
    bt = batch(g, n, e, dev, 60, 1)                    # a fifth key: the least recently used (training, batch 3) goes
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    assert g.last_fit_path == 'graph-capture' and len(g._fit_graphs) == 4
    bt = batch(g, n, e, dev, 61, 2)
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    assert g.last_fit_path == 'graph'                  # training at batch 2 was used after batch 3: kept
    bt = batch(g, n, e, dev, 62, 3)
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    assert g.last_fit_path == 'graph-capture'
    same_model(g, r)
    g.drop_fit_graphs()
    assert len(g._fit_graphs) == 0
    g.graphed_fit = False
    assert isinstance(g._optimizer, KerasAdam) and g._optimizer.t == r._optimizer.t
    g.graphed_fit = True
    assert isinstance(g._optimizer, HipKerasAdam)
    bt = batch(g, n, e, dev, 63, 2)
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    same_model(g, r)


def test_parameters_overwritten_in_place_are_honoured_by_the_next_replay(dev):
    g, r, n, e = pair(dev)
    for step in range(2):
        bt = batch(g, n, e, dev, 70 + step)
        same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    sd = {k: (v * 0.9 + 0.01).clone() for k, v in g.state_dict().items()}
    g.load_state_dict(sd)
    r.load_state_dict(sd)
    bt = batch(g, n, e, dev, 72)
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    assert g.last_fit_path == 'graph'
    same_model(g, r)


def test_a_nan_target_raises_updates_nothing_and_the_graph_stays_usable(dev):
    g, r, n, e = pair(dev)
    bt = batch(g, n, e, dev, 80)
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    before = [p.detach().clone() for p in g.parameters()] + [t.clone() for t in g._optimizer.m + g._optimizer.v]
    bad = list(batch(g, n, e, dev, 81))
    bad[3] = bad[3].clone()
    bad[3][0, 0, 0, 0] = float('nan')
    for m in (g, r):
        with pytest.raises(FloatingPointError, match='Loss contains NaN or Inf values.'):
            m.fit_eval(*bad)
    assert g.last_fit_path == 'graph' and g._optimizer.t == 1
    assert all(torch.equal(a, b) for a, b in zip(before, [p for p in g.parameters()] + g._optimizer.m + g._optimizer.v))
    bt = batch(g, n, e, dev, 82)
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    assert g.last_fit_path == 'graph' and g._optimizer.t == 2
    same_model(g, r)


def test_dropout_is_refused_and_runs_the_eager_step(dev):
    g, r, n, e = pair(dev, dropout=0.1)
    for step in range(2):
        bt = batch(g, n, e, dev, 90 + step)
        same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
        assert g.last_fit_path == 'eager' and 'dropout' in g.last_fit_refusal and g.fit_graph_refusal() == g.last_fit_refusal
    assert not getattr(g, '_fit_graphs', None)
    same_model(g, r)


def test_flag_off_builds_no_graph_and_no_hip_adam(dev):
    m, n, e = build(dev)
    assert m.graphed_fit is False
    m.fit_eval(*batch(m, n, e, dev, 95))
    m.fit_eval(*batch(m, n, e, dev, 96), fit=False)
    assert type(m._optimizer) is KerasAdam and not getattr(m, '_fit_graphs', None) and m.last_fit_path == 'eager' and m.last_fit_refusal is None
