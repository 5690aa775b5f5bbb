"""`gnn_uds_amd.fit` and `emulate_event` on the model of tests/test_gpu_fit_graph.py (astlingen, actuated GAT, tide, if_flood = 3,
T = 5, batch 2) and seeded series of 3 events of 30 rows: the loop against a hand-written loop on a twin model that uses the draw
restated in Python integers, `batch_torch` and `fit_eval` -- every loss, every parameter and both Adam slots with torch.equal --
with `graphed_fit` off and on; the event emulation against `simulate` on `batch_torch` windows."""
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd.emulator import HipKerasAdam
from tests import window_util as WU

pytestmark = pytest.mark.gpu

L, BATCH, EPOCHS, SEED = [30, 30, 30], 2, 3, 77


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def store_for(emul, n, e, dev, tide=True):
    series = WU.make_series(21, L, n, e, n_act=2, tide=tide, wet=0.2)
    wet_rows = (series['flood'] > 0).any(1).mean()
    assert 0.1 < wet_rows < 0.35                                   # flood > 0 on about a fifth of the rows
    return series, U.WindowStore(series['states'], series['flood'], series['edge_states'], L, settings=series['settings'], tide=series['tide'],
                                 emul=emul, device=dev)


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
@pytest.mark.parametrize('variant', ['base', 'roll2'])
def test_fit_equals_a_hand_written_loop_on_a_twin(dev, graphed, variant):
    over = dict(roll=2, tide=False) if variant == 'roll2' else {}
    g, n, e = WU.build(dev, **over)
    r, _, _ = WU.build(dev, **over)
    if graphed:
        g.graphed_fit = True
        r._optimizer = HipKerasAdam([p for p in r.parameters()], r.learning_rate, clipnorm=1.0)
    series, store = store_for(g, n, e, dev, tide=not over)
    assert store.t_out == WU.T * (2 if over else 1) and store.if_flood == 3 and store.seq_in == WU.T
    train, test = store.table(events=[0, 1], flood_weight=4, seed=SEED), store.table(events=[2], interval=2, seed=SEED + 1)
    assert set(train.weights.tolist()) == ({4} if over else {1, 4})     # (ten output rows: every window of events 0 and 1 meets a flood)
    got = U.fit(g, train, test, epochs=EPOCHS, batch_size=BATCH)
    assert store.last_path == 'hip' and g.last_fit_path == ('graph' if graphed else 'eager') and g.last_fit_refusal is None
    assert train.count.item() == test.count.item() == EPOCHS * BATCH

    twin_store = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, settings=series['settings'], tide=series['tide'],
                               emul=r, device=dev)
    tables = {True: (train.starts.tolist(), train.weights.tolist(), SEED), False: (test.starts.tolist(), test.weights.tolist(), SEED + 1)}
    want = {True: [], False: []}
    for epoch in range(EPOCHS):
        for fit in (True, False):
            starts = WU.draw_ref(*tables[fit], epoch * BATCH, BATCH)
            bt = twin_store.batch_torch(torch.tensor(starts, dtype=torch.int32, device=dev))
            want[fit].append(torch.stack(r.fit_eval(*bt, fit=fit)))
    assert r.last_fit_path == 'eager'
    assert got['train_loss'].shape == got['test_loss'].shape == (EPOCHS, 3) and got['train_loss'].is_cuda
    assert torch.equal(got['train_loss'], torch.stack(want[True])) and torch.equal(got['test_loss'], torch.stack(want[False]))
    assert bool(torch.isfinite(got['train_loss']).all()) and not torch.equal(got['train_loss'][0], got['train_loss'][2])
    for (name, a), b in zip(g.named_parameters(), r.parameters()):
        assert torch.equal(a, b), name
    assert g._optimizer.t == r._optimizer.t == EPOCHS and type(g._optimizer) is type(r._optimizer)
    for k, (a, b) in enumerate(zip(g._optimizer.m + g._optimizer.v, r._optimizer.m + r._optimizer.v)):
        assert torch.equal(a, b), 'slot %d' % k


def test_fit_saves_every_save_gap_epochs_and_runs_gradnorm(dev, tmp_path):
    g, n, e = WU.build(dev, gradnorm=True)
    _, store = store_for(g, n, e, dev)
    assert g.model_dir is None
    with pytest.raises(ValueError, match='needs a model_dir'):                # refused before any training, not after save_gap epochs
        U.fit(g, store.table(seed=1), None, epochs=2, batch_size=BATCH, save_gap=2)
    assert g._optimizer is None
    out = U.fit(g, store.table(seed=1), None, epochs=2, batch_size=BATCH, save_gap=2, model_dir=str(tmp_path))
    assert out['test_loss'] is None and out['train_loss'].shape == (2, 3)
    assert (tmp_path / 'model.pt').exists() and (tmp_path / 'gradnorm.pt').exists()
    assert not torch.equal(g._alpha.detach(), torch.ones_like(g._alpha))      # fit_grad_norm ran


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
def test_gradnorm_fit_equals_a_hand_written_loop_on_a_twin(dev, graphed):
    """`fit_grad_norm` after every TRAINING step, on the training batch, with the first epoch's training losses as `ini_loss`: the
    task weights, the losses and the parameters equal those of the loop written out."""
    g, n, e = WU.build(dev, gradnorm=True)
    r, _, _ = WU.build(dev, gradnorm=True)
    if graphed:
        g.graphed_fit = True
        r._optimizer = HipKerasAdam([p for p in r.parameters()], r.learning_rate, clipnorm=1.0)
    series, store = store_for(g, n, e, dev)
    train, test = store.table(events=[0, 1], flood_weight=4, seed=SEED), store.table(events=[2], seed=SEED + 1)
    got = U.fit(g, train, test, epochs=EPOCHS, batch_size=BATCH)
    twin_store = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, settings=series['settings'], tide=series['tide'],
                               emul=r, device=dev)
    want, ini, alphas = {True: [], False: []}, None, []
    for epoch in range(EPOCHS):
        for fit, tb, seed in ((True, train, SEED), (False, test, SEED + 1)):
            starts = WU.draw_ref(tb.starts.tolist(), tb.weights.tolist(), seed, epoch * BATCH, BATCH)
            bt = twin_store.batch_torch(torch.tensor(starts, dtype=torch.int32, device=dev))
            losses = r.fit_eval(*bt, fit=fit)
            want[fit].append(torch.stack(losses))
            if fit:
                ini = ini or [float(v) for v in losses]
                r.fit_grad_norm(*bt, ini)
                alphas.append(r._alpha.detach().clone())
    assert torch.equal(got['train_loss'], torch.stack(want[True])) and torch.equal(got['test_loss'], torch.stack(want[False]))
    assert torch.equal(g._alpha, r._alpha) and not torch.equal(alphas[0], alphas[-1]) and not torch.equal(alphas[0], torch.ones_like(alphas[0]))
    for (name, a), b in zip(g.named_parameters(), r.parameters()):
        assert torch.equal(a, b), name
    for k, (a, b) in enumerate(zip(g._optimizer.m + g._optimizer.v, r._optimizer.m + r._optimizer.v)):
        assert torch.equal(a, b), 'slot %d' % k


@pytest.mark.parametrize('variant', ['base', 'roll2'])
def test_emulate_event_equals_simulate_on_batch_torch_windows(dev, variant):
    over = dict(roll=2, tide=False) if variant == 'roll2' else {}
    g, n, e = WU.build(dev, **over)
    _, store = store_for(g, n, e, dev, tide=not over)
    k = 1
    starts = store.event_windows(k)
    assert starts.tolist() == list(range(30, 30 + 30 - 2 * WU.T + 1))        # t_out = seq_out, whatever roll is
    x, a, b, y, ex, ey = store.batch_torch(starts, normalized=False, t_out=store.seq_out)
    with torch.no_grad():
        want_y, want_ey = g.simulate(x, b, a, ex)
    got = U.emulate_event(g, store, k)
    assert store.last_path == 'hip'
    for name, u, v in zip(('y_pred', 'ey_pred', 'y_true', 'ey_true'), got, (want_y, want_ey, y, ey)):
        assert u.shape == v.shape and torch.equal(u, v), name
    assert got[0].shape == (len(starts), WU.T, n, 5) and bool(torch.isfinite(got[0]).all())
    chunked = U.emulate_event(g, store, k, chunk=4)
    for name, u, v in zip(('y_pred', 'ey_pred', 'y_true', 'ey_true'), chunked, got):
        assert torch.equal(u, v), name
