"""`uds_window_batch` / `uds_window_draw` on the device against their definitions: `WindowStore.batch` (one HIP launch) against
`batch_torch` on a CPU copy of the store, bit for bit, with every series and every output a view inside a NaN-filled parent buffer;
NaN windows for starts outside the series; `WindowTable.draw` against the restatement in Python integers; both inside a captured
graph."""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from tests import window_util as WU

pytestmark = pytest.mark.gpu

NAMES = ('x', 'a', 'b', 'y', 'ex', 'ey')
SERIES = ('states', 'flood', 'edge_states', 'settings', 'tide')
SIZES = [(1, 1), (30, 29), (67, 131)]                  # one item, astlingen, odd and past one wave
# (if_flood, tide, settings, roll, (seq_in, seq_out), normalized): the grid of tests/test_window_plan.py, thinned -- every value of
# every flag occurs with both values of `normalized`
CASES = [(3, True, True, 0, (5, 5), True), (3, True, True, 0, (5, 5), False), (0, False, False, 0, (5, 5), True), (0, True, False, 2, (6, 2), True),
         (3, False, True, 2, (6, 2), False), (3, False, False, 0, (1, 1), True), (0, False, True, 0, (1, 1), False), (0, True, True, 2, (1, 1), True),
         (3, True, False, 2, (5, 5), False), (0, False, True, 0, (6, 2), True), (3, True, False, 0, (6, 2), True), (0, True, True, 0, (5, 5), False)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def stores(dev, size, if_flood, tide, settings, roll, seq, seed=11):
    """(CUDA store whose series are views in NaN-filled parents, the parents, CPU store of the same data, event_len)."""
    (N, E), (seq_in, seq_out) = size, seq
    t_out = seq_out * max(roll, 1)
    L = [seq_in + t_out, 17, 40]
    series = WU.make_series(seed, L, N, E, n_act=2 if settings else 0, tide=tide)
    norms = WU.make_norms(seed + 1, N, E)
    kw = dict(settings=series['settings'], tide=series['tide'], seq_in=seq_in, seq_out=seq_out, roll=roll, if_flood=if_flood)
    gpu = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, device=dev, **kw)
    cpu = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, device='cpu', **kw)
    parents = {}
    for name in SERIES:
        if getattr(gpu, name) is not None:
            view, parents[name] = WU.nan_view(getattr(gpu, name))
            setattr(gpu, name, view)
    for s in (gpu, cpu):
        s.set_norm(*norms)
    return gpu, parents, cpu, L


def guarded_outputs(store, B, t_out, dev):
    cx, cb = store.cx, store.cb
    shapes = ((B, store.seq_in, store.N, cx), (B, t_out, store.n_act), (B, t_out, store.N, cb), (B, t_out, store.N, cx),
              (B, store.seq_in, store.E, 4), (B, t_out, store.E, 3))
    pairs = [None if (name == 'a' and store.n_act == 0) else WU.nan_view(torch.zeros(s), dev) for name, s in zip(NAMES, shapes)]
    return tuple(None if p is None else p[0] for p in pairs), [None if p is None else p[1] for p in pairs]


def last_starts(L, rows):
    """each event's LAST valid window (the final one reads the store's last row), first window first"""
    ends = np.cumsum(L)
    return [int(e - rows) for e in ends]


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('case', CASES, ids=['flood%d-tide%d-act%d-roll%d-%dx%d-norm%d' % (f, t, a, r, s[0], s[1], n) for f, t, a, r, s, n in CASES])
def test_batch_equals_batch_torch_inside_guards(dev, size, B, case):
    if_flood, tide, settings, roll, seq, normalized = case
    gpu, parents, cpu, L = stores(dev, size, if_flood, tide, settings, roll, seq)
    t_out = gpu.t_out
    starts = last_starts(L, seq[0] + t_out)[::-1][:B]               # the store's last window first
    out, out_parents = guarded_outputs(gpu, B, t_out, dev)
    got = gpu.batch(torch.tensor(starts, dtype=torch.int32, device=dev), normalized=normalized, out=out)
    assert gpu.last_path == 'hip'
    ref = cpu.batch_torch(starts, normalized=normalized)
    for name, g, r, o, par in zip(NAMES, got, ref, out, out_parents):
        if r is None:
            assert g is None, name
            continue
        assert g is o and torch.equal(g.cpu(), r), name
        assert not bool(torch.isnan(g).any()), name
        assert WU.guards_intact(par, g.numel()), name
    for name, par in parents.items():
        assert WU.guards_intact(par, getattr(gpu, name).numel()), name
    fresh = gpu.batch(starts, normalized=normalized)               # host starts, fresh outputs
    assert all((u is None and v is None) or torch.equal(u.cpu(), v) for u, v in zip(fresh, ref))


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
@pytest.mark.parametrize('normalized', [True, False])
def test_starts_outside_the_series_give_nan_windows(dev, size, normalized):
    gpu, parents, cpu, L = stores(dev, size, 3, True, True, 0, (5, 5))
    Ttot, valid = sum(L), L[0] + 3
    out, out_parents = guarded_outputs(gpu, 3, gpu.t_out, dev)
    got = gpu.batch(torch.tensor([-1, valid, Ttot - 1], dtype=torch.int32, device=dev), normalized=normalized, out=out)
    ref = cpu.batch_torch([valid], normalized=normalized)
    for name, g, r, par in zip(NAMES, got, ref, out_parents):
        assert bool(torch.isnan(g[0]).all()) and bool(torch.isnan(g[2]).all()), name
        assert torch.equal(g[1].cpu(), r[0]), name
        assert WU.guards_intact(par, g.numel()), name
    got = gpu.batch(torch.tensor([Ttot - 9, -(1 << 31), (1 << 31) - 1], dtype=torch.int32, device=dev), normalized=normalized)
    assert all(bool(torch.isnan(g).all()) for g in got)            # one row short of fitting; the int32 extremes


WEIGHTS = {'mixed': [1, 5, 1, 1, 7], 'equal': [1] * 23, 'one': [1]}


def table_with(dev, weights, seed):
    """A table over a small store whose starts / weights are replaced by the given ones (the draw reads only starts and cum)."""
    L = [40]
    series = WU.make_series(3, L, 2, 1)
    store = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, device=dev, seq_in=2, seq_out=1, roll=0, if_flood=0)
    tb = store.table(seed=seed)
    starts = [3 * k + 1 for k in range(len(weights))]
    tb.starts = torch.tensor(starts, dtype=torch.int32, device=dev)
    tb.cum = torch.tensor(weights, dtype=torch.int64, device=dev).cumsum(0)
    return tb, starts


@pytest.fixture(scope='module')
def draw_refs():
    """the restated stream, once per weight set: indices 0 .. 3 * 4096 - 1 (the resumed draws of B = 64 lie inside)"""
    seed = (0xC0FFEE << 32) | 12345
    return seed, {k: WU.draw_ref([3 * i + 1 for i in range(len(w))], w, seed, 0, 3 * 4096) for k, w in WEIGHTS.items()}


@pytest.mark.parametrize('B', [1, 64, 4096])
@pytest.mark.parametrize('which', list(WEIGHTS))
def test_three_draws_equal_the_restatement(dev, draw_refs, which, B):
    seed, refs = draw_refs
    tb, starts = table_with(dev, WEIGHTS[which], seed)
    got = [tb.draw(B).cpu().tolist() for _ in range(3)]
    assert sum(got, []) == refs[which][:3 * B]
    assert tb.count.item() == 3 * B and tb.state_dict() == {'seed': seed, 'count': 3 * B}
    if which == 'mixed' and B == 4096:
        share = sum(v == starts[4] for v in sum(got, [])) / (3 * B)
        assert abs(share - 7 / 15) < 0.02                          # the heavy window is drawn about 7 times in 15
    if B == 64:
        other, _ = table_with(dev, WEIGHTS[which], 0)
        other.load_state_dict(tb.state_dict())
        nxt = tb.draw(B).cpu().tolist()
        assert other.draw(B).cpu().tolist() == nxt == refs[which][3 * B:4 * B]


@pytest.mark.parametrize('spelling', ['cuda', 'cuda:0', 'object'])
def test_a_store_named_by_any_spelling_of_the_device_keeps_starts_on_the_device(dev, spelling, monkeypatch):
    """`device='cuda'` (no index) is how users name the device, while every tensor reports 'cuda:0': drawn starts must be taken as
    they are -- no read-back, no host check, no upload -- so `draw` + `batch` can be captured and a start outside the series gives
    a NaN window, not a ValueError."""
    L = [10, 17, 40]
    series = WU.make_series(5, L, 30, 29)
    store = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, settings=series['settings'], tide=series['tide'],
                          device=dev if spelling == 'object' else spelling, seq_in=5, seq_out=5, roll=0, if_flood=3)
    cpu = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, settings=series['settings'], tide=series['tide'],
                        device='cpu', seq_in=5, seq_out=5, roll=0, if_flood=3)
    for s in (store, cpu):
        s.set_norm(*WU.make_norms(6, 30, 29))
    assert store.device == store.states.device == dev
    table = store.table(flood_weight=3, seed=9)
    assert table.starts.device == store.device and table.count.device == store.device

    def no_host_path(*args, **kw):
        raise AssertionError('device starts went through the host check')
    monkeypatch.setattr(U.WindowStore, '_checked_starts', no_host_path)
    drawn = table.draw(8)                                          # warm-up outside the capture
    store.batch(drawn)
    table.load_state_dict({'seed': 9, 'count': 0})
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        drawn = table.draw(8)
        out = store.batch(drawn)
    graph.replay()
    want = WU.draw_ref(table.starts.tolist(), table.weights.tolist(), 9, 0, 8)
    assert drawn.tolist() == want and store.last_path == 'hip'
    monkeypatch.undo()
    assert all(torch.equal(u.cpu(), v) for u, v in zip(out, cpu.batch_torch(want)))
    monkeypatch.setattr(U.WindowStore, '_checked_starts', no_host_path)
    got = store.batch(torch.tensor([sum(L) - 9, 12, -1], dtype=torch.int32, device=dev))
    assert all(bool(torch.isnan(g[0]).all()) and bool(torch.isnan(g[2]).all()) and not bool(torch.isnan(g[1]).any()) for g in got)
    with pytest.raises(ValueError, match='int32'):
        store.batch(torch.tensor([12], dtype=torch.int64, device=dev))


def test_draw_carries_the_counter_across_2_to_the_32(dev, draw_refs):
    seed, _ = draw_refs
    tb, starts = table_with(dev, WEIGHTS['mixed'], seed)
    j0 = (1 << 32) - 3                                             # the second counter word comes into use inside the call
    tb.load_state_dict({'seed': seed, 'count': j0})
    assert tb.draw(8).cpu().tolist() == WU.draw_ref(starts, WEIGHTS['mixed'], seed, j0, 8)
    assert tb.count.item() == j0 + 8


def test_batch_and_draw_inside_a_captured_graph(dev, draw_refs):
    seed, refs = draw_refs
    gpu, _, cpu, L = stores(dev, (30, 29), 3, True, True, 0, (5, 5))
    tb, _ = table_with(dev, WEIGHTS['mixed'], seed)
    valid = [0, L[0] + 2, L[0] + L[1] + 30]
    starts = torch.tensor(valid, dtype=torch.int32, device=dev)
    drawn = torch.empty(64, dtype=torch.int32, device=dev)
    gpu.batch(starts)                                              # warm-up outside the capture: library, code objects
    tb.draw(64, out=drawn)
    tb.load_state_dict({'seed': seed, 'count': 0})
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu.batch(starts)
        tb.draw(64, out=drawn)
    for k, other in enumerate(([0, L[0] + 2, L[0] + L[1] + 30], [L[0], L[0] + 7, L[0] + L[1] + 1])):
        starts.copy_(torch.tensor(other, dtype=torch.int32))
        graph.replay()
        ref = cpu.batch_torch(other)
        assert all(torch.equal(u.cpu(), v) for u, v in zip(out, ref)), k
        assert drawn.cpu().tolist() == refs['mixed'][64 * k:64 * (k + 1)], k
    assert tb.count.item() == 128
    eager = gpu.batch(starts)
    assert all(torch.equal(u, v) for u, v in zip(out, eager))
