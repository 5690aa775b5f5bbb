"""gnn_uds_amd/data.py without a device: `WindowStore.batch_torch` on a CPU store against the loop-written restatement of the window
definitions (tests/window_util.py), window tables, flood weights and norms against brute force, the host checks of window starts, and
the argument checks of uds_window_batch / uds_window_draw (operands are aligned host addresses that are never read)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from tests import window_util as WU

N, E = 3, 2
GRID = list(itertools.product((0, 3), (True, False), (True, False), (0, 2), ((5, 5), (6, 2), (1, 1)), (True, False)))


def event_lens(seq_in, t_out):
    return [seq_in + t_out, seq_in + t_out - 1, 17, 40]


def store_of(series, L, seq_in, seq_out, roll, if_flood, norms=None):
    s = U.WindowStore(series['states'], series['flood'], series['edge_states'], L, settings=series['settings'], tide=series['tide'],
                      device='cpu', seq_in=seq_in, seq_out=seq_out, roll=roll, if_flood=if_flood)
    if norms is not None:
        s.set_norm(*norms)
    return s


@pytest.mark.parametrize('if_flood,tide,settings,roll,seq,normalized', GRID,
                         ids=['flood%d-tide%d-act%d-roll%d-%dx%d-norm%d' % (f, t, a, r, s[0], s[1], n) for f, t, a, r, s, n in GRID])
def test_batch_torch_equals_the_restatement(if_flood, tide, settings, roll, seq, normalized):
    seq_in, seq_out = seq
    t_out = seq_out * max(roll, 1)
    L = event_lens(seq_in, t_out)
    series = WU.make_series(1, L, N, E, n_act=2 if settings else 0, tide=tide)
    norms = WU.make_norms(2, N, E)
    store = store_of(series, L, seq_in, seq_out, roll, if_flood, norms)
    assert store.t_out == t_out
    starts = [0, sum(L[:2]) + 17 - seq_in - t_out, sum(L) - seq_in - t_out]      # the one window of event 0, the last of events 2 and 3
    got = store.batch(starts, normalized=normalized)
    assert store.last_path == 'torch'
    ref = WU.windows_ref(series, starts, seq_in, t_out, if_flood, norms if normalized else None)
    for name, g, r in zip(('x', 'a', 'b', 'y', 'ex', 'ey'), got, ref):
        if r is None:
            assert g is None, name
        else:
            assert g.dtype == torch.float32 and np.array_equal(g.numpy(), r), name
    again = store.batch_torch(torch.tensor(starts, dtype=torch.int32), normalized=normalized)
    assert all((u is None and v is None) or torch.equal(u, v) for u, v in zip(got, again))


@pytest.mark.parametrize('interval', [1, 3])
@pytest.mark.parametrize('roll', [0, 2])
def test_window_table_against_brute_force(interval, roll):
    seq_in, seq_out = 5, 3
    t_out = seq_out * max(roll, 1)
    L = event_lens(seq_in, t_out)
    series = WU.make_series(3, L, N, E)
    store = store_of(series, L, seq_in, seq_out, roll, 3)
    tb = store.table(interval=interval)
    ref = WU.table_ref(L, seq_in, t_out, interval)
    assert tb.starts.dtype == torch.int32 and tb.starts.tolist() == ref and len(tb) == len(ref)
    assert ref[0] == 0 and ref[1] == L[0] + L[1]                   # exactly one window of event 0, none of event 1
    assert tb.weights.dtype == torch.uint32 and tb.weights.tolist() == [1] * len(ref)
    assert tb.cum.dtype == torch.int64 and tb.cum.tolist() == list(range(1, len(ref) + 1))
    sub = store.table(events=[3, 0], interval=interval)
    assert sub.starts.tolist() == WU.table_ref(L, seq_in, t_out, interval, events=[3]) + WU.table_ref(L, seq_in, t_out, interval, events=[0])
    assert store.event_windows(2).tolist() == [L[0] + L[1] + i for i in range(17 - seq_in - seq_out + 1)]
    assert store.event_windows(1).tolist() == ([] if L[1] < seq_in + seq_out else [L[0] + i for i in range(L[1] - seq_in - seq_out + 1)])


@pytest.mark.parametrize('interval', [1, 3])
def test_flood_weights_against_brute_force(interval):
    seq_in, seq_out, w = 4, 3, 5
    L = [12, 20, 30]
    series = WU.make_series(4, L, N, E)
    series['flood'][:] = 0.0                                       # event 1 (rows 12 .. 31) never floods
    series['flood'][7, 1], series['flood'][40, 0], series['flood'][55:57, 2], series['flood'][61, 0] = 0.5, 0.2, 1.0, 3.0
    store = store_of(series, L, seq_in, seq_out, 0, 3)
    tb = store.table(interval=interval, flood_weight=w)
    starts = WU.table_ref(L, seq_in, seq_out, interval)
    ref = WU.weights_ref(series['flood'], starts, seq_in, seq_out, w)
    assert tb.starts.tolist() == starts and tb.weights.tolist() == ref
    assert tb.cum.tolist() == list(np.cumsum(ref))
    assert set(ref) == {1, w}                                      # both kinds occur
    assert all(v == 1 for s, v in zip(starts, ref) if 12 <= s < 32)
    sd = tb.state_dict()
    assert sd == {'seed': 0, 'count': 0}
    tb.load_state_dict({'seed': 9, 'count': 1 << 40})
    assert tb.state_dict() == {'seed': 9, 'count': 1 << 40}


@pytest.mark.parametrize('if_flood,tide,head', [(3, True, False), (0, False, True), (3, False, True)])
def test_get_norm_against_brute_force(if_flood, tide, head):
    L = [9, 14]
    series = WU.make_series(5, L, N, E, tide=tide)
    series['states'][:, 1] = 0.0                                   # a node whose series is all zero
    series['flood'][:, 1] = 0.0
    series['states'][..., 0] += 0.25                               # head never reaches 0: head=True has a minimum to find
    series['states'][:, 1, 0] = 0.0
    store = store_of(series, L, 3, 2, 0, if_flood)
    got, ref = store.get_norm(head=head), WU.norm_ref(series, if_flood, head)
    for item, g, r in zip('xbyre', got, ref):
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == r.shape and np.array_equal(g, r), item
    assert got[0].shape == (2, N, 5 if if_flood else 4) and got[1].shape == (2, N, 2 if tide else 1) and got[4].shape == (2, E, 4)
    assert np.all(got[0][0, 1] == np.float32(1e-6)) and np.all(got[0][1, 1] == 0)
    assert (got[0][1, 0, 0] > 0) == head and np.all(got[0][1, :, 1:] == 0)


def test_host_starts_are_checked_against_the_events():
    L = [12, 15]
    series = WU.make_series(6, L, N, E)
    store = store_of(series, L, 4, 3, 0, 0)
    store.batch([0, 5, 12, 20], normalized=False)                  # the last windows of both events are fine
    for bad in ([6], [11], [21], [27], [-1], [40]):                # straddling two events, past the store, before it
        with pytest.raises(ValueError, match='does not lie inside one event'):
            store.batch(bad, normalized=False)
    with pytest.raises(ValueError):
        store.batch(torch.tensor([0], dtype=torch.int64), normalized=False)       # a device tensor must be int32


def test_a_table_without_a_window_is_refused_when_it_is_built():
    L = [6, 5, 12]
    store = store_of(WU.make_series(8, L, N, E), L, 4, 3, 0, 0)
    assert len(store.table(events=[2])) == 6
    for events in ([0, 1], [1], []):
        with pytest.raises(ValueError, match='no window of 4 \\+ 3 rows fits'):
            store.table(events=events)
    assert store.event_windows(1).tolist() == []                   # (asking for an event's windows stays allowed)


def test_the_store_reports_the_device_its_tensors_report():
    L = [12, 15]
    store = store_of(WU.make_series(7, L, N, E), L, 4, 3, 0, 0)
    assert store.device == store.states.device == store.table().starts.device == torch.device('cpu')


def test_draw_on_a_cpu_store_raises():
    L = [12, 15]
    store = store_of(WU.make_series(7, L, N, E), L, 4, 3, 0, 0)
    with pytest.raises(_lib.UdsError):
        store.table().draw(4)
    with pytest.raises(_lib.UdsError):
        _lib.window_batch(store.states, store.flood, store.edge_states, store.settings, store.tide, torch.zeros(1, dtype=torch.int32), 4, 3, 0)


_BUF = np.zeros(64, dtype=np.float32)
P = _BUF.ctypes.data - _BUF.ctypes.data % 16 + 16       # a 16-byte aligned host address (never read)
Q = P + 4                                               # misaligned by one float


def _batch_call(lib, B=2, seq_in=5, t_out=5, norm=None, outs=None, **series):
    s = _lib.WindowSeries(P, P, P, P, P, 50, 30, 29, 2)
    for k, v in series.items():
        setattr(s, k, v)
    outs = dict(dict(x=P, a=P, b=P, y=P, ex=P, ey=P), **(outs or {}))
    rc = lib.uds_window_batch(ctypes.byref(s), None if norm is None else ctypes.byref(norm), P, B, seq_in, t_out, 1,
                              *[outs[k] for k in ('x', 'a', 'b', 'y', 'ex', 'ey')], None)
    return rc, lib.uds_last_error().decode()


def test_window_batch_refuses_bad_arguments():
    lib = _lib.load()
    for name in ('states', 'flood', 'edge_states'):
        rc, msg = _batch_call(lib, **{name: None})
        assert rc == -22 and 'NULL series' in msg, name
    for name in ('states', 'flood', 'edge_states', 'settings', 'tide'):
        rc, msg = _batch_call(lib, **{name: Q})
        assert rc == -22 and 'series must be 16-byte aligned' in msg, name
    for name in ('x', 'a', 'b', 'y', 'ex', 'ey'):
        rc, msg = _batch_call(lib, outs={name: Q})
        assert rc == -22 and 'output must be 16-byte aligned' in msg, name
        if name != 'a':
            rc, msg = _batch_call(lib, outs={name: None})
            assert rc == -22 and 'NULL argument' in msg, name
    rc, msg = _batch_call(lib, B=0)
    assert rc == -22 and 'B=0' in msg
    for B in (1 << 31, 214748365, 1 << 60, (1 << 63) - 1, -1):       # (B * rows would overflow 64 bits at the large ones)
        rc, msg = _batch_call(lib, B=B)
        assert rc == -22 and 'B=%d outside [1, 214748364]' % B in msg, B
    rc, msg = _batch_call(lib, seq_in=0)
    assert rc == -22 and 'seq_in=0' in msg
    rc, msg = _batch_call(lib, t_out=0)
    assert rc == -22 and 't_out=0' in msg
    for k, v in (('Ttot', 0), ('N', 0), ('E', 0), ('n_act', -1), ('N', 1 << 31)):
        rc, msg = _batch_call(lib, **{k: v})
        assert rc == -22 and '%s=%d' % (k, v) in msg, k
    rc, msg = _batch_call(lib, settings=None)                      # n_act = 2 without settings
    assert rc == -22 and 'exactly when n_act > 0' in msg
    rc, msg = _batch_call(lib, n_act=0)                            # settings without n_act
    assert rc == -22 and 'exactly when n_act > 0' in msg
    rc, msg = _batch_call(lib, outs={'a': None})
    assert rc == -22 and 'exactly when n_act > 0' in msg
    half = _lib.WindowNorm()
    half.span_b = P
    rc, msg = _batch_call(lib, norm=half)
    assert rc == -22 and 'norm pair 1' in msg
    rc = lib.uds_window_batch(None, None, P, 2, 5, 5, 1, P, P, P, P, P, P, None)
    assert rc == -22 and b'NULL argument' in lib.uds_last_error()


def test_window_draw_refuses_bad_arguments():
    lib = _lib.load()
    good = dict(table=P, cum=P, W=7, B=64, seed=1, count=P, out=P)
    call = lambda **over: (lib.uds_window_draw(*[dict(good, **over)[k] for k in ('table', 'cum', 'W', 'B', 'seed', 'count', 'out')], None),
                           lib.uds_last_error().decode())
    for name in ('table', 'cum', 'count', 'out'):
        rc, msg = call(**{name: None})
        assert rc == -22 and 'NULL argument' in msg, name
    for B in (0, 4097, -1):
        rc, msg = call(B=B)
        assert rc == -22 and 'B=%d outside [1, 4096]' % B in msg
    rc, msg = call(W=0)
    assert rc == -22 and 'W=0' in msg
    for name in ('cum', 'count'):
        rc, msg = call(**{name: Q})
        assert rc == -22 and '8-byte aligned' in msg, name
    for name in ('table', 'out'):
        rc, msg = call(**{name: P + 2})
        assert rc == -22 and '4-byte aligned' in msg, name
