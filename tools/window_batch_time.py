"""Cost of one training batch of sliding windows on ONE GPU: drawn and built on the device (`WindowTable.draw` + `WindowStore.batch`:
uds_window_draw, uds_window_batch) against the tensor code (`batch_torch`) and against a NumPy host pipeline with uploads, the form
the reference's loop has (`dataloader.py:106-143`, `main.py:209-232`).

    python tools/window_batch_time.py [--out profiles/window_batch_time.json] [--only astlingen|RedChicoSur]
    python tools/window_batch_time.py --trace-leg NETWORK BATCH      # 50 draw + batch calls of one shape, for a kernel trace

Networks and model as tools/fit_tail_time.py (same `build`): astlingen (30 nodes) and RedChicoSur (443 nodes), Conv1D, embed 64, at
batch 1, 64 and 256, seq_in = seq_out = 5; series of EVENTS seeded events of EVENT_ROWS rows each, two settings, tide, flood > 0 on
about a fifth of the rows, a table over all events with flood_weight 4.  Legs, per shape, alternated in one process after WARM calls
of each; every timed region is a host clock around the call and ends in a device synchronise (the host's share is what is measured):
  hip           draw on the device + one uds_window_batch launch into the buffers of the call before
  torch         starts drawn on the host (NumPy, the table's weights) and uploaded + `batch_torch` on the device
  numpy         starts drawn on the host + the host pipeline restated below (fancy indexing, stack, five normalisations) + six uploads
  epoch_hip     `hip` followed by `fit_eval` with graphed_fit on (one epoch of `gnn_uds_amd.fit`)
  epoch_numpy   `numpy` followed by the same `fit_eval`
REPS rounds, medians; the whole measurement RUNS times (`spread`: the largest relative difference of a median between runs).
`bytes_per_batch`: what the batch reads and writes, computed from the shapes.  `hip_slower_beyond_spread`: every shape where `hip`
loses to `torch` or `numpy` beyond the spread.  One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import fit_tail_time as FT                                  # noqa: E402  (puts this tree on sys.path and imports the package)

U = FT.U
WARM, REPS, RUNS, T = 5, 30, 2, FT.T
EVENTS, EVENT_ROWS = 8, 500
BATCHES = (1, 64, 256)


def series(n, e, seed=3):
    rng = np.random.default_rng(seed)
    rows = EVENTS * EVENT_ROWS
    f = np.float32
    wet = rng.random(rows) < 0.2
    return dict(states=rng.random((rows, n, 4)).astype(f), flood=(rng.random((rows, n)) * (rng.random((rows, n)) < 0.5) * wet[:, None]).astype(f),
                edge_states=rng.random((rows, e, 4)).astype(f), settings=(0.1 + 0.9 * rng.random((rows, 2))).astype(f),
                tide=(0.1 * rng.random((rows, n))).astype(f))


def numpy_batch(host, norms, starts, dev):
    """The host pipeline: windows by fancy indexing, channels by np.stack, five normalisations, six uploads."""
    rin = starts[:, None] + np.arange(T)
    rout = starts[:, None] + T + np.arange(T)
    si, so, fi, fo = host['states'][rin], host['states'][rout], host['flood'][rin], host['flood'][rout]
    x = np.stack([si[..., 0], si[..., 1] - si[..., 3], si[..., 2], (fi > 0).astype(np.float32), si[..., 3]], axis=-1)
    y = np.stack([so[..., 0], so[..., 1] - so[..., 3], so[..., 2], (fo > 0).astype(np.float32), fo], axis=-1)
    b = np.stack([so[..., 3], host['tide'][rout]], axis=-1)
    ex, ey, a = host['edge_states'][rin], host['edge_states'][rout][..., :3], host['settings'][rout]
    norm = lambda v, item: (v - norms[item][1, ..., :v.shape[-1]]) / (norms[item][0, ..., :v.shape[-1]] - norms[item][1, ..., :v.shape[-1]])
    x, b, y, ex, ey = norm(x, 'x'), norm(b, 'b'), norm(y, 'y'), norm(ex, 'e'), norm(ey, 'e')
    return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x, a, b, y, ex, ey))


def bytes_per_batch(n, e, batch, n_act=2):
    """(read, written) by one normalised batch: 16 B of states + flood (+ tide on output rows) per node row, 16 B per link row,
    the settings, the (span, min) pairs once per workgroup row at most (cached: counted once); the six outputs."""
    rows = 2 * T
    read = batch * (rows * (n * 20 + e * 16) + T * (n * 4 + n_act * 4)) + 2 * 4 * (n * (5 + 2 + 5) + e * 4) + batch * 4
    written = 4 * batch * T * (n * 5 + n_act + n * 2 + n * 5 + e * 4 + e * 3)
    return read, written


def setup(name, dev):
    emul, n, e = FT.build(name, 'Conv1D', dev)
    emul.graphed_fit = True
    host = series(n, e)
    store = U.WindowStore(host['states'], host['flood'], host['edge_states'], [EVENT_ROWS] * EVENTS, settings=host['settings'], tide=host['tide'],
                          emul=emul, device=dev)
    table = store.table(flood_weight=4, seed=5)
    return emul, n, e, host, store, table


def shape_fns(emul, host, store, table, batch, dev):
    norms = {k: v.cpu().numpy() for k, v in emul._norms.items()}
    starts_host, p = table.starts.cpu().numpy().astype(np.int64), table.weights.cpu().numpy().astype(np.float64)
    p /= p.sum()
    rng = np.random.default_rng(batch)
    bufs = [None, None]

    def hip():
        bufs[0] = table.draw(batch, out=bufs[0])
        bufs[1] = store.batch(bufs[0], out=bufs[1])
        return bufs[1]

    def torch_leg():
        s = rng.choice(starts_host, size=batch, p=p).astype(np.int32)
        return store.batch_torch(torch.from_numpy(s).to(dev))

    def numpy_leg():
        return numpy_batch(host, norms, rng.choice(starts_host, size=batch, p=p), dev)

    def epoch(leg):
        def fn():
            out = emul.fit_eval(*leg())
            assert emul.last_fit_path.startswith('graph'), (emul.last_fit_path, emul.last_fit_refusal)
            return out
        return fn
    return {'hip': hip, 'torch': torch_leg, 'numpy': numpy_leg, 'epoch_hip': epoch(hip), 'epoch_numpy': epoch(numpy_leg)}


def alternate(fns, reps):
    """name -> median ms per call on the host clock, every call ended by a device synchronise: WARM calls of each, then `reps` rounds
    calling each once in turn."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}


def trace_leg(name, batch, dev):
    emul, n, e, host, store, table = setup(name, dev)
    fn = shape_fns(emul, host, store, table, batch, dev)['hip']
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    return {'tool': 'window_batch_time --trace-leg', 'network': name, 'batch': batch, 'warm': WARM, 'calls': 50}


def main():
    dev = torch.device('cuda:0')
    if '--trace-leg' in sys.argv:
        i = sys.argv.index('--trace-leg')
        print(json.dumps(trace_leg(sys.argv[i + 1], int(sys.argv[i + 2]), dev)))
        return
    only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
    rec = {'tool': 'window_batch_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs_per_shape': RUNS, 'seq_in': T,
           'seq_out': T, 'events': EVENTS, 'event_rows': EVENT_ROWS, 'clock': 'host perf_counter around the call + device synchronise', 'shapes': []}
    for name in FT.NETWORKS:
        if only is not None and name != only:
            continue
        emul, n, e, host, store, table = setup(name, dev)
        for bs in BATCHES:
            fns = shape_fns(emul, host, store, table, bs, dev)
            runs = [alternate(fns, REPS) for _ in range(RUNS)]
            assert store.last_path == 'hip' and emul.last_fit_path == 'graph'
            ms = {k: round(float(np.median([run[k] for run in runs])), 4) for k in runs[0]}
            spread = {k: round(max(run[k] for run in runs) / min(run[k] for run in runs) - 1, 4) for k in runs[0]}
            read, written = bytes_per_batch(n, e, bs)
            rec['shapes'].append({'network': name, 'n_node': n, 'n_edge': e, 'batch': bs, 'windows_in_table': len(table), 'median_ms': ms, 'spread': spread,
                                  'bytes_per_batch': {'read': read, 'written': written},
                                  'torch_over_hip': round(ms['torch'] / ms['hip'], 3), 'numpy_over_hip': round(ms['numpy'] / ms['hip'], 3),
                                  'epoch_numpy_over_epoch_hip': round(ms['epoch_numpy'] / ms['epoch_hip'], 3)})
            print('%s batch %d: %r' % (name, bs, ms), file=sys.stderr, flush=True)
    rec['hip_slower_beyond_spread'] = [(s['network'], s['batch'], k) for s in rec['shapes'] for k in ('torch', 'numpy')
                                       if s['median_ms']['hip'] > s['median_ms'][k] * (1 + max(s['spread']['hip'], s['spread'][k]))]
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
