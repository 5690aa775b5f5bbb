"""Cost of a `fit_eval` training step on ONE GPU as one replay of a captured graph (`emul.graphed_fit = True`: forward, tail,
backward and the HIP Adam operator uds_adam_step in one hipGraph) against the eager step.

    python tools/fit_graph_time.py [--out profiles/fit_graph_time.json] [--only astlingen|RedChicoSur|c5] [--embed 64|128]
    python tools/fit_graph_time.py --control [--root TREE]      # one shape, flag off: this tree against another one
    python tools/fit_graph_time.py --trace-leg eager|graph      # 5 steps of one leg on astlingen at batch 64, for a kernel trace
    python tools/fit_graph_time.py --trace-summary eager=KERNEL_TRACE.csv graph=KERNEL_TRACE.csv      # per-step counts and gaps

Networks and model as tools/fit_tail_time.py (same `build`, same alternation): astlingen (30 nodes) and RedChicoSur (443 nodes) at
batch 1, 64 and 256, temporal net Conv1D and GRU, embed_size 64 and 128, and the C5-sized block-diagonal network (100 x 2 000
nodes, batch 1, Conv1D, embed 64), where the step is not launch-bound.  Three models per shape, same seed, one per leg:
  eager       graphed_fit off: the step as it was, `KerasAdam`
  eager_hip   graphed_fit off with a `HipKerasAdam` installed: the optimizer's own share
  graph       graphed_fit on: one replay per step
Per shape, in one process, WARM calls of every leg first (the graph leg captures in its first), then REPS rounds calling each leg
once in turn, device events around every call, medians; the whole measurement RUNS times (`spread`: the largest relative
difference of a median between runs).  `slower_beyond_spread`: every shape where the graph loses to eager beyond the spread.
At the C5 size the record also holds the device memory the graph's pool keeps per key (`graph_pool_bytes`: reserved memory after
the capture minus before).  --control times the flag-off step alone on one shape (RedChicoSur, batch 64, Conv1D) with the package
under --root: run on the parent commit's tree and on this one it shows that the default path kept its time.
One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import fit_tail_time as FT                                  # noqa: E402  (puts --root, or this tree, on sys.path and imports the package)

WARM, REPS, RUNS, T = FT.WARM, FT.REPS, FT.RUNS, FT.T
EMBED = (64, 128)


def build(name, recurrent, embed, dev):
    """fit_tail_time.build at another embed_size (the builder reads it from the SimpleNamespace it makes: patched through)."""
    if embed == 64:
        return FT.build(name, recurrent, dev)
    real = FT.SimpleNamespace

    def wide(**kw):
        kw.update(embed_size=embed, hidden_dim=embed)
        return real(**kw)
    FT.SimpleNamespace = wide
    try:
        return FT.build(name, recurrent, dev)
    finally:
        FT.SimpleNamespace = real


def inputs(n, e, batch, dev):
    gen = torch.Generator().manual_seed(batch + n)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    x, a, b, ex = r(batch, T, n, 5), 0.1 + 0.9 * r(batch, T, 2), r(batch, T, n, 2) * 0.1, r(batch, T, e, 4)
    y, ey = r(batch, T, n, 5), r(batch, T, e, 3)
    y[..., -2] = (y[..., -2] > 0.7).float()
    return x, a, b, y, ex, ey


def legs(name, recurrent, embed, dev):
    from gnn_uds_amd.emulator import HipKerasAdam
    models = {}
    for leg in ('eager', 'eager_hip', 'graph'):
        emul, n, e = build(name, recurrent, embed, dev)
        if leg == 'eager_hip':
            emul._optimizer = HipKerasAdam([p for p in emul.parameters()], emul.learning_rate, clipnorm=1.0)
        emul.graphed_fit = leg == 'graph'
        models[leg] = emul
    return models, n, e


def shape_fns(models, bt):
    def step(leg):
        emul = models[leg]

        def fn():
            out = emul.fit_eval(*bt)
            assert (emul.last_fit_path == 'eager') == (leg != 'graph'), (leg, emul.last_fit_path, emul.last_fit_refusal)
            return out
        return fn
    return {leg: step(leg) for leg in models}


def control(dev):
    emul, n, e = FT.build('RedChicoSur', 'Conv1D', dev)
    bt = inputs(n, e, 64, dev)
    runs = [FT._alternate({'step_eager': lambda: emul.fit_eval(*bt)}, 3 * REPS)['step_eager'] for _ in range(RUNS)]
    return {'tool': 'fit_graph_time --control', 'root': os.path.relpath(FT.PKG_ROOT, ROOT), 'network': 'RedChicoSur', 'batch': 64,
            'recurrent': 'Conv1D', 'step_eager_ms': runs}


def trace_leg(leg, dev):
    models, n, e = legs('astlingen', 'Conv1D', 64, dev)
    fn = shape_fns({leg: models[leg]}, inputs(n, e, 64, dev))[leg]
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    return {'tool': 'fit_graph_time --trace-leg', 'leg': leg, 'warm': WARM, 'steps': 5}


def trace_summary(path, delimiter='k_fit_reduce', steps=5):
    """Kernels (memsets run as fill kernels and are counted apart) and idle gaps of the last `steps` steps of a kernel trace CSV of
    rocprofv3: a step is what lies between two launches of `delimiter`, a kernel every step runs once."""
    import csv
    rows = sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(path))), key=lambda r: r[0])
    marks = [i for i, r in enumerate(rows) if delimiter in r[2]]
    out = []
    for lo, hi in zip(marks[-steps - 1:-1], marks[-steps:]):
        seg = rows[lo:hi + 1]
        gaps = [max(0, b[0] - a[1]) for a, b in zip(seg[:-1], seg[1:])]
        out.append({'kernels': hi - lo, 'fills': sum('fillBuffer' in r[2] for r in seg[:-1]), 'span_ms': round((seg[-1][0] - seg[0][0]) / 1e6, 3),
                    'busy_ms': round(sum(r[1] - r[0] for r in seg[:-1]) / 1e6, 3), 'median_gap_us': round(float(np.median(gaps)) / 1e3, 2),
                    'sum_gap_ms': round(sum(gaps) / 1e6, 3)})
    return out


def main():
    if '--trace-summary' in sys.argv:
        i = sys.argv.index('--trace-summary')
        print(json.dumps({'tool': 'fit_graph_time --trace-summary', 'steps': {leg_path.split('=')[0]: trace_summary(leg_path.split('=')[1])
                                                                              for leg_path in sys.argv[i + 1:]}}))
        return
    dev = torch.device('cuda:0')
    if '--control' in sys.argv:
        print(json.dumps(control(dev)))
        return
    if '--trace-leg' in sys.argv:
        print(json.dumps(trace_leg(sys.argv[sys.argv.index('--trace-leg') + 1], dev)))
        return
    only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
    rec = {'tool': 'fit_graph_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs_per_shape': RUNS, 'seq_out': T,
           'model': 'GAT, act, rated pumps on every link, node pumps, offsets, tide, flood channel, epsilon 0.1, no edge fusion', 'shapes': []}
    shapes = [(name, rc, d, bs) for name in FT.NETWORKS for rc in FT.RECURRENT for d in EMBED for bs in FT.BATCHES] + [('c5', 'Conv1D', 64, 1)]
    embed = int(sys.argv[sys.argv.index('--embed') + 1]) if '--embed' in sys.argv else None
    shapes = [s for s in shapes if (only is None or s[0] == only) and (embed is None or s[2] == embed)]
    models = {}
    for name, rc, d, bs in shapes:
        if (name, rc, d) not in models:
            models.clear()                                  # one network's three models at a time
            models[(name, rc, d)] = legs(name, rc, d, dev)
        ms3, n, e = models[(name, rc, d)]
        bt = inputs(n, e, bs, dev)
        fns = shape_fns(ms3, bt)
        pool = None
        if name == 'c5':                                    # what the capture adds to the allocator's reserved memory
            for leg in ('eager', 'eager_hip'):
                fns[leg]()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()                        # (the capture empties the cache too: compare like with like)
            before = torch.cuda.memory_reserved(dev)
            fns['graph']()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()                        # the graph's private pool stays reserved while the graph lives
            pool = int(torch.cuda.memory_reserved(dev) - before)
        runs = [FT._alternate(fns, REPS if name != 'c5' else 10) for _ in range(RUNS)]
        assert ms3['graph'].last_fit_path == 'graph' and ms3['eager'].last_fit_path == 'eager'
        ms = {k: round(float(np.median([run[k] for run in runs])), 4) for k in runs[0]}
        spread = {k: round(max(run[k] for run in runs) / min(run[k] for run in runs) - 1, 4) for k in runs[0]}
        row = {'network': name, 'n_node': n, 'n_edge': e, 'recurrent': rc, 'embed_size': d, 'batch': bs, 'median_ms': ms, 'spread': spread,
               'eager_over_graph': round(ms['eager'] / ms['graph'], 3), 'eager_over_eager_hip': round(ms['eager'] / ms['eager_hip'], 3)}
        if pool is not None:
            row['graph_pool_bytes'] = pool
        rec['shapes'].append(row)
        print('%s %s d=%d batch %d: %r' % (name, rc, d, bs, ms), file=sys.stderr, flush=True)
    rec['slower_beyond_spread'] = [(s['network'], s['recurrent'], s['embed_size'], s['batch']) for s in rec['shapes']
                                   if s['median_ms']['graph'] > s['median_ms']['eager'] * (1 + max(s['spread']['graph'], s['spread']['eager']))]
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
