"""Cost of training a `use_adj` GAT layer on ONE GPU: the node-side GAT step (GatFn forward + backward) on the headline network
with and without the per-snapshot edge mask.

    python tools/use_adj_train_time.py                 timing + a kernel-trace child run under rocprofv3
    python tools/use_adj_train_time.py --no-profile    timing only
    python tools/use_adj_train_time.py --count-run     (the child: STEPS masked steps at d = 64, nothing printed)

Headline network: `graph.synthetic_drainage_network(10 000, 12 000, seed 0)` (as bench.py), its node adjacency with the self
loops, S = 60 snapshots, F = d input features, d = 64 and d = 128, matrix-core linear part ('bf16x3', what the Emulator runs).
Three legs, alternated step by step in one process after WARM warm-up steps of every (leg, d), REPS timed steps each with
device events around every step:
  (a) no mask             -- GatFn without edge_mask: the parent's code path (uds_gat_aggregate / uds_gat_backward);
  (b) all-ones mask       -- uds_gat_aggregate_ex / uds_gat_backward_ex, every entry kept;
  (c) seeded mask         -- about 10 % of the off-diagonal entries off per snapshot.
Also (information only) the inference aggregation with the same mask as (c): the walking uds_gat_aggregate_masked against the
grouped uds_gat_aggregate_ex.  One JSON line; with --out PATH it is written there too.
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U                      # noqa: E402
from gnn_uds_amd import _lib                 # noqa: E402
from gnn_uds_amd import autograd as AG       # noqa: E402

N, E, S = 10000, 12000, 60
WIDTHS = (64, 128)
WARM, REPS, STEPS = 20, 60, 10


def _setup(dev, d):
    csr = U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0)).adj
    h = _lib.CsrHandle(csr)
    h.transposed(dev)
    g = torch.Generator().manual_seed(d)
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5)
    x = r(S, N, d).to(dev)
    kernel = (r(d, 1, d) * 0.2).to(dev).requires_grad_(True)
    a_s, a_n = r(d, 1, 1).to(dev).requires_grad_(True), r(d, 1, 1).to(dev).requires_grad_(True)
    bias = (r(d) * 0.1).to(dev).requires_grad_(True)
    gy = r(S, N, d).to(dev)
    rows = np.repeat(np.arange(csr.n_rows), np.diff(np.asarray(csr.rowptr, dtype=np.int64)))
    off = rows != np.asarray(csr.col)
    rng = np.random.default_rng(0)
    mask = np.ones((S, csr.nnz), dtype=np.float32)
    mask[:, off] = (rng.random((S, int(off.sum()))) > 0.1).astype(np.float32)
    masks = {'a_no_mask': None, 'b_all_ones': torch.ones((S, csr.nnz), device=dev), 'c_seeded_10pct': torch.from_numpy(mask).to(dev)}
    xr = x.requires_grad_(True)

    def step(mk):
        out = AG.GatFn.apply(xr, None, kernel, a_s, a_n, bias, 'relu', h, 'bf16x3', None, mk)
        out.backward(gy)

    hx = r(S, N, d).to(dev)
    ss, sn = (r(S, N) * 4).to(dev), (r(S, N) * 4).to(dev)
    infer = {'walking_masked': lambda: _lib.gat_aggregate(h, hx, ss, sn, bias.detach(), 'relu', edge_mask=masks['c_seeded_10pct']),
             'grouped_ex': lambda: _lib.gat_aggregate_ex(h, hx, ss, sn, bias.detach(), 'relu', edge_mask=masks['c_seeded_10pct'])}
    return csr, masks, step, infer, float(1.0 - masks['c_seeded_10pct'][:, torch.as_tensor(off, device=dev)].mean())


def _alternate(fns):
    """name -> mean ms per call: WARM calls of each, then REPS rounds calling each once in turn, one event pair per call."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            ev[k].append((t0, t1))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        ms = np.array([a.elapsed_time(b) for a, b in pairs])
        out[k] = {'mean_ms': round(float(ms.mean()), 4), 'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(float(ms.min()), 4)}
    return out


def _count_run():
    dev = torch.device('cuda:0')
    _, masks, step, _, _ = _setup(dev, 64)
    for _ in range(STEPS):
        step(masks['c_seeded_10pct'])
    torch.cuda.synchronize()


def _profile():
    out = tempfile.mkdtemp(prefix='use_adj_train_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__),
           '--count-run']
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    stats = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if res.returncode != 0 or not stats:
        return {'profile': 'unmeasured (rocprofv3 rc %d)' % res.returncode, 'profile_stderr': res.stderr[-500:]}
    gat = {}
    with open(stats[0]) as fh:
        for row in csv.DictReader(fh):
            if 'k_gat' in row['Name']:
                gat[row['Name']] = {'calls': int(row['Calls']), 'avg_us': round(float(row['AverageNs']) / 1e3, 2)}
    walking = [k for k in gat if 'k_gat_aggregate_masked(' in k or 'k_gat_bwd_rows(' in k]     # not the grouped k_gat_bwd_rows_g<..>
    return {'profile': {'leg': 'c_seeded_10pct', 'd': 64, 'steps': STEPS, 'gat_kernels': gat, 'walking_kernels_launched': walking}}


def main():
    if '--count-run' in sys.argv:
        _count_run()
        return
    dev = torch.device('cuda:0')
    rec = {'tool': 'use_adj_train_time', 'device': torch.cuda.get_device_name(0), 'N': N, 'S': S, 'warm': WARM, 'reps': REPS,
           'step': 'GatFn forward + backward, bf16x3 linear part'}
    for d in WIDTHS:
        csr, masks, step, infer, frac = _setup(dev, d)
        rec['nnz'], rec['masked_offdiag_fraction'] = int(csr.nnz), round(frac, 4)
        t = _alternate({k: (lambda mk=mk: step(mk)) for k, mk in masks.items()})
        a = t['a_no_mask']['mean_ms']
        for k in ('b_all_ones', 'c_seeded_10pct'):
            t[k]['over_a'] = round(t[k]['mean_ms'] / a, 3)
        rec['train_d%d' % d] = t
        ti = _alternate(infer)
        ti['grouped_over_walking'] = round(ti['grouped_ex']['mean_ms'] / ti['walking_masked']['mean_ms'], 3)
        rec['inference_aggregation_d%d' % d] = ti
        del masks, step, infer
        torch.cuda.empty_cache()
    rec['gate_1p2x'] = all(rec['train_d%d' % d][k]['over_a'] <= 1.2 for d in WIDTHS for k in ('b_all_ones', 'c_seeded_10pct'))
    if '--no-profile' not in sys.argv:
        rec.update(_profile())
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
