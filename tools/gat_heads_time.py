"""Cost of the multi-head GAT entries against the single-head ones on ONE GPU.

    python tools/gat_heads_time.py [--out profiles/gat_heads_time.json]

Headline network: `graph.synthetic_drainage_network(10 000, 12 000, seed 0)` (as bench.py), its node adjacency with the self
loops, S = 60 snapshots, row width d = 64.  Timed, alternated call by call in one process after WARM launches of every variant,
REPS timed launches each with device events around every launch, the whole measurement twice (run-to-run spread):
  aggregate   uds_gat_aggregate (the existing single-head entry, the yardstick) against uds_gat_aggregate_heads at
              H = 1, 2, 4, 8 (C = 64 / H), concatenated; also the mean over heads and the call that writes alpha_out at H = 4
  backward    uds_gat_backward against uds_gat_backward_heads at the same H
The gathered row bytes are equal across H (every variant reads 256-byte rows of hx); the score loads and the exp count grow
with H (H * nnz per snapshot).  One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U                      # noqa: E402
from gnn_uds_amd import _lib                 # noqa: E402

N, E, S, D = 10000, 12000, 60, 64
HEADS = (1, 2, 4, 8)
WARM, REPS, RUNS = 20, 200, 2


def _alternate(fns):
    """name -> ms per call: WARM calls of each, then REPS rounds calling each once in turn, one event pair per call."""
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


def main():
    dev = torch.device('cuda:0')
    csr = U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0)).adj
    h = _lib.CsrHandle(csr)
    ht, perm = h.transposed(dev)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)
    hx, grad, bias, a_s, a_n = r(S, N, D), r(S, N, D), r(D) * 0.1, r(D), r(D)
    out, d_hx = torch.empty_like(hx), torch.empty_like(hx)
    ss1, sn1 = r(S, N) * 4, r(S, N) * 4
    agg = {'single_head': lambda: _lib.gat_aggregate(h, hx, ss1, sn1, bias, 'relu', out=out)}
    ws1, o1 = torch.empty((2, S, csr.nnz), device=dev), (d_hx, torch.empty((S, N), device=dev), torch.empty((S, N), device=dev))
    bwd = {'single_head': lambda: _lib.gat_backward(h, ht, perm, grad, hx, ss1, sn1, a_s, a_n, out=o1, workspace=ws1)}
    for H in HEADS:
        ss, sn = r(S, N, H) * 4, r(S, N, H) * 4
        agg['heads_H%d' % H] = lambda ss=ss, sn=sn: _lib.gat_aggregate_heads(h, hx, ss, sn, bias, 'relu', out=out)
        ws, o = torch.empty((2, S, H, csr.nnz), device=dev), (d_hx, torch.empty((S, N, H), device=dev), torch.empty((S, N, H), device=dev))
        bwd['heads_H%d' % H] = lambda ss=ss, sn=sn, ws=ws, o=o: _lib.gat_backward_heads(h, ht, perm, grad, hx, ss, sn, a_s, a_n, out=o, workspace=ws)
        if H == 4:
            om, bm, al = torch.empty((S, N, D // H), device=dev), bias[:D // H].contiguous(), torch.empty((S, H, csr.nnz), device=dev)
            agg['heads_H4_mean'] = lambda ss=ss, sn=sn: _lib.gat_aggregate_heads(h, hx, ss, sn, bm, 'relu', concat=False, out=om)
            agg['heads_H4_alpha_out'] = lambda ss=ss, sn=sn: _lib.gat_aggregate_heads(h, hx, ss, sn, bias, 'relu', out=out, alpha_out=al)
    rec = {'tool': 'gat_heads_time', 'device': torch.cuda.get_device_name(0), 'N': N, 'S': S, 'd': D, 'nnz': int(csr.nnz), 'warm': WARM,
           'reps': REPS, 'runs': []}
    for _ in range(RUNS):
        run = {'aggregate': _alternate(agg), 'backward': _alternate(bwd)}
        for t in run.values():
            base = t['single_head']['median_ms']
            for k, v in t.items():
                v['over_single_head'] = round(v['median_ms'] / base, 3)
        rec['runs'].append(run)
    # run-to-run spread: the largest relative difference of a variant's median between the two runs
    rec['run_to_run_spread'] = round(max(abs(rec['runs'][0][leg][k]['median_ms'] - rec['runs'][1][leg][k]['median_ms']) / rec['runs'][0][leg][k]['median_ms']
                                         for leg in ('aggregate', 'backward') for k in rec['runs'][0][leg]), 4)
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
