"""DiffusionConv training cost on ONE GPU: the operator's forward and backward kernels at the headline size, and a small
Emulator's `fit_eval` step with conv='Diffusion' next to the same model with conv='GAT'.

    python tools/diffusion_train_time.py               timing + a kernel-trace child run under rocprofv3
    python tools/diffusion_train_time.py --no-profile  timing only

Reports (one JSON line):
  - one DiffusionConv at N = 10 000 nodes (CSR filter of the synthetic 10 000 / 12 000 network, no N x N array), S = 60,
    C = 64, K1 = 7: uds_diffusion_forward and uds_diffusion_backward, each timed over REPS back-to-back calls after WARM
    calls (long enough for the steady clock), and their ratio;
  - launches per backward and each kernel's mean duration, from a `rocprofv3 --kernel-trace --stats` run of a child
    process (--count-run) doing CALLS forward + backward pairs;
  - `Emulator.fit_eval` (B = 2, T = 5, d = 64, 3 spatial layers) on a 1 000-node / 1 200-link synthetic network with
    conv='Diffusion' and with conv='GAT'.
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U                      # noqa: E402
from gnn_uds_amd import _lib                 # noqa: E402
from oracle import graphs as OG              # noqa: E402

N, E, S, F, C = 10000, 12000, 60, 64, 64
WARM, REPS, CALLS = 300, 200, 20


def _operator(dev):
    gph = U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0))
    ah = U.DiffusionConv.preprocess(gph.adj)
    g = torch.Generator().manual_seed(0)
    layer = U.DiffusionConv(C, generator=g).to(dev)
    with torch.no_grad():
        layer.kernel.mul_(0.002)
    x = (torch.rand(S, N, F, generator=g) - 0.5).to(dev)
    h, vals, c0, a_sup = layer._filter(ah, dev)
    r = x.sum(-1).contiguous()
    tot = r.sum(-1).contiguous()
    y = _lib.diffusion_forward(h, vals, c0, r, tot, 'tanh')
    gy = (torch.rand(S, N, C, generator=g) - 0.5).to(dev)
    fwd = lambda: _lib.diffusion_forward(h, vals, c0, r, tot, 'tanh')
    bwd = lambda: _lib.diffusion_backward(h, a_sup, vals, c0, r, tot, y, gy, layer.K, 'tanh')
    return gph, fwd, bwd


def _time_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPS):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / REPS


def _emulator(dev, conv):
    n, e = 1000, 1200
    edges = U.synthetic_drainage_network(n, e, 0)
    a = SimpleNamespace(state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=64, kernel_size=3,
                        n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=edges, act=False,
                        adj=OG.adjacency(edges), edge_adj=OG.edge_adjacency(edges), node_edge=OG.node_edge_incidence(n, edges),
                        conv=conv, model_dir=None, learning_rate=1e-3)
    emul = U.Emulator(conv, True, 'Conv1D', a, generator=torch.Generator().manual_seed(1)).to(dev)
    emul.set_norm(*[np.stack([np.ones((k, c)), np.zeros((k, c))]) for k, c in ((n, 5), (n, 1), (n, 5), (n, 1), (e, 4))])
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    data = (r(2, 5, n, 5), None, r(2, 5, n, 1) * 0.1, r(2, 5, n, 5), r(2, 5, e, 4), r(2, 5, e, 3))
    for _ in range(3):
        emul.fit_eval(*data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        emul.fit_eval(*data)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / 10 * 1e3, 2)


def _count_run():
    dev = torch.device('cuda:0')
    _, fwd, bwd = _operator(dev)
    for _ in range(CALLS):
        fwd()
        bwd()
    torch.cuda.synchronize()


def _profile():
    out = tempfile.mkdtemp(prefix='diffusion_train_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__),
           '--count-run']
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    stats = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if res.returncode != 0 or not stats:
        return {'profile': 'unmeasured (rocprofv3 rc %d)' % res.returncode, 'profile_stderr': res.stderr[-500:]}
    rec, bwd_calls = {}, 0
    with open(stats[0]) as fh:
        for row in csv.DictReader(fh):
            name = row['Name']
            for k in ('k_diffusion_bwd_rows', 'k_diffusion_bwd_reduce', 'k_diffusion_bwd_input', 'k_diffusion('):
                if k in name:
                    key = k.rstrip('(')
                    rec[key + '_us'] = round(float(row['AverageNs']) / 1e3, 2)
                    if key != 'k_diffusion':
                        bwd_calls += int(row['Calls'])
    rec['launches_per_backward'] = bwd_calls / CALLS
    return {'profiled_calls': CALLS, 'kernels': rec}


def main():
    if '--count-run' in sys.argv:
        _count_run()
        return
    dev = torch.device('cuda:0')
    rec = {'tool': 'diffusion_train_time', 'device': torch.cuda.get_device_name(0)}
    gph, fwd, bwd = _operator(dev)
    rec['operator'] = {'N': N, 'nnz': int(gph.adj.nnz), 'S': S, 'F': F, 'C': C, 'K1': 7}
    rec['operator']['forward_ms'] = round(_time_ms(fwd), 4)
    rec['operator']['backward_ms'] = round(_time_ms(bwd), 4)
    rec['operator']['backward_over_forward'] = round(rec['operator']['backward_ms'] / rec['operator']['forward_ms'], 2)
    rec['fit_eval_ms'] = {'Diffusion': _emulator(dev, 'Diffusion'), 'GAT': _emulator(dev, 'GAT')}
    if '--no-profile' not in sys.argv:
        rec.update(_profile())
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
