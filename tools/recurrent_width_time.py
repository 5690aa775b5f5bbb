"""Cost of a GRU / LSTM temporal layer at hidden_dim 16, 32, 64 and 128 on ONE GPU: forward + backward of one layer (the Dense
input projection and RecurrentFn, what `_Recurrent.forward` runs under autograd) on the headline rows.

    python tools/recurrent_width_time.py                       timing + a kernel-trace child run under rocprofv3 + fit_eval
    python tools/recurrent_width_time.py --no-profile          timing only
    python tools/recurrent_width_time.py --widths 64 --layer-only --no-profile
                                                               the control: runs unchanged on a tree that only has the 64-unit kernel
    python tools/recurrent_width_time.py --count-run           (the child: STEPS steps of every (kind, H), nothing printed)

Workload: B = 1, T = 60, R = 10 000 rows, input width F = H (a second temporal layer), precision 'bf16x3', seeded input.
Timing: WARM warm-up steps of every (kind, H), then ROUNDS rounds; a round times REPS steps of each (kind, H) in turn, one
device-event pair per step -- every (kind, H) is timed ROUNDS times, alternating, so the spread between rounds is known.
Operations from shapes, per step and row: the three split-bf16 products of  h U  (recomputed) and of  d_arec U^T  are
2 * 3 * 2 G H^2 flop, 4 x per doubling of H; the forward recurrence is 2 G H^2 in fp32.
Also: whole `fit_eval` of the C2-size model (N = 2 000, E = 2 500, 3 + 3 spatial layers, 2 + 2 temporal layers, B = 2, T = 5)
with recurrent = 'GRU' at hidden_dim 64 and 128.  One JSON line; with --out PATH it is written there too.
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
from gnn_uds_amd.emulator import GRU, LSTM   # noqa: E402

B, T, R = 1, 60, 10000
WIDTHS = (16, 32, 64, 128)
WARM, REPS, ROUNDS, STEPS = 10, 50, 3, 5


def _widths():
    if '--widths' in sys.argv:
        return tuple(int(w) for w in sys.argv[sys.argv.index('--widths') + 1].split(','))
    return WIDTHS


def _step_fn(dev, kind, H):
    g = torch.Generator().manual_seed(H)
    mod = (GRU if kind == 'GRU' else LSTM)(H, in_features=H, generator=g, precision='bf16x3').to(dev)
    mod.requires_grad_(True)
    x = torch.randn(B, T, R, H, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(B, T, R, H, generator=g).to(dev)

    def step():
        mod(x).backward(gy)
    return step


def _layer_times(dev, widths):
    fns = {(kind, H): _step_fn(dev, kind, H) for kind in ('GRU', 'LSTM') for H in widths}
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            pairs = []
            for _ in range(REPS):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                pairs.append((t0, t1))
            torch.cuda.synchronize()
            rounds[k].append(float(np.mean([a.elapsed_time(b) for a, b in pairs])))
    out = {}
    for (kind, H), ms in rounds.items():
        G = 3 if kind == 'GRU' else 4
        out['%s_%d' % (kind, H)] = {'round_mean_ms': [round(m, 4) for m in ms], 'mean_ms': round(float(np.mean(ms)), 4),
                                    'spread': round((max(ms) - min(ms)) / min(ms), 4),
                                    'backward_mfma_gflop_per_step': round(2 * 3 * 2 * G * H * H * B * T * R / 1e9, 2)}
    for kind in ('GRU', 'LSTM'):
        base = out.get('%s_64' % kind)
        if base:
            for H in widths:
                out['%s_%d' % (kind, H)]['over_64'] = round(out['%s_%d' % (kind, H)]['mean_ms'] / base['mean_ms'], 3)
    return out


def _fit_eval_ms(dev, hidden):
    from oracle import graphs as OG          # the dense adjacency / incidence builders the reference-style args carry
    n, e = 2000, 2500
    edges = U.synthetic_drainage_network(n, e, 0)
    a = SimpleNamespace(state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=hidden, kernel_size=3,
                        n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=edges, act=False,
                        adj=OG.adjacency(edges), edge_adj=OG.edge_adjacency(edges), node_edge=OG.node_edge_incidence(n, edges),
                        conv='GAT', model_dir=None, learning_rate=1e-3)
    emul = U.Emulator('GAT', True, 'GRU', a, generator=torch.Generator().manual_seed(1)).to(dev)
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
    for kind in ('GRU', 'LSTM'):
        for H in _widths():
            fn = _step_fn(dev, kind, H)
            for _ in range(STEPS):
                fn()
    torch.cuda.synchronize()


def _profile():
    out = tempfile.mkdtemp(prefix='recurrent_width_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__),
           '--count-run']
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    stats = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if res.returncode != 0 or not stats:
        return {'profile': 'not measured (rocprofv3 rc %d)' % res.returncode, 'profile_stderr': res.stderr[-500:]}
    kernels, launches = {}, 0
    with open(stats[0]) as fh:
        for row in csv.DictReader(fh):
            launches += int(row['Calls'])
            if 'k_recurrent' in row['Name']:
                kernels[row['Name']] = {'calls': int(row['Calls']), 'avg_us': round(float(row['AverageNs']) / 1e3, 2)}
    n_steps = STEPS * 2 * len(_widths())
    return {'profile': {'steps_per_kind_and_width': STEPS, 'recurrent_kernels': kernels, 'launches_total': launches,
                        'launches_per_step_mean': round(launches / n_steps, 1)}}


def main():
    if '--count-run' in sys.argv:
        _count_run()
        return
    dev = torch.device('cuda:0')
    widths = _widths()
    rec = {'tool': 'recurrent_width_time', 'device': torch.cuda.get_device_name(0), 'B': B, 'T': T, 'R': R, 'warm': WARM, 'reps': REPS,
           'rounds': ROUNDS, 'step': 'Dense projection + RecurrentFn, forward + backward, F = H, bf16x3'}
    rec['layer'] = _layer_times(dev, widths)
    if '--layer-only' not in sys.argv:
        rec['fit_eval_ms_c2_gru'] = {'hidden_dim_%d' % h: _fit_eval_ms(dev, h) for h in (64, 128)}
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
