"""Cost of the training tail on ONE GPU: everything `Emulator.fit_eval` does after the network forward as one HIP operator
(`emul.fused_fit_tail = True`: uds_fit_tail / uds_fit_tail_backward through autograd.FitTailFn) against the tensor code (`False`).

    python tools/fit_tail_time.py [--out profiles/fit_tail_time.json]
    python tools/fit_tail_time.py --control [--root TREE]      # one shape, tensor route only: this tree against another one

Networks: astlingen (30 nodes) and RedChicoSur (443 nodes) from tests/golden/networks.json at batch 1, 64 and 256, and one
block-diagonal network of 100 mini-graphs x (2 000 nodes, 2 500 links), the C5-sized batch of tests/test_gpu_train.py, at batch 1;
an actuated GAT model with rated pumps on every link, node pumps, offsets, a tide boundary and a flood channel (no edge fusion),
embed 64, 2 + 2 spatial layers, seq_in = seq_out = 5, temporal net Conv1D and GRU (the large network: Conv1D only).
Per shape, in one process, WARM calls of every variant first, then REPS rounds calling each variant once in turn, device events
around every call, medians; the whole measurement RUNS times (`spread`: the largest relative difference of a median between runs):
  tail_hip / tail_torch     forward of the tail + its backward to the network outputs y and ey (fixed outputs as leaves)
  step_hip / step_torch     a whole `fit_eval` training step (forward, tail, backward, Adam)
`tail_share_torch`: tail_torch / step_torch, the part of a step the tensor-code tail is.
--control times step_torch alone on one shape (RedChicoSur, batch 64, Conv1D) with the package found under --root (default: this
tree): run on the parent commit's tree and on this one, it shows that the tensor route is what it was.
One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = os.path.abspath(sys.argv[sys.argv.index('--root') + 1]) if '--root' in sys.argv else ROOT
sys.path.insert(0, PKG_ROOT)
import gnn_uds_amd as U                                     # noqa: E402

NETWORKS, BATCHES, RECURRENT = ('astlingen', 'RedChicoSur'), (1, 64, 256), ('Conv1D', 'GRU')
WARM, REPS, RUNS = 5, 30, 2
T = 5


def network(name):
    if name == 'c5':
        n1, e1, G = 2000, 2500, 100
        edges = np.concatenate([U.synthetic_drainage_network(n1, e1, seed=k) + n1 * k for k in range(G)])
        return edges, n1 * G, (np.arange(n1 * G) % n1 == 0).astype(float)
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))[name]
    return np.asarray(net['edges']), net['n_node'], np.asarray(net['is_outfall'], dtype=float)


def build(name, recurrent, dev):
    edges, n, outfall = network(name)
    e = len(edges)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv='GAT', resnet=True, recurrent=recurrent, roll=0, model_dir=None, tide=True,
        is_outfall=outfall, hmax=1.0 + rng.random(n), hmin=np.zeros(n), area=0.2 + rng.random(n), learning_rate=1e-5,
        pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
        offset=rng.random(e) * (rng.random(e) > 0.5), ehmax=0.3 + rng.random(e))
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, 4))
    return emul, n, e


def _alternate(fns, reps):
    """name -> median ms per call: WARM calls of each, then `reps` rounds calling each once in turn, one event pair per call."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            ev[k].append((t0, t1))
    torch.cuda.synchronize()
    return {k: round(float(np.median([a.elapsed_time(b) for a, b in pairs])), 4) for k, pairs in ev.items()}


def shape_fns(emul, n, e, batch, dev):
    gen = torch.Generator().manual_seed(batch + n)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    x, a, b, ex = r(batch, T, n, 5), 0.1 + 0.9 * r(batch, T, 2), r(batch, T, n, 2) * 0.1, r(batch, T, e, 4)
    y, ey = r(batch, T, n, 5), r(batch, T, e, 3)
    y[..., -2] = (y[..., -2] > 0.7).float()
    with torch.no_grad():
        ny, ney = emul.forward(x, b, ex, emul.get_edge_action(a, True))
    ly, ley = ny.clone().requires_grad_(True), ney.clone().requires_grad_(True)
    route = lambda fused: 'hip' if fused else 'torch'

    def tail(fused):
        def fn():
            emul.fused_fit_tail = fused
            emul.forward = lambda *args, **kw: (ly, ley)
            try:
                node, fl, edge = emul._fit_losses(x, a, b, y, ex, ey, emul.get_edge_action(a, True), False)
            finally:
                del emul.forward
            assert emul.last_fit_tail_path == route(fused)
            return torch.autograd.grad(node + fl + edge, [ly, ley])
        return fn

    def step(fused):
        def fn():
            emul.fused_fit_tail = fused
            out = emul.fit_eval(x, a, b, y, ex, ey)
            assert getattr(emul, 'last_fit_tail_path', 'torch') == route(fused)
            return out
        return fn
    fns = {}
    for fused in (True, False):
        fns['tail_' + route(fused)], fns['step_' + route(fused)] = tail(fused), step(fused)
    return fns


def control(dev):
    """step_torch on one shape with the package under PKG_ROOT (which may be a tree from before the operator existed)."""
    emul, n, e = build('RedChicoSur', 'Conv1D', dev)
    emul.fused_fit_tail = False                             # a tree from before the operator ignores it: fit_eval is the tensor code there
    gen = torch.Generator().manual_seed(64 + n)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    x, a, b, ex = r(64, T, n, 5), 0.1 + 0.9 * r(64, T, 2), r(64, T, n, 2) * 0.1, r(64, T, e, 4)
    y, ey = r(64, T, n, 5), r(64, T, e, 3)
    y[..., -2] = (y[..., -2] > 0.7).float()
    runs = [_alternate({'step_torch': lambda: emul.fit_eval(x, a, b, y, ex, ey)}, 3 * REPS)['step_torch'] for _ in range(RUNS)]
    return {'tool': 'fit_tail_time --control', 'root': os.path.relpath(PKG_ROOT, ROOT), 'network': 'RedChicoSur', 'batch': 64, 'recurrent': 'Conv1D',
            'step_torch_ms': runs}


def main():
    dev = torch.device('cuda:0')
    if '--control' in sys.argv:
        print(json.dumps(control(dev)))
        return
    rec = {'tool': 'fit_tail_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs_per_shape': RUNS, 'seq_out': T,
           'model': 'GAT, act, rated pumps on every link, node pumps, offsets, tide, flood channel, epsilon 0.1, no edge fusion', 'shapes': []}
    shapes = [(name, rc, bs) for name in NETWORKS for rc in RECURRENT for bs in BATCHES] + [('c5', 'Conv1D', 1)]
    models = {}
    for name, rc, bs in shapes:
        if (name, rc) not in models:
            models[(name, rc)] = build(name, rc, dev)
        emul, n, e = models[(name, rc)]
        fns = shape_fns(emul, n, e, bs, dev)
        runs = [_alternate(fns, REPS if name != 'c5' else 10) for _ in range(RUNS)]
        emul.fused_fit_tail = type(emul).fused_fit_tail
        ms = {k: round(float(np.median([run[k] for run in runs])), 4) for k in runs[0]}
        spread = {k: round(max(run[k] for run in runs) / min(run[k] for run in runs) - 1, 4) for k in runs[0]}
        rec['shapes'].append({'network': name, 'n_node': n, 'n_edge': e, 'recurrent': rc, 'batch': bs, 'median_ms': ms, 'spread': spread,
                              'torch_over_hip': {k: round(ms[k + '_torch'] / ms[k + '_hip'], 3) for k in ('tail', 'step')},
                              'tail_share_torch': round(ms['tail_torch'] / ms['step_torch'], 3)})
        print('%s %s batch %d: %r' % (name, rc, bs, ms), file=sys.stderr, flush=True)
        if name == 'c5':
            del models[(name, rc)]
    rec['slower_beyond_spread'] = [(s['network'], s['recurrent'], s['batch'], k) for s in rec['shapes'] for k in ('tail', 'step')
                                   if s['median_ms'][k + '_hip'] > s['median_ms'][k + '_torch'] * (1 + max(s['spread'][k + '_hip'], s['spread'][k + '_torch']))]
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
