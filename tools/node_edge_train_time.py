"""Cost of training dense-parameter NodeEdge layers on ONE GPU: each layer as one autograd Function (`NodeEdge.dense_train` /
`Emulator.dense_node_edge_train = True`: autograd.NodeEdgeDenseFn, the whole matrix on the split-bf16 GEMM, d bias and d weight
from uds_node_edge_wgrad) against the default chain (`False`: spmm on the support + RemainderFn, sddmm, indexed reads, the mask
product, a library GEMM for d rest).

    python tools/node_edge_train_time.py [--out profiles/node_edge_train_time.json]

Networks: astlingen (30 nodes, 29 links) and RedChicoSur (443 nodes, 444 links) from tests/golden/networks.json at batch 1, 64
and 256, embed_size 64 and 128 (the NodeEdge input is embed_size / 2 wide); the actuated GAT model of tools/fit_tail_time.py,
2 + 2 spatial layers (8 NodeEdge layers), seq_in = seq_out = 5, temporal net Conv1D.
Per shape, in one process, WARM calls of every variant first, then REPS rounds calling each variant once in turn, device events
around every call, medians; the whole measurement RUNS times (`spread`: the largest relative difference of a median between runs):
  layer_on / layer_off      one NodeEdge (the node side: (N, E) parameters) forward on xs (batch * 5, E, embed / 2) + backward to
                            weight, bias and xs
  step_on / step_off        a whole `fit_eval` training step (forward, tail, backward, Adam)
`off_over_on` is the ratio of the medians in the same run; nothing is compared against a stored figure.
One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U                                     # noqa: E402
from gnn_uds_amd.layers import NodeEdge                     # noqa: E402

NETWORKS, BATCHES, EMBEDS = ('astlingen', 'RedChicoSur'), (1, 64, 256), (64, 128)
WARM, REPS, RUNS = 5, 20, 2
T = 5


def network(name):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))[name]
    return np.asarray(net['edges']), net['n_node'], np.asarray(net['is_outfall'], dtype=float)


def build(name, embed, dev):
    edges, n, outfall = network(name)
    e = len(edges)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=embed, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv='GAT', resnet=True, recurrent='Conv1D', roll=0, model_dir=None, tide=True,
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


def shape_fns(emul, n, e, batch, embed, dev):
    gen = torch.Generator().manual_seed(batch + n)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    x, a, b, ex = r(batch, T, n, 5), 0.1 + 0.9 * r(batch, T, 2), r(batch, T, n, 2) * 0.1, r(batch, T, e, 4)
    y, ey = r(batch, T, n, 5), r(batch, T, e, 3)
    y[..., -2] = (y[..., -2] > 0.7).float()
    layer = next(m for m in emul.modules() if isinstance(m, NodeEdge))
    layer.requires_grad_(True)
    xs, gy = r(batch * T, layer.shape[1], embed // 2).requires_grad_(True), r(batch * T, layer.shape[0], embed // 2)
    route = lambda on: 'dense' if on else 'support+remainder'
    name = lambda on: 'on' if on else 'off'

    def one_layer(on):
        def fn():
            layer.dense_train = on
            out = layer(xs)
            assert layer.last_train_path == route(on)
            return torch.autograd.grad(out, [layer.weight, layer.bias, xs], gy)
        return fn

    def step(on):
        def fn():
            emul.dense_node_edge_train = on
            out = emul.fit_eval(x, a, b, y, ex, ey)
            assert layer.last_train_path == route(on)
            return out
        return fn
    fns = {}
    for on in (True, False):
        fns['layer_' + name(on)], fns['step_' + name(on)] = one_layer(on), step(on)
    return fns


def main():
    dev = torch.device('cuda:0')
    rec = {'tool': 'node_edge_train_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs_per_shape': RUNS, 'seq_out': T,
           'model': 'GAT, act, 2 + 2 spatial layers (8 NodeEdge layers), Conv1D, hidden_dim 64, dense (R, M) NodeEdge parameters', 'shapes': []}
    for name in NETWORKS:
        for embed in EMBEDS:
            emul, n, e = build(name, embed, dev)
            for bs in BATCHES:
                fns = shape_fns(emul, n, e, bs, embed, dev)
                runs = [_alternate(fns, REPS) for _ in range(RUNS)]
                emul.dense_node_edge_train = False
                ms = {k: round(float(np.median([run[k] for run in runs])), 4) for k in runs[0]}
                spread = {k: round(max(run[k] for run in runs) / min(run[k] for run in runs) - 1, 4) for k in runs[0]}
                rec['shapes'].append({'network': name, 'n_node': n, 'n_edge': e, 'embed_size': embed, 'batch': bs, 'median_ms': ms, 'spread': spread,
                                      'off_over_on': {k: round(ms[k + '_off'] / ms[k + '_on'], 3) for k in ('layer', 'step')}})
                print('%s embed %d batch %d: %r' % (name, embed, bs, ms), file=sys.stderr, flush=True)
            del emul
    rec['slower_beyond_spread'] = [(s['network'], s['embed_size'], s['batch'], k) for s in rec['shapes'] for k in ('layer', 'step')
                                   if s['median_ms'][k + '_on'] > s['median_ms'][k + '_off'] * (1 + max(s['spread'][k + '_on'], s['spread'][k + '_off']))]
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
