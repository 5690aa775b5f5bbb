"""Cost of the GAT layer's backward on ONE GPU: `GATConv.fused_backward` / `Emulator.fused_gat_backward` on (one
uds_gat_backward_act call: activation backward, attention / aggregation backward, bias and attention-kernel gradients in three
launches) against off (act_grad, uds_gat_backward, the bias sum and the attention-kernel weight_grad as separate steps).

    python tools/gat_backward_time.py [--out profiles/gat_backward_time.json]

Layer: one GATConv (relu, bias, 64 input channels, precision bf16x3) forward + backward to the input and every parameter --
  c5_nodes / c5_links   1000 mini-graphs x (2 000 nodes / 2 500 links) as one block-diagonal pattern, one snapshot, d = 64 and 128
  astlingen / RedChicoSur (tests/golden/networks.json), node side, 64 x 5 snapshots, d = 64 and 128
Step: a whole `fit_eval` training step of the model of tools/fit_tail_time.py (Conv1D temporal net) on 100 mini-graphs at batch 1
(the C5-sized batch of tests/test_gpu_train.py) and on astlingen at batch 64.
Per shape, in one process, WARM calls of both variants first, then REPS rounds calling each once in turn, device events around every
call, medians; the whole measurement RUNS times (`spread`: the largest relative difference of a median between runs).  Every time
is compared with the flag-off path of the same commit in the same process.  One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gnn_uds_amd as U                                     # noqa: E402
from gnn_uds_amd import _lib                                # noqa: E402
from gnn_uds_amd import autograd as AG                      # noqa: E402
from gnn_uds_amd.layers import GATConv                      # noqa: E402
import fit_tail_time as FT                                  # noqa: E402

WARM, REPS, RUNS = 5, 30, 2
FIN = 64


def pattern(name):
    """(CSR with self loops, snapshots) of a layer shape."""
    if name.startswith('c5'):
        g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(2000, 2500, seed=0), 2000).replicated(1000)
        return (g.adj if name == 'c5_nodes' else g.edge_adj), 1
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))[name]
    return U.DrainageGraph.from_edges(np.asarray(net['edges']), net['n_node']).adj, 64 * 5


def layer_fns(csr, S, d, dev):
    h = _lib.CsrHandle(csr)
    layer = GATConv(d, activation='relu', in_channels=FIN, generator=torch.Generator().manual_seed(1)).to(dev)
    layer.precision = 'bf16x3'
    layer.requires_grad_(True)
    gen = torch.Generator().manual_seed(d + csr.n_rows)
    x = (torch.rand(S, csr.n_rows, FIN, generator=gen) - 0.5).to(dev).requires_grad_(True)
    gy = (torch.rand(S, csr.n_rows, d, generator=gen) - 0.5).to(dev)
    leaves = [x] + list(layer.parameters())

    def run(fused):
        def fn():
            layer.fused_backward = fused
            before = dict(AG.GAT_BWD_COUNTS)
            out = layer([x, h])
            grads = torch.autograd.grad(out, leaves, gy)
            assert AG.GAT_BWD_COUNTS['fused' if fused else 'chain'] == before['fused' if fused else 'chain'] + 1
            return grads
        return fn
    return {'on': run(True), 'off': run(False)}


def step_fns(emul, n, e, batch, dev):
    fns = FT.shape_fns(emul, n, e, batch, dev)

    def run(fused):
        def fn():
            emul.fused_gat_backward = fused
            return fns['step_hip']()
        return fn
    return {'on': run(True), 'off': run(False)}


def measure(fns, reps):
    runs = [FT._alternate(fns, reps) for _ in range(RUNS)]
    ms = {k: round(float(np.median([run[k] for run in runs])), 4) for k in runs[0]}
    spread = {k: round(max(run[k] for run in runs) / min(run[k] for run in runs) - 1, 4) for k in runs[0]}
    return {'median_ms': ms, 'spread': spread, 'off_over_on': round(ms['off'] / ms['on'], 3)}


def main():
    dev = torch.device('cuda:0')
    FT.WARM = WARM
    rec = {'tool': 'gat_backward_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs_per_shape': RUNS,
           'layer': 'GATConv relu + bias, %d input channels, bf16x3, forward + backward to input and parameters' % FIN, 'layers': [], 'steps': []}
    for name in ('astlingen', 'RedChicoSur', 'c5_nodes', 'c5_links'):
        csr, S = pattern(name)
        for d in (64, 128):
            m = measure(layer_fns(csr, S, d, dev), 10 if name.startswith('c5') else REPS)
            rec['layers'].append(dict({'shape': name, 'rows': csr.n_rows, 'nnz': csr.nnz, 'snapshots': S, 'd': d}, **m))
            print('layer %s d %d: %r' % (name, d, m), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    for name, batch in (('astlingen', 64), ('c5', 1)):
        emul, n, e = FT.build(name, 'Conv1D', dev)
        m = measure(step_fns(emul, n, e, batch, dev), 10 if name == 'c5' else REPS)
        rec['steps'].append(dict({'network': name, 'n_node': n, 'n_edge': e, 'batch': batch, 'recurrent': 'Conv1D'}, **m))
        print('step %s batch %d: %r' % (name, batch, m), file=sys.stderr, flush=True)
        del emul
        torch.cuda.empty_cache()
    rec['slower_beyond_spread'] = [[r.get('shape', r.get('network')), r.get('d', r.get('batch'))] for r in rec['layers'] + rec['steps']
                                   if r['median_ms']['on'] > r['median_ms']['off'] * (1 + max(r['spread'].values()))]
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
