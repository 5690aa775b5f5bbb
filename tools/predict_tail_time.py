"""Cost of the predict tail on ONE GPU: `Emulator.predict_tf` and `mpc.objective_and_gradient` with the tail as one HIP operator
(`emul.fused_tail = True`: uds_predict_tail / uds_predict_tail_backward) against the tensor code it replaces (`False`).

    python tools/predict_tail_time.py [--out profiles/predict_tail_time.json]

Networks: astlingen (30 nodes) and RedChicoSur (443 nodes) from tests/golden/networks.json, as an actuated model with rated
pumps on every link, node pumps, offsets and a tide boundary (no edge fusion: node gates, pumped-storage depth scan, epsilon
band), seq_in = seq_out = 5, one prediction chunk; pop = 1 and 64 candidates.  Per shape, alternated call by call in one
process after WARM calls of every variant, REPS timed calls each with device events around every call, medians; the whole
measurement twice (run-to-run spread):
  predict_tf_hip / predict_tf_torch     `predict_tf` under no_grad, the whole call (network forward + tail)
  tail_hip / tail_torch                 the same call with the network forward replaced by fixed outputs: the tail alone
  mpc_hip / mpc_torch                   `mpc.objective_and_gradient`: forward, objective and the gradient w.r.t. the decision vector
  mpc_tail_hip / mpc_tail_torch         forward + backward of the tail alone (fixed network outputs as leaves)
`launch-bound` shapes: the times are those of the launch sequence, not of the bytes moved (a few hundred KB).
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
from gnn_uds_amd import mpc as M                            # noqa: E402

NETWORKS, POPS = ('astlingen', 'RedChicoSur'), (1, 64)
WARM, REPS, RUNS = 10, 100, 2
T = 5


def build(name, dev):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))[name]
    edges, n = np.asarray(net['edges']), net['n_node']
    e = len(edges)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv='GAT', resnet=True, recurrent='Conv1D', roll=0, model_dir=None, tide=True,
        is_outfall=np.asarray(net['is_outfall'], dtype=float), hmax=1.0 + rng.random(n), hmin=np.zeros(n), area=0.2 + rng.random(n),
        pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
        offset=rng.random(e) * (rng.random(e) > 0.5), ehmax=0.3 + rng.random(e))
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, 4))
    return emul, n, e


def _alternate(fns):
    """name -> median ms per call: WARM calls of each, then REPS rounds calling each once in turn, one event pair per call."""
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
    return {k: round(float(np.median([a.elapsed_time(b) for a, b in pairs])), 4) for k, pairs in ev.items()}


def shape_fns(emul, n, e, pop, dev):
    gen = torch.Generator().manual_seed(pop + n)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    state, runoff, edge_state = r(T, n, 5), r(T, n, 2) * 0.05, r(T, e, 4)
    y = 0.2 + 0.6 * r(pop, 2)
    rep = lambda t: t.unsqueeze(0).expand((pop,) + tuple(t.shape)).contiguous()
    X, Bd, Ex, a = rep(state), rep(runoff), rep(edge_state), M.expand_settings(y, 1, 2, T, T)
    targets = dict(flood_idx=torch.arange(0, n, 3, device=dev), flood_w=torch.ones(len(range(0, n, 3)), device=dev),
                   outflow_idx=torch.tensor([0], device=dev), outflow_w=torch.tensor([0.3], device=dev))
    with torch.no_grad():
        ny, ney = emul.forward(emul.normalize(X, 'x'), emul.normalize(Bd, 'b'), emul.normalize(Ex, 'e'), emul.get_edge_action(a, True))
    gy, gey = r(pop, T, n, 5), r(pop, T, e, 3)

    def predict(fused, tail_only):
        def fn():
            emul.fused_tail = fused
            if tail_only:
                emul.forward = lambda *args, **kw: (ny, ney)
            try:
                with torch.no_grad():
                    out = emul.predict_tf(X, Bd, a, Ex)
            finally:
                if tail_only:
                    del emul.forward
            assert emul.last_tail_path == ('hip' if fused else 'torch')
            return out
        return fn

    def mpc(fused):
        def fn():
            emul.fused_tail = fused
            out = M.objective_and_gradient(emul, y, state, runoff, edge_state, 1, 2, T, targets)
            assert emul.last_tail_path == ('hip-train' if fused else 'torch')
            return out
        return fn

    def mpc_tail(fused):
        ly, ley, la = ny.clone().requires_grad_(True), ney.clone().requires_grad_(True), a.clone().requires_grad_(True)
        lx = X.clone().requires_grad_(True)

        def fn():
            emul.fused_tail = fused
            emul.forward = lambda *args, **kw: (ly, ley)
            try:
                oy, oey = emul.predict_tf(lx, Bd, la, Ex)
            finally:
                del emul.forward
            assert emul.last_tail_path == ('hip-train' if fused else 'torch')
            return torch.autograd.grad([oy, oey], [ly, ley, la, lx], [gy, gey])
        return fn
    return {'predict_tf_hip': predict(True, False), 'predict_tf_torch': predict(False, False), 'tail_hip': predict(True, True),
            'tail_torch': predict(False, True), 'mpc_hip': mpc(True), 'mpc_torch': mpc(False), 'mpc_tail_hip': mpc_tail(True),
            'mpc_tail_torch': mpc_tail(False)}


def main():
    dev = torch.device('cuda:0')
    rec = {'tool': 'predict_tail_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'seq_out': T,
           'model': 'act, rated pumps on every link, node pumps, offsets, tide, epsilon 0.1, no edge fusion', 'runs': []}
    models = {name: build(name, dev) for name in NETWORKS}
    for _ in range(RUNS):
        run = []
        for name in NETWORKS:
            emul, n, e = models[name]
            for pop in POPS:
                ms = _alternate(shape_fns(emul, n, e, pop, dev))
                emul.fused_tail = True
                run.append({'network': name, 'n_node': n, 'n_edge': e, 'pop': pop, 'median_ms': ms,
                            'torch_over_hip': {k: round(ms[k + '_torch'] / ms[k + '_hip'], 3) for k in ('predict_tf', 'tail', 'mpc', 'mpc_tail')}})
        rec['runs'].append(run)
    rec['run_to_run_spread'] = round(max(abs(p['median_ms'][k] - q['median_ms'][k]) / p['median_ms'][k]
                                         for p, q in zip(*rec['runs']) for k in p['median_ms']), 4)
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
