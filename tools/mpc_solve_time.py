"""Cost of an MPC population evaluation and of one cross-entropy iteration on ONE GPU: `mpc.Problem` (history shared by the
population, objective as one HIP operator) against the replicated path it sits next to (`mpc.objective_and_gradient`).

    python tools/mpc_solve_time.py [--out profiles/mpc_solve_time.json] [--quick]

Networks: astlingen (30 nodes) and RedChicoSur (443 nodes) from tests/golden/networks.json, the actuated model of
tools/predict_tail_time.py without its tide (rated pumps, node pumps, offsets; no edge fusion), seq_in = seq_out = 5; pop = 16, 64, 256
candidates; a horizon of one chunk and of three.  Per shape, alternated call by call in one process after WARM calls of every
variant, REPS timed calls each with device events around every call, medians; the whole measurement twice (run-to-run spread):
  forward_shared / forward_replicated     `Problem.objective` with shared_history on / off (fused objective on both)
  grad_shared / grad_replicated           `Problem.objective_and_gradient` with shared_history on / `mpc.objective_and_gradient`
                                          (the replicated prefix and the tensor objective: what the package offered before)
  objective_hip / objective_torch         the objective alone on fixed predictions: uds_mpc_objective / `mpc.objective_pred`
  objective_grad_hip / objective_grad_torch   ... forward and backward (d_preds)
  ce_iteration                            draw + `Problem.objective` + update: one iteration of `solve_ce` (n_elite = pop / 4)
Launch-bound shapes: the times are those of the launch sequences, not of the bytes moved.  --quick: RUNS = 1, fewer calls.
One JSON line; with --out PATH it is written there too.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnn_uds_amd import _lib                                # noqa: E402
from gnn_uds_amd import autograd as AG                      # noqa: E402
from gnn_uds_amd import mpc as M                            # noqa: E402
import gnn_uds_amd as U                                     # noqa: E402

NETWORKS, POPS, CHUNKS = ('astlingen', 'RedChicoSur'), (16, 64, 256), (1, 3)
QUICK = '--quick' in sys.argv
WARM, REPS, RUNS = (3, 15, 1) if QUICK else (5, 30, 2)
T, N_ACT = 5, 2


def build(name, dev):
    """The model of tools/predict_tail_time.py without its tide boundary (a fed-back chunk has no tide channel to carry)."""
    from types import SimpleNamespace
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))[name]
    edges, n = np.asarray(net['edges']), net['n_node']
    e = len(edges)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv='GAT', resnet=True, recurrent='Conv1D', roll=0, model_dir=None, tide=False,
        is_outfall=np.asarray(net['is_outfall'], dtype=float), hmax=1.0 + rng.random(n), hmin=np.zeros(n), area=0.2 + rng.random(n),
        pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
        offset=rng.random(e) * (rng.random(e) > 0.5), ehmax=0.3 + rng.random(e))
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 1), mk(n, 5), mk(n, 1), mk(e, 4))
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


def shape_fns(emul, n, e, pop, chunks, dev):
    gen = torch.Generator().manual_seed(pop + n + chunks)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    Th = T * chunks
    state, runoff, edge_state = r(T, n, 5), r(Th, n, 1) * 0.05, r(T, e, 4)
    n_step, r_step = chunks, T
    y = 0.2 + 0.6 * r(pop, n_step * N_ACT)
    k = len(range(0, n, 3))
    targets = dict(flood_idx=torch.arange(0, n, 3, device=dev), flood_w=torch.ones(k, device=dev), outflow_idx=torch.tensor([0], device=dev),
                   outflow_w=torch.tensor([0.3], device=dev), smooth_idx=torch.arange(1, n, 5, device=dev),
                   smooth_w=torch.full((len(range(1, n, 5)),), 0.2, device=dev))
    gamma = (0.97 ** torch.arange(Th)).float().to(dev)
    shared = M.Problem(emul, state, runoff, edge_state, n_step, N_ACT, r_step, targets, gamma)
    repl = M.Problem(emul, state, runoff, edge_state, n_step, N_ACT, r_step, targets, gamma, shared_history=False)
    with torch.no_grad():
        preds = shared.predict(y)[0].contiguous()
    st = state.unsqueeze(0).expand((pop,) + tuple(state.shape))
    w, q0 = shared.weights, state[-1, :, 1].contiguous()
    leaf = preds.clone().requires_grad_(True)
    mean, std = torch.full((shared.n_var,), 0.5, device=dev), torch.full((shared.n_var,), 0.3, device=dev)
    count, status = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    best_y, best_obj, cand = torch.zeros(shared.n_var, device=dev), torch.full((1,), float('inf'), device=dev), torch.empty(pop, shared.n_var, device=dev)

    def ce_iteration():
        mean.fill_(0.5), std.fill_(0.3)               # the same distribution every call: the same work
        _lib.ce_draw(mean, std, 1, count, pop, out=cand)
        _lib.ce_update(cand, shared.objective(cand).contiguous(), max(1, pop // 4), 0.3, 1e-3, mean, std, best_y, best_obj, status)

    def checked(problem, paths, fn):
        def run():
            out = fn()
            assert problem.last_paths == paths, problem.last_paths
            return out
        return run
    return {
        'forward_shared': checked(shared, {'prefix': 'shared', 'objective': 'hip'}, lambda: shared.objective(y)),
        'forward_replicated': checked(repl, {'prefix': 'replicated', 'objective': 'hip'}, lambda: repl.objective(y)),
        'grad_shared': checked(shared, {'prefix': 'shared', 'objective': 'hip'}, lambda: shared.objective_and_gradient(y)),
        'grad_replicated': lambda: M.objective_and_gradient(emul, y, state, runoff, edge_state, n_step, N_ACT, r_step, targets, gamma),
        'objective_hip': lambda: _lib.mpc_objective(preds, q0, w['flood'], w['outflow'], w['smooth'], gamma),
        'objective_torch': lambda: M.objective_pred(preds, st, gamma=gamma, **targets),
        'objective_grad_hip': lambda: torch.autograd.grad(AG.MpcObjectiveFn.apply(leaf, q0, w['flood'], w['outflow'], w['smooth'], gamma).sum(), leaf),
        'objective_grad_torch': lambda: torch.autograd.grad(M.objective_pred(leaf, st, gamma=gamma, **targets).sum(), leaf),
        'ce_iteration': ce_iteration,
    }


def main():
    dev = torch.device('cuda:0')
    rec = {'tool': 'mpc_solve_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'seq_out': T,
           'model': 'act, rated pumps on every link, node pumps, offsets, epsilon 0.1, no edge fusion', 'runs': []}
    models = {name: build(name, dev) for name in NETWORKS}
    for _ in range(RUNS):
        run = []
        for name in NETWORKS:
            emul, n, e = models[name]
            for chunks in CHUNKS:
                for pop in POPS:
                    ms = _alternate(shape_fns(emul, n, e, pop, chunks, dev))
                    run.append({'network': name, 'n_node': n, 'n_edge': e, 'pop': pop, 'chunks': chunks, 'median_ms': ms,
                                'replicated_over_shared': {k: round(ms[k + '_replicated'] / ms[k + '_shared'], 3) for k in ('forward', 'grad')},
                                'torch_over_hip': {k: round(ms[k + '_torch'] / ms[k + '_hip'], 3) for k in ('objective', 'objective_grad')}})
        rec['runs'].append(run)
    if RUNS > 1:
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
