"""Cost of the weight gradients of a default-size model (embed_size 128, hidden_dim 64) on ONE GPU: the wide split-K entry
(uds_wgrad_wide through _lib.wgrad_wide) against the route these shapes took before it existed (torch.mm, the library GEMM) and
against a composition of uds_wgrad calls over slices it takes.

    python tools/wgrad_wide_time.py [--out profiles/wgrad_wide_time.json] [--quick]

Per shape (F [+ bias row], H) of the model -- Dense 128+b -> 64, the GAT kernels 192 x 128 / 64 x 128, 64+b -> 128 (res_x / res_e),
128+b -> 3 (e_out), the GRU / LSTM projections 128+b -> 192 and 64+b -> 256 -- at 600 000 rows (N = 10 000 nodes x T = 60) and
720 000 rows (E = 12 000 links x T = 60), in one process, WARM calls of every variant first, then REPS rounds calling each variant
once in turn, device events around every call, medians; the whole measurement RUNS times (`spread`: the largest relative
difference of a median between runs):
  wide        _lib.wgrad_wide
  library     a^T @ g by torch.mm, plus g.sum(0) where the bias is wanted: what autograd.weight_grad did for these shapes
  composed    _lib.wgrad over column slices of 64 and row slices of at most 128 (127 with the bias row), the slicing copies included
`floor_us`: rows (F + H) 4 bytes over the HBM rate a float4 copy reaches on this GPU (6.29 TB/s; the data sheet says 8).
Then a whole `fit_eval` training step of the default-size model (2 + 2 layers, Conv1D and GRU) on a synthetic network with
autograd.WIDE_WGRAD on and off, and autograd.ROUTE_COUNTS of one step each way.
One JSON line; with --out PATH it is written there too.  --quick: a twentieth of the rows, 3 rounds (a rehearsal, not a measurement).
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
from gnn_uds_amd import _lib                                # noqa: E402
from gnn_uds_amd import autograd as AG                      # noqa: E402

QUICK = '--quick' in sys.argv
SHAPES = [(128, 64, True), (192, 128, False), (64, 128, False), (64, 128, True), (128, 3, True), (128, 192, True), (64, 256, True)]
ROWS = (30000, 36000) if QUICK else (600000, 720000)
WARM, REPS, RUNS = (2, 3, 2) if QUICK else (5, 30, 2)
HBM_BYTES_PER_S = 6.29e12
STEP_NET = (500, 600, 4) if QUICK else (2000, 2500, 16)      # nodes, links, batch
T = 5


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


def _measure(fns, reps):
    runs = [_alternate(fns, reps) for _ in range(RUNS)]
    ms = {k: round(float(np.median([run[k] for run in runs])), 4) for k in runs[0]}
    spread = {k: round(max(run[k] for run in runs) / min(run[k] for run in runs) - 1, 4) for k in runs[0]}
    return ms, spread


def composed(a, g, bias):
    """(dW, db) from uds_wgrad alone: column slices of 64, row slices of at most 128 rows of the output the bias row included."""
    F, H = a.shape[-1], g.shape[-1]
    nf = -(-(F + int(bias)) // 128)
    fstep = -(-F // nf)
    dk = torch.empty(F, H, device=a.device)
    db = torch.empty(H, device=a.device) if bias else None
    for c0 in range(0, H, 64):
        gc = g if H <= 64 else g[..., c0:c0 + 64].contiguous()
        for f0 in range(0, F, fstep):
            last = f0 + fstep >= F
            ac = a if nf == 1 else a[..., f0:f0 + fstep].contiguous()
            k, b = _lib.wgrad(ac, gc, 0, bias and last)
            dk[f0:f0 + fstep, c0:c0 + 64] = k
            if b is not None:
                db[c0:c0 + 64] = b
    return dk, db


def shape_record(F, H, bias, rows, dev):
    gen = torch.Generator().manual_seed(F * 1000 + H)
    a = (torch.rand(1, 1, rows, F, generator=gen) - 0.5).to(dev)
    g = (torch.rand(1, 1, rows, H, generator=gen) - 0.5).to(dev)
    a2, g2 = a.reshape(rows, F), g.reshape(rows, H)
    fns = {'wide': lambda: _lib.wgrad_wide(a, g, 0, bias),
           'library': lambda: (a2.t().mm(g2), g2.sum(0) if bias else None),
           'composed': lambda: composed(a, g, bias)}
    ref = fns['library']()
    for k in ('wide', 'composed'):                         # faster and different is not faster
        got = fns[k]()
        tol = 4e-5 * max(1.0, (rows / 1000.0) ** 0.5) * max(1.0, float(ref[0].abs().max()))
        assert float((got[0] - ref[0]).abs().max()) <= tol, (k, F, H)
        assert not bias or float((got[1] - ref[1]).abs().max()) <= tol * 4, (k, F, H)
    ms, spread = _measure(fns, REPS)
    floor_us = rows * (F + H) * 4 / HBM_BYTES_PER_S * 1e6
    return {'F': F, 'H': H, 'bias': bias, 'rows': rows, 'median_ms': ms, 'spread': spread, 'floor_us': round(floor_us, 1),
            'library_over_wide': round(ms['library'] / ms['wide'], 3), 'composed_over_wide': round(ms['composed'] / ms['wide'], 3),
            'wide_over_floor': round(ms['wide'] * 1e3 / floor_us, 2)}


def build(recurrent, dev):
    n, e, _ = STEP_NET
    edges = U.synthetic_drainage_network(n, e, seed=1)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=128, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv='GAT', resnet=True, recurrent=recurrent, roll=0, model_dir=None, tide=True,
        is_outfall=(np.arange(n) == 0).astype(float), hmax=1.0 + rng.random(n), hmin=np.zeros(n), area=0.2 + rng.random(n), learning_rate=1e-5,
        pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
        offset=rng.random(e) * (rng.random(e) > 0.5), ehmax=0.3 + rng.random(e))
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, 4))
    return emul


def step_record(recurrent, dev):
    n, e, batch = STEP_NET
    emul = build(recurrent, dev)
    gen = torch.Generator().manual_seed(batch + n)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    x, a, b, ex = r(batch, T, n, 5), 0.1 + 0.9 * r(batch, T, 2), r(batch, T, n, 2) * 0.1, r(batch, T, e, 4)
    y, ey = r(batch, T, n, 5), r(batch, T, e, 3)
    y[..., -2] = (y[..., -2] > 0.7).float()

    def step(wide):
        def fn():
            before, AG.WIDE_WGRAD = AG.WIDE_WGRAD, wide
            try:
                return emul.fit_eval(x, a, b, y, ex, ey)
            finally:
                AG.WIDE_WGRAD = before
        return fn
    fns = {'step_wide': step(True), 'step_library': step(False)}
    counts = {}
    for k, fn in fns.items():
        fn()
        for key in AG.ROUTE_COUNTS:
            AG.ROUTE_COUNTS[key] = 0
        fn()
        counts[k] = dict(AG.ROUTE_COUNTS)
    ms, spread = _measure(fns, max(3, REPS // 3))
    return {'recurrent': recurrent, 'n_node': n, 'n_edge': e, 'batch': batch, 'seq': T, 'median_ms': ms, 'spread': spread,
            'route_counts': counts, 'library_over_wide': round(ms['step_library'] / ms['step_wide'], 3)}


def main():
    dev = torch.device('cuda:0')
    rec = {'tool': 'wgrad_wide_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs': RUNS, 'quick': QUICK,
           'hbm_bytes_per_s': HBM_BYTES_PER_S, 'shapes': [], 'steps': []}
    for F, H, bias in SHAPES:
        for rows in ROWS:
            s = shape_record(F, H, bias, rows, dev)
            rec['shapes'].append(s)
            print('%3d%s x %3d, %d rows: %r floor %.0f us' % (F, '+b' if bias else '  ', H, rows, s['median_ms'], s['floor_us']), file=sys.stderr, flush=True)
    rec['slower_than_library_beyond_spread'] = [(s['F'], s['H'], s['bias'], s['rows']) for s in rec['shapes']
                                                if s['median_ms']['wide'] > s['median_ms']['library'] * (1 + max(s['spread']['wide'], s['spread']['library']))]
    for rc in ('Conv1D', 'GRU'):
        s = step_record(rc, dev)
        rec['steps'].append(s)
        print('%s step: %r %r' % (rc, s['median_ms'], s['route_counts']), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
