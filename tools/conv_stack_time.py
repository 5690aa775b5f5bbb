"""Cost of a temporal Conv1D stack on ONE GPU: the one-launch kernel (`_lib.conv_stack_forward`, uds_conv_stack_forward) against
the layer chain it replaces (L `_lib.rowgemm_forward(..., taps=3, dilation=2**i)` calls, k_conv3_stream from 256 streams on), and
the whole `Emulator.forward` of the headline model with `fused_temporal` on and off.

    python tools/conv_stack_time.py [--out profiles/conv_stack_time.json]

Shapes (B, T, R) of x (B, T, R, 64), relu, L = 3 and L = 2: (1, 60, 10000) and (1, 60, 12000) -- the node and the link side of
the headline model --, (32, 6, 2000), and (1, 6, 4096), the 256-stream threshold.  The model: the benchmark's rollout model
(N = 10000, E = 12000, T_in = T_out = 60, 3 + 3 spatial layers, n_tp_layer = 3 and 2, B = 1) under no_grad.
Per shape, alternated call by call in one process after WARM calls of every variant, REPS timed calls each with device events
around every call, medians; the whole measurement twice (run-to-run spread).  Stack and chain are also compared with torch.equal.
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
from gnn_uds_amd import _lib                                # noqa: E402

SHAPES = ((1, 60, 10000), (1, 60, 12000), (32, 6, 2000), (1, 6, 4096))
WARM, REPS, RUNS = 10, 100, 2
MODEL_WARM, MODEL_REPS = 5, 30


def _alternate(fns, warm, reps):
    """name -> median ms per call: `warm` calls of each, then `reps` rounds calling each once in turn, one event pair per call."""
    for fn in fns.values():
        for _ in range(warm):
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


def kernel_fns(shape, L, dev):
    B, T, R = shape
    gen = torch.Generator().manual_seed(B + T + R + L)
    x = (torch.rand(B, T, R, 64, generator=gen) - 0.5).to(dev)
    lim = (6.0 / 384) ** 0.5
    layers = [(_lib.rowgemm_pack(((torch.rand(192, 64, generator=gen) * 2 - 1) * lim).to(dev)), ((torch.rand(64, generator=gen) - 0.5) * 0.2).to(dev))
              for _ in range(L)]
    out = torch.empty_like(x)
    tmp = [torch.empty_like(x), torch.empty_like(x)]

    def stack():
        return _lib.conv_stack_forward(x, layers, 'relu', out=out)

    def chain():
        y = x
        for i, (pk, b) in enumerate(layers):
            y = _lib.rowgemm_forward(y, pk, b, 64, 'relu', taps=3, dilation=2 ** i, out=tmp[i % 2])
        return y
    same = bool(torch.equal(stack(), chain()))
    return {'stack': stack, 'chain': chain}, same


def model_fns(n_tp_layer, dev):
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(10000, 12000, seed=0))
    T = 60
    a = SimpleNamespace(state_shape=(g.n_node, 4), edge_state_shape=(g.n_edge, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64,
                        kernel_size=3, n_sp_layer=3, n_tp_layer=n_tp_layer, activation='relu', if_flood=3, edge_fusion=True, edges=g.edges,
                        act=False, graph=g, model_dir=None)
    emul = U.Emulator('GAT', True, 'Conv1D', a, precision='bf16x3', generator=torch.Generator().manual_seed(1)).to(dev)
    X, B, E = torch.rand(1, T, g.n_node, 5, device=dev), torch.rand(1, T, g.n_node, 1, device=dev), torch.rand(1, T, g.n_edge, 4, device=dev)

    def forward(fused):
        def fn():
            emul.fused_temporal = fused
            with torch.no_grad():
                out = emul(X, B, E)
            assert emul.last_temporal_path == ('stack' if fused else 'layers')
            return out
        return fn
    on, off = forward(True)(), forward(False)()
    same = all(bool(torch.equal(p, q)) for p, q in zip(on, off))
    return {'forward_stack': forward(True), 'forward_layers': forward(False)}, same


def main():
    dev = torch.device('cuda:0')
    n_seg = {'%dx%dx%d-L%d' % (s + (L,)): _lib.conv_stack_plan(s[0], s[1], s[2], L)[0] for s in SHAPES for L in (3, 2)}
    rec = {'tool': 'conv_stack_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'model_warm': MODEL_WARM,
           'model_reps': MODEL_REPS, 'activation': 'relu', 'planned_n_seg': n_seg, 'runs': []}
    kernels = {(s, L): kernel_fns(s, L, dev) for s in SHAPES for L in (3, 2)}
    models = {L: model_fns(L, dev) for L in (3, 2)}
    for _ in range(RUNS):
        run = []
        for (s, L), (fns, same) in kernels.items():
            ms = _alternate(fns, WARM, REPS)
            run.append({'what': 'kernel', 'B': s[0], 'T': s[1], 'R': s[2], 'L': L, 'bitwise_equal': same, 'median_ms': ms,
                        'chain_over_stack': round(ms['chain'] / ms['stack'], 3)})
        for L, (fns, same) in models.items():
            ms = _alternate(fns, MODEL_WARM, MODEL_REPS)
            run.append({'what': 'Emulator.forward N=10000 E=12000 T=60', 'n_tp_layer': L, 'bitwise_equal': same, 'median_ms': ms,
                        'layers_over_stack': round(ms['forward_layers'] / ms['forward_stack'], 3)})
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
