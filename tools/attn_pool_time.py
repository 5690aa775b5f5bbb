"""Cost of GlobalAttnSumPool under autograd on ONE GPU: the HIP path against the torch composition it replaces.

    python tools/attn_pool_time.py [--out profiles/attn_pool_time.json]

The RL agents update on batches of single-snapshot observations, so the shapes are B samples of Rx node rows and Re link rows of
width F: B = 256 and 1024, (Rx, Re) = (140, 141) and (443, 444), F = 64 and 128.  Per shape, forward plus backward (the
gradients of x, e and attn_kernel for a fixed upstream gradient, through torch.autograd.grad), alternated call by call in one
process after WARM calls of every variant, REPS timed calls each with device events around every call, medians; the whole
measurement twice (run-to-run spread):
  hip           the module as it is: autograd.AttnSumPoolFn (uds_attn_sum_pool_pair, then uds_attn_sum_pool_backward)
  torch         the same module with the HIP route switched off (pool.hip = False): torch.cat of the two blocks, matmul, softmax,
                matmul and their autograd -- what ran before the HIP backward existed
  torch_no_cat  that composition on an already stacked tensor: the difference to `torch` is what the concatenation and the
                split of its gradient cost
  hip_entries   the two C entries alone on preallocated outputs: the kernels without the autograd round trip
Floor of the formulation: the forward reads the rows once, the backward reads them once and writes their gradients once,
3 * B * (Rx + Re) * F * 4 bytes; `floor_GBps` is that over the median time.  `cat_bytes` is the traffic the removed
concatenation added: the stack written and read in the forward, its gradient written and split in the backward.
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
from gnn_uds_amd.agent import GlobalAttnSumPool             # noqa: E402

BATCHES, ROWS, WIDTHS = (256, 1024), ((140, 141), (443, 444)), (64, 128)
WARM, REPS, RUNS = 20, 200, 2


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


def shape_fns(dev, B, Rx, Re, F):
    gen = torch.Generator().manual_seed(B + Rx + F)
    r = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(dev)
    x, e, g = r(B, Rx, F).requires_grad_(True), r(B, Re, F).requires_grad_(True), r(B, F)
    stack = torch.cat([x, e], dim=-2).detach().requires_grad_(True)
    pool = GlobalAttnSumPool(F, generator=gen).to(dev).requires_grad_(True)
    k = pool.attn_kernel

    def module(hip, *rows):
        def fn():
            pool.hip = hip
            out = pool(*rows)
            assert pool.last_path == ('hip-train' if hip else 'torch')
            return torch.autograd.grad(out, rows + (k,), g)
        return fn
    kd = k.detach().reshape(-1).contiguous()
    xd, ed = x.detach(), e.detach()
    dx, de, dk, ws = torch.empty_like(xd), torch.empty_like(ed), torch.empty(F, device=dev), torch.empty(B, F, device=dev)

    def entries():
        out, stat = _lib.attn_sum_pool_pair(xd, ed, kd, want_stat=True)
        _lib.attn_sum_pool_backward(xd, ed, kd, out, stat, g, dx=dx, de=de, dk=dk, dk_ws=ws)
    return {'hip': module(True, x, e), 'torch': module(False, x, e), 'torch_no_cat': module(False, stack), 'hip_entries': entries}


def main():
    dev = torch.device('cuda:0')
    rec = {'tool': 'attn_pool_time', 'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'runs': []}
    for _ in range(RUNS):
        run = []
        for B in BATCHES:
            for Rx, Re in ROWS:
                for F in WIDTHS:
                    ms = _alternate(shape_fns(dev, B, Rx, Re, F))
                    row_bytes = B * (Rx + Re) * F * 4
                    run.append({'B': B, 'Rx': Rx, 'Re': Re, 'F': F, 'median_ms': ms, 'floor_bytes': 3 * row_bytes, 'cat_bytes': 4 * row_bytes,
                                'floor_GBps': {k: round(3 * row_bytes / (v * 1e-3) / 1e9, 1) for k, v in ms.items()},
                                'torch_over_hip': round(ms['torch'] / ms['hip'], 3)})
                    torch.cuda.empty_cache()
        rec['runs'].append(run)
    rec['run_to_run_spread'] = round(max(abs(a['median_ms'][k] - b['median_ms'][k]) / a['median_ms'][k]
                                         for a, b in zip(*rec['runs']) for k in a['median_ms']), 4)
    line = json.dumps(rec)
    print(line)
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
