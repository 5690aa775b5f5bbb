"""The two forms of DiffusionConv on ONE GPU, on the same layer: the table form (uds_diffusion_forward / uds_diffusion_backward,
vals (nnz, C) prepared per parameter version) against the moment form (uds_diffusion_forward_m / uds_diffusion_backward_m, no
table), forward and forward + backward.

    python tools/diffusion_form_time.py [--out profiles/diffusion_form_time.json]

Shapes: a shipped network (astlingen node filter, S = 1024, C = 64), the headline (N = 10 000 node filter, S = 60, C = 64) and
BASELINE's C3 (N = 50 000 / E = 65 000: node filter and line-graph filter, S = 32, C = 128); K1 = 7.  Every shape and form is
warmed; a repetition is INNER back-to-back calls between two device events, REPS repetitions per form, the two forms
alternating in one process.  Reported per form: median, 10th / 90th percentile and spread (p90 - p10) of the per-call time; the
table's bytes; the bytes each form moves per snapshot, computed from the shapes (table or a, col, gathered r, theta, output);
and the largest difference between the two forms' outputs.  `gate` (C3 shapes): the moment form's median must not exceed the
table form's by more than the table form's own spread.  The table's preparation per parameter update (fp64 Horner over
(nnz, C)) is NOT in the table form's times: they are its kernels alone.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U                      # noqa: E402
from gnn_uds_amd import _lib                 # noqa: E402

K1, WARM, REPS, INNER = 7, 20, 60, 10


def _shapes():
    with open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')) as fh:
        net = json.load(fh)['astlingen']
    small = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    head = U.DrainageGraph.from_edges(U.synthetic_drainage_network(10000, 12000, 0))
    c3 = U.DrainageGraph.from_edges(U.synthetic_drainage_network(50000, 65000, 0))
    return [('astlingen-node', small.raw_adj, 1024, 64, False), ('headline-node', head.raw_adj, 60, 64, False),
            ('c3-node', c3.raw_adj, 32, 128, True), ('c3-line', c3.raw_edge_adj, 32, 128, True)]


def _forms(raw, S, C, dev):
    ah = U.DiffusionConv.preprocess(raw)
    g = torch.Generator().manual_seed(0)
    layer = U.DiffusionConv(C, K=K1 - 1, generator=g).to(dev)
    with torch.no_grad():
        layer.kernel.mul_(0.002)
    h, vals, c0, a_sup = layer._filter(ah, dev)
    theta = layer.kernel.detach().contiguous()
    r = (torch.rand(S, ah.n_cols, generator=g) * 8 - 4).to(dev)
    tot = r.sum(-1).contiguous()
    gy = (torch.rand(S, ah.n_rows, C, generator=g) - 0.5).to(dev)
    y_t = _lib.diffusion_forward(h, vals, c0, r, tot, 'tanh')
    y_m = _lib.diffusion_forward_m(h, a_sup, theta, r, tot, 'tanh')
    dr_t, dk_t = _lib.diffusion_backward(h, a_sup, vals, c0, r, tot, y_t, gy, K1, 'tanh')
    dr_m, dk_m = _lib.diffusion_backward_m(h, a_sup, theta, r, tot, y_m, gy, 'tanh')
    diff = {'out': float((y_t - y_m).abs().max()), 'dr': float((dr_t - dr_m).abs().max()), 'dr_scale': float(dr_t.abs().max()),
            'dtheta': float((dk_t - dk_m).abs().max()), 'dtheta_scale': float(dk_t.abs().max())}

    def table_fb():
        y = _lib.diffusion_forward(h, vals, c0, r, tot, 'tanh')
        _lib.diffusion_backward(h, a_sup, vals, c0, r, tot, y, gy, K1, 'tanh')

    def moment_fb():
        y = _lib.diffusion_forward_m(h, a_sup, theta, r, tot, 'tanh')
        _lib.diffusion_backward_m(h, a_sup, theta, r, tot, y, gy, 'tanh')
    calls = {'forward': {'table': lambda: _lib.diffusion_forward(h, vals, c0, r, tot, 'tanh'),
                         'moment': lambda: _lib.diffusion_forward_m(h, a_sup, theta, r, tot, 'tanh')},
             'forward_backward': {'table': table_fb, 'moment': moment_fb}}
    return ah, calls, diff


def _window_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(INNER):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / INNER


def _alternate(pair):
    for fn in pair.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in pair}
    for _ in range(REPS):
        for k, fn in pair.items():
            times[k].append(_window_ms(fn))
    out = {}
    for k, t in times.items():
        p10, med, p90 = (float(v) for v in np.percentile(t, [10, 50, 90]))
        out[k] = {'median_ms': round(med, 5), 'p10_ms': round(p10, 5), 'p90_ms': round(p90, 5), 'spread_ms': round(p90 - p10, 5)}
    return out


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'diffusion_form_time.json')
    if not torch.cuda.is_available():
        raise SystemExit('diffusion_form_time needs the GPU: nothing is measured without it')
    dev = torch.device('cuda:0')
    rec = {'tool': 'diffusion_form_time', 'device': torch.cuda.get_device_name(0), 'K1': K1, 'reps': REPS, 'calls_per_rep': INNER,
           'warm_calls': WARM, 'spread': 'p90 - p10 of the per-call time over the repetitions', 'shapes': {}}
    ok = True
    for name, raw, S, C, gated in _shapes():
        ah, calls, diff = _forms(raw, S, C, dev)
        n, nnz = ah.n_rows, ah.nnz
        common = nnz * 8 + n * C * 4                       # col + gathered r per entry, the output row
        e = {'n_rows': n, 'nnz': nnz, 'S': S, 'C': C, 'table_bytes': nnz * C * 4,
             'bytes_per_snapshot': {'table': nnz * C * 4 + common + C * 4, 'moment': nnz * 4 + common + C * K1 * 4},
             'max_abs_difference_between_forms': diff}
        for mode, pair in calls.items():
            e[mode] = _alternate(pair)
        if gated:
            e['gate'] = {mode: bool(e[mode]['moment']['median_ms'] <= e[mode]['table']['median_ms'] + e[mode]['table']['spread_ms'])
                         for mode in calls}
            ok = ok and all(e['gate'].values())
        rec['shapes'][name] = e
        print(name, json.dumps(e), flush=True)
    rec['c3_gate_met'] = ok
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps({'tool': rec['tool'], 'c3_gate_met': ok, 'out': out_path}))


if __name__ == '__main__':
    main()
