"""Shared by tests/test_predict_tail_math.py (CPU) and tests/test_gpu_predict_tail.py (GPU): the configurations of the predict
tail (everything `Emulator.predict_tf` / `predict` does after the network forward), their seeded inputs, and the reference.

The reference is what the project already trusts: `oracle.emulator_ref.predict` / `predict_np` with `forward` patched to return
the chosen network outputs (y, ey) -- exactly the tail, nothing restated.  Every constant and every input is an fp64 number that
fp32 represents exactly, so the device sees the same values.  Gradients: torch.autograd through the same patched call.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import emulator_ref as OE
from tests.util import emulator_args, emulator_norms, f32_exact

B = 2
TOL_FLOW = 1e-6            # the project's tolerance of the de-normalised link outputs (tests/test_gpu_tail_entries.py)
BWD_MARGIN = 3.0           # fused route vs fp64 <= BWD_MARGIN x (tensor route vs fp64), the project's backward margin
BWD_FLOOR = 1e-7           # ... with a floor of BWD_FLOOR x max|reference gradient|
TENSOR_ROUTE_GATE = 1e-4   # the tensor route itself must be this close (x max|ref grad|): the inputs sit on no kink flip


def tol_y(T):
    """The depth scan chains T steps of a handful of fp32 roundings each."""
    return T * 1e-6


def synthetic_edges(n_node=300, self_loop=True, seed=0):
    """A chain over nodes 0 .. n-3 with random chords; node n-2 is isolated (no link touches it), node n-1 closes the index
    range; link 3 is a parallel copy of link 2; with self_loop, link 5 runs from node 7 to node 7 (no from-node)."""
    rng = np.random.default_rng(seed)
    chain = [(i, i + 1) for i in range(n_node - 3)]
    chords = [(int(u), int(v)) for u, v in rng.integers(0, n_node - 2, (24, 2)) if u != v]
    edges = chain + chords + [(n_node - 3, n_node - 1)]
    edges[3] = edges[2]
    if self_loop:
        edges[5] = (7, 7)
    return np.asarray(edges, dtype=np.int64)


def _dense_graph(edges, n_node):
    """adj / edge_adj for a link list networkx would merge (parallel link, self loop): neighbours + diagonal."""
    adj = np.eye(n_node)
    inc = np.zeros((n_node, len(edges)))
    for i, (u, v) in enumerate(edges):
        adj[u, v] = adj[v, u] = 1
        inc[u, i] = inc[v, i] = 1
    return adj, ((inc.T @ inc) > 0).astype(np.float64)


def _config(name, net, seed, T=5, **over):
    return dict(name=name, net=net, seed=seed, T=T, over=over)


def _pumps(rng, n, e, all_links):
    some = np.ones(e, dtype=bool) if all_links else rng.random(e) > 0.6
    return dict(pump=(0.1 + rng.random(e)) * some, offset=rng.random(e) * (rng.random(e) > 0.5), area=rng.random(n) * (rng.random(n) > 0.2))


def configs(networks):
    """name -> configuration.  `over` goes to tests.util.emulator_args."""
    net = networks['astlingen']
    n, e = net['n_node'], len(net['edges'])
    rng = np.random.default_rng(11)
    node_pumps = dict(pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7))
    out = [
        _config('ef_act', 'astlingen', 1, edge_fusion=True, act=True),
        _config('ef_pumps_offset_tide', 'astlingen', 2, edge_fusion=True, act=True, tide=True, **_pumps(rng, n, e, False)),
        _config('ef_all_pumps', 'astlingen', 3, edge_fusion=True, act=True, tide=True, **_pumps(rng, n, e, True)),
        _config('node_gates', 'astlingen', 4, edge_fusion=False, act=True, tide=True, epsilon=0.1, **node_pumps, **_pumps(rng, n, e, True)),
        _config('eps0', 'astlingen', 5, edge_fusion=True, act=True, epsilon=0.0),
        _config('plain', 'astlingen', 6, edge_fusion=False, act=False, if_flood=0),
        _config('T1', 'astlingen', 7, T=1, edge_fusion=True, act=True, tide=True, **_pumps(rng, n, e, False)),
    ]
    for name, loop in (('synth300', True), ('synth300_noloop', False)):      # the second: the backward comparison (see the GPU file)
        edges = synthetic_edges(300, loop)
        adj, eadj = _dense_graph(edges, 300)
        r2 = np.random.default_rng(12)
        out.append(_config(name, edges, 8, edge_fusion=True, act=True, tide=True, adj=adj, edge_adj=eadj, act_edges=edges[[1, 40]],
                           **_pumps(r2, 300, len(edges), False)))
    return {c['name']: c for c in out}


FLOAT_KEYS = ('is_outfall', 'hmax', 'hmin', 'area', 'pump', 'pump_in', 'pump_out', 'offset', 'ehmax')


def setup(cfg, networks):
    """(args, norms): the reference-style namespace and the [max, min] norms, every float an fp32 number."""
    if isinstance(cfg['net'], str):
        edges, n_node = np.asarray(networks[cfg['net']]['edges']), networks[cfg['net']]['n_node']
    else:
        edges, n_node = cfg['net'], 300
    args = emulator_args(edges, n_node, seed=cfg['seed'], seq_out=cfg['T'], **cfg['over'])
    for k in FLOAT_KEYS:
        setattr(args, k, f32_exact(getattr(args, k)))
    norms = {k: v.float().double() for k, v in emulator_norms(args, seed=cfg['seed']).items()}
    return args, norms


def inputs(args, seed):
    """fp64 tensors of fp32 values: X (B, seq_in, N, n_in), b (B, T, N, 1 or 2), Ex (B, seq_in, E, 4), a (B, T, 2) in (0.1, 1),
    and the network outputs the patched forward returns: y (B, T, N, cy) in (-0.2, 1.2), ey (B, T, E, 3) in (-1, 1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    r32 = lambda t: t.float().double()
    uni = lambda lo, hi, *shape: r32(lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64))
    c = OE.config(args)
    N, E, T = c.n_node, c.n_edge, c.seq_out
    cy = (1 if c.edge_fusion else 3) + (1 if c.if_flood else 0)
    return SimpleNamespace(X=uni(0.0, 1.5, B, c.seq_in, N, c.n_in), b=uni(0.0, 0.2, B, T, N, c.b_in), Ex=uni(-0.5, 0.5, B, c.seq_in, E, 4),
                           a=uni(0.1, 1.0, B, T, 2) if c.act else None, y=uni(-0.2, 1.2, B, T, N, cy), ey=uni(-1.0, 1.0, B, T, E, 3))


def reference(args, norms, inp, np_form, dtype=torch.float64, y=None, ey=None, a=None, X=None):
    """The tail in `dtype` through the patched oracle: predict (predict_tf) or predict_np (predict).  y / ey / a / X replace the
    case's tensors (leaves that require grad, for the gradients)."""
    t = lambda v: None if v is None else v.to(dtype)
    y, ey = t(inp.y) if y is None else y, t(inp.ey) if ey is None else ey
    a, X = t(inp.a) if a is None else a, t(inp.X) if X is None else X
    saved = OE.forward
    OE.forward = lambda *args_, **kw: (y, ey)
    try:
        fn = OE.predict_np if np_form else OE.predict
        return fn(args, None, {k: v.to(dtype) for k, v in norms.items()}, X, t(inp.b), a, t(inp.Ex))
    finally:
        OE.forward = saved


def reference_grads(args, norms, inp, gy, gey, X=None):
    """fp64 gradients of sum(out_y * gy) + sum(out_ey * gey) w.r.t. y, ey, a (None without act) and X[:, -1, :, 0] through the
    patched oracle (predict_tf mode: `predict` is torch throughout)."""
    leaf = lambda v: None if v is None else v.clone().double().requires_grad_(True)
    y, ey, a, X = leaf(inp.y), leaf(inp.ey), leaf(inp.a), leaf(inp.X if X is None else X)
    oy, oey = reference(args, norms, inp, False, torch.float64, y, ey, a, X)
    ((oy * gy).sum() + (oey * gey).sum()).backward()
    zero = lambda v: None if v is None else (torch.zeros_like(v) if v.grad is None else v.grad)
    return dict(y=zero(y), ey=zero(ey), a=zero(a), h0=zero(X)[:, -1, :, 0])


def upstream(inp, args, seed):
    """Random upstream gradients of both outputs, fp64 of fp32 values."""
    g = torch.Generator().manual_seed(2000 + seed)
    c = OE.config(args)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) - 0.5).float().double()
    return r(B, c.seq_out, c.n_node, 5 if c.if_flood else 4), r(B, c.seq_out, c.n_edge, 3)
