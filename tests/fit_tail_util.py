"""Shared by tests/test_fit_tail_math.py (CPU) and tests/test_gpu_fit_tail.py (GPU): the cases of the training tail (everything
`Emulator.fit_eval` / `fit_grad_norm` do after the network forward), their seeded inputs and targets, and the reference.

The reference is what the project already trusts: `oracle.train_ref.losses` with `oracle.emulator_ref.forward` patched to return the
chosen network outputs (y, ey) -- exactly the tail, nothing restated; the method, the configurations and the inputs are those of
tests/predict_tail_util.py.  Every constant, input, target and weight is an fp64 number that fp32 represents exactly.  Gradients:
torch.autograd through the same patched call and `oracle.emulator_ref.post_proc` (the outputs the rollout feeds back).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import emulator_ref as OE
from oracle import train_ref as OT
from tests.predict_tail_util import B, BWD_FLOOR, BWD_MARGIN, TENSOR_ROUTE_GATE, configs, inputs, setup      # noqa: F401
from tests.util import f32_exact

PLAIN = ['ef_act', 'ef_pumps_offset_tide', 'ef_all_pumps', 'node_gates', 'eps0', 'plain', 'T1', 'synth300', 'synth300_noloop']
BALANCE = ['node_gates_balance', 'plain_balance']
ROLL = 'ef_act_roll2'
BIG = 'reduction'              # B T N = 2 x 9 x 300 = 5400 rows: more than 21 workgroups of 256 rows, and no multiple of 256
CASES = PLAIN + BALANCE + [ROLL, BIG]


def loss_bound(n):
    """Relative error allowed on a loss of n summed per-sample terms: the terms are non-negative, the reduction is a tree of depth
    log2(n), each term carries a few roundings."""
    return (math.log2(n) + 8) * 2.0 ** -24


def case_configs(networks):
    """name -> configuration (the form of predict_tail_util.configs): its cases, each with seeded loss weights; `balance` variants
    of two of them; one with roll = 2; one whose row count spans several workgroups."""
    base = configs(networks)
    out = {}

    def weights(cfg, seed):
        rng = np.random.default_rng(seed)
        if isinstance(cfg['net'], str):
            n, e = networks[cfg['net']]['n_node'], len(networks[cfg['net']]['edges'])
        else:
            n, e = 300, len(cfg['net'])
        return dict(nwei=f32_exact(0.5 + rng.random(n)), ewei=f32_exact(0.5 + rng.random(e)), poswei=f32_exact(1.0 + 3.0 * rng.random(n)))

    for i, name in enumerate(PLAIN):
        out[name] = dict(base[name], over=dict(base[name]['over'], **weights(base[name], 40 + i)))
    for i, name in enumerate(BALANCE):
        src = base[name[:-len('_balance')]]
        out[name] = dict(src, name=name, over=dict(src['over'], balance=True, **weights(src, 60 + i)))
    out[ROLL] = dict(base['ef_act'], name=ROLL, T=2, over=dict(base['ef_act']['over'], roll=2, seq_in=5, **weights(base['ef_act'], 70)))
    out[BIG] = dict(base['synth300_noloop'], name=BIG, T=9, over=dict(base['synth300_noloop']['over'], seq_in=9, **weights(base['synth300_noloop'], 71)))
    return out


def case_inputs(args, seed):
    """predict_tail_util.inputs per chunk (joined along time for roll > 1) plus the targets: y_true (B, T, N, 5) in (0, 1) with a
    0 / 1 flood channel at -2, ey_true (B, T, E, 3) in (-1, 1)."""
    c = OE.config(args)
    chunks = [inputs(args, seed + 100 * i) for i in range(max(c.roll, 1))]
    cat = lambda k: None if getattr(chunks[0], k) is None else torch.cat([getattr(ch, k) for ch in chunks], dim=1)
    inp = SimpleNamespace(X=chunks[0].X, Ex=chunks[0].Ex, b=cat('b'), a=cat('a'), y=cat('y'), ey=cat('ey'))
    g = torch.Generator().manual_seed(3000 + seed)
    T = c.seq_out * max(c.roll, 1)
    r32 = lambda t: t.float().double()
    inp.y_true = r32(torch.rand(B, T, c.n_node, 5, generator=g, dtype=torch.float64))
    inp.y_true[..., -2] = (inp.y_true[..., -2] > 0.6).double()
    inp.ey_true = r32(2 * torch.rand(B, T, c.n_edge, 3, generator=g, dtype=torch.float64) - 1)
    return inp


class patched_forward:
    """`with patched_forward(y, ey, seq_out):` -- oracle.emulator_ref.forward returns the chosen outputs, chunk after chunk."""

    def __init__(self, y, ey, so):
        self.y, self.ey, self.so, self.i = y, ey, so, 0

    def __call__(self, *args, **kw):
        sl = slice(self.i * self.so, (self.i + 1) * self.so)
        self.i += 1
        return self.y[:, sl], self.ey[:, sl]

    def __enter__(self):
        self.saved, OE.forward = OE.forward, self
        return self

    def __exit__(self, *exc):
        OE.forward = self.saved


def counts(args, inp):
    """Per-sample terms of the node, flood and edge loss."""
    c = OE.config(args)
    rows = inp.y_true.shape[0] * inp.y_true.shape[1]
    return rows * c.n_node, rows * c.n_node, rows * c.n_edge


def reference_losses(args, norms, inp, dtype=torch.float64, y=None, ey=None):
    """[node, flood (0 where fit_eval has none), edge] of oracle.train_ref.losses in `dtype` on the patched forward."""
    c = OE.config(args)
    t = lambda v: None if v is None else v.to(dtype)
    y, ey = t(inp.y) if y is None else y, t(inp.ey) if ey is None else ey
    with patched_forward(y, ey, c.seq_out):
        ls = OT.losses(args, None, {k: v.to(dtype) for k, v in norms.items()}, t(inp.X), t(inp.a), t(inp.b), t(inp.y_true), t(inp.Ex), t(inp.ey_true))
    return [ls[0], ls[1] if len(ls) == 3 else torch.zeros((), dtype=dtype), ls[-1]]


def upstream(args, inp, seed, outputs):
    """g_loss (3,) in (0.5, 1.5) and, with `outputs`, gradients arriving at out_y / out_ey in (-0.5, 0.5) / 100 (the losses'
    own gradients are of that size: sums of B T N terms divided by nothing); fp64 of fp32 values."""
    c = OE.config(args)
    g = torch.Generator().manual_seed(4000 + seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    g_loss = (0.5 + r(3)).float().double()
    T = inp.y.shape[1]
    if not outputs:
        return g_loss, None, None
    return g_loss, ((r(B, T, c.n_node, 4 if c.if_flood else 3) - 0.5) / 100).float().double(), ((r(B, T, c.n_edge, 3) - 0.5) / 100).float().double()


def reference_grads(args, norms, inp, g_loss, gy, gey, dtype=torch.float64):
    """Gradients w.r.t. y and ey of sum_k g_loss[k] * (loss_k * its sample count) + sum(out_y gy) + sum(out_ey gey) in `dtype` on the
    CPU: one chunk (roll = 0; the feedback of a rollout is what gy / gey stand for)."""
    t = lambda v: None if v is None else v.to(dtype)
    y, ey = t(inp.y).clone().requires_grad_(True), t(inp.ey).clone().requires_grad_(True)
    ls = reference_losses(args, norms, inp, dtype, y, ey)
    total = sum(t(g_loss)[k] * ls[k] * n for k, n in enumerate(counts(args, inp)))
    if gy is not None:
        oy, oey = OE.post_proc(args, {k: v.to(dtype) for k, v in norms.items()}, y, ey, t(inp.a), t(inp.b))
        total = total + (oy * t(gy)).sum() + (oey * t(gey)).sum()
    total.backward()
    return dict(y=y.grad.double(), ey=ey.grad.double())
