"""Keras Adam with per-variable clipnorm restated in fp64, and the cases tests/test_adam_math.py (CPU: `KerasAdam` against the
restatement) and tests/test_gpu_adam.py (GPU: `HipKerasAdam` / uds_adam_step against it) share."""
import numpy as np
import torch

SHAPES = [(1,), (3,), (64,), (4097,), (30, 29), (192, 64), (5,)]
SCALES = [1.0, 1e-3, 10.0, 1e-2, 3.0, 1e-4, 0.0]      # clipped (norm > 1), unclipped, and one all-zero gradient
STEPS = 3
LR, B1, B2, EPS, CLIP = 1e-3, 0.9, 0.999, 1e-7, 1.0


def make_inputs(shapes, scales, seed=0, steps=STEPS):
    """(p0, grads): fp32 parameters with 0.5 <= |p| < 1.5 (so that an ulp of max|p| is an ulp of most elements) and `steps`
    lists of fp32 gradients, N(0, 1) * scale."""
    gen = torch.Generator().manual_seed(seed)
    p0 = [(0.5 + torch.rand(s, generator=gen)) * (1 - 2 * (torch.rand(s, generator=gen) > 0.5).float()) for s in shapes]
    grads = [[torch.randn(s, generator=gen) * sc for s, sc in zip(shapes, scales)] for _ in range(steps)]
    return p0, grads


def restate(p0, grads, lr=LR, b1=B1, b2=B2, eps=EPS, clip=CLIP):
    """TF 2.10 Adam(lr, clipnorm=clip) in fp64 on the fp32 inputs: (p, m, v) lists after len(grads) steps."""
    p = [t.double().clone() for t in p0]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    for t, gs in enumerate(grads, start=1):
        lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
        for i, g in enumerate(gs):
            g = g.double()
            if clip is not None:
                n = float(g.pow(2).sum().sqrt())
                g = g * (clip / max(n, clip))
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            p[i] = p[i] - lr_t * m[i] / (v[i].sqrt() + eps)
    return p, m, v


def ulp32(x):
    """Spacing of fp32 at |x|."""
    return float(np.spacing(np.float32(abs(float(x)))))


def max_err(out, ref):
    return float((out.detach().double().cpu() - ref).abs().max()) if ref.numel() else 0.0


def keras_errors(opt_cls, p0, grads, device, **kw):
    """(errors of p, m, v per tensor against the restatement, t) of `opt_cls` (KerasAdam) after the steps, on `device`."""
    ps = [torch.nn.Parameter(t.clone().to(device)) for t in p0]
    opt = opt_cls(ps, LR, B1, B2, EPS, clipnorm=CLIP, **kw)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone().to(device)
        opt.step()
    rp, rm, rv = restate(p0, grads)
    return ([max_err(a, b) for a, b in zip(ps, rp)], [max_err(a, b) for a, b in zip(opt.m, rm)], [max_err(a, b) for a, b in zip(opt.v, rv)],
            opt.t)
