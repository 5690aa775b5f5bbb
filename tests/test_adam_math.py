"""The fp64 restatement of Keras Adam with per-variable clipnorm (tests/adam_util.py) is what `KerasAdam` computes: three steps
on CPU tensors, at the shapes and gradient scales tests/test_gpu_adam.py holds uds_adam_step to.

Bound, per tensor and step: the final `p - update` rounds once (half an ulp of max|p|), and the update itself -- at most about lr in
the first steps, where m_hat / sqrt(v_hat) is within [-1, 1] -- carries the roundings of the clip factor, m, v, sqrt, the division and
the product, eight at most (8 * 2^-24 * lr).  Measured: 4.1e-7 at the worst tensor, on parameters that moved about 3e-3."""
import torch

from gnn_uds_amd.emulator import KerasAdam
from tests import adam_util as AU


def test_cases_clip_and_do_not_clip():
    _, grads = AU.make_inputs(AU.SHAPES, AU.SCALES)
    norms = [float(g.norm()) for g in grads[0]]
    assert sum(n > AU.CLIP for n in norms) >= 3 and sum(0 < n < AU.CLIP for n in norms) >= 2 and norms[-1] == 0.0


def test_restatement_moves_the_parameters():
    p0, grads = AU.make_inputs(AU.SHAPES, AU.SCALES)
    rp, rm, rv = AU.restate(p0, grads)
    for a, b, s in zip(p0, rp, AU.SCALES):
        moved = float((b - a.double()).abs().max())
        # three steps of at most about lr each; an element whose gradient keeps its sign moves by all three
        assert (moved == 0.0) if s == 0 else (0 < moved < 3.1e-3 and (a.numel() < 64 or moved > 2.5e-3)), moved
    # one step, one element, by hand: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1, g clipped to norm 1
    p, m, v = AU.restate([torch.tensor([1.0])], [[torch.tensor([4.0])]])
    assert abs(float(m[0]) - 0.1) < 1e-15 and abs(float(v[0]) - 0.001) < 1e-15
    lr_t = AU.LR * 0.001 ** 0.5 / 0.1
    assert abs(float(p[0]) - (1.0 - lr_t * 0.1 / (0.001 ** 0.5 + AU.EPS))) < 1e-15


def test_keras_adam_matches_the_restatement():
    p0, grads = AU.make_inputs(AU.SHAPES, AU.SCALES)
    ep, em, ev, t = AU.keras_errors(KerasAdam, p0, grads, 'cpu')
    assert t == AU.STEPS
    rp, rm, rv = AU.restate(p0, grads)
    for i, s in enumerate(AU.SHAPES):
        lim = AU.STEPS * (0.5 * AU.ulp32(rp[i].abs().max()) + 8 * 2.0 ** -24 * AU.LR)
        assert ep[i] <= lim, (s, ep[i], lim)
        # slots: three roundings per step and the clipped gradient's own (five ulp of the slot's largest element per step)
        assert em[i] <= AU.STEPS * 5 * AU.ulp32(rm[i].abs().max()), (s, em[i])
        assert ev[i] <= AU.STEPS * 5 * AU.ulp32(rv[i].abs().max()), (s, ev[i])
