"""Plain-torch restatements of the one-launch tail and rollout-step entries of the C ABI, from the formulas in
include/uds_hip.h (TEST INFRASTRUCTURE ONLY; fp64 inputs give the fp64 reference of the GPU parity tests).

tests/test_tail_ref_math.py pins both to what the project already trusts: the tail of `oracle.emulator_ref.forward` and one
post-forward step of `oracle.emulator_ref.model_rollout`.
"""
import torch

from . import spektral_dense as OD


def _dense(t, kernel, bias, act):
    return OD.dense(t, kernel, bias, act)


def dense_cumsum_heads_ref(x, W, b, res, act, A, a_bias, act_a, hidden=(), act_h='linear', Fk=None, f_bias=None, act_f='linear'):
    """uds_dense_cumsum_heads: y = act(cumsum_t(x @ W + b) + res), x (B,T,R,64), res (B,1,R,64) or None;
    out = [act_a(y @ A + a_bias) | act_f(h_n @ Fk + f_bias)] with h_0 = y, h_i = act_h(h_{i-1} @ H_i + hb_i) for
    hidden = [(H_i, hb_i), ...]; the second part only when `hidden` is not empty.  Any bias may be None.
    Returns (B, T, R, n_a + (1 if hidden else 0))."""
    z = x @ W
    if b is not None:
        z = z + b
    z = torch.cumsum(z, dim=1)
    if res is not None:
        z = z + res
    y = OD.activation(act)(z)
    out = _dense(y, A, a_bias, act_a)
    if len(hidden):
        h = y
        for H, hb in hidden:
            h = _dense(h, H, hb, act_h)
        out = torch.cat([out, _dense(h, Fk, f_bias, act_f)], dim=-1)
    return out


def roll_update_ref(inc_n_dense_signed, span_e, mini_e, scale_in, scale_out, y, ey, b, x, ex, flood):
    """uds_roll_update: inc (N,E) with +1 at a link's from-node and -1 at its to-node; span_e, mini_e (E); scale_in, scale_out (N);
    y (B,so,N,cy), ey (B,so,E,ce), b (B,so,N,1); the windows x (B,T,N,cy+3), ex (B,T,E,ce+1).
    Returns (preds (B,so,N,cy+2), x_new, ex_new): the windows shifted by `so` steps and fed with the prediction."""
    dt = y.dtype
    so, T = y.shape[1], x.shape[1]
    inc = inc_n_dense_signed.to(dt)
    pos, neg = inc.clamp(0, 1), inc.clamp(-1, 0).abs()
    flow = ey[..., -1] * span_e + mini_e                                 # (B,so,E): the de-normalised link flow
    fp, fn = flow.clamp(min=0), (-flow).clamp(min=0)
    q_out = (fp @ pos.T + fn @ neg.T) * scale_out
    q_in = (fp @ neg.T + fn @ pos.T) * scale_in
    preds = torch.cat([y[..., :1], q_in.unsqueeze(-1), q_out.unsqueeze(-1), y[..., 1:]], dim=-1)
    fed = preds
    if flood and y.shape[-1] >= 2:                                       # the flood bit is a y channel of its own after the depth
        fed = torch.cat([preds[..., :-1], (preds[..., -1:] > 0.5).to(dt)], dim=-1)
    x_in = torch.cat([fed, b], dim=-1)
    ex_in = torch.cat([ey, torch.ones(ey.shape[:-1] + (1,), dtype=dt)], dim=-1)
    x_new = torch.cat([x[:, so:], x_in], dim=1) if T > so else x_in
    ex_new = torch.cat([ex[:, so:], ex_in], dim=1) if T > so else ex_in
    return preds, x_new, ex_new
