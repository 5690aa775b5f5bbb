"""GlobalAttnSumPool over two row blocks: the cases, the seeded inputs and the closed-form fp64 reference shared by
tests/test_attn_pool_math.py (CPU: the closed form against autograd of the softmax form, and what plain fp32 arithmetic reaches)
and tests/test_gpu_attn_pool_train.py (GPU parity of uds_attn_sum_pool_pair / uds_attn_sum_pool_backward).

Per sample b the rows r = 0 .. Rx+Re-1 are the rows of x[b] followed by the rows of e[b]:
    s_r = <row_r, k>,  M = max_r s_r,  L = sum_r exp(s_r - M),  alpha_r = exp(s_r - M) / L,  out = sum_r alpha_r row_r
and for an upstream gradient g = grad[b], with t_r = <g, row_r> - <g, out[b]>:
    ds_r = alpha_r t_r,  d row_r = alpha_r g + ds_r k,  dk = sum_b sum_r ds_r row_r
"""
import torch

# (B, Rx, Re, F, scale).  With 256 threads a workgroup holds 256 / (F / 4) row slots per step:
#   (5, 30, 29, 128, 1)     8 slots: the RL encoder's shape (astlingen), the x / e boundary inside a step (30 = 3 * 8 + 6)
#   (3, 443, 557, 64, 1)    16 slots, 63 steps, boundary inside a step (443 = 27 * 16 + 11)
#   (2, 4, 3, 8, 1)         128 slots for 7 rows: far more row slots than rows
#   (1, 129, 128, 256, 1)   4 slots: one wave per row, boundary inside a step (129 = 32 * 4 + 1)
#   (4, 1, 0, 64, 1)        a single row, no second block (e = None)
#   (3, 257, 43, 4, 1)      one lane per row, 256 slots: a second, partly live step that holds the boundary
#   (6, 443, 444, 128, 1)   many steps (111) at the width of the reference's default agents
#   (1, 129, 128, 256, 12)  scores up to about +-190: only the running maximum keeps exp finite
POOL_CASES = [(5, 30, 29, 128, 1), (3, 443, 557, 64, 1), (2, 4, 3, 8, 1), (1, 129, 128, 256, 1), (4, 1, 0, 64, 1), (3, 257, 43, 4, 1),
              (6, 443, 444, 128, 1), (1, 129, 128, 256, 12)]

TOL_FWD = 5e-6      # out and (M, L): tests/test_gpu_emulator.py test_attn_sum_pool_kernel
TOL_BWD = 1e-5      # dx, de, dk: the sparse backward bound (tests/test_gpu_sparse_widths.py)


def case_id(c):
    return 'B%d-Rx%d-Re%d-F%d-s%d' % c


def pool_inputs(case):
    """fp64 (x (B, Rx, F), e (B, Re, F) or None, k (F, 1), g (B, F)): the stacked rows uniform in +-2, split after Rx rows; k uniform in
    +-0.5 * scale; the upstream gradient uniform in +-1."""
    B, Rx, Re, F, scale = case
    gen = torch.Generator().manual_seed(B + Rx + Re)
    rows = torch.rand(B, Rx + Re, F, generator=gen, dtype=torch.float64) * 4 - 2
    k = (torch.rand(F, 1, generator=gen, dtype=torch.float64) - 0.5) * scale
    g = torch.rand(B, F, generator=gen, dtype=torch.float64) * 2 - 1
    return rows[:, :Rx].contiguous(), (rows[:, Rx:].contiguous() if Re else None), k, g


def pool_closed_form(x, e, k, g):
    """The formulas of the module docstring in the dtype of the inputs: out (B, F), stat (B, 2) = (M, L), dx, de (None without e),
    dk (F, 1)."""
    rows = x if e is None else torch.cat([x, e], dim=-2)
    s = (rows @ k).squeeze(-1)                                    # (B, R)
    M = s.max(dim=-1, keepdim=True).values
    w = torch.exp(s - M)
    L = w.sum(dim=-1, keepdim=True)
    alpha = w / L
    out = (alpha.unsqueeze(-1) * rows).sum(dim=-2)
    t = (rows * g.unsqueeze(-2)).sum(dim=-1) - (g * out).sum(dim=-1, keepdim=True)
    ds = alpha * t
    drows = alpha.unsqueeze(-1) * g.unsqueeze(-2) + ds.unsqueeze(-1) * k.reshape(-1)
    dk = (ds.unsqueeze(-1) * rows).sum(dim=(0, 1)).reshape(k.shape)
    Rx = x.shape[1]
    return dict(out=out, stat=torch.cat([M, L], dim=-1), dx=drows[:, :Rx].contiguous(), de=None if e is None else drows[:, Rx:].contiguous(), dk=dk)


def softmax_form(x, e, k):
    """spektral's GlobalAttnSumPool as the reference writes it (and as the module's torch path runs it), differentiable."""
    rows = x if e is None else torch.cat([x, e], dim=-2)
    alpha = torch.softmax(torch.matmul(rows, k).squeeze(-1), dim=-1)
    return torch.matmul(alpha.unsqueeze(-2), rows).squeeze(-2)


def pool_autograd(x, e, k, g):
    """out, dx, de, dk by torch autograd of the softmax form for the loss (out * g).sum()."""
    leaves = [t.clone().requires_grad_(True) for t in (x, e, k) if t is not None]
    xx, ee, kk = (leaves[0], leaves[1], leaves[2]) if e is not None else (leaves[0], None, leaves[1])
    out = softmax_form(xx, ee, kk)
    grads = torch.autograd.grad((out * g).sum(), leaves)
    return dict(out=out.detach(), dx=grads[0], de=grads[1] if e is not None else None, dk=grads[-1])


_REF = {}


def pool_ref(case):
    """(inputs, fp64 closed form) of a case, computed once per session."""
    if case not in _REF:
        inp = pool_inputs(case)
        _REF[case] = (inp, pool_closed_form(*inp))
    return _REF[case]


def rel_err(got, ref):
    """max|got - ref| / max(1, max|ref|): the measure of tests.util.close."""
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
