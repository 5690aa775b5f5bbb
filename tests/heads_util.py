"""Shared helpers of the multi-head GAT tests (tests/test_gat_heads_math.py on the CPU, tests/test_gpu_gat_heads.py and
tests/test_gpu_gat_heads_model.py on the GPU): the fp64 multi-head reference, composed head by head from
oracle.gat_csr_ref, and the seeded operands on the degree-ladder patterns of tests/util.py.

Layouts are those of uds_gat_aggregate_heads / uds_gat_backward_heads: hx (S, n, H*C) with head-major columns, scores
(S, n, H), the edge mask (S, nnz) shared by the heads, coef and the coefficients (S, H, nnz) in the pattern's entry order."""
import numpy as np

from oracle.gat_csr_ref import masked_backward, masked_forward
from tests.util import f32_exact, ladder_coef, ladder_mask, ladder_operands, ladder_scores

# (H, C) of tests/test_gpu_gat_heads.py and what each reaches (group_shape of kernels_sparse.hpp on C / 4)
HEAD_CASES = [(1, 64), (8, 8), (4, 16), (2, 32), (3, 32), (2, 64), (2, 128), (16, 4), (3, 12)]
VARIANTS = {'plain': (False, False), 'mask': (True, False), 'coef': (False, True), 'both': (True, True)}
HEADS_COEF_SEED = 23


def heads_ref(rowptr, col, mask, coef, hx, ss, sn, H, concat, a_self=None, a_nbr=None, grad=None):
    """The multi-head reference: oracle.gat_csr_ref.masked_forward / masked_backward once per head -- head h sees
    hx[..., h*C:(h+1)*C], ss[..., h], sn[..., h], the shared mask and coef[:, h] -- then the heads concatenated or averaged.
    mask (S, nnz) / coef (S, H, nnz): None = ones.  Returns pre (before bias and activation; (S, n, H*C) or (S, n, C)), alpha
    (S, H, nnz; the softmax) and alpha_coef = alpha * coef (what the aggregation used); with grad = dL/dpre (shaped like pre)
    and a_self / a_nbr (H*C,) also d_hx (S, n, H*C), ds_self and ds_nbr (S, n, H)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    S, n, width = hx.shape
    C, nnz = width // H, len(col)
    mk = np.ones((S, nnz)) if mask is None else mask
    cf = np.ones((S, H, nnz)) if coef is None else coef
    pres, alphas, back = [], [], []
    for h in range(H):
        sl = slice(h * C, (h + 1) * C)
        pre, alpha = masked_forward(rowptr, col, mk, cf[:, h], hx[..., sl], ss[..., h], sn[..., h], np.zeros(C), 'linear')
        pres.append(pre)
        alphas.append(alpha)
        if grad is not None:
            gh = grad[..., sl] if concat else grad / H
            back.append(masked_backward(rowptr, col, mk, cf[:, h], hx[..., sl], ss[..., h], sn[..., h], a_self[sl], a_nbr[sl], alpha, pre,
                                        gh, 'linear')[:3])
    alpha = np.stack(alphas, axis=1)
    out = dict(pre=np.concatenate(pres, axis=-1) if concat else np.mean(pres, axis=0), alpha=alpha, alpha_coef=alpha * cf)
    if grad is not None:
        out.update(d_hx=np.concatenate([b[0] for b in back], axis=-1), ds_self=np.stack([b[1] for b in back], axis=-1),
                   ds_nbr=np.stack([b[2] for b in back], axis=-1))
    return out


def heads_scores(csr, H):
    """(s_self, s_nbr), (3, n, H) each: tests.util.ladder_scores with seed h for head h, so every head keeps the overflow
    snapshot (a logit of 92 in the last row of snapshot 2) and both leaky slopes in every multi-entry row."""
    per = [ladder_scores(csr, seed=h) for h in range(H)]
    return np.stack([p[0] for p in per], axis=-1), np.stack([p[1] for p in per], axis=-1)


def heads_coef(nnz, H, seed=HEADS_COEF_SEED):
    """(3, H, nnz) attention-dropout multiplier, 0 or 2: the CPU restatement of _lib.dropout(ones((3, H, nnz)), 0.5, seed, 0)."""
    return ladder_coef(H * nnz, seed).reshape(3, H, nnz)


def heads_operands(n, H, C, concat):
    """hx (3, n, H*C), a_self / a_nbr (H*C,), grad and bias shaped for the output ((.., H*C) or (.., C)): fp64 arrays of fp32 values."""
    op = ladder_operands(n, H * C, seed=7 * H)
    if not concat:
        op['grad'], op['bias'] = np.ascontiguousarray(op['grad'][..., :C]), np.ascontiguousarray(op['bias'][:C])
    return op


def heads_case(csr, H, C, concat, variant, backward=True):
    """Operands, scores, mask, coef and the fp64 reference of one case (backward=False: the forward reference only)."""
    use_mask, use_coef = VARIANTS[variant]
    op = heads_operands(csr.n_rows, H, C, concat)
    ss, sn = heads_scores(csr, H)
    mask = ladder_mask(csr) if use_mask else None
    coef = heads_coef(csr.nnz, H) if use_coef else None
    ref = heads_ref(csr.rowptr, csr.col, mask, coef, op['hx'], ss, sn, H, concat, op['a_self'], op['a_nbr'], op['grad'] if backward else None)
    return dict(op=op, ss=ss, sn=sn, mask=mask, coef=coef, ref=ref)


def dense_entries(csr, values):
    """values (..., nnz) in the pattern's entry order -> dense (..., n, n), zero off the pattern."""
    rows, cols = csr.rows(), np.asarray(csr.col, dtype=np.int64)
    out = np.zeros(values.shape[:-1] + (csr.n_rows, csr.n_cols))
    out[..., rows, cols] = values
    return out


__all__ = ['HEAD_CASES', 'VARIANTS', 'heads_ref', 'heads_scores', 'heads_coef', 'heads_operands', 'heads_case', 'dense_entries', 'f32_exact']
