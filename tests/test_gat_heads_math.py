"""The multi-head GAT reference of the GPU tests (tests.heads_util.heads_ref: oracle.gat_csr_ref once per head, the heads
concatenated or averaged) pinned on the CPU against oracle.spektral_dense.gat_conv_dense -- Spektral's layer restated for a
(F, H, C) kernel -- and against fp64 torch autograd over it.  Forward and coefficients to 1e-12; the backward (d_hx, ds_self,
ds_nbr folded into the gradients of x, kernel, both attention kernels and the bias) to 1e-12 relative to max(1, max|ref|), the
bound tests/test_use_adj_grad_math.py uses for one head.  Plain, mask, coef and both; concatenation and mean.  Every case can
see a failure: with two heads' attention kernels swapped the reference moves by far more than the GPU tolerance (5e-6)."""
import numpy as np
import pytest
import torch

from oracle import spektral_dense as OD
from oracle.gat_csr_ref import act_fn, act_grad, survivors
from tests.heads_util import VARIANTS, dense_entries, heads_ref
from tests.util import ladder, ladder_mask, thick

S, F = 3, 6
PATTERNS = {'ladder67': lambda: ladder(67), 'thick67': lambda: thick(67)}


@pytest.fixture(scope='module')
def patterns():
    return {k: v() for k, v in PATTERNS.items()}


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('concat', [True, False], ids=['concat', 'mean'])
@pytest.mark.parametrize('H,C', [(2, 8), (3, 4), (4, 16)])
@pytest.mark.parametrize('name', list(PATTERNS))
def test_heads_ref_matches_the_dense_layer_and_its_autograd(patterns, name, H, C, concat, variant, monkeypatch):
    csr = patterns[name]
    n, nnz = csr.n_rows, csr.nnz
    use_mask, use_coef = VARIANTS[variant]
    act = 'tanh'
    g = torch.Generator().manual_seed(100 * H + C)
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5
    x, kernel, a_s, a_n = r(S, n, F) + 0.1, r(F, H, C), r(C, H, 1) * 2, r(C, H, 1) * 2
    width = H * C if concat else C
    bias, gout = r(width) * 0.2, r(S, n, width)
    mask = ladder_mask(csr) if use_mask else None
    if use_mask:
        # a row left without a survivor (the ladder row without a diagonal, in snapshot 0) is 0 on the CSR kernels and a uniform
        # average over all N nodes in the dense layer (every logit -10e9): not a case the two can agree on; it keeps its first entry
        on = survivors(csr.rowptr.astype(np.int64), np.asarray(csr.col, dtype=np.int64), mask)
        for s_, i_ in zip(*np.nonzero(np.add.reduceat(on, csr.rowptr[:-1].astype(np.int64), axis=1) == 0)):
            mask[s_, csr.rowptr[i_]] = 1.0
    coef = np.where(np.random.default_rng(3).random((S, H, nnz)) < 0.5, 0.0, 2.0) if use_coef else None

    # what the dense layer sees: per snapshot the pattern with the masked entries removed and the diagonal entries kept (the
    # layer's set_diag); one ladder row has no diagonal in the pattern, so the layer must not add one: add_self_loops=False
    seen = np.ones((S, nnz)) if mask is None else mask.copy()
    seen[:, csr.rows() == np.asarray(csr.col)] = 1.0
    adj = torch.from_numpy(dense_entries(csr, seen))
    if use_coef:
        dense_coef = torch.from_numpy(dense_entries(csr, coef)).permute(0, 2, 1, 3)          # (S, H, N, N) -> (S, N, H, N)
        monkeypatch.setattr(OD, 'ATTN_DROPOUT', lambda cf, a: cf * dense_coef)
    leaves = [t.clone().requires_grad_(True) for t in (x, kernel, a_s, a_n, bias)]
    y, attn = OD.gat_conv_dense(leaves[0], adj, *leaves[1:], act=act, add_self_loops=False, concat_heads=concat,
                                 return_attn=True)
    (y * gout).sum().backward()

    xn = x.numpy()
    W2 = kernel.numpy().reshape(F, H * C)
    hx = xn @ W2
    as_hm, an_hm = a_s.numpy().reshape(C, H).T, a_n.numpy().reshape(C, H).T                  # (H, C), head-major
    hx4 = hx.reshape(S, n, H, C)
    ss, sn = np.einsum('snhc,hc->snh', hx4, as_hm), np.einsum('snhc,hc->snh', hx4, an_hm)
    fwd = heads_ref(csr.rowptr, csr.col, mask, coef, hx, ss, sn, H, concat)
    out = act_fn(fwd['pre'] + bias.numpy(), act)
    assert np.abs(out - y.detach().numpy()).max() <= 1e-12
    # the dense layer returns alpha * coef under dropout (its `coef` after ATTN_DROPOUT), (S, N, H, N)
    dense_attn = dense_entries(csr, fwd['alpha_coef']).transpose(0, 2, 1, 3)
    assert np.abs(dense_attn - attn.detach().numpy()).max() <= 1e-12
    if not use_mask:
        assert np.abs(fwd['alpha'].sum(axis=-1) - n).max() <= 1e-9                           # every row's softmax sums to one

    gz = act_grad(out, gout.numpy(), act)
    ref = heads_ref(csr.rowptr, csr.col, mask, coef, hx, ss, sn, H, concat, as_hm.reshape(-1), an_hm.reshape(-1), gz)
    mine = dict(x=ref['d_hx'] @ W2.T,
                kernel=np.einsum('snf,snc->fc', xn, ref['d_hx']).reshape(F, H, C),
                a_s=np.einsum('snh,snhc->ch', ref['ds_self'], hx4).reshape(C, H, 1),
                a_n=np.einsum('snh,snhc->ch', ref['ds_nbr'], hx4).reshape(C, H, 1),
                bias=gz.sum(axis=(0, 1)))
    for key, leaf in zip(('x', 'kernel', 'a_s', 'a_n', 'bias'), leaves):
        want = leaf.grad.numpy()
        assert np.abs(want).max() > 1e-3, key                                                # the check bites
        assert np.abs(mine[key] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), key

    # the case can see a failure: heads 0 and 1 with their attention kernels (their scores) swapped
    swap = list(range(H))
    swap[0], swap[1] = 1, 0
    wrong = heads_ref(csr.rowptr, csr.col, mask, coef, hx, ss[..., swap], sn[..., swap], H, concat)
    assert np.abs(wrong['pre'] - fwd['pre']).max() > 1e-3 * max(1.0, np.abs(fwd['pre']).max())
    assert np.abs(wrong['alpha_coef'] - fwd['alpha_coef']).max() > 1e-3
