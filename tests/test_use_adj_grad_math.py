"""The masked GAT forward and backward that uds_gat_aggregate_ex / uds_gat_backward_ex compute, restated in fp64 on the CSR
pattern (oracle/gat_csr_ref.py, whose header holds the formulas) and pinned against torch autograd of the dense restatement
(oracle.spektral_dense.gat_conv_dense) fed the per-snapshot (S, N, N) adjacency of `use_adj`."""
import numpy as np
import pytest
import torch

from oracle import spektral_dense as OD
from oracle.gat_csr_ref import act_fn, act_grad, leaky, masked_backward, masked_forward, survivors  # noqa: F401


def hub_pattern(n=24, seed=0):
    """Symmetric pattern with self loops: row 0 a hub of 21 entries (more than 16 lanes), plus sparse random edges."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, n))
    a[0, 1:21] = a[1:21, 0] = 1.0
    e = rng.random((n, n)) < 0.12
    a[e | e.T] = 1.0
    np.fill_diagonal(a, 1.0)
    nz = a != 0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))])
    rows, cols = np.nonzero(nz)
    return rowptr, cols, rows


def draw_mask(rowptr, col, rows, S, seed):
    """(S, nnz) 0/1, about a third of the off-diagonal entries off, with row 5 losing every off-diagonal entry in snapshot 0
    and the hub row losing some of its entries in every snapshot."""
    rng = np.random.default_rng(seed)
    mask = (rng.random((S, len(col))) > 0.3).astype(np.float64)
    off = rows != col
    mask[0, (rows == 5) & off] = 0.0
    mask[:, (rows == 0) & (col == 3)] = 0.0
    return mask


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('with_coef', [False, True])
def test_masked_gat_gradients_match_autograd_of_the_dense_call(act, with_coef, monkeypatch):
    S, F, C = 3, 6, 8
    rowptr, col, rows = hub_pattern()
    n = len(rowptr) - 1
    mask = draw_mask(rowptr, col, rows, S, seed=1)
    off = rows != col
    # the cases the kernels branch on are present
    assert np.diff(rowptr)[0] > 16
    assert (mask[:, (rows == 0) & off] == 0).any() and (mask[:, (rows == 0) & off] != 0).any()
    assert not mask[0, (rows == 5) & off].any() and ((rows == 5) & off).any()
    key = {(r, c): p for p, (r, c) in enumerate(zip(rows, col))}
    asym = [(s, p) for s in range(S) for p in range(len(col)) if off[p] and mask[s, p] == 0 and mask[s, key[(col[p], rows[p])]] != 0]
    assert asym, 'no entry masked while its transpose survives'

    g = torch.Generator().manual_seed(7)
    x = torch.rand(S, n, F, generator=g, dtype=torch.float64) - 0.4
    kernel = (torch.rand(F, 1, C, generator=g, dtype=torch.float64) - 0.5)
    a_s = (torch.rand(C, 1, 1, generator=g, dtype=torch.float64) - 0.5) * 2
    a_n = (torch.rand(C, 1, 1, generator=g, dtype=torch.float64) - 0.5) * 2
    bias = (torch.rand(C, generator=g, dtype=torch.float64) - 0.5) * 0.2
    gout = torch.rand(S, n, C, generator=g, dtype=torch.float64) - 0.5
    coef = np.ones(mask.shape)
    if with_coef:
        coef = np.where(np.random.default_rng(3).random(mask.shape) < 0.5, 0.0, 2.0)

    # the (S, N, N) adjacency the reference sees: the static pattern with the masked entries removed
    adj = np.zeros((S, n, n))
    for s in range(S):
        adj[s, rows, col] = mask[s]
    if with_coef:
        dense_coef = np.zeros((S, n, 1, n))
        for s in range(S):
            dense_coef[s, rows, 0, col] = coef[s]
        monkeypatch.setattr(OD, 'ATTN_DROPOUT', lambda cf, a: cf * torch.from_numpy(dense_coef))
    leaves = [t.clone().requires_grad_(True) for t in (x, kernel, a_s, a_n, bias)]
    y = OD.gat_conv_dense(leaves[0], torch.from_numpy(adj), *leaves[1:], act=act)
    (y * gout).sum().backward()

    xn, W = x.numpy(), kernel.numpy().reshape(F, C)
    hx = xn @ W
    ss, sn = hx @ a_s.numpy().reshape(-1), hx @ a_n.numpy().reshape(-1)
    out, alpha = masked_forward(rowptr, col, mask, coef, hx, ss, sn, bias.numpy(), act)
    assert np.abs(out - y.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(out).max())
    on = survivors(rowptr, col, mask)
    assert (alpha[~on] == 0).all() and (alpha[on] > 0).all()
    d_hx, ds_self, ds_nbr, gz = masked_backward(rowptr, col, mask, coef, hx, ss, sn, a_s.numpy().reshape(-1), a_n.numpy().reshape(-1),
                                                alpha, out, gout.numpy(), act)
    mine = dict(x=d_hx @ W.T,
                kernel=np.einsum('snf,snc->fc', xn, d_hx).reshape(F, 1, C),
                a_s=np.einsum('sn,snc->c', ds_self, hx).reshape(C, 1, 1),
                a_n=np.einsum('sn,snc->c', ds_nbr, hx).reshape(C, 1, 1),
                bias=gz.sum(axis=(0, 1)))
    for name, leaf in zip(('x', 'kernel', 'a_s', 'a_n', 'bias'), leaves):
        ref = leaf.grad.numpy()
        assert np.abs(ref).max() > 1e-3, name                                    # the check bites
        assert np.abs(mine[name] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name


def test_the_mask_changes_the_gradients():
    """The restatement with an all-ones mask differs from the masked one: the cases above do exercise the mask."""
    S, F, C = 2, 5, 4
    rowptr, col, rows = hub_pattern()
    n = len(rowptr) - 1
    mask = draw_mask(rowptr, col, rows, S, seed=1)
    rng = np.random.default_rng(0)
    hx = rng.random((S, n, C)) - 0.5
    a_s, a_n = rng.random(C) - 0.5, rng.random(C) - 0.5
    ss, sn = hx @ a_s, hx @ a_n
    coef = np.ones(mask.shape)
    gout = rng.random((S, n, C)) - 0.5
    res = []
    for mk in (mask, np.ones_like(mask)):
        out, alpha = masked_forward(rowptr, col, mk, coef, hx, ss, sn, np.zeros(C), 'tanh')
        res.append(masked_backward(rowptr, col, mk, coef, hx, ss, sn, a_s, a_n, alpha, out, gout, 'tanh')[0])
    assert np.abs(res[0] - res[1]).max() > 1e-3
