"""The collapsed DiffusionConv gradients the HIP backward (uds_diffusion_backward) rests on, pinned in fp64 against torch
autograd of the dense restatement (oracle.spektral_dense.diffusion_conv_dense).  With r = x.sum(-1), tot = r.sum(-1),
c0 = theta[:, K], v[p, q] = polyval(theta_q, a_p) - c0[q] and gz = act'(y) gy:

    dr[s, j]     = sum_{i, q} c0[q] gz[s, i, q] + sum_{p : col p = j} sum_q v[p, q] gz[s, row p, q]      (dx[s, j, f] = dr[s, j])
    dtheta[q, k] = sum_{s, i} gz[s, i, q] M_{K-k}[s, i],   M_0 = tot[s],  M_m[s, i] = sum_{p in row i} a_p^m r[s, col p]

No N x N array: `collapsed_grads` works on the CSR support (numpy, fp64) and is also the reference of the GPU test at size."""
import numpy as np
import pytest
import torch

from oracle import spektral_dense as OD


def act_from_pre(z, act):
    return {'linear': lambda t: t, 'relu': lambda t: np.maximum(t, 0.0), 'tanh': np.tanh,
            'sigmoid': lambda t: 1.0 / (1.0 + np.exp(-t))}[act](z)


def act_grad_from_out(y, gy, act):
    return {'linear': gy, 'relu': gy * (y > 0), 'tanh': gy * (1.0 - y * y), 'sigmoid': gy * y * (1.0 - y)}[act]


def _support(rowptr, col, aval, theta):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    K1 = theta.shape[1]
    v = np.broadcast_to(theta[:, 0], (len(col), theta.shape[0])).copy()
    for k in range(1, K1):                                         # Horner on the support values, as tf.math.polyval
        v = v * aval[:, None] + theta[:, k]
    return rows, v - theta[:, K1 - 1]


def collapsed_forward(rowptr, col, aval, theta, r, act):
    """y (S, n_rows, C) in fp64 from r (S, n_cols): act(c0 tot + sum_p v[p] r[col p])."""
    rows, v = _support(rowptr, col, aval, theta)
    n_rows, S = len(rowptr) - 1, r.shape[0]
    z = np.empty((S, n_rows, theta.shape[0]))
    for s in range(S):
        acc = np.zeros((n_rows, theta.shape[0]))
        np.add.at(acc, rows, v * r[s, col][:, None])
        z[s] = acc + theta[:, -1] * r[s].sum()
    return act_from_pre(z, act)


def collapsed_grads(rowptr, col, aval, theta, r, y, gy, act):
    """(dr (S, n_cols), dtheta (C, K1)) in fp64 by the collapsed formulas above."""
    rows, v = _support(rowptr, col, aval, theta)
    S, n_cols = r.shape
    n_rows, K1 = len(rowptr) - 1, theta.shape[1]
    K = K1 - 1
    gz = act_grad_from_out(y, gy, act)
    c0 = theta[:, K]
    dr = np.empty((S, n_cols))
    dtheta = np.zeros(theta.shape)
    for s in range(S):
        t = (v * gz[s, rows]).sum(axis=1)                           # per entry: sum_q v[p, q] gz[s, row p, q]
        drs = np.zeros(n_cols)
        np.add.at(drs, col, t)
        dr[s] = drs + float((gz[s] @ c0).sum())
        rc = r[s, col]
        dtheta[:, K] += gz[s].sum(axis=0) * r[s].sum()
        pw = np.ones(len(col))
        for m in range(1, K1):
            pw = pw * aval
            M = np.zeros(n_rows)
            np.add.at(M, rows, pw * rc)
            dtheta[:, K - m] += gz[s].T @ M
    return dr, dtheta


def nonsymmetric_filter(n=9, seed=0):
    """A directed filter with an isolated row (row 4 and column 4 empty), normalised like DiffusionConv.preprocess."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, n)) < 0.3).astype(np.float64)
    np.fill_diagonal(a, 0.0)
    a[4, :] = a[:, 4] = 0.0
    a[0, 1], a[1, 0], a[2, 3] = 1.0, 0.0, 1.0                    # certainly not symmetric
    a = a * (0.5 + rng.random((n, n)))
    return OD.diffusion_preprocess(torch.from_numpy(a)).numpy()


def csr_of(dense):
    nz = dense != 0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))])
    rows, cols = np.nonzero(nz)
    return rowptr, cols, dense[rows, cols]


@pytest.mark.parametrize('act', ['tanh', 'relu', 'linear', 'sigmoid'])
def test_collapsed_gradients_match_autograd_of_the_dense_call(act):
    g = torch.Generator().manual_seed(3)
    ah = nonsymmetric_filter()
    S, N, F, C, K1 = 3, ah.shape[0], 5, 8, 7
    assert not np.allclose(ah, ah.T) and not ah[4].any() and not ah[:, 4].any()
    x = torch.rand(S, N, F, generator=g, dtype=torch.float64) - 0.3
    theta = (torch.rand(C, K1, generator=g, dtype=torch.float64) * 2 - 1) * 0.3
    gy = torch.rand(S, N, C, generator=g, dtype=torch.float64) - 0.5
    xr, tr = x.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    y = OD.diffusion_conv_dense(xr, torch.from_numpy(ah), tr, act)
    (y * gy).sum().backward()
    rowptr, col, aval = csr_of(ah)
    r = x.sum(-1).numpy()
    y_c = collapsed_forward(rowptr, col, aval, theta.numpy(), r, act)
    assert np.abs(y_c - y.detach().numpy()).max() < 1e-13
    dr, dtheta = collapsed_grads(rowptr, col, aval, theta.numpy(), r, y.detach().numpy(), gy.numpy(), act)
    dx = np.broadcast_to(dr[:, :, None], x.shape)
    assert np.abs(dx - xr.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(xr.grad.numpy()).max())
    assert np.abs(dtheta - tr.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(tr.grad.numpy()).max())
    assert np.abs(tr.grad.numpy()).max() > 1e-3 and np.abs(xr.grad.numpy()).max() > 1e-3     # the check bites
