"""uds_gat_backward_act restated in fp64: the whole reverse mode of a single-head GAT layer after its projection -- activation
backward, softmax / leaky-relu / aggregation backward, bias gradient, attention-kernel gradients -- as one function of the
operator's own arguments, `restate`.  Pinned here against torch autograd of the dense restatement of the layer
(oracle.spektral_dense.gat_conv_dense) for the five activations with and without edge mask / attention-dropout coef;
tests/test_gpu_gat_backward_act.py trusts it as the reference of db and da.  Also on the CPU: the host-side refusals of
_lib.gat_backward_act and the workspace size function."""
import types

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from oracle import spektral_dense as OD

ACTS = ['linear', 'relu', 'tanh', 'sigmoid', 'hard_sigmoid']
WG_MAX = 2048       # GAT_ACT_WG_MAX of csrc/kernels_backward.hpp: the most partials a pass of the operator writes


def act_grad64(out, gout, act):
    """dL/dz from dL/dy for y = act(z), from y alone: autograd.act_grad."""
    if act == 'linear':
        return gout
    if act == 'relu':
        return torch.where(out > 0, gout, torch.zeros_like(gout))
    if act == 'tanh':
        return gout * (1.0 - out * out)
    if act == 'sigmoid':
        return gout * out * (1.0 - out)
    if act == 'hard_sigmoid':
        return gout * 0.2 * ((out > 0) & (out < 1)).to(gout.dtype)
    raise ValueError(act)


def restate(rows, col, out, gout, act, hx, s_self, s_nbr, a_self, a_nbr, mask=None, coef=None):
    """(d_hx, ds_self, ds_nbr, db, da) in the arithmetic of the arguments (fp64 tensors: fp64).  rows / col: the pattern's
    entries in row-major order (int64 tensors); out, gout, hx (S,n,d); s_self, s_nbr (S,n); a_self, a_nbr (d,); mask, coef
    (S,nnz) or None.  An entry takes part iff mask != 0 or it is its row's diagonal."""
    S, n, d = out.shape
    nnz = rows.numel()
    on = torch.ones((S, nnz), dtype=torch.bool) if mask is None else (mask != 0) | (rows == col)[None]
    cf = torch.ones((S, nnz), dtype=out.dtype) if coef is None else coef
    idx = rows[None].expand(S, nnz)
    jdx = col[None].expand(S, nnz)
    g = act_grad64(out, gout, act)
    lgt = s_self[:, rows] + s_nbr[:, col]
    e = torch.where(lgt > 0, lgt, 0.2 * lgt)
    e = torch.where(on, e, torch.full_like(e, -float('inf')))
    m = torch.full((S, n), -float('inf'), dtype=out.dtype).scatter_reduce(1, idx, e, 'amax')
    w = torch.where(on, torch.exp(e - m[:, rows]), torch.zeros_like(e))
    den = torch.zeros((S, n), dtype=out.dtype).scatter_add(1, idx, w)
    alpha = torch.where(on, w / den[:, rows], torch.zeros_like(w))
    q = (g[:, rows] * hx[:, col]).sum(-1) * cf
    cbar = torch.zeros((S, n), dtype=out.dtype).scatter_add(1, idx, alpha * q)
    dl = alpha * (q - cbar[:, rows])
    de = torch.where(lgt > 0, dl, 0.2 * dl)
    ds_self = torch.zeros((S, n), dtype=out.dtype).scatter_add(1, idx, de)
    ds_nbr = torch.zeros((S, n), dtype=out.dtype).scatter_add(1, jdx, de)
    d_hx = torch.zeros_like(hx).index_add_(1, col, (alpha * cf)[..., None] * g[:, rows])
    d_hx = d_hx + ds_self[..., None] * a_self + ds_nbr[..., None] * a_nbr
    db = g.sum((0, 1))
    da = torch.stack([torch.einsum('sn,snd->d', ds_self, hx), torch.einsum('sn,snd->d', ds_nbr, hx)])
    return d_hx, ds_self, ds_nbr, db, da


def hub_pattern(n=24, seed=0):
    """Symmetric pattern with self loops: row 0 a hub of 21 entries (more than 16 lanes), plus sparse random edges."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, n))
    a[0, 1:21] = a[1:21, 0] = 1.0
    e = rng.random((n, n)) < 0.12
    a[e | e.T] = 1.0
    np.fill_diagonal(a, 1.0)
    rows, cols = np.nonzero(a != 0)
    return torch.from_numpy(rows), torch.from_numpy(cols)


@pytest.mark.parametrize('variant', ['plain', 'mask', 'coef', 'both'])
@pytest.mark.parametrize('act', ACTS)
def test_restatement_matches_autograd_of_the_dense_layer(act, variant, monkeypatch):
    S, F, C, n = 3, 6, 8, 24
    rows, col = hub_pattern(n)
    nnz = rows.numel()
    off = rows != col
    rng = np.random.default_rng(1)
    mask = coef = None
    if variant in ('mask', 'both'):
        mask = torch.from_numpy((rng.random((S, nnz)) > 0.3).astype(np.float64))
        mask[0, (rows == 5) & off] = 0.0                     # a row emptied down to its diagonal
        mask[:, (rows == 0) & (col == 3)] = 0.0
        assert ((rows == 5) & off).any() and bool((mask[:, off] == 0).any()) and bool((mask[:, off] != 0).any())
    if variant in ('coef', 'both'):
        coef = torch.from_numpy(np.where(rng.random((S, nnz)) < 0.5, 0.0, 2.0))
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    # scales that put hard_sigmoid on both sides of both of its kinks and tanh / sigmoid away from their flat ends
    x, kernel = (rnd(S, n, F) - 0.4) * 3, (rnd(F, 1, C) - 0.5) * 3
    a_s, a_n = (rnd(C, 1, 1) - 0.5) * 2, (rnd(C, 1, 1) - 0.5) * 2
    bias, gout = (rnd(C) - 0.5) * 0.2, rnd(S, n, C) - 0.5

    adj = torch.zeros(S, n, n, dtype=torch.float64)
    adj[:, rows, col] = 1.0 if mask is None else mask
    if coef is not None:
        dense_coef = torch.zeros(S, n, 1, n, dtype=torch.float64)
        dense_coef[:, rows, 0, col] = coef
        monkeypatch.setattr(OD, 'ATTN_DROPOUT', lambda c_, a_: c_ * dense_coef)
    leaves = [t.clone().requires_grad_(True) for t in (x, kernel, a_s, a_n, bias)]
    y = OD.gat_conv_dense(leaves[0], adj, *leaves[1:], act=act)
    (y * gout).sum().backward()
    y = y.detach()
    if act == 'hard_sigmoid':
        assert bool((y == 0).any()) and bool((y == 1).any()) and bool(((y > 0) & (y < 1)).any())
    if act == 'relu':
        assert bool((y == 0).any()) and bool((y > 0).any())

    W = kernel.reshape(F, C)
    hx = x @ W
    ss, sn = hx @ a_s.reshape(-1), hx @ a_n.reshape(-1)
    d_hx, ds_self, ds_nbr, db, da = restate(rows, col, y, gout, act, hx, ss, sn, a_s.reshape(-1), a_n.reshape(-1), mask, coef)
    mine = dict(x=d_hx @ W.t(), kernel=torch.einsum('snf,snc->fc', x, d_hx).reshape(F, 1, C), a_s=da[0].reshape(C, 1, 1),
                a_n=da[1].reshape(C, 1, 1), bias=db)
    for name, leaf in zip(('x', 'kernel', 'a_s', 'a_n', 'bias'), leaves):
        ref = leaf.grad
        assert float(ref.abs().max()) > 1e-3, name                                    # the check bites
        assert float((mine[name] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), name


def test_mask_and_coef_change_the_restated_gradients():
    S, C, n = 2, 4, 24
    rows, col = hub_pattern(n)
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) - 0.5
    out, gout, hx, a_s, a_n = rnd(S, n, C), rnd(S, n, C), rnd(S, n, C), rnd(C), rnd(C)
    mask = (torch.rand(S, rows.numel(), generator=g) > 0.3).double()
    coef = (torch.rand(S, rows.numel(), generator=g) > 0.5).double() * 2
    base = restate(rows, col, out, gout, 'tanh', hx, hx @ a_s, hx @ a_n, a_s, a_n)
    for kw in (dict(mask=mask), dict(coef=coef)):
        other = restate(rows, col, out, gout, 'tanh', hx, hx @ a_s, hx @ a_n, a_s, a_n, **kw)
        assert float((other[4] - base[4]).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------- host side, no device

@pytest.mark.parametrize('S,n,nnz,d', [(1, 37, 120, 64), (3, 37, 121, 12), (1, 1, 1, 4), (4, 1000, 2999, 128), (1000, 2000, 5998, 64)])
def test_workspace_floats(S, n, nnz, d):
    """alpha and de (S * nnz each, rounded up to a multiple of 4), g (S * n * d) and 3 d floats per partial, of which a pass
    writes at most min(S * n, WG_MAX): the partials do not grow with the batch."""
    a4 = (S * nnz + 3) // 4 * 4
    want = 2 * a4 + S * n * d + 3 * d * min(S * n, WG_MAX)
    assert _lib.gat_backward_act_workspace_floats(S, n, nnz, d) == want
    assert want % 4 == 0


def test_workspace_floats_of_an_empty_call():
    for S, n, nnz, d in [(0, 37, 120, 64), (3, 0, 0, 64), (3, 37, -1, 64), (3, 37, 120, 0)]:
        assert _lib.gat_backward_act_workspace_floats(S, n, nnz, d) == 0


def test_partials_are_bounded_at_the_c5_batch():
    """1000 graphs x 2000 nodes at d = 64: 1.5 MiB of partials beside 512 MB of g."""
    S, n, nnz, d = 1000, 2000, 5998, 64
    parts = _lib.gat_backward_act_workspace_floats(S, n, nnz, d) - 2 * ((S * nnz + 3) // 4 * 4) - S * n * d
    assert parts == 3 * d * WG_MAX and parts * 4 == 1536 * 1024


def _cpu_call(n=5, S=2, d=8, nnz=9, **over):
    h = types.SimpleNamespace(n_rows=n, n_cols=n, nnz=nnz, ptr=None)
    z = lambda *s: torch.zeros(*s)
    kw = dict(handle=h, handle_t=h, perm_t=torch.zeros(nnz, dtype=torch.int32), out=z(S, n, d), gout=z(S, n, d), act='relu', hx=z(S, n, d),
              s_self=z(S, n), s_nbr=z(S, n), a_self=z(d), a_nbr=z(d))
    kw.update(over)
    return _lib.gat_backward_act(**kw)


@pytest.mark.parametrize('over,text', [
    (dict(gout=torch.zeros(2, 5, 4)), 'one shape'),
    (dict(out=torch.zeros(10, 8), gout=torch.zeros(10, 8)), 'one shape'),
    (dict(act='gelu'), 'unknown activation'),
    (dict(hx=torch.zeros(2, 5, 4)), 'do not match'),
    (dict(s_self=torch.zeros(2, 4)), 'do not match'),
    (dict(s_nbr=torch.zeros(5)), 'do not match'),
    (dict(n=6, out=torch.zeros(2, 5, 8), gout=torch.zeros(2, 5, 8), hx=torch.zeros(2, 5, 8), s_self=torch.zeros(2, 5), s_nbr=torch.zeros(2, 5)),
     'do not match a 6-row pattern'),
    (dict(a_self=torch.zeros(4)), 'expected 8 values'),
    (dict(edge_mask=torch.zeros(2, 8)), 'edge_mask'),
    (dict(coef=torch.zeros(1, 9)), 'coef'),
    (dict(outputs=(torch.zeros(2, 5, 4), None, None, None, None)), 'd_hx'),
    (dict(outputs=(None, None, None, torch.zeros(4), None)), 'db'),
    (dict(outputs=(None, None, None, None, torch.zeros(8, 2))), 'da'),
    (dict(workspace=torch.zeros(8)), 'workspace'),
    (dict(workspace=torch.zeros(2, 4096)), 'workspace'),
])
def test_host_side_refusals(over, text):
    with pytest.raises(_lib.UdsError, match=text):
        _cpu_call(**over)


def test_cpu_tensors_are_refused_not_computed():
    with pytest.raises(_lib.UdsError):
        _cpu_call()
