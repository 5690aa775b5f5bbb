"""CPU checks behind tests/test_gpu_sparse_widths.py: the degree-ladder patterns and the operands are what that file says they
are (every case a lane-group kernel branches on is present), the fp64 references carry signal where the GPU tests need it, and
oracle.gat_csr_ref agrees with oracle.sparse_csr.gat_conv_csr and its autograd on the ladder, the diagonal-less row included.

The kernels visit rows in the handle's degree-sorted schedule, DESCENDING degree with ties in row order, so the row that comes
last in order[] is a lowest-degree one: the 49-entry hub row 66 of ladder(67) is last in ROW order (the unordered backward row
pass and, through the transposed pattern, the column pass shadow it with their surplus groups) and FIRST in order[].  The
ordered kernels' surplus groups shadow a multi-chunk row on thick(67), whose lowest degree is 33, and an empty row on
ladder_rect()."""
import numpy as np
import pytest
import torch

from oracle import sparse_csr as OS
from oracle.gat_csr_ref import act_fn, leaky, masked_backward, masked_forward, masked_forward_backward_f32
from tests.util import (HUB_DEGREE, LADDER_DEGREES, LADDER_NO_DIAG, SPARSE_WIDTHS, gat_ref, ladder, ladder_coef, ladder_mask,
                        ladder_operands, ladder_rect, ladder_scores, sparse_lanes, thick)

GS = (2, 4, 8, 16)
TOL_FWD, TOL_BWD = 5e-6, 1e-5          # the GPU tolerances of tests/test_gpu_sparse_widths.py


def transposed_degrees(csr):
    return np.bincount(csr.col, minlength=csr.n_cols)


def tails(deg, G):
    """nk mod 4 of the last chunk of a row of `deg` entries walked G at a time."""
    return ((deg - 1) % G + 1) % 4


@pytest.mark.parametrize('n', [128, 67])
def test_ladder_degrees(n):
    csr = ladder(n)
    deg, tdeg = csr.degrees(), transposed_degrees(csr)
    assert csr.n_rows == csr.n_cols == n and (np.diff(csr.col)[np.diff(csr.rows()) == 0] > 0).all()      # columns ascend in a row
    assert list(deg[1:15]) == list(LADDER_DEGREES) and deg[n - 1] == HUB_DEGREE
    assert list(tdeg[15:29]) == list(LADDER_DEGREES) and tdeg[0] >= 33
    for G in GS:
        for want in (G - 1, G, G + 1, 2 * G, 2 * G + 1):
            assert want in deg and want in tdeg, (G, want)
        for d_ in (deg, tdeg):      # a chunk of G = 2 entries holds 1 or 2, so 0 and 3 (mod 4) cannot occur there; every other G sees all four
            assert set(tails(d_[d_ > 0], G)) == ({1, 2} if G == 2 else {0, 1, 2, 3}), G
    assert deg.max() == HUB_DEGREE and -(-HUB_DEGREE // 16) >= 4                                        # three chunks of 16 and more
    dense = csr.to_dense()
    assert (dense != dense.T).any()
    targets = np.flatnonzero(dense[n - 1])
    assert not dense[targets[targets != n - 1], n - 1].any()                                            # the hub's targets do not point back
    no_diag = np.flatnonzero(np.diag(dense) == 0)
    assert list(no_diag) == [LADDER_NO_DIAG] and deg[LADDER_NO_DIAG] >= 1


def test_launch_shapes():
    """n = 128: rows * G is a multiple of 256 for every G, no surplus groups; n = 67: ragged for every G."""
    for G in GS:
        assert 128 * G % 256 == 0 and 67 * G % 256 != 0
    assert [sparse_lanes(d) for d in SPARSE_WIDTHS] == [(0, 1), (2, 1), (0, 1), (4, 1), (8, 1), (16, 1), (0, 1), (16, 2), (0, 1)]
    csr = ladder(67)
    order = csr.degree_sorted_rows()
    assert csr.degrees()[66] == HUB_DEGREE and order[0] == 66         # last row, first in the descending schedule
    assert csr.degrees()[order[-1]] == 1                              # what the ordered kernels' surplus groups shadow here
    tk = thick(67)
    deg = tk.degrees()
    assert deg.min() == 33 and deg[tk.degree_sorted_rows()[-1]] == 33 and deg[66] > 33      # multi-chunk in both schedules
    assert (np.diag(tk.to_dense()) == 1).all()


def test_ladder_rect():
    csr = ladder_rect()
    deg = csr.degrees()
    assert (csr.n_rows, csr.n_cols) == (67, 41) and csr.val is not None and len(csr.val) == csr.nnz
    assert list(np.flatnonzero(deg == 0)) == [0, 33, 66] and csr.degree_sorted_rows()[-1] == 66
    assert list(deg[1:15]) == list(LADDER_DEGREES) and deg[65] == 41
    assert (np.diff(csr.col)[np.diff(csr.rows()) == 0] > 0).all()


@pytest.mark.parametrize('make', [lambda: ladder(128), lambda: ladder(67), lambda: thick(67)], ids=['ladder128', 'ladder67', 'thick67'])
def test_operands(make):
    csr = make()
    n, rp, col, rows = csr.n_rows, csr.rowptr, csr.col.astype(np.int64), csr.rows()
    ss, sn = ladder_scores(csr)
    for a in (ss, sn):
        assert (a.astype(np.float32).astype(np.float64) == a).all()
    lg = ss[:, rows] + sn[:, col]
    assert (lg[:2] != 0).all()                                        # no logit on the leaky kink (snapshot 2 forms its sums exactly)
    for s in range(2):
        assert np.abs(ss[s]).max() <= 2 and np.abs(sn[s]).max() <= 2
        for i in np.flatnonzero(csr.degrees() > 1):
            row = lg[s, rp[i]:rp[i + 1]]
            assert (row > 0).any() and (row < 0).any(), (s, i)
    # the overflow snapshot
    assert (np.abs(ss[2]) <= 48).all() and (np.abs(sn[2]) <= 48).all() and (ss[2] * 4 == np.round(ss[2] * 4)).all() and (sn[2] * 4 == np.round(sn[2] * 4)).all()
    sum32 = (ss[2].astype(np.float32)[rows] + sn[2].astype(np.float32)[col]).astype(np.float64)
    assert (sum32 == lg[2]).all()                                     # fp32 forms the sums exactly
    top = leaky(lg[2, rp[n - 1]:rp[n]]).max()
    with np.errstate(over='ignore'):
        assert top >= 89 and not np.isfinite(np.exp(np.float32(top)))  # an unshifted fp32 exp overflows
    # the mask
    mask = ladder_mask(csr)
    off = rows != col
    assert 0.25 < 1 - mask[:, off].mean() < 0.42
    assert (mask[:, ~off] == 0).any() and (mask[:, ~off] != 0).any()  # diagonals are drawn like any entry
    for r in (n - 1, 11):
        assert not mask[0, (rows == r) & off].any() and ((rows == r) & off).sum() >= 16
    hub = mask[1, rp[n - 1]:rp[n]]
    for G in GS:
        for b0 in range(0, len(hub), G):
            chunk = hub[b0:b0 + G]
            assert len(chunk) < 2 or ((chunk == 0).any() and (chunk != 0).any()), (G, b0)
    for r in np.flatnonzero(np.diag(csr.to_dense()) == 0):
        assert not mask[0, rows == r].any()                           # the row without a survivor
    coef = ladder_coef(csr.nnz)
    assert set(np.unique(coef)) == {0.0, 2.0} and 0.4 < (coef == 0).mean() < 0.6


@pytest.fixture(scope='module')
def cases():
    """(name, csr, ss, sn, mask, coef) of the three square patterns."""
    out = []
    for name, csr in (('ladder128', ladder(128)), ('ladder67', ladder(67)), ('thick67', thick(67))):
        ss, sn = ladder_scores(csr)
        out.append((name, csr, ss, sn, ladder_mask(csr), ladder_coef(csr.nnz)))
    return out


@pytest.mark.parametrize('d', [4, 64, 256])
def test_references_carry_signal(cases, d):
    for name, csr, ss, sn, mask, coef in cases:
        op = ladder_operands(csr.n_rows, d)
        plain = gat_ref(csr, ss, sn, None, None, op)
        keys = ('pre',) if name == 'thick67' else ('pre', 'd_hx', 'ds_self', 'ds_nbr')      # thick67 is a forward-only pattern
        for key in keys:
            assert np.abs(plain[key]).max() > 0.05, (name, key)
        relu = act_fn(plain['pre'] + op['bias'], 'relu')
        assert (relu == 0).any() and (relu > 0).any()
        for mk, cf in ((mask, None), (None, coef), (mask, coef)):
            other = gat_ref(csr, ss, sn, mk, cf, op)
            assert np.abs(other['pre'] - plain['pre']).max() > 1e-3 and np.abs(other['d_hx'] - plain['d_hx']).max() > 1e-3
            for key in keys:
                assert np.abs(other[key]).max() > 0.05, (name, key)
        # the overflow snapshot moves the result: the same snapshot with its scores scaled into +-2 gives something else
        ss2, sn2 = ss.copy(), sn.copy()
        ss2[2], sn2[2] = ss[2] / 24, sn[2] / 24
        assert np.abs(gat_ref(csr, ss2, sn2, None, None, op)['pre'][2] - plain['pre'][2]).max() > 1e-3
        # dropping the ds_self or the ds_nbr term of d_hx is 100 GPU tolerances away
        lim = 100 * TOL_BWD * max(1.0, np.abs(plain['d_hx']).max())
        if name != 'thick67':
            assert np.abs(plain['ds_self'][..., None] * op['a_self']).max() > lim and np.abs(plain['ds_nbr'][..., None] * op['a_nbr']).max() > lim


def test_spmm_and_sddmm_references_carry_signal():
    csr = ladder_rect()
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, (3, csr.n_cols, 8)))
    out = OS.incidence_aggregate_csr(x, csr.rowptr, csr.col, csr.val, csr.n_rows)
    assert float(out.abs().max()) > 0.05 and float(out[:, [0, 33, 66]].abs().max()) == 0.0
    assert float((out - OS.incidence_aggregate_csr(x, csr.rowptr, csr.col, np.ones(csr.nnz), csr.n_rows)).abs().max()) > 1e-3


def test_gat_csr_ref_matches_the_csr_oracle_and_its_autograd():
    """All-ones mask and coef on ladder(67): forward and the three gradients against oracle.sparse_csr.gat_conv_csr, 1e-12."""
    csr = ladder(67)
    d = 8
    op = ladder_operands(csr.n_rows, d)
    leaves = [torch.from_numpy(op[k]).clone().requires_grad_(True) for k in ('hx', 'a_self', 'a_nbr', 'bias')]
    hx, a_s, a_n, bias = leaves
    # gat_conv_csr computes hx = x @ kernel itself: feed it hx through the identity kernel
    for act in ('relu', 'tanh', 'linear'):
        for t in leaves:
            t.grad = None
        y = OS.gat_conv_csr(hx, csr.rowptr, csr.col, torch.eye(d, dtype=torch.float64), a_s, a_n, bias, act)
        gout = torch.from_numpy(op['grad'])
        (y * gout).sum().backward()
        ss, sn = op['hx'] @ op['a_self'], op['hx'] @ op['a_nbr']
        rp, col = csr.rowptr.astype(np.int64), csr.col.astype(np.int64)
        ones = np.ones((3, csr.nnz))
        out, alpha = masked_forward(rp, col, ones, ones, op['hx'], ss, sn, op['bias'], act)
        assert np.abs(out - y.detach().numpy()).max() <= 1e-12
        d_hx, ds_self, ds_nbr, gz = masked_backward(rp, col, ones, ones, op['hx'], ss, sn, op['a_self'], op['a_nbr'], alpha, out, op['grad'], act)
        # d_hx already holds the a_self / a_nbr terms (s_self = hx @ a_self); the attention vectors get <ds, hx>
        mine = dict(hx=d_hx, a_self=np.einsum('sn,snc->c', ds_self, op['hx']), a_nbr=np.einsum('sn,snc->c', ds_nbr, op['hx']), bias=gz.sum(axis=(0, 1)))
        for name, leaf in zip(('hx', 'a_self', 'a_nbr', 'bias'), leaves):
            ref = leaf.grad.numpy()
            assert np.abs(ref).max() > 1e-3, name
            assert np.abs(mine[name] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (act, name)
    assert csr.degrees()[LADDER_NO_DIAG] >= 1 and LADDER_NO_DIAG not in csr.col[csr.rowptr[LADDER_NO_DIAG]:csr.rowptr[LADDER_NO_DIAG + 1]]


@pytest.mark.parametrize('d', [4, 64, 256])
def test_plain_fp32_evaluation_order_meets_the_gpu_tolerances(cases, d):
    """The fp32 restatement of oracle.gat_csr_ref on ladder(67), plain and with mask + coef, against the fp64 reference: inside
    TOL_FWD / TOL_BWD (observed / allowed 0.003 - 0.06, printed), so a GPU result outside them is not explained by fp32 rounding."""
    name, csr, ss, sn, mask, coef = cases[1]
    assert name == 'ladder67'
    op = ladder_operands(csr.n_rows, d)
    rp, col, ones = csr.rowptr.astype(np.int64), csr.col.astype(np.int64), np.ones(mask.shape)
    for mk, cf in ((None, None), (mask, coef)):
        ref = gat_ref(csr, ss, sn, mk, cf, op)
        got = masked_forward_backward_f32(rp, col, ones if mk is None else mk, ones if cf is None else cf, op['hx'], ss, sn, op['a_self'],
                                          op['a_nbr'], op['grad'])
        for key, g, tol in zip(('pre', 'd_hx', 'ds_self', 'ds_nbr'), got, (TOL_FWD, TOL_BWD, TOL_BWD, TOL_BWD)):
            ratio = np.abs(g.astype(np.float64) - ref[key]).max() / (tol * max(1.0, np.abs(ref[key]).max()))
            print('fp32 restatement d%d %s %s: observed / allowed %.3f' % (d, 'plain' if mk is None else 'mask + coef', key, ratio))
            assert ratio <= 1.0, (key, ratio)
