"""fp64 parity of the sparse row kernels at every lane-group shape: uds_csr_spmm, uds_csr_sddmm, uds_gat_aggregate[_ex / _masked /
_coef] and uds_gat_backward[_ex / _coef] at the widths SPARSE_WIDTHS = 4 .. 256 on the degree-ladder patterns of tests/util.py.
References: oracle/gat_csr_ref.py (fp64 NumPy, pinned on the CPU by tests/test_use_adj_grad_math.py and
tests/test_sparse_ref_math.py), oracle.sparse_csr.incidence_aggregate_csr, and an fp64 einsum for the SDDMM.

Which width reaches which kernel (group_shape of kernels_sparse.hpp, lanes_per_item of kernels_backward.hpp):
  d = 8, 16, 32, 64   k_csr_spmm_g / k_gat_aggregate_g / k_gat_bwd_rows_g / k_gat_bwd_cols_g <G, 1>, G = d / 4 = 2, 4, 8, 16
  d = 128             the same templates <16, 2>
  d = 4, 12, 96, 256  the walking kernels k_csr_spmm, k_gat_aggregate[_x], k_gat_bwd_rows (1, 2, 16, 16 lanes per row), k_gat_bwd_cols
  uds_gat_aggregate_masked / _coef and uds_gat_backward_coef with a coef: their walking kernels at every width (test (d))
  k_csr_sddmm: 1, 2, 2, 4, 8, 16, 16, 16, 16 lanes per entry; d = 12 and 96 give a strided loop whose trip count differs by lane
The _ex entries run the EX = true instantiations; mask / coef / both each get their own fp64 reference.

Patterns (tests/util.py; tests/test_sparse_ref_math.py asserts what is claimed here):
  ladder(128)   row degrees 1 2 3 4 5 7 8 9 15 16 17 31 32 33 in rows 1 .. 14 and 49 in row 127, the same ladder of column degrees
                in columns 15 .. 28, a hub column 0, one row without its diagonal; 128 G is a multiple of 256: no surplus groups
  ladder(67)    the same on 67 nodes: ragged launches for every G; row 66, the last, is the 49-entry hub, so the surplus groups of
                the backward row pass (rows in row order) shadow a four-chunk row
  thick(67)     forward only: every row has 33 .. 49 entries.  The handle's schedule order[] runs by DESCENDING degree, so the row
                last in order[] -- the one the aggregation kernels' surplus groups shadow -- is a lowest-degree row: degree 1 on
                ladder(67), 33 (three chunks of 16) here
  ladder_rect() 67 x 41 with values; rows 0, 33 and 66 are empty, 66 last in order[]; a 41-entry row
Scores: snapshots 0 and 1 in +-2 with both leaky slopes in every multi-entry row; snapshot 2 multiples of 0.25 in [-48, 48] with a
logit of 92 in the last row (only the row-maximum shift keeps expf finite).  Mask and coef as tests.util.ladder_mask / ladder_coef.

Every input is a view inside a NaN-filled allocation, every output a view inside a sentinel-filled one that is checked on both
sides and for finiteness; the backward's alpha / de workspace is a guarded tensor pre-filled with NaN, so finite outputs prove
that the row pass wrote every entry the column pass reads.  Plain allocations: nothing here is meant to fault.

Tolerances, relative to max(1, max|ref|) through tests.util.close (UDS_TOL_REPORT=1 prints observed / allowed): forward, SpMM and
SDDMM TOL = 5e-6 (tests/test_gpu_parity.py, test_spmm_backward_and_sddmm), GAT backward outputs 1e-5 (test_gat_backward).

MEASURED on an MI355X (UDS_TOL_REPORT=1), worst observed / allowed per test over all its cases [case]:
  (a) test_gat_aggregate                   0.040  [64-thick67]
  (b) test_gat_backward                    0.032  [256-ladder128]
  (c) test_gat_ex                          0.062  [12-thick67-both]
  (d) test_gat_legacy_entries              0.038  [64-ladder128]
  (e) test_csr_spmm, test_csr_spmm_thick   0.076  [64]
  (f) test_csr_sddmm                       0.034  [256-ladder67-3]
(g), (h) are bitwise comparisons.  No bound was raised.  Plain fp32 evaluation in entry order on the CPU
(oracle.gat_csr_ref.masked_forward_backward_f32, tests/test_sparse_ref_math.py) gives 0.003 - 0.06 for the GAT outputs.
"""
import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from oracle import sparse_csr as OS
from oracle.gat_csr_ref import act_fn
from tests.util import (SPARSE_WIDTHS, Guarded, close, f32_exact, gat_ref, ladder, ladder_coef, ladder_mask, ladder_operands, ladder_rect,
                        ladder_scores, nan_in, thick)

pytestmark = pytest.mark.gpu

TOL = 5e-6
TOL_BWD = 1e-5
S = 3
COEF_SEED = 11
LADDERS = ['ladder128', 'ladder67']
SQUARE = LADDERS + ['thick67']
LEGACY_WIDTHS = [4, 8, 12, 64, 96, 128]
SUBSET_WIDTHS = [8, 32, 96, 128]
VARIANTS = {'mask': (True, False), 'coef': (False, True), 'both': (True, True)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


class Pattern:
    """A square pattern with its handles, scores, mask and coef, on the host in fp64 and on the device in NaN-padded fp32."""

    def __init__(self, csr, dev):
        self.csr, self.n = csr, csr.n_rows
        self.h = _lib.CsrHandle(csr)
        self.ht, self.perm = self.h.transposed(dev)
        assert list(self.h.row_order()) == list(csr.degree_sorted_rows())
        self.ss, self.sn = ladder_scores(csr)
        self.mask = ladder_mask(csr)
        coef = _lib.dropout(torch.ones((S, csr.nnz), device=dev), 0.5, COEF_SEED, 0)
        self.coef = coef.double().cpu().numpy()
        assert (self.coef == ladder_coef(csr.nnz, COEF_SEED)).all()
        lg = self.ss[2, self.n - 1] + self.sn[2, csr.col[csr.rowptr[self.n - 1]:csr.rowptr[self.n]]]
        assert lg.max() >= 89                                   # an unshifted expf overflows in the last row of snapshot 2
        f = lambda a: nan_in(torch.from_numpy(a), dev)
        self.d_ss, self.d_sn, self.d_mask, self.d_coef = f(self.ss), f(self.sn), f(self.mask), f(self.coef)
        self.ops, self.refs = {}, {}

    def operands(self, d, dev):
        """(host dict, device dict) of hx, grad, bias, a_self, a_nbr at width d."""
        if d not in self.ops:
            op = ladder_operands(self.n, d)
            self.ops[d] = (op, {k: nan_in(torch.from_numpy(v), dev) for k, v in op.items()})
        return self.ops[d]

    def ref(self, d, variant):
        """fp64 reference (tests.util.gat_ref) of variant 'plain', 'mask', 'coef' or 'both' at width d, computed once."""
        if (d, variant) not in self.refs:
            mk, cf = VARIANTS.get(variant, (False, False))
            self.refs[(d, variant)] = gat_ref(self.csr, self.ss, self.sn, self.mask if mk else None, self.coef if cf else None, self.ops[d][0])
        return self.refs[(d, variant)]


@pytest.fixture(scope='module')
def pats(dev):
    return {'ladder128': Pattern(ladder(128), dev), 'ladder67': Pattern(ladder(67), dev), 'thick67': Pattern(thick(67), dev)}


def check(what, got, ref, tol):
    """tests.util.close (which records observed / allowed for UDS_TOL_REPORT and names both in its failure), then the figure."""
    ref = torch.from_numpy(np.ascontiguousarray(ref)) if isinstance(ref, np.ndarray) else ref
    err = close(got, ref, tol, _depth=2)
    print('%-72s err %.3e  ratio %.3f' % (what, err, err / (tol * max(1.0, float(ref.abs().max())))))
    return err


def forward(entry, pt, dv, dev, bias, act, **kw):
    """One guarded aggregation call: the result view, checked on both sides and for finiteness."""
    out = Guarded((S, pt.n, dv['hx'].shape[-1]), dev)
    got = entry(pt.h, dv['hx'], pt.d_ss, pt.d_sn, dv['bias'] if bias else None, act, out=out.view, **kw)
    assert got is out.view
    torch.cuda.synchronize()
    out.check('out')
    return got


def backward(entry, pt, dv, dev, **kw):
    """One guarded backward call: (d_hx, ds_self, ds_nbr), the outputs and the NaN-pre-filled workspace checked."""
    d = dv['hx'].shape[-1]
    outs = [Guarded((S, pt.n, d), dev), Guarded((S, pt.n), dev), Guarded((S, pt.n), dev)]
    ws = Guarded((2, S, pt.csr.nnz), dev, torch.full((2, S, pt.csr.nnz), float('nan')))
    got = entry(pt.h, pt.ht, pt.perm, dv['grad'], dv['hx'], pt.d_ss, pt.d_sn, dv['a_self'], dv['a_nbr'], out=tuple(o.view for o in outs),
                workspace=ws.view, **kw)
    torch.cuda.synchronize()
    for o, g, name in zip(outs, got, ('d_hx', 'ds_self', 'ds_nbr')):
        assert g is o.view
        o.check(name)
    ws.check('alpha / de workspace (an entry the row pass did not write?)')
    return got


def check_backward(what, got, ref):
    for g, name in zip(got, ('d_hx', 'ds_self', 'ds_nbr')):
        check('%s %s' % (what, name), g, ref[name], TOL_BWD)


def ex_args(pt, variant):
    mk, cf = VARIANTS[variant]
    return dict(edge_mask=pt.d_mask if mk else None, coef=pt.d_coef if cf else None)


# ---- (a) uds_gat_aggregate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SQUARE)
@pytest.mark.parametrize('d', SPARSE_WIDTHS)
def test_gat_aggregate(dev, pats, d, name):
    pt = pats[name]
    op, dv = pt.operands(d, dev)
    pre = pt.ref(d, 'plain')['pre']
    for act in ('relu', 'tanh', 'linear'):
        for bias in (True, False):
            got = forward(_lib.gat_aggregate, pt, dv, dev, bias, act)
            check('aggregate %s d%d %s bias=%d' % (name, d, act, bias), got, act_fn(pre + (op['bias'] if bias else 0.0), act), TOL)


# ---- (b) uds_gat_backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LADDERS)
@pytest.mark.parametrize('d', SPARSE_WIDTHS)
def test_gat_backward(dev, pats, d, name):
    pt = pats[name]
    _, dv = pt.operands(d, dev)
    check_backward('backward %s d%d' % (name, d), backward(_lib.gat_backward, pt, dv, dev), pt.ref(d, 'plain'))


# ---- (c) uds_gat_aggregate_ex / uds_gat_backward_ex ---------------------------------------------------------------------------
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', SQUARE)
@pytest.mark.parametrize('d', SPARSE_WIDTHS)
def test_gat_ex(dev, pats, d, name, variant):
    pt = pats[name]
    op, dv = pt.operands(d, dev)
    ref = pt.ref(d, variant)
    for act, bias in (('relu', True), ('linear', False)):
        got = forward(_lib.gat_aggregate_ex, pt, dv, dev, bias, act, **ex_args(pt, variant))
        check('aggregate_ex %s d%d %s %s' % (name, d, variant, act), got, act_fn(ref['pre'] + (op['bias'] if bias else 0.0), act), TOL)
    if name in LADDERS:
        check_backward('backward_ex %s d%d %s' % (name, d, variant), backward(_lib.gat_backward_ex, pt, dv, dev, **ex_args(pt, variant)), ref)


# ---- (d) the legacy entries: uds_gat_aggregate_masked, uds_gat_aggregate_coef, uds_gat_backward_coef ----------------------------
@pytest.mark.parametrize('name', LADDERS)
@pytest.mark.parametrize('d', LEGACY_WIDTHS)
def test_gat_legacy_entries(dev, pats, d, name):
    pt = pats[name]
    op, dv = pt.operands(d, dev)
    got = forward(_lib.gat_aggregate, pt, dv, dev, True, 'tanh', edge_mask=pt.d_mask)
    check('aggregate(edge_mask=) %s d%d' % (name, d), got, act_fn(pt.ref(d, 'mask')['pre'] + op['bias'], 'tanh'), TOL)
    got = forward(_lib.gat_aggregate, pt, dv, dev, True, 'relu', coef=pt.d_coef)
    check('aggregate(coef=) %s d%d' % (name, d), got, act_fn(pt.ref(d, 'coef')['pre'] + op['bias'], 'relu'), TOL)
    check_backward('backward(coef=) %s d%d' % (name, d), backward(_lib.gat_backward, pt, dv, dev, coef=pt.d_coef), pt.ref(d, 'coef'))


# ---- (e) uds_csr_spmm, (f) uds_csr_sddmm ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rect(dev):
    csr = ladder_rect()
    return csr, _lib.CsrHandle(csr), nan_in(torch.from_numpy(csr.val), dev)


def uniform(seed, *shape):
    return f32_exact(np.random.default_rng(seed).uniform(-0.5, 0.5, shape))


@pytest.mark.parametrize('F', SPARSE_WIDTHS)
def test_csr_spmm(dev, rect, F):
    csr, h, val = rect
    assert list(h.row_order())[-1] == 66 and csr.degrees()[66] == 0
    x, bias = uniform(40 + F, S, csr.n_cols, F), uniform(41 + F, F)
    xd, bd = nan_in(torch.from_numpy(x), dev), nan_in(torch.from_numpy(bias), dev)
    xt = torch.from_numpy(x)
    cases = [('val', val, None, 'linear', OS.incidence_aggregate_csr(xt, csr.rowptr, csr.col, csr.val, csr.n_rows)),
             ('val=None', None, None, 'linear', OS.incidence_aggregate_csr(xt, csr.rowptr, csr.col, np.ones(csr.nnz), csr.n_rows))]
    cases.append(('bias + relu', val, bd, 'relu', torch.relu(cases[0][4] + torch.from_numpy(bias))))
    for what, v, b, act, ref in cases:
        out = Guarded((S, csr.n_rows, F), dev)
        got = _lib.csr_spmm(h, v, xd, b, act, out=out.view)
        assert got is out.view
        torch.cuda.synchronize()
        out.check('out')
        check('spmm F%d %s' % (F, what), got, ref, TOL)
    assert float(ref[:, [0, 33, 66]].abs().max()) > 0 and torch.equal(got[:, 0].cpu(), got[:, 66].cpu())      # empty rows: relu(bias)


@pytest.mark.parametrize('F', SPARSE_WIDTHS)
def test_csr_spmm_thick(dev, pats, F):
    """thick(67): the row last in order[], the one the surplus groups of k_csr_spmm_g shadow, has 33 entries (three chunks at G = 16)."""
    pt = pats['thick67']
    csr = pt.csr
    val, x = uniform(44 + F, csr.nnz), uniform(45 + F, S, csr.n_cols, F)
    xd = nan_in(torch.from_numpy(x), dev)
    for what, v in (('val', val), ('val=None', None)):
        out = Guarded((S, csr.n_rows, F), dev)
        got = _lib.csr_spmm(pt.h, None if v is None else nan_in(torch.from_numpy(v), dev), xd, out=out.view)
        assert got is out.view
        torch.cuda.synchronize()
        out.check('out')
        ref = OS.incidence_aggregate_csr(torch.from_numpy(x), csr.rowptr, csr.col, np.ones(csr.nnz) if v is None else v, csr.n_rows)
        check('spmm thick67 F%d %s' % (F, what), got, ref, TOL)


@pytest.mark.parametrize('n_snap', [1, 3])
@pytest.mark.parametrize('which', ['rect', 'ladder67'])
@pytest.mark.parametrize('F', SPARSE_WIDTHS)
def test_csr_sddmm(dev, rect, pats, F, which, n_snap):
    csr, h = (rect[0], rect[1]) if which == 'rect' else (pats['ladder67'].csr, pats['ladder67'].h)
    a, b = uniform(50 + F + n_snap, n_snap, csr.n_rows, F), uniform(51 + F + n_snap, n_snap, csr.n_cols, F)
    ref = np.einsum('skf,skf->k', a[:, csr.rows()], b[:, csr.col.astype(np.int64)])
    assert np.abs(ref).max() > 0.05
    out = Guarded((csr.nnz,), dev)
    got = _lib.csr_sddmm(h, nan_in(torch.from_numpy(a), dev), nan_in(torch.from_numpy(b), dev), out=out.view)
    assert got is out.view
    torch.cuda.synchronize()
    out.check('out')
    check('sddmm %s F%d S%d' % (which, F, n_snap), got, ref, TOL)


# ---- (g) snapshot independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LADDERS)
@pytest.mark.parametrize('d', SUBSET_WIDTHS)
def test_snapshots_are_independent(dev, pats, rect, d, name):
    """The S = 3 result is the three S = 1 results stacked, bit for bit: a wrong per-snapshot stride of any operand shows."""
    pt = pats[name]
    _, dv = pt.operands(d, dev)
    one = lambda t, s: nan_in(t[s:s + 1], dev)
    kw = ex_args(pt, 'both')
    full_f = _lib.gat_aggregate_ex(pt.h, dv['hx'], pt.d_ss, pt.d_sn, dv['bias'], 'relu', **kw)
    full_b = _lib.gat_backward_ex(pt.h, pt.ht, pt.perm, dv['grad'], dv['hx'], pt.d_ss, pt.d_sn, dv['a_self'], dv['a_nbr'], **kw)
    for s in range(S):
        kws = dict(edge_mask=one(pt.d_mask, s), coef=one(pt.d_coef, s))
        hx, ss, sn = one(dv['hx'], s), one(pt.d_ss, s), one(pt.d_sn, s)
        assert torch.equal(_lib.gat_aggregate_ex(pt.h, hx, ss, sn, dv['bias'], 'relu', **kws)[0], full_f[s]), s
        part = _lib.gat_backward_ex(pt.h, pt.ht, pt.perm, one(dv['grad'], s), hx, ss, sn, dv['a_self'], dv['a_nbr'], **kws)
        for p_, f_ in zip(part, full_b):
            assert torch.equal(p_[0], f_[s]), s
    csr, h, val = rect
    x = nan_in(torch.from_numpy(uniform(60 + d, S, csr.n_cols, d)), dev)
    full = _lib.csr_spmm(h, val, x, dv['bias'], 'relu')
    for s in range(S):
        assert torch.equal(_lib.csr_spmm(h, val, one(x, s), dv['bias'], 'relu')[0], full[s]), s


# ---- (h) repeatability --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LADDERS)
@pytest.mark.parametrize('d', SUBSET_WIDTHS)
def test_backward_repeats_bitwise(dev, pats, d, name):
    pt = pats[name]
    _, dv = pt.operands(d, dev)
    runs = [lambda: backward(_lib.gat_backward, pt, dv, dev), lambda: backward(_lib.gat_backward, pt, dv, dev, coef=pt.d_coef),
            lambda: backward(_lib.gat_backward_ex, pt, dv, dev, **ex_args(pt, 'both')),
            lambda: (_lib.csr_sddmm(pt.h, dv['grad'], dv['hx']),)]
    for run in runs:
        first, second = run(), run()
        for x, y in zip(first, second):
            assert torch.equal(x, y)
