"""fp64 parity of the multi-head GAT entries, uds_gat_aggregate_heads and uds_gat_backward_heads, called directly.  S = 3 on the
degree-ladder patterns of tests/util.py (ladder(128), ladder(67); thick(67) forward only, as tests/test_gpu_sparse_widths.py).
Reference: tests.heads_util.heads_ref (oracle.gat_csr_ref once per head; pinned on the CPU by tests/test_gat_heads_math.py).

(H, C) and what each reaches (group_shape of kernels_sparse.hpp on C / 4; one lane group per (row, head), per row for the mean):
  (1, 64)   bitwise against uds_gat_aggregate_ex / uds_gat_backward_ex        (8, 8)    k_*_hg<2, 1>
  (4, 16)   <4, 1>              (2, 32)  <8, 1>              (3, 32)  <8, 1>, odd head count        (2, 64)  <16, 1>
  (2, 128)  <16, 2>             (16, 4)  the walking kernels, one lane per item   (3, 12)  the walking kernels, odd heads
Each case runs plain, mask, coef and both, with the heads concatenated and averaged, with and without alpha_out.
Scores: tests.util.ladder_scores with seed h for head h (every head keeps its overflow snapshot); mask tests.util.ladder_mask,
shared by the heads; coef (3, H, nnz) = _lib.dropout(ones, 0.5, 23, 0), restated on the CPU by oracle.dropout_ref.

Every input is a view inside a NaN-filled allocation, every output and the NaN-pre-filled alpha / de workspace a view inside a
sentinel-filled one (tests.util.Guarded), checked on both sides and for finiteness.  Plain allocations: nothing here is meant
to fault.

Tolerances, relative to max(1, max|ref|) through tests.util.close, are those of tests/test_gpu_sparse_widths.py: forward 5e-6,
backward outputs 1e-5, alpha_out 5e-6.

MEASURED on an MI355X (UDS_TOL_REPORT=1), worst observed / allowed per test over all its cases [case]:
  test_aggregate_heads         0.095  [16-4-ladder128-coef]
  test_backward_heads          0.047  [2-128-ladder67-mask]
The remaining tests are bitwise comparisons or refusals.  No bound was raised.
"""
import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from oracle.gat_csr_ref import act_fn
from tests.heads_util import HEAD_CASES, HEADS_COEF_SEED, VARIANTS, heads_case
from tests.util import Guarded, close, ladder, nan_in, thick

pytestmark = pytest.mark.gpu

TOL = 5e-6
TOL_BWD = 1e-5
TOL_ALPHA = 5e-6
S = 3
LADDERS = ['ladder128', 'ladder67']
SQUARE = LADDERS + ['thick67']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


class Pattern:
    def __init__(self, csr, dev, backward):
        self.csr, self.n, self.backward = csr, csr.n_rows, backward
        self.h = _lib.CsrHandle(csr)
        self.ht, self.perm = self.h.transposed(dev)
        self.cases = {}

    def case(self, H, C, concat, variant, dev):
        """Host case (operands, scores, mask, coef, fp64 reference) and its NaN-padded device tensors, computed once."""
        key = (H, C, concat, variant)
        if key not in self.cases:
            c = heads_case(self.csr, H, C, concat, variant, backward=self.backward)
            f = lambda a: None if a is None else nan_in(torch.from_numpy(a), dev)
            dv = {k: f(v) for k, v in c['op'].items()}
            dv.update(ss=f(c['ss']), sn=f(c['sn']), mask=f(c['mask']), coef=f(c['coef']))
            if c['coef'] is not None:      # the device draws the same multiplier
                drawn = _lib.dropout(torch.ones((S, H, self.csr.nnz), device=dev), 0.5, HEADS_COEF_SEED, 0)
                assert (drawn.double().cpu().numpy() == c['coef']).all()
            self.cases[key] = (c, dv)
        return self.cases[key]


@pytest.fixture(scope='module')
def pats(dev):
    return {'ladder128': Pattern(ladder(128), dev, True), 'ladder67': Pattern(ladder(67), dev, True), 'thick67': Pattern(thick(67), dev, False)}


def check(what, got, ref, tol):
    ref = torch.from_numpy(np.ascontiguousarray(ref)) if isinstance(ref, np.ndarray) else ref
    err = close(got, ref, tol, _depth=2)
    print('%-76s err %.3e  ratio %.3f' % (what, err, err / (tol * max(1.0, float(ref.abs().max())))))
    return err


def forward(pt, dv, dev, concat, bias, act, with_alpha):
    """One guarded aggregation call: (out, alpha or None), both checked on both sides and for finiteness."""
    H = dv['ss'].shape[-1]
    width = dv['hx'].shape[-1] if concat else dv['hx'].shape[-1] // H
    out = Guarded((S, pt.n, width), dev)
    alpha = Guarded((S, H, pt.csr.nnz), dev, torch.full((S, H, pt.csr.nnz), float('nan'))) if with_alpha else None
    got = _lib.gat_aggregate_heads(pt.h, dv['hx'], dv['ss'], dv['sn'], dv['bias'] if bias else None, act, concat=concat,
                                   edge_mask=dv['mask'], coef=dv['coef'], out=out.view, alpha_out=alpha.view if with_alpha else None)
    torch.cuda.synchronize()
    out.check('out')
    if not with_alpha:
        assert got is out.view
        return got, None
    assert got[0] is out.view and got[1] is alpha.view
    alpha.check('alpha_out (an entry that was not written?)')
    return got


def backward(pt, dv, dev, concat):
    """One guarded backward call: (d_hx, ds_self, ds_nbr), the outputs and the NaN-pre-filled workspace checked."""
    H = dv['ss'].shape[-1]
    outs = [Guarded((S, pt.n, dv['hx'].shape[-1]), dev), Guarded((S, pt.n, H), dev), Guarded((S, pt.n, H), dev)]
    ws = Guarded((2, S, H, pt.csr.nnz), dev, torch.full((2, S, H, pt.csr.nnz), float('nan')))
    got = _lib.gat_backward_heads(pt.h, pt.ht, pt.perm, dv['grad'], dv['hx'], dv['ss'], dv['sn'], dv['a_self'], dv['a_nbr'], concat=concat,
                                  edge_mask=dv['mask'], coef=dv['coef'], out=tuple(o.view for o in outs), workspace=ws.view)
    torch.cuda.synchronize()
    for o, g, name in zip(outs, got, ('d_hx', 'ds_self', 'ds_nbr')):
        assert g is o.view
        o.check(name)
    ws.check('alpha / de workspace (an entry the row pass did not write?)')
    return got


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', SQUARE)
@pytest.mark.parametrize('H,C', HEAD_CASES)
def test_aggregate_heads(dev, pats, H, C, name, variant):
    pt = pats[name]
    for concat in (True, False):
        c, dv = pt.case(H, C, concat, variant, dev)
        what = 'aggregate_heads %s H%d C%d %s %s' % (name, H, C, variant, 'concat' if concat else 'mean')
        outs = []
        for act, bias, with_alpha in (('relu', True, True), ('relu', True, False), ('linear', False, True)):
            got, alpha = forward(pt, dv, dev, concat, bias, act, with_alpha)
            check('%s %s' % (what, act), got, act_fn(c['ref']['pre'] + (c['op']['bias'] if bias else 0.0), act), TOL)
            if with_alpha:
                check('%s %s alpha_out' % (what, act), alpha, c['ref']['alpha_coef'], TOL_ALPHA)
                if c['mask'] is not None:      # a masked entry is written as exactly 0
                    assert bool((alpha.cpu()[torch.from_numpy(c['ref']['alpha_coef'] == 0)] == 0).all())
            outs.append(got.clone())
        assert torch.equal(outs[0], outs[1])      # asking for the coefficients does not change the aggregation


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', LADDERS)
@pytest.mark.parametrize('H,C', HEAD_CASES)
def test_backward_heads(dev, pats, H, C, name, variant):
    pt = pats[name]
    for concat in (True, False):
        c, dv = pt.case(H, C, concat, variant, dev)
        got = backward(pt, dv, dev, concat)
        for g, key in zip(got, ('d_hx', 'ds_self', 'ds_nbr')):
            check('backward_heads %s H%d C%d %s %s %s' % (name, H, C, variant, 'concat' if concat else 'mean', key), g, c['ref'][key], TOL_BWD)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', SQUARE)
def test_one_head_is_bitwise_the_single_head_entries(dev, pats, name, variant):
    """H = 1 with concatenation: bitwise uds_gat_aggregate_ex / uds_gat_backward_ex."""
    pt = pats[name]
    _, dv = pt.case(1, 64, True, variant, dev)
    ss, sn = nan_in(dv['ss'][..., 0], dev), nan_in(dv['sn'][..., 0], dev)
    coef = None if dv['coef'] is None else nan_in(dv['coef'][:, 0], dev)
    for act, bias in (('relu', dv['bias']), ('linear', None)):
        one = _lib.gat_aggregate_ex(pt.h, dv['hx'], ss, sn, bias, act, edge_mask=dv['mask'], coef=coef)
        got = _lib.gat_aggregate_heads(pt.h, dv['hx'], dv['ss'], dv['sn'], bias, act, edge_mask=dv['mask'], coef=dv['coef'])
        assert torch.equal(got, one), act
    if name in LADDERS:
        one = _lib.gat_backward_ex(pt.h, pt.ht, pt.perm, dv['grad'], dv['hx'], ss, sn, dv['a_self'], dv['a_nbr'], edge_mask=dv['mask'], coef=coef)
        got = backward(pt, dv, dev, True)
        for g, o, key in zip(got, one, ('d_hx', 'ds_self', 'ds_nbr')):
            assert torch.equal(g.reshape(o.shape), o), key


@pytest.mark.parametrize('name', LADDERS)
@pytest.mark.parametrize('H,C', [(3, 32), (2, 128), (3, 12)])
def test_backward_repeats_bitwise_and_snapshots_are_independent(dev, pats, H, C, name):
    """The backward run twice is equal bit for bit (no atomics), and the S = 3 results are the three S = 1 results stacked: a
    wrong per-snapshot or per-head stride of any operand shows."""
    pt = pats[name]
    for concat in (True, False):
        _, dv = pt.case(H, C, concat, 'both', dev)
        first, second = backward(pt, dv, dev, concat), backward(pt, dv, dev, concat)
        for x, y in zip(first, second):
            assert torch.equal(x, y)
        full_f, full_a = forward(pt, dv, dev, concat, True, 'relu', True)
        one = lambda t, s: nan_in(t[s:s + 1], dev)
        for s in range(S):
            kw = dict(concat=concat, edge_mask=one(dv['mask'], s), coef=one(dv['coef'], s))
            hx, ss, sn = one(dv['hx'], s), one(dv['ss'], s), one(dv['sn'], s)
            out, alpha = _lib.gat_aggregate_heads(pt.h, hx, ss, sn, dv['bias'], 'relu', alpha_out=True, **kw)
            assert torch.equal(out[0], full_f[s]) and torch.equal(alpha[0], full_a[s]), s
            part = _lib.gat_backward_heads(pt.h, pt.ht, pt.perm, one(dv['grad'], s), hx, ss, sn, dv['a_self'], dv['a_nbr'], **kw)
            for p_, f_ in zip(part, first):
                assert torch.equal(p_[0], f_[s]), s


def test_refusals(dev, pats):
    pt = pats['ladder67']
    n, nnz = pt.n, pt.csr.nnz
    z = lambda *shape: torch.zeros(shape, device=dev)
    with pytest.raises(_lib.UdsError, match='multiple of 4'):                       # C = 6
        _lib.gat_aggregate_heads(pt.h, z(S, n, 12), z(S, n, 2), z(S, n, 2))
    with pytest.raises(_lib.UdsError, match='multiple of 4'):
        _lib.gat_backward_heads(pt.h, pt.ht, pt.perm, z(S, n, 12), z(S, n, 12), z(S, n, 2), z(S, n, 2), z(12), z(12))
    hx, ss = z(S, n, 16), z(S, n, 2)
    with pytest.raises(_lib.UdsError, match='coef'):                                # coef without its head axis
        _lib.gat_aggregate_heads(pt.h, hx, ss, ss, coef=z(S, nnz))
    with pytest.raises(_lib.UdsError, match='coef'):
        _lib.gat_aggregate_heads(pt.h, hx, ss, ss, coef=z(S, 3, nnz))
    with pytest.raises(_lib.UdsError, match='edge_mask'):                           # a mask per head
        _lib.gat_aggregate_heads(pt.h, hx, ss, ss, edge_mask=z(S, 2, nnz))
    with pytest.raises(_lib.UdsError, match='edge_mask'):
        _lib.gat_backward_heads(pt.h, pt.ht, pt.perm, hx, hx, ss, ss, z(16), z(16), edge_mask=z(S, nnz + 1))
    with pytest.raises(_lib.UdsError, match='coef'):
        _lib.gat_backward_heads(pt.h, pt.ht, pt.perm, hx, hx, ss, ss, z(16), z(16), coef=z(2, 2, nnz))
    with pytest.raises(_lib.UdsError, match='grad'):                                # the mean takes a (S, n, C) gradient
        _lib.gat_backward_heads(pt.h, pt.ht, pt.perm, hx, hx, ss, ss, z(16), z(16), concat=False)
    with pytest.raises(_lib.UdsError, match='bias'):
        _lib.gat_aggregate_heads(pt.h, hx, ss, ss, z(16), concat=False)
