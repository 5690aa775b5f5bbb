"""Argument checks of the C entries that sit behind a pattern handle: the single-head and multi-head GAT entries, the four
Diffusion entries and the two one-launch halo entries of the backward exchange (tests/test_entry_checks.py has the rest).

No case launches a kernel: a bad call returns UDS_EINVAL (-22) with its message, S == 0 and a pattern without rows return
UDS_OK and write nothing.  The operands are real device tensors, large enough for the sizes asked, so that a check that wrongly
passed would run on valid memory.  Some messages name a sibling on purpose (uds_gat_backward_coef says uds_gat_backward).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib

pytestmark = pytest.mark.gpu
EINVAL = -22
SENTINEL = -7.5
FLOATS = 8 << 20        # per buffer: S = 65536 snapshots of 5 rows of 16 floats fit


def _pattern(n_rows, n_cols, cols_of_row):
    rowptr = np.cumsum([0] + [len(c) for c in cols_of_row]).astype(np.int32)
    col = np.array([j for c in cols_of_row for j in c], dtype=np.int32)
    return SimpleNamespace(n_rows=n_rows, n_cols=n_cols, nnz=int(col.size), rowptr=rowptr, col=col)


@pytest.fixture(scope='module')
def ctx():
    assert torch.cuda.is_available()
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    c = SimpleNamespace(lib=lib)
    c.sq = _lib.CsrHandle(_pattern(5, 5, [[i, (i + 1) % 5] for i in range(5)]))          # square, self loops
    c.rect = _lib.CsrHandle(_pattern(4, 5, [[i, i + 1] for i in range(4)]))               # 4 x 5
    c.none = _lib.CsrHandle(_pattern(0, 0, []))                                           # no rows
    c.sq_t, c.perm = c.sq.transposed(dev)
    c.rect_t, c.rect_perm = c.rect.transposed(dev)
    c.inp = torch.zeros(FLOATS, device=dev)
    c.out = torch.full((FLOATS,), SENTINEL, device=dev)
    c.dtheta = torch.full((64,), SENTINEL, device=dev)
    c.idx = torch.tensor([0, 1, 2, 3, 0, 0, 0, 0], dtype=torch.int32, device=dev)        # rows / offsets [0, 1, 2, 3]
    c.I, c.O, c.N, c.T = c.inp.data_ptr(), c.out.data_ptr(), c.idx.data_ptr(), c.dtheta.data_ptr()
    assert c.I % 16 == 0 and c.O % 16 == 0
    return c


def _good(c):
    """entry -> (argument names in ABI order, a call that passes every check) on the 5-row square pattern (Diffusion: 4 x 5)."""
    I, O, N = c.I, c.O, c.N
    g, gt, perm = c.sq.ptr, c.sq_t.ptr, c.perm.data_ptr()
    agg = dict(g=g, hx=I, s_self=I, s_nbr=I, bias=None, S=2, d=8, act=1, out=O)
    bwd = dict(g=g, gt=gt, perm_t=perm, grad=I, hx=I, s_self=I, s_nbr=I, a_self=I, a_nbr=I, S=2, d=8, alpha_ws=O, de_ws=O, d_hx=O, ds_self=O,
               ds_nbr=O)
    dif = dict(csr=c.rect.ptr, csr_t=c.rect_t.ptr, perm_t=c.rect_perm.data_ptr(), a=I, r=I, tot=I, y=I, gy=I, S=2, C=8, K1=3, act=2, workspace=O,
               dr=O, dtheta=c.T)
    halo = dict(x=O, n_x=9, e=O, n_e=7, S=2, F=8, off_x=N, off_e=N, P=1)
    return {
        'uds_gat_forward': ('g xa fa xb fb S W a_self a_nbr bias d act ws out',
                            dict(g=g, xa=I, fa=4, xb=None, fb=0, S=2, W=I, a_self=I, a_nbr=I, bias=None, d=8, act=1, ws=O, out=O)),
        'uds_gat_aggregate': ('g hx s_self s_nbr bias S d act out', agg),
        'uds_gat_aggregate_coef': ('g hx s_self s_nbr bias coef S d act out', dict(agg, coef=I)),
        'uds_gat_aggregate_masked': ('g hx s_self s_nbr bias edge_mask S d act out', dict(agg, edge_mask=I)),
        'uds_gat_aggregate_ex': ('g hx s_self s_nbr bias edge_mask coef S d act out', dict(agg, edge_mask=I, coef=None)),
        'uds_gat_backward': ('g gt perm_t grad hx s_self s_nbr a_self a_nbr S d alpha_ws de_ws d_hx ds_self ds_nbr', bwd),
        'uds_gat_backward_coef': ('g gt perm_t grad hx s_self s_nbr a_self a_nbr coef S d alpha_ws de_ws d_hx ds_self ds_nbr', dict(bwd, coef=I)),
        'uds_gat_backward_ex': ('g gt perm_t grad hx s_self s_nbr a_self a_nbr edge_mask coef S d alpha_ws de_ws d_hx ds_self ds_nbr',
                                dict(bwd, edge_mask=I, coef=None)),
        'uds_gat_aggregate_heads': ('g hx s_self s_nbr bias edge_mask coef S H d concat act out alpha_out',
                                    dict(agg, edge_mask=None, coef=None, H=2, concat=1, alpha_out=None)),
        'uds_gat_backward_heads': ('g gt perm_t grad hx s_self s_nbr a_self a_nbr edge_mask coef S H d concat alpha_ws de_ws d_hx ds_self ds_nbr',
                                   dict(bwd, edge_mask=None, coef=None, H=2, concat=1)),
        'uds_diffusion_forward': ('csr vals c0 r tot S C act out', dict(csr=c.rect.ptr, vals=I, c0=I, r=I, tot=I, S=2, C=8, act=2, out=O)),
        'uds_diffusion_backward': ('csr csr_t perm_t a vals c0 r tot y gy S C K1 act workspace dr dtheta', dict(dif, vals=I, c0=I)),
        'uds_diffusion_forward_m': ('csr a theta r tot S C K1 act out', dict(csr=c.rect.ptr, a=I, theta=I, r=I, tot=I, S=2, C=8, K1=3, act=2, out=O)),
        'uds_diffusion_backward_m': ('csr csr_t perm_t a theta r tot y gy S C K1 act workspace dr dtheta', dict(dif, theta=I)),
        'uds_halo_pack_clear_all': ('x n_x e n_e S F idx_x nx idx_e ne off_x off_e P buf', dict(halo, idx_x=N, nx=1, idx_e=N, ne=2, buf=O)),
        'uds_halo_accumulate_all': ('buf S F off_x off_e P tgt_x tx tgt_e te ptr src n_src x n_x e n_e',
                                    dict(halo, buf=I, tgt_x=N, tx=1, tgt_e=N, te=2, ptr=N, src=N, n_src=3)),
    }


AGG1 = ('uds_gat_aggregate', 'uds_gat_aggregate_coef', 'uds_gat_aggregate_masked', 'uds_gat_aggregate_ex')
AGG = AGG1 + ('uds_gat_aggregate_heads',)
BWD1 = ('uds_gat_backward', 'uds_gat_backward_coef', 'uds_gat_backward_ex')
BWD = BWD1 + ('uds_gat_backward_heads',)
HEADS = ('uds_gat_aggregate_heads', 'uds_gat_backward_heads')
DIFF_M = ('uds_diffusion_backward', 'uds_diffusion_forward_m', 'uds_diffusion_backward_m')
DIFF_BWD = ('uds_diffusion_backward', 'uds_diffusion_backward_m')
DIFF = ('uds_diffusion_forward',) + DIFF_M
HALO = ('uds_halo_pack_clear_all', 'uds_halo_accumulate_all')
NAMED = {'uds_gat_backward_coef': 'uds_gat_backward'}      # the entry whose name the messages carry
WIDTH = {e: 'C' if e in HEADS else 'd' for e in AGG + BWD}


def _named(e):
    return NAMED.get(e, e)


def _bad_cases():
    """(entry, changed arguments -- a string names a ctx attribute, 'O+4' the output buffer off by 4 bytes --, message)"""
    cases = []
    for e in AGG + ('uds_gat_forward',):
        cases.append((e, dict(g='rect'), _named(e) + ': pattern must be square' + (' (4 x 5)' if e == 'uds_gat_forward' else '')))
    for e in BWD:
        cases += [(e, dict(g='rect'), _named(e) + ': the pattern and its transpose must be square with the same shape and entry count'),
                  (e, dict(gt='rect_t'), _named(e) + ': the pattern and its transpose must be square with the same shape and entry count'),
                  (e, dict(d_hx='O+4'), _named(e) + ': grad/hx/d_hx/a_self/a_nbr must be 16-byte aligned')]
    for e in AGG + BWD + ('uds_gat_forward',):
        cases += [(e, dict(d=6), '%s: %s=6 must be a multiple of 4, at most 256' % (_named(e), WIDTH.get(e, 'd'))),
                  (e, dict(S=65536), _named(e) + ': S=65536 outside [0,65535]')]
    for e in AGG:
        cases += [(e, dict(act=9), e + ': unknown activation 9'), (e, dict(out='O+4'), e + ': hx/out/bias must be 16-byte aligned')]
    cases.append(('uds_gat_forward', dict(out='O+4'), 'uds_gat_forward: workspace/out/bias must be 16-byte aligned'))
    for e in HEADS:
        cases.append((e, dict(H=65), e + ': H=65 outside [1,64]'))
    cases += [('uds_diffusion_forward', dict(C=6), 'uds_diffusion_forward: S=2 C=6 (needs S <= 65535, C % 4 == 0)'),
              ('uds_diffusion_forward', dict(S=65536), 'uds_diffusion_forward: S=65536 C=8 (needs S <= 65535, C % 4 == 0)'),
              ('uds_diffusion_forward', dict(out='O+4'), 'uds_diffusion_forward: vals / c0 / out must be 16-byte aligned'),
              ('uds_diffusion_forward_m', dict(out='O+4'), 'uds_diffusion_forward_m: theta / out must be 16-byte aligned'),
              ('uds_diffusion_backward', dict(workspace='O+4'), 'uds_diffusion_backward: vals / c0 / y / gy / workspace must be 16-byte aligned'),
              ('uds_diffusion_backward_m', dict(workspace='O+4'), 'uds_diffusion_backward_m: theta / y / gy / workspace must be 16-byte aligned')]
    for e in DIFF_M:
        cases += [(e, dict(C=6), e + ': S=2 C=6 K1=3 (needs S <= 65535, C % 4 == 0, C <= 256, 1 <= K1 <= 16)'),
                  (e, dict(S=65536), e + ': S=65536 C=8 K1=3 (needs'), (e, dict(K1=17), e + ': S=2 C=8 K1=17 (needs')]
    for e in DIFF:
        cases.append((e, dict(act=9), e + ': unknown activation 9'))
    for e in DIFF_BWD:
        cases.append((e, dict(csr_t='sq'), e + ': csr_t (5 x 5, 10 entries) is not the transpose of a 4 x 5 pattern with 8 entries'))
    cases += [('uds_halo_pack_clear_all', dict(S=65536), 'uds_halo_pack_clear_all: bad sizes (S=65536 nx=1 ne=2 F=8 P=1; needs S <= 65535, F >= 1, P >= 1)'),
              ('uds_halo_pack_clear_all', dict(off_e=None), 'uds_halo_pack_clear_all: NULL argument'),
              ('uds_halo_pack_clear_all', dict(nx=1 << 31), 'uds_halo_pack_clear_all: messages too large'),
              ('uds_halo_accumulate_all', dict(S=65536),
               'uds_halo_accumulate_all: bad sizes (S=65536 tx=1 te=2 n_src=3 F=8 P=1; needs S <= 65535, F >= 1, P >= 1)'),
              ('uds_halo_accumulate_all', dict(ptr=None), 'uds_halo_accumulate_all: NULL argument'),
              ('uds_halo_accumulate_all', dict(tx=1 << 31), 'uds_halo_accumulate_all: too many rows')]
    return cases


BAD = _bad_cases()


def _call(c, entry, changes):
    names, good = _good(c)[entry]
    names = names.split()
    assert set(names) == set(good) and set(changes) <= set(good), entry
    args = dict(good)
    for k, v in changes.items():
        args[k] = c.O + 4 if v == 'O+4' else getattr(c, v).ptr if isinstance(v, str) else v
    rc = getattr(c.lib, entry)(*[args[n] for n in names], torch.cuda.current_stream().cuda_stream)
    return rc, c.lib.uds_last_error().decode()


@pytest.mark.parametrize('case', BAD, ids=['%s-%s' % (e, '-'.join('%s=%s' % kv for kv in ch.items())) for e, ch, _ in BAD])
def test_bad_argument_is_refused_with_its_message(ctx, case):
    entry, changes, text = case
    rc, msg = _call(ctx, entry, changes)
    assert rc == EINVAL and msg.startswith(text), (rc, msg)


def test_every_entry_behind_a_handle_is_in_the_table(ctx):
    assert {e for e, _, _ in BAD} == set(_good(ctx)) == set(AGG + BWD + DIFF + HALO + ('uds_gat_forward',))


def test_nothing_to_do_returns_ok_and_writes_nothing(ctx):
    c = ctx
    for e in AGG + BWD + ('uds_gat_forward',):
        assert _call(c, e, dict(S=0))[0] == 0, e
        assert _call(c, e, dict(g='none', gt='none') if e in BWD else dict(g='none'))[0] == 0, e
    for e in ('uds_diffusion_forward', 'uds_diffusion_forward_m'):
        assert _call(c, e, dict(S=0))[0] == 0 and _call(c, e, dict(csr='none'))[0] == 0, e
    assert _call(c, 'uds_halo_pack_clear_all', dict(S=0))[0] == 0 and _call(c, 'uds_halo_pack_clear_all', dict(nx=0, ne=0))[0] == 0
    assert _call(c, 'uds_halo_accumulate_all', dict(S=0))[0] == 0 and _call(c, 'uds_halo_accumulate_all', dict(tx=0, te=0))[0] == 0
    torch.cuda.synchronize()
    assert bool((c.dtheta == SENTINEL).all())
    # the Diffusion backward entries without a snapshot: no dr, and dtheta (C, K1) = 0 by a memset, not a kernel
    for e in DIFF_BWD:
        c.dtheta.fill_(SENTINEL)
        assert _call(c, e, dict(S=0))[0] == 0, e
        torch.cuda.synchronize()
        assert bool((c.dtheta[:24] == 0).all()) and bool((c.dtheta[24:] == SENTINEL).all()), e
    assert bool((c.out == SENTINEL).all()) and bool((c.inp == 0).all())
