"""Argument checks of the C entries that need no device: return code and uds_last_error() text, entry by entry.

Every entry returns UDS_EINVAL (-22) before it touches a device, so the table below runs on a CPU-only machine: the operands
are one aligned host address (never read).  Siblings of one family -- entries that share their checks -- get the same bad
argument each, so a forward that drops an argument or swaps two shows up as a wrong message or as the wrong numbers in it.
Some messages name a sibling on purpose (the entry that owns the checks); they are pinned as they are.
"""
import ctypes

import numpy as np
import pytest

from gnn_uds_amd import _lib

_BUF = np.zeros(64, dtype=np.float32)
P = _BUF.ctypes.data - _BUF.ctypes.data % 16 + 16       # a 16-byte aligned address
Q = P + 4                                               # misaligned by one float
EINVAL = -22

_HEADS = _lib._Heads()
_HEADS.a_packed, _HEADS.n_a = P, 1
_HEADS5 = _lib._Heads()
_HEADS5.a_packed, _HEADS5.n_a = P, 5

# entry -> (argument names in ABI order, a call that passes every check)
GOOD = {
    'uds_dense_act': ('xa fa xb fb rows W bias f_out act a_self a_nbr out s_self s_nbr',
                      dict(xa=P, fa=8, xb=None, fb=0, rows=3, W=P, bias=None, f_out=8, act=0, a_self=None, a_nbr=None, out=P, s_self=None,
                           s_nbr=None)),
    'uds_dense_route': ('fa fb taps attn f_out rows wb_aligned info5', dict(fa=8, fb=0, taps=0, attn=0, f_out=8, rows=3, wb_aligned=1, info5=P)),
    'uds_conv1d_causal': ('x B T R F kernel bias taps dil H act out', dict(x=P, B=2, T=3, R=5, F=8, kernel=P, bias=None, taps=2, dil=1, H=16, act=0, out=P)),
    'uds_recurrent_fused': ('x F packed b_in b_rec B T R kind out', dict(x=P, F=64, packed=P, b_in=P, b_rec=P, B=2, T=3, R=5, kind=0, out=P)),
    'uds_recurrent_forward': ('xp U rb B T R H kind out', dict(xp=P, U=P, rb=None, B=2, T=3, R=5, H=32, kind=0, out=P)),
    'uds_recurrent_forward_train': ('xp U rb B T R H kind out c_out', dict(xp=P, U=P, rb=None, B=2, T=3, R=5, H=32, kind=0, out=P, c_out=None)),
    'uds_recurrent_backward': ('xp packed b_rec h c gh B T R kind dxp darec',
                               dict(xp=P, packed=P, b_rec=None, h=P, c=None, gh=P, B=2, T=3, R=5, kind=0, dxp=P, darec=P)),
    'uds_recurrent_backward_h': ('xp packed b_rec h c gh B T R H kind dxp darec',
                                 dict(xp=P, packed=P, b_rec=None, h=P, c=None, gh=P, B=2, T=3, R=5, H=32, kind=0, dxp=P, darec=P)),
    'uds_recurrent_pack_bwd': ('U H kind packed', dict(U=P, H=32, kind=0, packed=P)),
    'uds_rowgemm_pack': ('W k_total f_out packed', dict(W=P, k_total=32, f_out=16, packed=P)),
    'uds_remainder_pack': ('rest R M packed', dict(rest=P, R=8, M=7, packed=P)),
    'uds_remainder_forward': ('packed R M x S h workspace out', dict(packed=P, R=8, M=7, x=P, S=2, h=32, workspace=P, out=P)),
    'uds_remainder_forward_dense': ('packed R M e F packed_w bias act S h workspace out',
                                    dict(packed=P, R=8, M=7, e=P, F=64, packed_w=P, bias=None, act=0, S=2, h=32, workspace=P, out=P)),
    'uds_rowgemm_forward': ('x B T R F packed bias taps dil f_out act out',
                            dict(x=P, B=2, T=3, R=5, F=32, packed=P, bias=None, taps=1, dil=1, f_out=16, act=0, out=P)),
    'uds_rowgemm_forward_cat': ('x F1 x2 F2 B T R packed bias taps dil f_out act out ldo col0',
                                dict(x=P, F1=32, x2=None, F2=0, B=2, T=3, R=5, packed=P, bias=None, taps=1, dil=1, f_out=16, act=0, out=P, ldo=16,
                                     col0=0)),
    'uds_rowgemm_forward_pair': ('x0 R0 packed0 bias0 out0 x1 R1 packed1 bias1 out1 B T F taps dil f_out act',
                                 dict(x0=P, R0=5, packed0=P, bias0=None, out0=P, x1=P, R1=7, packed1=P, bias1=None, out1=P, B=2, T=3, F=32, taps=1,
                                      dil=1, f_out=16, act=0)),
    'uds_dense_cumsum': ('x B T R packed bias res act out', dict(x=P, B=2, T=3, R=5, packed=P, bias=None, res=None, act=0, out=P)),
    'uds_dense_cumsum_heads': ('x B T R packed bias res act heads out',
                               dict(x=P, B=2, T=3, R=5, packed=P, bias=None, res=None, act=0, heads=ctypes.addressof(_HEADS), out=P)),
    'uds_cumsum_act': ('x res B T R F act out', dict(x=P, res=None, B=2, T=3, R=5, F=8, act=0, out=P)),
    'uds_attn_sum_pool': ('x k B R F out', dict(x=P, k=P, B=2, R=5, F=8, out=P)),
    'uds_attn_sum_pool_pair': ('x Rx e Re k B F out stat', dict(x=P, Rx=5, e=P, Re=3, k=P, B=2, F=8, out=P, stat=None)),
    'uds_attn_sum_pool_backward': ('x Rx e Re k out stat grad B F dx de dk_ws dk',
                                   dict(x=P, Rx=5, e=P, Re=3, k=P, out=P, stat=P, grad=P, B=2, F=8, dx=P, de=P, dk_ws=P, dk=P)),
    'uds_dropout': ('x n rate seed offset out', dict(x=P, n=10, rate=0.5, seed=1, offset=0, out=P)),
    'uds_wgrad': ('a g B T R F H shift with_bias workspace d_kernel d_bias',
                  dict(a=P, g=P, B=2, T=3, R=5, F=8, H=16, shift=0, with_bias=1, workspace=P, d_kernel=P, d_bias=P)),
    'uds_halo_pack': ('x n_x e n_e S F idx_x nx idx_e ne buf', dict(x=P, n_x=9, e=P, n_e=7, S=2, F=8, idx_x=P, nx=1, idx_e=P, ne=3, buf=P)),
    'uds_halo_unpack': ('buf S F idx_x nx idx_e ne x n_x e n_e', dict(buf=P, S=2, F=8, idx_x=P, nx=1, idx_e=P, ne=3, x=P, n_x=9, e=P, n_e=7)),
    'uds_halo_pack_all': ('x n_x e n_e S F idx_x nx idx_e ne off_x off_e P buf',
                          dict(x=P, n_x=9, e=P, n_e=7, S=2, F=8, idx_x=P, nx=1, idx_e=P, ne=3, off_x=P, off_e=P, P=4, buf=P)),
    'uds_halo_unpack_all': ('buf S F idx_x nx idx_e ne off_x off_e P x n_x e n_e',
                            dict(buf=P, S=2, F=8, idx_x=P, nx=1, idx_e=P, ne=3, off_x=P, off_e=P, P=4, x=P, n_x=9, e=P, n_e=7)),
    'uds_halo_pack_clear_all': ('x n_x e n_e S F idx_x nx idx_e ne off_x off_e P buf',
                                dict(x=P, n_x=9, e=P, n_e=7, S=2, F=8, idx_x=P, nx=1, idx_e=P, ne=3, off_x=P, off_e=P, P=4, buf=P)),
    'uds_halo_accumulate_all': ('buf S F off_x off_e P tgt_x tx tgt_e te ptr src n_src x n_x e n_e',
                                dict(buf=P, S=2, F=8, off_x=P, off_e=P, P=4, tgt_x=P, tx=1, tgt_e=P, te=3, ptr=P, src=P, n_src=6, x=P, n_x=9, e=P,
                                     n_e=7)),
}

NO_STREAM = {'uds_dense_route'}      # host-only entries of the table: their argument list does not end in a stream

BIG = 1 << 31


def _family(entries, changes, text, named=None):
    """The same bad argument for every entry of a family; `text` takes the entry's name (or `named`, the sibling the
    message names) for '%s'."""
    return [(e, changes, text.replace('%s', named or e)) for e in entries]


REC_FWD = ('uds_recurrent_forward', 'uds_recurrent_forward_train')
REC_BWD = ('uds_recurrent_backward', 'uds_recurrent_backward_h')
CUMSUM = ('uds_dense_cumsum', 'uds_dense_cumsum_heads')
HALO = ('uds_halo_pack', 'uds_halo_unpack')
HALO_ALL = ('uds_halo_pack_all', 'uds_halo_unpack_all', 'uds_halo_pack_clear_all')
REMAINDER = ('uds_remainder_forward', 'uds_remainder_forward_dense')
ROWGEMM = ('uds_rowgemm_forward', 'uds_rowgemm_forward_cat')
POOL_PAIR = ('uds_attn_sum_pool_pair', 'uds_attn_sum_pool_backward')

# (entry, arguments changed against GOOD, text that uds_last_error() must contain)
CASES = (
    # ---- GRU / LSTM forward: uds_recurrent_forward forwards to _train, whose messages name uds_recurrent_forward
    _family(REC_FWD, dict(xp=None), '%s: NULL argument', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(U=None), '%s: NULL argument', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(out=None), '%s: NULL argument', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(kind=2), '%s: kind 2 (0 = GRU, 1 = LSTM)', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(H=257), '%s: bad sizes B=2 T=3 R=5 H=257', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(H=0), '%s: bad sizes B=2 T=3 R=5 H=0', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(B=-1), '%s: bad sizes B=-1 T=3 R=5 H=32', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(T=-1), '%s: bad sizes B=2 T=-1 R=5 H=32', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(R=-1), '%s: bad sizes B=2 T=3 R=-1 H=32', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(B=1 << 40, R=1), '%s: too many rows', 'uds_recurrent_forward')
    + _family(REC_FWD, dict(B=1 << 40, R=1, H=256), '%s: too many rows', 'uds_recurrent_forward')
    # ---- GRU / LSTM backward: the 64-unit entry and the one for the other widths
    + _family(REC_BWD, dict(xp=None), '%s: NULL argument')
    + _family(REC_BWD, dict(packed=None), '%s: NULL argument')
    + _family(REC_BWD, dict(h=None), '%s: NULL argument')
    + _family(REC_BWD, dict(gh=None), '%s: NULL argument')
    + _family(REC_BWD, dict(dxp=None), '%s: NULL argument')
    + _family(REC_BWD, dict(darec=None), '%s: NULL argument')
    + _family(REC_BWD, dict(kind=2), '%s: kind 2 (0 = GRU, 1 = LSTM)')
    + _family(REC_BWD, dict(kind=1), '%s: the LSTM needs the cell states of the forward pass (uds_recurrent_forward_train)')
    + _family(REC_BWD, dict(B=-1), '%s: bad sizes B=-1 T=3 R=5')
    + _family(REC_BWD, dict(T=-1), '%s: bad sizes B=2 T=-1 R=5')
    + _family(REC_BWD, dict(R=-1), '%s: bad sizes B=2 T=3 R=-1')
    + [(e, {k: Q}, e + ': buffers must be 16-byte aligned') for e in REC_BWD for k in ('xp', 'packed', 'b_rec', 'h', 'gh', 'dxp', 'darec')]
    + _family(REC_BWD, dict(kind=1, c=Q), '%s: buffers must be 16-byte aligned')
    + _family(REC_BWD, dict(B=BIG), '%s: too many rows')
    + _family(REC_BWD, dict(T=BIG), '%s: too many rows')
    + [('uds_recurrent_backward_h', dict(H=24), 'uds_recurrent_backward_h: 24 units (a multiple of 16 from 16 to 128)'),
       ('uds_recurrent_backward_h', dict(H=144), 'uds_recurrent_backward_h: 144 units'),
       ('uds_recurrent_pack_bwd', dict(U=None), 'uds_recurrent_pack_bwd: NULL / misaligned argument'),
       ('uds_recurrent_pack_bwd', dict(packed=Q), 'uds_recurrent_pack_bwd: NULL / misaligned argument'),
       ('uds_recurrent_pack_bwd', dict(H=40), 'uds_recurrent_pack_bwd: H=40 kind=0'),
       ('uds_recurrent_pack_bwd', dict(kind=2), 'uds_recurrent_pack_bwd: H=32 kind=2'),
       ('uds_recurrent_fused', dict(x=None), 'uds_recurrent_fused: NULL argument'),
       ('uds_recurrent_fused', dict(b_in=None), 'uds_recurrent_fused: NULL argument'),
       ('uds_recurrent_fused', dict(kind=2), 'uds_recurrent_fused: kind 2 (0 = GRU, 1 = LSTM)'),
       ('uds_recurrent_fused', dict(F=32), 'uds_recurrent_fused: input width 32'),
       ('uds_recurrent_fused', dict(B=-1), 'uds_recurrent_fused: bad sizes B=-1 T=3 R=5'),
       ('uds_recurrent_fused', dict(out=Q), 'uds_recurrent_fused: buffers must be 16-byte aligned'),
       ('uds_recurrent_fused', dict(b_rec=Q), 'uds_recurrent_fused: buffers must be 16-byte aligned'),
       ('uds_recurrent_fused', dict(B=BIG), 'uds_recurrent_fused: too many rows')]
    # ---- Dense + cumsum, with and without heads
    + _family(('uds_dense_cumsum',), dict(x=None), '%s: NULL x/packed/out')
    + _family(('uds_dense_cumsum',), dict(packed=None), '%s: NULL x/packed/out')
    + _family(('uds_dense_cumsum',), dict(out=None), '%s: NULL x/packed/out')
    + _family(('uds_dense_cumsum_heads',), dict(x=None), '%s: NULL x/packed/heads/out')
    + _family(('uds_dense_cumsum_heads',), dict(packed=None), '%s: NULL x/packed/heads/out')
    + _family(('uds_dense_cumsum_heads',), dict(out=None), '%s: NULL x/packed/heads/out')
    + _family(('uds_dense_cumsum_heads',), dict(heads=None), '%s: NULL x/packed/heads/out')
    + _family(CUMSUM, dict(T=0), '%s: bad sizes B=2 T=0 R=5')
    + _family(CUMSUM, dict(R=0), '%s: bad sizes B=2 T=3 R=0')
    + _family(CUMSUM, dict(B=-1), '%s: bad sizes B=-1 T=3 R=5')
    + _family(CUMSUM, dict(act=9), '%s: unknown activation 9')
    + _family(CUMSUM, dict(act=-1), '%s: unknown activation -1')
    + [(e, {k: Q}, e + ': pointers must be 16-byte aligned') for e in CUMSUM for k in ('x', 'packed', 'bias', 'res')]
    + [('uds_dense_cumsum', dict(out=Q), 'uds_dense_cumsum: pointers must be 16-byte aligned')]
    + _family(CUMSUM, dict(B=1 << 16, T=1 << 16), '%s: 21474836480 rows exceed the int32 row index')
    + [('uds_dense_cumsum_heads', dict(heads=ctypes.addressof(_HEADS5)), 'uds_dense_cumsum_heads: first head needs 1..4 outputs (got 5)'),
       ('uds_cumsum_act', dict(x=None), 'uds_cumsum_act: NULL x/out'),
       ('uds_cumsum_act', dict(F=6), 'uds_cumsum_act: bad sizes (F must be a multiple of 4)'),
       ('uds_cumsum_act', dict(res=Q), 'uds_cumsum_act: x/res/out must be 16-byte aligned'),
       ('uds_cumsum_act', dict(act=9), 'uds_cumsum_act: unknown activation 9')]
    # ---- halo exchange: per peer, and the one-launch forms
    + _family(HALO, dict(F=6), '%s: bad sizes (S=2 nx=1 ne=3 F=6)')
    + _family(HALO, dict(S=-1), '%s: bad sizes (S=-1 nx=1 ne=3 F=8)')
    + _family(HALO, dict(nx=-1), '%s: bad sizes (S=2 nx=-1 ne=3 F=8)')
    + _family(HALO, dict(n_e=-1), '%s: bad sizes (S=2 nx=1 ne=3 F=8)')
    + _family(HALO, dict(buf=None), '%s: NULL argument')
    + _family(HALO, dict(idx_x=None), '%s: NULL argument')
    + _family(HALO, dict(e=None), '%s: NULL argument')
    + _family(HALO, dict(buf=Q), '%s: buffers must be 16-byte aligned')
    + _family(HALO, dict(x=Q), '%s: buffers must be 16-byte aligned')
    + _family(HALO, dict(e=Q), '%s: buffers must be 16-byte aligned')
    + _family(HALO, dict(nx=BIG), '%s: message too large')
    + _family(HALO_ALL, dict(S=65536), '%s: bad sizes (S=65536 nx=1 ne=3 F=8 P=4; needs S <= 65535, F >= 1, P >= 1)')
    + _family(HALO_ALL, dict(F=0), '%s: bad sizes (S=2 nx=1 ne=3 F=0 P=4;')
    + _family(HALO_ALL, dict(P=0), '%s: bad sizes (S=2 nx=1 ne=3 F=8 P=0;')
    + _family(HALO_ALL, dict(ne=-1), '%s: bad sizes (S=2 nx=1 ne=-1 F=8 P=4;')
    + _family(HALO_ALL, dict(n_x=-1), '%s: bad sizes (S=2 nx=1 ne=3 F=8 P=4;')
    + _family(HALO_ALL, dict(buf=None), '%s: NULL argument')
    + _family(HALO_ALL, dict(off_x=None), '%s: NULL argument')
    + _family(HALO_ALL, dict(off_e=None), '%s: NULL argument')
    + _family(HALO_ALL, dict(x=None), '%s: NULL argument')
    + _family(HALO_ALL, dict(idx_e=None), '%s: NULL argument')
    + _family(HALO_ALL, dict(nx=BIG), '%s: messages too large')
    + _family(HALO_ALL, dict(P=BIG), '%s: messages too large')
    + _family(HALO_ALL, dict(F=BIG), '%s: messages too large')
    + [('uds_halo_accumulate_all', dict(S=65536),
        'uds_halo_accumulate_all: bad sizes (S=65536 tx=1 te=3 n_src=6 F=8 P=4; needs S <= 65535, F >= 1, P >= 1)'),
       ('uds_halo_accumulate_all', dict(n_src=-1), 'uds_halo_accumulate_all: bad sizes (S=2 tx=1 te=3 n_src=-1 F=8 P=4;'),
       ('uds_halo_accumulate_all', dict(P=0), 'uds_halo_accumulate_all: bad sizes (S=2 tx=1 te=3 n_src=6 F=8 P=0;'),
       ('uds_halo_accumulate_all', dict(off_x=None), 'uds_halo_accumulate_all: NULL argument'),
       ('uds_halo_accumulate_all', dict(ptr=None), 'uds_halo_accumulate_all: NULL argument'),
       ('uds_halo_accumulate_all', dict(buf=None), 'uds_halo_accumulate_all: NULL argument'),
       ('uds_halo_accumulate_all', dict(tgt_e=None), 'uds_halo_accumulate_all: NULL argument'),
       ('uds_halo_accumulate_all', dict(tx=BIG), 'uds_halo_accumulate_all: too many rows'),
       ('uds_halo_accumulate_all', dict(n_src=BIG), 'uds_halo_accumulate_all: too many rows')]
    # ---- remainder GEMM: from x, and from e through the Dense
    + _family(REMAINDER, dict(R=0), '%s: bad shape')
    + _family(REMAINDER, dict(M=0), '%s: bad shape')
    + _family(REMAINDER, dict(S=-1), '%s: bad shape')
    + _family(REMAINDER, dict(packed=None), '%s: NULL argument')
    + _family(REMAINDER, dict(workspace=None), '%s: NULL argument')
    + _family(REMAINDER, dict(out=None), '%s: NULL argument')
    + _family(REMAINDER, dict(out=Q), '%s: buffers must be 16-byte aligned')
    + _family(REMAINDER, dict(packed=Q), '%s: buffers must be 16-byte aligned')
    + _family(REMAINDER, dict(S=65536), '%s: shape exceeds the launch grid')
    + [('uds_remainder_forward', dict(x=None), 'uds_remainder_forward: NULL argument'),
       ('uds_remainder_forward', dict(h=5), 'uds_remainder_forward: h = 5 (needs h % 4 == 0, h <= 64)'),
       ('uds_remainder_forward', dict(h=68), 'uds_remainder_forward: h = 68'),
       ('uds_remainder_forward_dense', dict(e=None), 'uds_remainder_forward_dense: NULL argument'),
       ('uds_remainder_forward_dense', dict(packed_w=None), 'uds_remainder_forward_dense: NULL argument'),
       ('uds_remainder_forward_dense', dict(F=65), 'uds_remainder_forward_dense: F = 65, h = 32 (F 64 or 128, h 32 or 64)'),
       ('uds_remainder_forward_dense', dict(h=16), 'uds_remainder_forward_dense: F = 64, h = 16'),
       ('uds_remainder_forward_dense', dict(act=9), 'uds_remainder_forward_dense: unknown activation 9'),
       ('uds_remainder_forward_dense', dict(bias=Q), 'uds_remainder_forward_dense: buffers must be 16-byte aligned'),
       ('uds_remainder_pack', dict(rest=None), 'uds_remainder_pack: NULL / misaligned argument'),
       ('uds_remainder_pack', dict(packed=Q), 'uds_remainder_pack: NULL / misaligned argument'),
       ('uds_remainder_pack', dict(R=0), 'uds_remainder_pack: bad shape (0, 7)')]
    # ---- row GEMM: uds_rowgemm_forward forwards to _cat, whose later messages name uds_rowgemm_forward
    + _family(ROWGEMM, dict(x=None), '%s: NULL x/packed/out', 'uds_rowgemm_forward')
    + _family(ROWGEMM, dict(packed=None), '%s: NULL x/packed/out', 'uds_rowgemm_forward')
    + _family(ROWGEMM, dict(out=None), '%s: NULL x/packed/out', 'uds_rowgemm_forward')
    + _family(ROWGEMM, dict(act=9), '%s: unknown activation 9', 'uds_rowgemm_forward')
    + _family(ROWGEMM, dict(out=Q), '%s: pointers must be 16-byte aligned', 'uds_rowgemm_forward')
    + _family(ROWGEMM, dict(bias=Q), '%s: pointers must be 16-byte aligned', 'uds_rowgemm_forward')
    + _family(ROWGEMM, dict(B=BIG), '%s: 32212254720 rows exceed the int32 row index', 'uds_rowgemm_forward')
    + [('uds_rowgemm_forward', dict(F=33), 'uds_rowgemm_forward: needs F % 32 == 0, f_out <= 64 (B=2 T=3 R=5 F=33 taps=1 f_out=16)'),
       ('uds_rowgemm_forward', dict(f_out=68), 'uds_rowgemm_forward: needs F % 32 == 0, f_out <= 64 (B=2 T=3 R=5 F=32 taps=1 f_out=68)'),
       ('uds_rowgemm_forward', dict(taps=16, F=1024, f_out=64), 'uds_rowgemm_forward: K=16384 x f_out=64 weights do not fit the LDS'),
       ('uds_rowgemm_forward_cat', dict(F1=33), 'uds_rowgemm_forward: needs F % 32 == 0, f_out <= 64 (B=2 T=3 R=5 F=33 taps=1 f_out=16)'),
       ('uds_rowgemm_forward_cat', dict(F2=32), 'uds_rowgemm_forward_cat: x2 / F2 disagree'),
       ('uds_rowgemm_forward_cat', dict(x2=P), 'uds_rowgemm_forward_cat: x2 / F2 disagree'),
       ('uds_rowgemm_forward_cat', dict(x2=P, F2=32, taps=2), 'uds_rowgemm_forward_cat: a two-tensor row needs taps = 1 and both widths multiples of 32'),
       ('uds_rowgemm_forward_cat', dict(x2=Q, F2=32), 'uds_rowgemm_forward_cat: a two-tensor row needs taps = 1 and both widths multiples of 32'),
       ('uds_rowgemm_forward_cat', dict(ldo=8), 'uds_rowgemm_forward_cat: output block [0, 16) does not fit rows of 8 floats (4-float aligned)'),
       ('uds_rowgemm_forward_cat', dict(ldo=32, col0=18), 'uds_rowgemm_forward_cat: output block [18, 34) does not fit rows of 32 floats'),
       ('uds_rowgemm_forward_pair', dict(x1=None), 'uds_rowgemm_forward_pair: NULL argument'),
       ('uds_rowgemm_forward_pair', dict(dil=-1), 'uds_rowgemm_forward_pair: needs F % 32 == 0, f_out <= 64, dil > 0'),
       ('uds_rowgemm_forward_pair', dict(act=9), 'uds_rowgemm_forward_pair: unknown activation 9'),
       ('uds_rowgemm_forward_pair', dict(out1=Q), 'uds_rowgemm_forward_pair: pointers must be 16-byte aligned'),
       ('uds_rowgemm_pack', dict(W=None), 'uds_rowgemm_pack: NULL / misaligned argument'),
       ('uds_rowgemm_pack', dict(packed=Q), 'uds_rowgemm_pack: NULL / misaligned argument'),
       ('uds_rowgemm_pack', dict(k_total=33), 'uds_rowgemm_pack: needs K % 32 == 0 and f_out <= 64 (K=33 f_out=16)')]
    # ---- pooling
    + _family(POOL_PAIR, dict(x=None), '%s: NULL argument')
    + _family(POOL_PAIR, dict(e=None), '%s: NULL argument')
    + _family(POOL_PAIR, dict(F=6), '%s: B=2 Rx=5 Re=3 F=6 (F a power of two, 4 .. 256)')
    + _family(POOL_PAIR, dict(Rx=0), '%s: B=2 Rx=0 Re=3 F=8')
    + _family(POOL_PAIR, dict(Re=-1), '%s: B=2 Rx=5 Re=-1 F=8')
    + _family(POOL_PAIR, dict(B=BIG), '%s: too many rows')
    + _family(POOL_PAIR, dict(Rx=BIG - 2), '%s: too many rows')
    + [('uds_attn_sum_pool_pair', dict(e=Q), 'uds_attn_sum_pool_pair: x/e/k/out must be 16-byte aligned'),
       ('uds_attn_sum_pool_backward', dict(stat=None), 'uds_attn_sum_pool_backward: NULL argument'),
       ('uds_attn_sum_pool_backward', dict(dk_ws=None), 'uds_attn_sum_pool_backward: dk needs the workspace dk_ws (B, F)'),
       ('uds_attn_sum_pool_backward', dict(de=Q), 'uds_attn_sum_pool_backward: x/e/k/out/grad/dx/de/dk_ws/dk must be 16-byte aligned'),
       ('uds_attn_sum_pool', dict(k=None), 'uds_attn_sum_pool: NULL argument'),
       ('uds_attn_sum_pool', dict(F=6), 'uds_attn_sum_pool: B=2 R=5 F=6 (F a power of two, 4 .. 256)'),
       ('uds_attn_sum_pool', dict(out=Q), 'uds_attn_sum_pool: x/k/out must be 16-byte aligned'),
       ('uds_attn_sum_pool', dict(R=BIG), 'uds_attn_sum_pool: too many rows')]
    # ---- Dense, Conv1D, dropout, weight gradient
    + [('uds_dense_act', dict(xa=None), 'uds_dense_act: NULL xa/W/out'),
       ('uds_dense_act', dict(out=Q), 'uds_dense_act: out must be 16-byte aligned'),
       ('uds_dense_act', dict(fb=4), 'uds_dense_act: fa=8 fb=4 xb='),
       ('uds_dense_act', dict(f_out=257), 'uds_dense_act: rows=3 f_out=257 (max 256) f_in=8'),
       ('uds_dense_act', dict(act=9), 'uds_dense_act: unknown activation 9'),
       ('uds_dense_act', dict(a_self=P), 'uds_dense_act: a_self/a_nbr/s_self/s_nbr must be given together'),
       ('uds_dense_route', dict(info5=None), 'uds_dense_route: info5 is NULL'),
       ('uds_dense_route', dict(fa=0), 'uds_dense_route: fa=0 fb=0 rows=3 (max 2^40) f_out=8 (max 256) f_in=0 (max 4096)'),
       ('uds_dense_route', dict(fb=-1), 'uds_dense_route: fa=8 fb=-1 rows=3'),
       ('uds_dense_route', dict(rows=-1), 'uds_dense_route: fa=8 fb=0 rows=-1'),
       ('uds_dense_route', dict(rows=(1 << 40) + 1), 'uds_dense_route: fa=8 fb=0 rows=1099511627777 (max 2^40)'),
       ('uds_dense_route', dict(f_out=257), 'uds_dense_route: fa=8 fb=0 rows=3 (max 2^40) f_out=257 (max 256)'),
       ('uds_dense_route', dict(f_out=0), 'uds_dense_route: fa=8 fb=0 rows=3 (max 2^40) f_out=0 (max 256)'),
       ('uds_dense_route', dict(fa=4000, fb=97), 'uds_dense_route: fa=4000 fb=97 rows=3 (max 2^40) f_out=8 (max 256) f_in=4097 (max 4096)'),
       ('uds_dense_route', dict(taps=17), 'uds_dense_route: taps=17 (0 .. 16;'),
       ('uds_dense_route', dict(taps=-1), 'uds_dense_route: taps=-1 (0 .. 16;'),
       ('uds_dense_route', dict(taps=2, fb=4), 'uds_dense_route: taps=2 (0 .. 16; a convolution has no xb and no attention scalars'),
       ('uds_dense_route', dict(taps=2, attn=1), 'uds_dense_route: taps=2 (0 .. 16; a convolution has no xb and no attention scalars'),
       ('uds_dense_route', dict(taps=16, fa=257), 'taps * fa = 4112 <= 4096)'),
       ('uds_dense_route', dict(rows=1 << 40, f_out=256, fa=9), 'uds_dense_route: rows=1099511627776 need 68719476736 workgroups, more than a launch grid holds'),
       ('uds_conv1d_causal', dict(kernel=None), 'uds_conv1d_causal: NULL x/kernel/out'),
       ('uds_conv1d_causal', dict(taps=17), 'uds_conv1d_causal: bad sizes B=2 T=3 R=5 F=8 taps=17 dil=1 H=16'),
       ('uds_conv1d_causal', dict(act=9), 'uds_conv1d_causal: unknown activation 9'),
       ('uds_conv1d_causal', dict(out=Q), 'uds_conv1d_causal: out must be 16-byte aligned'),
       ('uds_dropout', dict(x=None), 'uds_dropout: NULL argument'),
       ('uds_dropout', dict(n=-1), 'uds_dropout: NULL argument'),
       ('uds_dropout', dict(rate=1.0), 'uds_dropout: rate=1 outside [0, 1)'),
       ('uds_dropout', dict(n=1 << 62), 'uds_dropout: n=4611686018427387904 too large for one launch'),
       ('uds_wgrad', dict(a=None), 'uds_wgrad: NULL argument'),
       ('uds_wgrad', dict(d_bias=None), 'uds_wgrad: with_bias needs d_bias'),
       ('uds_wgrad', dict(T=0), 'uds_wgrad: bad sizes'),
       ('uds_wgrad', dict(F=200), 'uds_wgrad: F=200 (at most 128 rows incl. the bias row) or H=16 (at most 64) not supported'),
       ('uds_wgrad', dict(H=65), 'uds_wgrad: F=8 (at most 128 rows incl. the bias row) or H=65 (at most 64) not supported'),
       ('uds_wgrad', dict(B=BIG), 'uds_wgrad: 32212254720 rows exceed the int32 row index')]
)

# entries whose checks sit behind a pattern / network handle: (entry, text) of the all-NULL call
NULL_HANDLE = (
    ('uds_csr_shape', 'uds_csr_shape: NULL handle'),
    ('uds_csr_row_order', 'uds_csr_row_order: NULL argument'),
    ('uds_flow_balance', 'uds_flow_balance: NULL argument'),
    ('uds_diffusion_forward', 'uds_diffusion_forward: NULL argument'),
    ('uds_diffusion_backward', 'uds_diffusion_backward: NULL argument'),
    ('uds_diffusion_forward_m', 'uds_diffusion_forward_m: NULL argument'),
    ('uds_diffusion_backward_m', 'uds_diffusion_backward_m: NULL argument'),
    ('uds_roll_update', 'uds_roll_update: NULL argument'),
    ('uds_csr_spmm', 'uds_csr_spmm: NULL csr/x/out'),
    ('uds_gat_forward', 'uds_gat_forward: NULL argument'),
    ('uds_gat_aggregate', 'uds_gat_aggregate: NULL argument'),
    ('uds_gat_aggregate_coef', 'uds_gat_aggregate_coef: NULL argument'),
    ('uds_gat_aggregate_masked', 'uds_gat_aggregate_masked: NULL argument'),
    ('uds_gat_aggregate_ex', 'uds_gat_aggregate_ex: NULL argument'),
    ('uds_gat_aggregate_heads', 'uds_gat_aggregate_heads: NULL argument'),
    ('uds_gat_backward', 'uds_gat_backward: NULL argument'),
    ('uds_gat_backward_coef', 'uds_gat_backward: NULL argument'),            # names the entry it grew out of
    ('uds_gat_backward_ex', 'uds_gat_backward_ex: NULL argument'),
    ('uds_gat_backward_heads', 'uds_gat_backward_heads: NULL argument'),
    ('uds_csr_sddmm', 'uds_csr_sddmm: NULL argument'),
    ('uds_network_prepare', 'uds_network_prepare: NULL network'),
    ('uds_network_plan_info', 'uds_network_plan_info: NULL argument'),
    ('uds_network_fused_launches', 'uds_network_fused_launches: NULL argument'),
    ('uds_fused_chunk', 'uds_fused_chunk: NULL argument'),
    ('uds_tile_plan_sizes', 'uds_tile_plan_sizes: NULL plan'),
    ('uds_tile_plan_copy', 'uds_tile_plan_copy: NULL argument'),
    ('uds_tile_plan_blocks', 'uds_tile_plan_blocks: NULL plan'),
    ('uds_spatial_pack_weights', 'uds_spatial_pack_weights: NULL argument'),
    ('uds_spatial_layer_forward', 'uds_spatial_layer_forward: NULL argument'),
    ('uds_spatial_layer_forward_split', 'uds_spatial_layer_forward: NULL argument'),
    ('uds_spatial_layer_forward_rem', 'uds_spatial_layer_forward_rem: NULL remainder'),
)


def call_args(entry, changes):
    """The ABI-order argument list of `entry`: GOOD with `changes` applied, and a NULL stream (none for the NO_STREAM entries)."""
    names, good = GOOD[entry]
    names = names.split()
    assert set(names) == set(good) and set(changes) <= set(good), entry
    args = dict(good, **changes)
    return [args[n] for n in names] + ([] if entry in NO_STREAM else [None])


def null_args(entry):
    """Every pointer NULL, every number 0."""
    return [0.0 if t is ctypes.c_float else None if t is _lib._c_ptr or hasattr(t, 'contents') else 0 for t in _lib.SYMBOLS[entry][1]]


def _id(case):
    """Addresses differ from one process to the next, so an id names them: the same test keeps the same id in every run."""
    names = {P: 'P', Q: 'Q', ctypes.addressof(_HEADS): 'HEADS', ctypes.addressof(_HEADS5): 'HEADS5'}
    return '%s-%s' % (case[0], '-'.join('%s=%s' % (k, names.get(v, v) if isinstance(v, int) else v) for k, v in case[1].items()))


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_bad_argument_is_refused_with_its_message(case):
    entry, changes, text = case
    lib = _lib.load()
    rc = getattr(lib, entry)(*call_args(entry, changes))
    msg = lib.uds_last_error().decode()
    assert rc == EINVAL and text in msg, (rc, msg)


@pytest.mark.parametrize('entry,text', NULL_HANDLE, ids=[e for e, _ in NULL_HANDLE])
def test_null_handle_is_refused_with_its_message(entry, text):
    lib = _lib.load()
    rc = getattr(lib, entry)(*null_args(entry))
    msg = lib.uds_last_error().decode()
    assert rc == EINVAL and msg.startswith(text), (rc, msg)


def test_every_family_member_is_in_the_table():
    tested = {c[0] for c in CASES} | {e for e, _ in NULL_HANDLE}
    for fam in (REC_FWD, REC_BWD, CUMSUM, HALO, HALO_ALL, REMAINDER, ROWGEMM, POOL_PAIR):
        assert set(fam) <= tested
    assert set(GOOD) <= tested | {'uds_halo_accumulate_all'}
