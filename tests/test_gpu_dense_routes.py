"""fp64 parity of the exact-fp32 Dense / Conv1D / cumsum family at every kernel route: uds_dense_act, uds_conv1d_causal,
uds_cumsum_act and uds_gat_forward.  This family is what every layer of a precision='fp32' model, every shape the row GEMM
refuses, the input gradients (rows_matmul, the causal convolution at a negative dilation), the GAT linear map with its attention
scalars, the GRU / LSTM input projection and the embeddings run on.

Which case reaches which kernel is in tests/dense_util.py (cases, seeded inputs, fp64 references; tests/test_dense_route_math.py
checks on the CPU that the tables are what they claim).  Every dense and conv case first asserts its route -- kernel, template
parameter, workgroups -- from uds_dense_route, which the launch takes its choice from: a case that stops reaching its kernel fails.
  (i)    k_dense_act<1 .. 64> at every width class, float4 and scalar stores, idle column groups, 1 / ROWS - 1 / ROWS / 2 ROWS + 1 rows
  (ii)   K around the 32-wide chunk, narrow K below 64 rows, K = 4096
  (iii)  [xa | xb] with the boundary on, inside and at the start of a K chunk: fp64, and the bits of the call on the concatenated rows
  (iv)   k_embed_act<1 .. 8>, odd lane counts per row, ragged grids, two capped grids whose grid-stride loop makes a second trip; rows
         0 .. 62 alone (the tiled kernel) give the same bits for all five activations
  (v)    five activations x bias given / none, pre-activations across zero and both clamps
  (vi)   attention scalars at every CG, with idle column groups, with and without xb; `out` has the bits of the call without them
  (vii)  uds_conv1d_causal at +dil and -dil, workgroups that straddle time steps and batch elements; the bits of uds_dense_act on the
         host-built shifted rows
  (viii) uds_cumsum_act: five activations x res given / none, ragged last workgroup, lanes of different b in one wave
  (ix)   uds_gat_forward = uds_dense_act with attention scalars + uds_gat_aggregate, bit for bit, workspace included
  (x)    row independence: the batch call against calls on row slices / one batch element, bit for bit
  (B)    W and bias offset by one float: the route says tiled, the bits are those of the aligned call

Every input is a view inside a NaN-filled allocation, every output (s_self / s_nbr and the GAT workspace included) a view inside a
sentinel-filled one that is checked on both sides and for finiteness.  Plain allocations: nothing here is meant to fault.

Tolerances, relative to max(1, max|ref|) through tests.util.close (UDS_TOL_REPORT=1 prints observed / allowed): dense, conv and
attention outputs TOL = 5e-6 (tests/test_gpu_parity.py), cumsum 1e-6 (test_cumsum_act_and_flow_balance).

MEASURED on an MI355X (UDS_TOL_REPORT=1), worst observed / allowed per test over all its cases [case]:
  test_dense_parity                              0.303  [k-fa4096-fo8-r70-linear]
  test_concat                                    0.089  [cat-fa33+200-fo64-r129-hard_sigmoid]
  test_embed                                     0.023  [embed-fa7-fo64-r200-tanh]
  test_attention_scalars                         0.107  [attn-fa40+24-fo250-r33-linear-nobias-attn]
  test_conv1d_causal                             0.177  [B1T6R3F64H64k16-dil-1]
  test_cumsum_act                                0.504  [B2T60R9F8-tanh-res]   (linear at the same shape: 0.314)
  test_gat_forward_is_dense_act_then_aggregate   0.067  [256]
Every bit-equality above holds, the stream against the tiled kernel for all five activations included.  No bound was raised.  The
228 tests take 3 s.  Planted in scratch builds, never committed (each keeps every access inside the tensors): the tap order
reversed fails all 16 test_conv1d_causal cases here; `% T` dropped from the time index fails the 12 of them with B > 1 and both
test_conv_batch_elements_are_independent; the grid rounding of the stream dropped fails the route assertion of the 10 cases whose
workgroup count it changes (test_embed, the bitwise and the row-subset test), and the capped f_out = 252 case -- the only one of
them where lanes make a second trip -- is then off by 3e12 x its bound, the other nine stay right.
"""
import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from tests import dense_util as D
from tests.util import PAD, Guarded, close, ladder, nan_in

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def check(what, got, ref, tol):
    """tests.util.close (which records observed / allowed for UDS_TOL_REPORT and names both in its failure), then the figure."""
    err = close(got, ref, tol, _depth=2)
    print('%-60s err %.3e  ratio %.3f' % (what, err, err / (tol * max(1.0, float(ref.abs().max())))))
    return err


def nan_in_off(t, dev, off):
    """tests.util.nan_in with the view `off` floats past a 16-byte boundary."""
    if t is None or off == 0:
        return nan_in(t, dev)
    buf = torch.full((t.numel() + 2 * PAD,), float('nan'), dtype=torch.float32, device=dev)
    v = buf[PAD + off:PAD + off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        '%s: %d of %d values differ in their bits' % (what, int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum()), a.numel())


def dense_call(dev, x, W, b, act, xb=None, attn=None, expect=None, off=0):
    """One guarded uds_dense_act call on host tensors: the route is read for the operands as placed (and compared with `expect` =
    (kernel, param, workgroups)), outputs are checked on both sides and for finiteness.  Returns (out, s_self, s_nbr, route)."""
    rows, fa = x.shape
    fo = W.shape[1]
    dW, db = nan_in_off(W, dev, off), nan_in_off(b, dev, off)
    aligned = dW.data_ptr() % 16 == 0 and (db is None or db.data_ptr() % 16 == 0)
    r = _lib.dense_route(fa, fo, rows, fb=0 if xb is None else xb.shape[1], attn=attn is not None, aligned=aligned)
    if expect is not None:
        assert (r['kernel'], r['param'], r['workgroups']) == tuple(expect), r
    out = Guarded((rows, fo), dev)
    s = (Guarded((rows,), dev), Guarded((rows,), dev)) if attn is not None else None
    got = _lib.dense_act(nan_in(x, dev), dW, db, act, nan_in(xb, dev), attn=None if attn is None else tuple(nan_in(a, dev) for a in attn),
                         out=out.view, s_out=None if s is None else (s[0].view, s[1].view))
    torch.cuda.synchronize()
    out.check('out')
    if attn is None:
        assert got is out.view
        return out.view, None, None, r
    assert got[0] is out.view and got[1] is s[0].view and got[2] is s[1].view
    s[0].check('s_self'); s[1].check('s_nbr')
    return out.view, s[0].view, s[1].view, r


def case_call(dev, c, p, act=None, **kw):
    return dense_call(dev, p['x'], p['W'], p['b'], act or c['act'], p['xb'], (p['a_self'], p['a_nbr']) if c['attn'] else None,
                      expect=(c['kernel'], c['param'], c['wgs']), **kw)


def ids(cases):
    return [c['id'] for c in cases]


# ---- (i), (ii), (v): fp64 parity on the tiled kernel and the stream
@pytest.mark.parametrize('c', D.TILED_WIDTH_CASES + D.K_CASES + D.ACT_CASES, ids=ids(D.TILED_WIDTH_CASES + D.K_CASES + D.ACT_CASES))
def test_dense_parity(dev, c):
    p = D.dense_inputs(c)
    out = case_call(dev, c, p)[0]
    check(c['id'], out, D.dense_ref(c, p)[0], D.TOL)


# ---- (iii): the split input
@pytest.mark.parametrize('c', D.CONCAT_CASES, ids=ids(D.CONCAT_CASES))
def test_concat(dev, c):
    p = D.dense_inputs(c)
    out = case_call(dev, c, p)[0]
    check(c['id'], out, D.dense_ref(c, p)[0], D.TOL)
    r = D.route_py(c['fa'] + c['fb'], c['fo'], c['rows'])            # (3, 2) concatenated is narrow enough for the stream: the same bits still
    whole = dense_call(dev, torch.cat([p['x'], p['xb']], -1), p['W'], p['b'], c['act'], expect=(r['kernel'], r['param'], r['workgroups']))[0]
    same_bits(out, whole, 'split input against the concatenated rows')


# ---- (iv): the narrow-input stream
@pytest.mark.parametrize('c', D.EMBED_CASES + D.CAPPED_CASES, ids=ids(D.EMBED_CASES + D.CAPPED_CASES))
def test_embed(dev, c):
    p = D.dense_inputs(c)
    out, _, _, r = case_call(dev, c, p)
    if c in D.CAPPED_CASES:
        lanes = c['rows'] * c['fo'] // 4
        assert lanes > r['stride'] and lanes - r['stride'] == D.CAPPED_SECOND_TRIP[c['id']]
    check(c['id'], out, D.dense_ref(c, p)[0], D.TOL)


@pytest.mark.parametrize('c', D.EMBED_BITWISE_CASES, ids=ids(D.EMBED_BITWISE_CASES))
def test_embed_rows_have_the_bits_of_the_tiled_kernel(dev, c):
    """Both kernels run the same ascending-k fmaf chain and the same apply_act: rows 0 .. 62 called alone (the tiled kernel) equal the
    same rows of the stream's call bit for bit, for all five activations."""
    p = D.dense_inputs(c)
    n = D.EMBED_BITWISE_ROWS
    cg = D.tiled_cg(c['fo'])
    for act in D.ACTS:
        out = case_call(dev, c, p, act=act)[0]
        head = dense_call(dev, p['x'][:n], p['W'], p['b'], act, expect=('tiled', cg, -(-n // D.TILE_ROWS[cg])))[0]
        same_bits(out[:n], head, '%s: stream against tiled' % act)


# ---- (vi): attention scalars
@pytest.mark.parametrize('c', D.ATTN_CASES, ids=ids(D.ATTN_CASES))
def test_attention_scalars(dev, c):
    p = D.dense_inputs(c)
    out, ss, sn, _ = case_call(dev, c, p)
    ref, rs, rn = D.dense_ref(c, p)
    check(c['id'] + ' out', out, ref, D.TOL)
    check(c['id'] + ' s_self', ss, rs, D.TOL)
    check(c['id'] + ' s_nbr', sn, rn, D.TOL)
    plain = dense_call(dev, p['x'], p['W'], p['b'], c['act'], p['xb'], expect=(c['kernel'], c['param'], c['wgs']))[0]
    same_bits(out, plain, 'out with attention scalars against out without')


# ---- (B): W and bias off a 16-byte boundary
def test_misaligned_weights_run_on_the_tiled_kernel(dev):
    c = D.MISALIGNED_CASE
    p = D.dense_inputs(c)
    aligned = case_call(dev, c, p)[0]
    check(c['id'], aligned, D.dense_ref(c, p)[0], D.TOL)
    cg = D.tiled_cg(c['fo'])
    off, _, _, r = dense_call(dev, p['x'], p['W'], p['b'], c['act'], expect=('tiled', cg, -(-c['rows'] // D.TILE_ROWS[cg])), off=1)
    assert r['kernel'] == 'tiled'
    same_bits(off, aligned, 'W and bias offset by one float against the aligned call')


# ---- (vii): the causal convolution, both directions
def conv_call(dev, c, x, kernel, b):
    B, T, R, F = x.shape
    taps, _, H = kernel.shape
    r = _lib.dense_route(F, H, B * T * R, taps=taps)
    assert (r['kernel'], r['param'], r['workgroups']) == ('tiled', D.tiled_cg(H), -(-B * T * R // D.TILE_ROWS[D.tiled_cg(H)])), r
    out = Guarded((B, T, R, H), dev)
    got = _lib.conv1d_causal(nan_in(x, dev), nan_in(kernel, dev), nan_in(b, dev), c['dil'], c['act'], out=out.view)
    torch.cuda.synchronize()
    assert got is out.view
    out.check('out')
    return got


@pytest.mark.parametrize('c', D.CONV_CASES, ids=ids(D.CONV_CASES))
def test_conv1d_causal(dev, c):
    B, T, R, F, H, taps = c['shape']
    p = D.conv_inputs(c)
    out = conv_call(dev, c, p['x'], p['kernel'], p['b'])
    check(c['id'], out, D.conv_ref(c, p), D.TOL)
    rows = D.conv_shifted_rows(p['x'], taps, c['dil'])
    gemm = dense_call(dev, rows, p['kernel'].reshape(taps * F, H), p['b'], c['act'])
    assert gemm[3]['kernel'] == 'tiled'
    same_bits(out.view(B * T * R, H), gemm[0], 'convolution against uds_dense_act on the shifted rows')


# ---- (viii): cumsum
@pytest.mark.parametrize('c', D.CUMSUM_CASES, ids=ids(D.CUMSUM_CASES))
def test_cumsum_act(dev, c):
    p = D.cumsum_inputs(c)
    out = Guarded(c['shape'], dev)
    got = _lib.cumsum_act(nan_in(p['x'], dev), nan_in(p['res'], dev), c['act'], out=out.view)
    torch.cuda.synchronize()
    assert got is out.view
    out.check('out')
    check(c['id'], got, D.cumsum_ref(c, p), D.TOL_CUMSUM)


# ---- (ix): the GAT forward is its two halves
@pytest.fixture(scope='module')
def gat_handle(dev):
    return _lib.CsrHandle(ladder(D.GAT_N))


@pytest.mark.parametrize('d,cg', D.GAT_WIDTHS, ids=[str(d) for d, _ in D.GAT_WIDTHS])
def test_gat_forward_is_dense_act_then_aggregate(dev, gat_handle, d, cg):
    p = D.gat_inputs(d)
    S, n, m = D.GAT_S, D.GAT_N, D.GAT_S * D.GAT_N
    r = _lib.dense_route(D.GAT_FA, d, m, fb=D.GAT_FB, attn=True)
    assert (r['kernel'], r['param'], r['workgroups']) == ('tiled', cg, -(-m // D.TILE_ROWS[cg])), r
    dv = {k: nan_in(v, dev) for k, v in p.items()}
    out, ws = Guarded((S, n, d), dev), Guarded((_lib.load().uds_gat_workspace_floats(n, S, d),), dev)
    got, (hx, ss, sn) = _lib.gat_forward(gat_handle, dv['xa'], dv['W'], dv['a_self'], dv['a_nbr'], dv['bias'], 'relu', dv['xb'],
                                         return_workspace=True, out=out.view, workspace=ws.view)
    torch.cuda.synchronize()
    assert got is out.view
    out.check('out'); ws.check('workspace')
    flat = lambda t: t.reshape(m, t.shape[-1])
    hx2, ss2, sn2, _ = dense_call(dev, flat(p['xa']), p['W'], None, 'linear', flat(p['xb']), (p['a_self'], p['a_nbr']),
                                  expect=('tiled', cg, r['workgroups']))
    same_bits(hx.reshape(m, d), hx2, 'workspace hx'); same_bits(ss.reshape(m), ss2, 'workspace s_self'); same_bits(sn.reshape(m), sn2, 'workspace s_nbr')
    agg = Guarded((S, n, d), dev)
    _lib.gat_aggregate(gat_handle, hx2.view(S, n, d), ss2.view(S, n), sn2.view(S, n), dv['bias'], 'relu', out=agg.view)
    torch.cuda.synchronize()
    agg.check('aggregate')
    same_bits(got, agg.view, 'uds_gat_forward against dense_act + gat_aggregate')
    x = torch.cat([p['xa'], p['xb']], -1)
    check('gat-d%d hx' % d, hx, x @ p['W'], D.TOL)
    check('gat-d%d s_self' % d, ss, (x @ p['W']) @ p['a_self'], D.TOL)


# ---- (x): row independence
@pytest.mark.parametrize('c,slices', D.ROW_SUBSETS, ids=[c['id'] for c, _ in D.ROW_SUBSETS])
def test_dense_rows_are_independent(dev, c, slices):
    p = D.dense_inputs(c)
    out = case_call(dev, c, p)[0]
    for lo, hi in slices:
        part, _, _, r = dense_call(dev, p['x'][lo:hi].contiguous(), p['W'], p['b'], c['act'])
        assert (r['kernel'], r['param']) == (c['kernel'], c['param'])
        same_bits(out[lo:hi], part, 'rows %d .. %d alone' % (lo, hi - 1))


@pytest.mark.parametrize('c', D.CONV_BATCH_SUBSET, ids=ids(D.CONV_BATCH_SUBSET))
def test_conv_batch_elements_are_independent(dev, c):
    p = D.conv_inputs(c)
    out = conv_call(dev, c, p['x'], p['kernel'], p['b'])
    for b in range(c['shape'][0]):
        one = conv_call(dev, c, p['x'][b:b + 1].contiguous(), p['kernel'], p['b'])
        same_bits(out[b:b + 1], one, 'batch element %d alone' % b)


# ---- out= / s_out= on the device: what tests/test_dense_route_math.py cannot reach without one
def test_out_arguments_are_checked(dev):
    x, k = torch.zeros(5, 4, device=dev), torch.zeros(4, 8, device=dev)
    with pytest.raises(_lib.UdsError, match='out must be float32'):
        _lib.dense_act(x, k, out=torch.zeros(5, 8, device=dev, dtype=torch.float64))
    with pytest.raises(_lib.UdsError, match='s_nbr must be float32'):
        _lib.dense_act(x, k, attn=(torch.zeros(8, device=dev), torch.zeros(8, device=dev)),
                       s_out=(torch.zeros(5, device=dev), torch.zeros(5, device=dev, dtype=torch.float16)))
    with pytest.raises(_lib.UdsError, match=r'out must be \(5, 8\)'):
        _lib.dense_act(x, k, out=torch.zeros(5, 8))
    with pytest.raises(_lib.UdsError, match='out must be contiguous'):
        _lib.conv1d_causal(torch.zeros(1, 2, 3, 4, device=dev), torch.zeros(2, 4, 8, device=dev), out=torch.zeros(1, 2, 8, 3, device=dev).transpose(2, 3))
    with pytest.raises(_lib.UdsError, match='out must be float32'):
        _lib.cumsum_act(torch.zeros(1, 2, 3, 4, device=dev), out=torch.zeros(1, 2, 3, 4, device=dev, dtype=torch.float64))
    assert np.isfinite(float(_lib.dense_act(x, k, out=torch.empty(5, 8, device=dev)).sum()))
