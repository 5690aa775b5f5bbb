"""GPU parity of the spatial layer with the fp64 oracle at every activation: the fused kernels on every route that reaches them,
the C entry of the exact-fp32 layer, and the unfused chain forward and backward.

The fused kernels apply the activation in two epilogues per side (the secondary Dense and the GAT output).  relu is compiled in;
linear, tanh, sigmoid and hard_sigmoid run a separate instantiation of every kernel (ACT = -1: apply_act at run time).  The
parameters come from tests/fused_act_util.py: biases spread over +-4, so the pre-activations of both epilogues cover +-4.6 and every
clamp and both tails are reached (tests/test_fused_act_math.py shows on the CPU that each region holds 10 % or more of the elements
and that a wrong epilogue -- a missing clamp, a neighbouring activation -- moves both outputs by 50 x the bound or more).  relu
runs as the control: the well-tested instantiation on the new inputs.

Rows (letters, constructor arguments and launch keys of tests/test_gpu_fused_chunks.py), each at every activation of ACTS:
  a  64 / 64 / 64            fused         k_fused_ws                        f  128 / 128 / 128          fused     k_fused_cs<128, 128>
  b  96 / 96 / 64            fused         k_fused_tile<96, 96>              g  128 / 64 / 128           fused     k_fused_cs<128, 64> + <64, 128>
  c  96 / 64 / 64            fused         k_fused_tile<96, 64> + <64, 96>   h  128 / 128 / 128 trained  rem-d128  k_fused_cs<128, 128>
  d  64 / 64 / 64 trained    rem-ws        k_fused_ws                        j  astlingen, 4 * 16 + 3 snapshots    fused-tiled, k_fused_ws
  e  64 / 64 / 64 trained    rem-split96   k_fused_tile<96, 96>              s  astlingen d = 64 / 128 trained, snapshot_remainder
  n  64 / 64 / 64 and 8 / 8 / 8, precision = 'fp32': the C entry (route 'entry'), no fused launch
a-h and n run on 600 / 720 with 3 snapshots (chunk 1 for every launch there).  Every (row, activation) asserts, in this order:
  1  route and launch: layer.last_route (and last_remainder on d, e, h, s) and the kernels uds_network_fused_launches names;
  2  parity: every element of both outputs finite (the inputs are views inside NaN-filled allocations) and within the bound of the
     fp64 reference, relative to max(1, max|ref|): TOL_BF16X3 = 1e-5 for a-j and s, the exact-fp32 layer bound 5e-6 for n;
  3  a second run gives the same bits.
test_multi_snapshot_chunks runs a-h again for hard_sigmoid at (chunk 3, tail 1), so the pipelined code of each ACT = -1
instantiation runs too.  test_chain runs a and f with autograd recording (route 'chain'): the forward at all five activations
against the same references at the per-operator split-bf16 bound 4e-5 (tests/test_gpu_train.py), the backward for linear, tanh and
sigmoid against autograd over the fp64 oracle (x, e and every parameter, a seeded signed upstream gradient; GRAD_TOL['GAT'] of the
tensor's largest gradient + 1e-7 of the largest of all, as test_c5_block_diagonal_batch_forward_backward).

Instantiations with ACT = -1 that now run: k_fused_ws (a, d, j, s), k_fused_tile<96, 96> (b, e), <96, 64> and <64, 96> (c),
k_fused_cs<128, 128> (f, h, s), <128, 64> and <64, 128> (g), each at chunk 1 and at chunk 3 with a ragged last chunk.
k_fused_tile<64, 64, -1> stays uncovered, for the reason tests/test_gpu_fused_chunks.py gives for <64, 64>.
Left out on purpose: relu and hard_sigmoid in the chain backward.  Their derivative jumps at a kink, and of ~10^5 pre-activations
some lie within fp32 rounding of it; DenseFn covers hard_sigmoid on its own in tests/test_gpu_train.py.

Measured on an MI355X (the tests print every figure): worst observed / allowed over both outputs, per row and activation.
              relu   linear  tanh   sigmoid  hard_sigmoid   hard_sigmoid at chunk 3 tail 1
  a           0.080  0.107   0.129  0.025    0.020          0.027  600/720   S=40
  b           0.056  0.089   0.093  0.024    0.022          0.024  600/720   S=31
  c           0.052  0.079   0.088  0.026    0.023          0.028  1200/1500 S=37 (both launches; on 600/720 its side launches need more than 64 snapshots)
  d           0.113  0.183   0.151  0.027    0.023          0.028  600/720   S=40
  e           0.090  0.136   0.151  0.026    0.022          0.028  600/720   S=31
  f           0.050  0.089   0.078  0.018    0.017          0.021  600/720   S=19
  g           0.042  0.079   0.084  0.020    0.017          0.019  600/720   S=37 and 49 (one per launch; this one case g reaches on 600/720)
  h           0.052  0.082   0.094  0.018    0.022          0.022  600/720   S=19
  j           0.063  0.092   0.111  0.021    0.017
  s d=64      0.041  0.058   0.081  0.020    0.016
  s d=128     0.033  0.056   0.049  0.013    0.012
  n d=64      0.013  0.014   0.023  0.018    0.012          (of 5e-6)
  n d=8       0.014  0.013   0.017  0.018    0.012          (of 5e-6)
  chain a, f  0.002  0.002   0.003  0.002    0.002          (of 4e-5: errors of 1e-7, the size of fp32 rounding)
  chain gradients, worst tensor: a 0.016 / 0.010 / 0.011, f 0.023 / 0.014 / 0.008 for linear / tanh / sigmoid
relu on the new parameters stays where rows a-h of tests/test_gpu_fused_chunks.py measured it (0.04-0.07 there, 0.04-0.11 here: the
largest are d and e, whose dense NodeEdge weights act_params raises), so LIM stayed at 4.0.  sigmoid and hard_sigmoid shrink the
error of the products with their slope of 0.25 and 0.2; linear passes it on whole, tanh where its argument is small.
No activation fails a row that relu passes, and no bound was raised: every test passed at its first run.
With the upper clamp of hard_sigmoid (its fminf) taken out of apply_act in a scratch build of the library, the 23 hard_sigmoid cases of
this file fail their parity check and the 60 others pass.
Wall time of this file: 5.2 s for its 83 tests, the slowest 0.5 s.
"""
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from tests import fused_act_util as FA
from tests import fused_chunk_util as FC
from tests.test_gpu_fused_chunks import dev, handle, launch_key, make_layer, same_bits      # noqa: F401 (dev is a fixture)
from tests.util import load_spatial_layer, nan_in

pytestmark = pytest.mark.gpu
TOL = FC.TOL_BF16X3
TOL_FP32 = 5e-6          # the exact-fp32 layer (tests/test_gpu_parity.py: TOL)
TOL_CHAIN = 4e-5         # per operator, split-bf16 (tests/test_gpu_train.py)
GRAD_TOL = 1e-3          # tests/test_gpu_train.py: GRAD_TOL['GAT']
ACTS, ROWS = FA.ACTS, FA.ROWS
GRAD_ACTS = ('linear', 'tanh', 'sigmoid')


def parity(test, case, outs, refs, tol=TOL):
    """Finite, and within tol of the reference relative to max(1, max|ref|); prints observed / allowed as Worst does."""
    worst = 0.0
    for side, out, ref in zip(('nodes', 'links'), outs, refs):
        assert bool(torch.isfinite(out).all()), '%s %s %s: non-finite output (an input was read outside its tensor?)' % (test, case, side)
        err = float((out.detach().double().cpu() - ref).abs().max())
        ratio = err / (tol * max(1.0, float(ref.abs().max())))
        print('fused-acts %s %s %s: observed / allowed = %.3f' % (test, case, side, ratio))
        worst = max(worst, ratio)
    assert worst <= 1.0, '%s %s: observed / allowed = %.3f' % (test, case, worst)
    return worst


def run_twice(layer, xs, es, route, remainder=None):
    ox, oe = layer(xs, es)
    assert layer.last_route == route, layer.last_route
    if remainder is not None:
        assert layer.last_remainder == remainder, layer.last_remainder
    return (ox, oe), lambda: same_bits(layer(xs, es), (ox, oe)) and layer.last_route == route


def row_layer(dev, row, name, act):
    r = ROWS[row]
    g, net = FC.graph(name), handle(name)
    p = FA.act_params(g, r['fx'], r['fe'], r['d'], trained=r['trained'])
    layer = make_layer(dev, g, p, r['fx'], r['fe'], r['d'], act, net)
    layer._ws_rem_ok = r['ws_rem_ok']
    return r, net, layer


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('row', sorted(ROWS))
def test_row(dev, row, act):
    """Rows a-h on 600 / 720, three snapshots, one per workgroup."""
    r, net, layer = row_layer(dev, row, FA.NET, act)
    g, p, x, e, ref = FA.case(FA.NET, r['fx'], r['fe'], r['d'], r['trained'], False, act, FA.S_ROW)
    launches = net.fused_launches(*r['query'])
    assert launch_key(launches) == r['expect'], launches
    assert all(_lib.fused_chunk(FA.S_ROW, l['n_tiles']) == 1 for l in launches), launches
    outs, again = run_twice(layer, nan_in(x, dev), nan_in(e, dev), r['route'], ('gemm', 'gemm') if r['trained'] else (None, None))
    assert net.fused_launches(*r['query']) == launches
    parity(row, act, outs, ref)
    assert again()


@pytest.mark.parametrize('row', sorted(ROWS))
def test_multi_snapshot_chunks(dev, row):
    """hard_sigmoid at (chunk 3, tail 1) for every launch of rows a-h, on the smallest network of FC.SIZES that reaches it within
    FC.S_CAP snapshots: the pipelined code of the ACT = -1 instantiations."""
    act, r = 'hard_sigmoid', ROWS[row]
    for n, m in FC.SIZES:
        name = '%d/%d' % (n, m)
        launches = handle(name).fused_launches(*r['query'])
        todo = [FC.find_S(l['n_tiles'], 3, 1) for l in launches]
        if launches and all(todo):
            break
    else:
        raise AssertionError('row %s: no network of %r reaches chunk 3 with a tail of 1 within %d snapshots' % (row, FC.SIZES, FC.S_CAP))
    r, net, layer = row_layer(dev, row, name, act)
    assert launch_key(launches) == r['expect'], launches
    g, p, x, e, ref = FA.case(name, r['fx'], r['fe'], r['d'], r['trained'], False, act, max(todo))
    for S in sorted(set(todo)):
        for l, s in zip(launches, todo):
            if s == S:
                assert _lib.fused_chunk(S, l['n_tiles']) == 3 and S % 3 == 1, (S, l)
        outs, again = run_twice(layer, nan_in(x[:S], dev), nan_in(e[:S], dev), r['route'], ('gemm', 'gemm') if r['trained'] else (None, None))
        assert net.fused_launches(*r['query']) == launches
        parity(row + ' chunk 3 tail 1', '%s %s S=%d' % (act, name, S), outs, (ref[0][:S], ref[1][:S]))
        assert again()


@pytest.mark.parametrize('act', ACTS)
def test_row_j_packed_tiles(dev, act):
    """astlingen, dense NodeEdge parameters without a remainder: four snapshots share a tile ('fused-tiled'), 16 packed groups and
    3 left-over snapshots one per tile."""
    g, net = FC.graph('astlingen'), handle('astlingen')
    _, p, x, e, ref = FA.case('astlingen', 64, 64, 64, False, True, act, FA.S_PACKED)
    layer = make_layer(dev, g, p, 64, 64, 64, act, net)
    assert layer.pack_factor() == 4 and FA.S_PACKED == 4 * 16 + 3
    rep = layer._replica(4)
    assert launch_key(rep.fused_launches(64, 64, 64)) == [FA.WS] and launch_key(net.fused_launches(64, 64, 64)) == [FA.WS]
    outs, again = run_twice(layer, nan_in(x, dev), nan_in(e, dev), 'fused-tiled', (None, None))
    assert layer._rep[0] == 4 and layer._rep[1] is rep
    parity('j', act, outs, ref)
    assert again()


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('d', [64, 128])
def test_row_s_snapshot_remainder(dev, d, act):
    """astlingen with a trained NodeEdge bias and snapshot_remainder set: the Dense epilogue of the one-launch remainder kernel, then
    the fused kernel's two."""
    g, net = FC.graph('astlingen'), handle('astlingen')
    _, p, x, e, ref = FA.case('astlingen', d, d, d, True, True, act, FA.S_ROW)
    layer = make_layer(dev, g, p, d, d, d, act, net)
    layer.snapshot_remainder = True
    assert launch_key(net.fused_launches(d, d, d)) == [FA.WS if d == 64 else FA.CS128]
    outs, again = run_twice(layer, nan_in(x, dev), nan_in(e, dev), 'rem-ws' if d == 64 else 'rem-d128', ('snapshot', 'snapshot'))
    assert layer.last_path == 'fused+remainder'
    parity('s-d%d' % d, act, outs, ref)
    assert again()


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('d', [64, 8])
def test_row_n_entry_fp32(dev, d, act):
    """precision = 'fp32': the C entry composes the layer from the exact-fp32 kernels; no fused launch."""
    g, net = FC.graph(FA.NET), handle(FA.NET)
    _, p, x, e, ref = FA.case(FA.NET, d, d, d, False, False, act, FA.S_ROW)
    layer = load_spatial_layer(U.SpatialLayer(g, d, act, fx=d, fe=d, sparse_params=True, net=net, precision='fp32'), p, dev)
    outs, again = run_twice(layer, nan_in(x, dev), nan_in(e, dev), 'entry', (None, None))
    assert layer.last_path == 'unfused'
    parity('n-d%d' % d, act, outs, ref, TOL_FP32)
    assert again()


PARAMS = {'dense_xe.kernel': 'xe_k', 'dense_xe.bias': 'xe_b', 'dense_ex.kernel': 'ex_k', 'dense_ex.bias': 'ex_b',
          'node_edge_n.weight': 'ne_n_v', 'node_edge_n.bias': 'ne_n_v', 'node_edge_e.weight': 'ne_e_v', 'node_edge_e.bias': 'ne_e_v',
          'gat_x.kernel': 'gx_k', 'gat_x.attn_kernel_self': 'gx_as', 'gat_x.attn_kernel_neighs': 'gx_an', 'gat_x.bias': 'gx_b',
          'gat_e.kernel': 'ge_k', 'gat_e.attn_kernel_self': 'ge_as', 'gat_e.attn_kernel_neighs': 'ge_an', 'gat_e.bias': 'ge_b'}


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('row', ['a', 'f'])
def test_chain(dev, row, act):
    """Rows a and f with autograd recording: every operator its own launch.  Forward at every activation; backward for linear,
    tanh and sigmoid (relu and hard_sigmoid: see the module docstring).  A support-only NodeEdge computes weight * 1 + bias on the
    support, so its weight and its bias both receive the gradient of the support values."""
    r, net, layer = row_layer(dev, row, FA.NET, act)
    g, p, x, e, ref = FA.case(FA.NET, r['fx'], r['fe'], r['d'], False, False, act, FA.S_ROW)
    layer.requires_grad_(True)
    xs, es = nan_in(x, dev).requires_grad_(True), nan_in(e, dev).requires_grad_(True)
    ox, oe = layer(xs, es)
    assert layer.last_route == 'chain' and layer.last_path == 'unfused'
    parity('chain-' + row, act, (ox, oe), ref, TOL_CHAIN)
    if act not in GRAD_ACTS:
        return
    gx, ge = FC.signed(51, *ref[0].shape), FC.signed(52, *ref[1].shape)
    (ox * gx.float().to(dev)).sum().add((oe * ge.float().to(dev)).sum()).backward()
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr, er = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    rx, re = FA.epilogue_ref(g, q, xr, er, act, act)
    ((rx * gx).sum() + (re * ge).sum()).backward()
    named = dict(layer.named_parameters())
    assert set(named) == set(PARAMS), sorted(named)
    pairs = [('x', xs.grad, xr.grad), ('e', es.grad, er.grad)] + [(n, named[n].grad, q[PARAMS[n]].grad) for n in sorted(named)]
    top = max(float(want.abs().max()) for _, _, want in pairs)
    worst = (0.0, None)
    for name, got, want in pairs:
        assert got is not None and bool(torch.isfinite(got).all()), name
        err = float((got.double().cpu().reshape(want.shape) - want).abs().max())
        lim = GRAD_TOL * float(want.abs().max()) + 1e-7 * top
        print('fused-acts chain-%s %s grad %s: observed / allowed = %.3f' % (row, act, name, err / lim))
        worst = max(worst, (err / lim, name))
    assert worst[0] <= 1.0, worst
