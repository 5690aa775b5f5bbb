"""GPU parity of the fused spatial kernels (k_fused_ws, k_fused_tile<FP, FS>, k_fused_cs<128, FP, FS>) with the fp64 oracles at
every snapshot-chunk length: chunks of 2, 3 and 4 or more snapshots, each with a ragged last chunk, on every route that reaches
them.  Chunk 1 is what the rest of the suite runs.

A case is a (chunk, tail) pair.  Its S comes from the tile count of the launch at run time (tests/fused_chunk_util.py), and every
case asserts, in this order:
  1  route and launch: layer.last_route, the kernel / variant / side mask that uds_network_fused_launches names, and that
     uds_fused_chunk gives exactly the claimed (chunk, tail) for the tiles of that launch;
  2  parity: every element of both outputs against the fp64 reference, TOL_BF16X3 = 1e-5 relative to max(1, max|ref|); the inputs
     are views inside NaN-filled allocations, so a read outside a tensor shows as a non-finite output;
  3  bit-equality with single-snapshot launches (S = 1: the chunk-1 path), every snapshot, no tolerance;
  4  a second run gives the same bits.

(3) per row: a, b, c, f, g run the layer itself on each snapshot alone.  d, e, h, i (a trained NodeEdge bias) compare the fused
kernel only: the remainder rows are computed once for all S snapshots and the single-snapshot launches are given their slices,
because the remainder GEMM's own bits do depend on S (its kernel and its cut along K follow S * h: remainder_plan in uds_hip.hip).
j has no such check: packed and unpacked tiles sum in different orders.

Inputs are signed (uniform in [-0.5, 0.5), different in every snapshot); tests/test_fused_chunk_math.py shows on the CPU that a
row taken from a neighbouring snapshot moves these references by more than 100 x the bound.

Still uncovered at chunk > 1: k_fused_tile<64, 64>.  It runs only on a network whose <64, 64> plan does not fit the
wave-specialised kernel (plan bit 1 without bit 32).  The hub network of test_hub_network_rows_with_more_than_16_neighbours is
not such a plan (its plan bits are 33 on an MI355X: k_fused_ws takes it), nor is any network used here, so there is no row k.

Measured on an MI355X (UDS_TOL_REPORT=1; the tests print every figure): worst observed / allowed per test, its network and case.
The split-bf16 arithmetic stays far from the bound with these inputs, so the total is bounded by 1e-5 and nothing else.
  a relu   600/720     0.070  S=40 chunk 3 tail 1, nodes        f relu   600/720     0.046  S=19 chunk 3 tail 1, nodes
  a tanh   600/720     0.065  S=40 chunk 3 tail 1, nodes        f tanh   600/720     0.049  S=20 chunk 3 tail 2, nodes
  b        600/720     0.065  S=46 chunk 4 tail 2, nodes        g        1200/1500   0.044  S=16 link launch chunk 3 tail 1, links
  c        1200/1500   0.069  S=20 node launch chunk 2, nodes   h        600/720     0.040  S=29 chunk 4 tail 1, nodes
  d        600/720     0.056  S=20 chunk 2 tail 0, nodes        i d=64   astlingen   0.061  S=897 chunk 8 tail 1, nodes
  e        600/720     0.061  S=31 chunk 3 tail 1, nodes        i d=128  astlingen   0.039  S=897 chunk 8 tail 1, links
  j        astlingen   0.061  S=519 = 4 * 129 + 3, chunk 2 tail 1, nodes
Tiles per launch there: 600/720 has 13 (<64, 64>), 17 (<96, 96>) and 26 (<128, 128>); rows c and g moved to 1200/1500 (14 + 15
and 24 + 34 tiles: on 600/720 a side launch of 6 or 7 tiles needs up to 127 snapshots); astlingen has 2, packed by four also 2.
Wall time of this file: 5.2 s for its 13 tests, the slowest 0.6 s.
"""
import functools
import time

import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from tests import fused_chunk_util as FC
from tests import util
from tests.util import load_spatial_layer, nan_in

pytestmark = pytest.mark.gpu
TOL = FC.TOL_BF16X3

WS = ('k_fused_ws', 64, 64, 3)
_HANDLES = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


def handle(name):
    if name not in _HANDLES:
        _HANDLES[name] = _lib.NetworkHandle(FC.graph(name))
    return _HANDLES[name]


def launch_key(launches):
    return [(l['kernel'], l['fp'], l['fs'], l['side_mask']) for l in launches]


@functools.lru_cache(maxsize=None)
def plan(fx, fe, d):
    """The smallest synthetic network on which every launch of a layer (fx, fe, d) reaches every case with S <= S_CAP ->
    (graph name, launches, cases per launch)."""
    seen = []
    for n, e in FC.SIZES:
        name = '%d/%d' % (n, e)
        launches = handle(name).fused_launches(fx, fe, d)
        cases = [FC.cases_for(l['n_tiles']) for l in launches]
        seen.append((name, [l['n_tiles'] for l in launches], cases))
        if launches and all(c is not None for cs in cases for c in cs):
            return name, launches, cases
    raise AssertionError('no network of %r reaches every chunk shape within %d snapshots: %r' % (FC.SIZES, FC.S_CAP, seen))


class Worst:
    """The largest observed / allowed ratio of a test, with its case; printed for the docstring above."""

    def __init__(self, test):
        self.test, self.ratio, self.case, self.t0 = test, 0.0, None, time.time()

    def parity(self, case, outs, refs):
        for side, out, ref in zip(('nodes', 'links'), outs, refs):
            assert bool(torch.isfinite(out).all()), '%s %s: non-finite output (an input was read outside its tensor?)' % (case, side)
            err = float((out.double().cpu() - ref).abs().max())
            ratio = err / (TOL * max(1.0, float(ref.abs().max())))
            print('fused-chunks %s %s %s: observed / allowed = %.3f' % (self.test, case, side, ratio))
            if ratio > self.ratio:
                self.ratio, self.case = ratio, '%s %s' % (case, side)
            util.close(out, ref, TOL)

    def done(self):
        print('fused-chunks WORST %s: %.3f at %s (%.1f s)' % (self.test, self.ratio, self.case, time.time() - self.t0))


def make_layer(dev, g, p, fx, fe, d, act, net=None):
    layer = U.SpatialLayer(g, d, act, fx=fx, fe=fe, sparse_params='ne_n_v' in p, net=net, precision='bf16x3')
    return load_spatial_layer(layer, p, dev)


def same_bits(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def singles_of_layer(layer, xs, es, route):
    """Every snapshot through the layer alone (S = 1: the chunk-1 path), stacked."""
    outs = []
    for s in range(xs.shape[0]):
        outs.append(layer(xs[s:s + 1], es[s:s + 1]))
        assert layer.last_route == route
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def fused_launcher(layer, net, route, xs, es):
    """The fused launch of a remainder route as the layer makes it (SpatialLayer._fused_rem / _rem_split96), with the remainder rows
    of all S snapshots computed once -> (launch(lo, hi) for the snapshots [lo, hi))."""
    ne = (layer.node_edge_n.support_values(), layer.node_edge_e.support_values())
    assert ne[0][1] is not None and ne[1][1] is not None                 # a remainder on both sides
    rem_n, rem_e = layer._remainders(ne, xs, es)
    if route == 'rem-split96':
        p = layer._params(ne)
        packed, aug = layer._packed_weights(p, 96, 96, remainder=True)
        net.prepare(96, 96)
        p, names = dict(p, packed=packed, **aug), ('xb', 'eb')
    else:
        p, names = layer._params(ne, xs.shape[-1], es.shape[-1]), ('rem_x', 'rem_e')
    return lambda lo, hi: layer._launch(net, p, xs[lo:hi], es[lo:hi], **{names[0]: rem_n[lo:hi], names[1]: rem_e[lo:hi]})


def run_cases(dev, worst, layer, net, g, p, query, expect_route, expect, todo, act='relu', bit_equal='layer', dense_oracle=False,
              split=False):
    """todo: [(launch index, S, chunk, tail)].  One forward per distinct S; the reference is computed once, for the largest S."""
    fx, fe = p['ex_k'].shape[0], p['xe_k'].shape[0]
    launches = net.fused_launches(*query)
    assert launch_key(launches) == expect, launches
    S_max = max(t[1] for t in todo)
    x_all, e_all = FC.inputs(g, fx, fe, S_max)
    rx_all, re_all = FC.reference(g, p, x_all, e_all, act, dense_oracle=dense_oracle)
    for S in sorted({t[1] for t in todo}):
        claims = [t for t in todo if t[1] == S]
        case = 'S=%d %s' % (S, ' '.join('launch%d:chunk%d+%d' % (i, c, t) for i, _, c, t in claims))
        xs, es = nan_in(x_all[:S], dev), nan_in(e_all[:S], dev)
        ox, oe = layer(xs, es)
        # 1: route and launch
        assert layer.last_route == expect_route, (case, layer.last_route)
        assert net.fused_launches(*query) == launches
        for i, _, chunk, tail in claims:
            got = _lib.fused_chunk(S, launches[i]['n_tiles'])
            assert (got, S % got) == (chunk, tail) and chunk > 1, (case, launches[i], got)
        # 2: parity
        worst.parity(case, (ox, oe), (rx_all[:S], re_all[:S]))
        # 3: every snapshot alone gives the same bits
        if bit_equal == 'layer':
            assert same_bits(singles_of_layer(layer, xs, es, expect_route), (ox, oe)), case
        elif bit_equal == 'rem':
            launch = fused_launcher(layer, net, expect_route, xs, es)
            assert same_bits(launch(0, S), (ox, oe)), case                  # the launch the layer made
            one = [launch(s, s + 1) for s in range(S)]
            assert same_bits((torch.cat([o[0] for o in one]), torch.cat([o[1] for o in one])), (ox, oe)), case
        if split:       # 96-wide rows given as 64 + 32 columns from two tensors: the same bits as the concatenated call
            xa, xb = (nan_in(x_all[:S, :, :64], dev), nan_in(x_all[:S, :, 64:], dev)) if fx == 96 else (xs, None)
            ea, eb = (nan_in(e_all[:S, :, :64], dev), nan_in(e_all[:S, :, 64:], dev)) if fe == 96 else (es, None)
            assert same_bits(layer(xa, ea, xb, eb), (ox, oe)) and layer.last_route == expect_route, case
        # 4: repeatable
        assert same_bits(layer(xs, es), (ox, oe)), case


def run_row(dev, test, fx, fe, d, expect_route, expect, act='relu', trained=False, ws_rem_ok=None, query=None, bit_equal='layer',
            split=False):
    """Rows a-h: SHAPES and the long chunk for every launch of the layer, on the network `plan` picks."""
    query = query or (fx, fe, d)
    name, launches, cases = plan(*query)
    g, net = FC.graph(name), handle(name)
    p = FC.params(g, fx, fe, d, dense=trained, trained=trained)
    layer = make_layer(dev, g, p, fx, fe, d, act, net)
    layer._ws_rem_ok = ws_rem_ok
    todo = [(i,) + c for i, cs in enumerate(cases) for c in cs]
    for i in range(len(launches)):                           # every launch sees chunks of 2, 3 and >= 4 and ragged last chunks
        mine = [t for t in todo if t[0] == i]
        assert [t[2:] for t in mine[:4]] == list(FC.SHAPES) and mine[4][2] >= FC.LONG_CHUNK and mine[4][3] > 0
    worst = Worst(test + ' ' + name)
    run_cases(dev, worst, layer, net, g, p, query, expect_route, expect, todo, act, bit_equal, split=split)
    worst.done()


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_row_a_ws(dev, act):
    """d = 64, 64 / 64: k_fused_ws, relu compiled in and the run-time activation (ACT = -1)."""
    run_row(dev, 'a-' + act, 64, 64, 64, 'fused', [WS], act=act)


def test_row_b_tile_96_96(dev):
    run_row(dev, 'b', 96, 96, 64, 'fused', [('k_fused_tile', 96, 96, 3)])


def test_row_c_tile_96_64_pair(dev):
    """fx = 96, fe = 64: node tiles <96, 64> and link tiles <64, 96>, each launch with its own tiles and chunk; the split call."""
    run_row(dev, 'c', 96, 64, 64, 'fused', [('k_fused_tile', 96, 64, 1), ('k_fused_tile', 64, 96, 2)], split=True)


def test_row_d_rem_ws(dev):
    run_row(dev, 'd', 64, 64, 64, 'rem-ws', [WS], trained=True, bit_equal='rem')


def test_row_e_rem_split96(dev):
    """The remainder as 32 extra input columns of k_fused_tile<96, 96>."""
    run_row(dev, 'e', 64, 64, 64, 'rem-split96', [('k_fused_tile', 96, 96, 3)], trained=True, ws_rem_ok=False, query=(96, 96, 64),
            bit_equal='rem')


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_row_f_cs_128(dev, act):
    run_row(dev, 'f-' + act, 128, 128, 128, 'fused', [('k_fused_cs', 128, 128, 3)], act=act)


def test_row_g_cs_128_64_pair(dev):
    run_row(dev, 'g', 128, 64, 128, 'fused', [('k_fused_cs', 128, 64, 1), ('k_fused_cs', 64, 128, 2)])


def test_row_h_rem_d128(dev):
    run_row(dev, 'h', 128, 128, 128, 'rem-d128', [('k_fused_cs', 128, 128, 3)], trained=True, bit_equal='rem')


@pytest.mark.parametrize('d', [64, 128])
def test_row_i_small_network_long_chunk(dev, d):
    """astlingen with a trained bias, the production shape: few tiles, many snapshots -- the smallest S with a chunk of 8 or more
    snapshots and a ragged last chunk."""
    g, net = FC.graph('astlingen'), handle('astlingen')
    p = FC.params(g, d, d, d, dense=True, trained=True)
    layer = make_layer(dev, g, p, d, d, d, 'relu', net)
    launches = net.fused_launches(d, d, d)
    assert len(launches) == 1
    S, chunk, tail = FC.find_long(launches[0]['n_tiles'], 8, cap=4096)
    assert chunk >= 8 and tail > 0
    worst = Worst('i-d%d astlingen' % d)
    run_cases(dev, worst, layer, net, g, p, (d, d, d), 'rem-ws' if d == 64 else 'rem-d128', [WS if d == 64 else ('k_fused_cs', 128, 128, 3)],
              [(0, S, chunk, tail)], bit_equal='rem', dense_oracle=True)
    worst.done()


def test_row_j_packed_tiles(dev):
    """astlingen, d = 64, no remainder: four snapshots share a tile ('fused-tiled'); packed groups at chunk 2 and at chunk 3, plus 3
    left-over snapshots (one per tile, chunk 1)."""
    g = FC.graph('astlingen')
    p = FC.params(g, 64, 64, 64, dense=True)
    layer = make_layer(dev, g, p, 64, 64, 64, 'relu', handle('astlingen'))
    assert layer.pack_factor() == 4
    rep = layer._replica(4)
    launches = rep.fused_launches(64, 64, 64)
    assert launch_key(launches) == [WS], launches
    tiles = launches[0]['n_tiles']
    groups = [FC.find_S(tiles, 2, 1, cap=4096), FC.find_S(tiles, 3, 1, cap=4096) or FC.find_S(tiles, 3, 2, cap=4096)]
    assert all(groups), (tiles, groups)
    todo = [(0, 4 * G + 3, _lib.fused_chunk(G, tiles), G % _lib.fused_chunk(G, tiles)) for G in groups]
    assert [t[2] for t in todo] == [2, 3] and all(t[3] for t in todo)
    S_max = max(t[1] for t in todo)
    x_all, e_all = FC.inputs(g, 64, 64, S_max)
    rx, re = FC.reference(g, p, x_all, e_all, dense_oracle=True)
    worst = Worst('j astlingen x 4')
    for _, S, chunk, tail in todo:
        case = 'S=%d=4*%d+3 chunk%d+%d' % (S, S // 4, chunk, tail)
        xs, es = nan_in(x_all[:S], dev), nan_in(e_all[:S], dev)
        ox, oe = layer(xs, es)
        assert layer.last_route == 'fused-tiled' and layer._rep[0] == 4 and layer._rep[1] is rep, case
        assert rep.fused_launches(64, 64, 64) == launches and _lib.fused_chunk(S // 4, tiles) == chunk and (S // 4) % chunk == tail
        worst.parity(case, (ox, oe), (rx[:S], re[:S]))
        assert same_bits(layer(xs, es), (ox, oe)), case
    worst.done()
