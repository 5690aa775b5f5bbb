"""GPU parity of k_fused_ws on the shapes at which its workgroup set-up can go wrong.

The set-up issues its loads in two round trips: {tile block, attention vectors, the team's weights, every lane's row ids read
straight from the block in global memory}, one barrier, then {first-snapshot rows, NodeEdge gather incl. the overflow list, the
remainder rows of a trained bias} with the static P3 state computed underneath; the NodeEdge values are ordered in front of
their only reader by the first barrier of the snapshot pipeline.  What can break is an id read with a clamped index, a wave
with no block at all, a gather that has not landed when the aggregate reads it, and a hand-counted wait in the first
intervals -- so the shapes are small ones:

  1  waves without work: 6 nodes, 4 links (nodes 3 and 5 isolated, link 1 a self loop), two tiles of 4 and 6 rows with 4 and 3
     secondary rows: Y waves 1-3 and X waves 1-3 have no block, every row id they read is a clamped one;
  2  astlingen (30 / 29 rows): one partly filled 32-row block per side;
  3  synthetic 600/720 (13 tiles): full 128-row tiles beside tiles of 44-63 rows;
  4  a 20-leaf star: link rows with 19 neighbours (ELL_FLAG_LONG_ROWS), node 0 with 20 incident links (ELL_FLAG_INC_OVF): the
     overflow gather;
  5  case 3 with a trained dense NodeEdge bias (route 'rem-ws'): the remainder rows join the second trip.  The fused kernel only
     is compared (rows d / e / h of tests/test_gpu_fused_chunks.py say why).

Every case runs S = 1, 2, 3, 5 and asserts, in this order: the launch is k_fused_ws; every element within TOL_BF16X3 of the fp64
reference and finite (the inputs are views inside NaN-filled allocations); every snapshot bit-equal to its S = 1 launch; a second
run gives the same bits.

S = 1, 2, 3, 5 do NOT enter the snapshot loops with 1, 2, 3 and more intervals: uds_fused_chunk gives chunk 1 for every one of
them on these tile counts (few workgroups: a longer chunk buys nothing), so each workgroup sees one snapshot.  The loops are
entered with 2, 3 and >= 4 snapshots by the further S of `long_S`: the smallest S at which the library's own chunk function
gives chunk 2, chunk 3 and a chunk >= 4 with a ragged last chunk (129 / 257 / 385 on a two-tile plan).  On the three small
networks the layer would route those S to 'fused-tiled' (copies of the network side by side: another graph), so there the fused
launch is made as the layer makes it below that threshold (SpatialLayer._fused); the route assertion is made where the layer
itself takes the route.

Measured on an MI355X (the tests print every figure): the worst observed / allowed ratio is 0.122 (star, S = 385, nodes), the
other cases stay below 0.08; all five tests take 1.2 s together, the slowest 0.5 s.
"""
import functools

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from tests import fused_chunk_util as FC
from tests import util
from tests.util import load_spatial_layer, nan_in

pytestmark = pytest.mark.gpu
TOL = FC.TOL_BF16X3
WS = [('k_fused_ws', 64, 64, 3)]
SHORT_S = (1, 2, 3, 5)
ISOLATED = 'isolated'      # the graph of tests/test_tile_plan.py::test_plan_with_isolated_rows_and_self_loop_link
STAR = 'star20'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == ISOLATED:
        return U.DrainageGraph.from_edges(np.array([[0, 1], [1, 1], [1, 2], [4, 2]]), n_node=6)
    if name == STAR:
        return U.DrainageGraph.from_edges(np.array([[i, 0] for i in range(1, 21)]), n_node=21)
    return FC.graph(name)


@functools.lru_cache(maxsize=None)
def handle(name):
    return _lib.NetworkHandle(graph(name))


def long_S(tiles):
    """The smallest S with chunk 2, chunk 3 and a chunk >= 4, each with a ragged last chunk."""
    c2 = FC.find_S(tiles, 2, 1, cap=4096)
    c3 = FC.find_S(tiles, 3, 1, cap=4096) or FC.find_S(tiles, 3, 2, cap=4096)
    c4 = FC.find_long(tiles, 4, cap=4096)
    assert c2 and c3 and c4, (tiles, c2, c3, c4)
    assert (_lib.fused_chunk(c2, tiles), _lib.fused_chunk(c3, tiles)) == (2, 3) and c4[1] >= 4 and c4[2] > 0
    return c2, c3, c4[0]


def same_bits(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def parity(case, outs, refs):
    for side, out, ref in zip(('nodes', 'links'), outs, refs):
        assert bool(torch.isfinite(out).all()), '%s %s: non-finite output (an input was read outside its tensor?)' % (case, side)
        err = float((out.double().cpu() - ref).abs().max())
        print('ws-setup %s %s: observed / allowed = %.3f' % (case, side, err / (TOL * max(1.0, float(ref.abs().max())))))
        util.close(out, ref, TOL)


def run_case(dev, name, trained=False):
    g, net = graph(name), handle(name)
    p = FC.params(g, 64, 64, 64, dense=trained, trained=trained)
    layer = U.SpatialLayer(g, 64, 'relu', fx=64, fe=64, sparse_params=not trained, net=net, precision='bf16x3')
    layer = load_spatial_layer(layer, p, dev)
    route = 'rem-ws' if trained else 'fused'
    launches = net.fused_launches(64, 64, 64)
    assert [(l['kernel'], l['fp'], l['fs'], l['side_mask']) for l in launches] == WS, launches      # 1: the launch is k_fused_ws
    tiles = launches[0]['n_tiles']
    todo = SHORT_S + long_S(tiles)
    assert [_lib.fused_chunk(S, tiles) for S in SHORT_S] == [1, 1, 1, 1]       # (the docstring: these S run chunk 1)
    x_all, e_all = FC.inputs(g, 64, 64, max(todo))
    rx, re = FC.reference(g, p, x_all, e_all, 'relu', dense_oracle=trained and g.n_node <= 64)
    assert bool(torch.isfinite(rx).all()) and bool(torch.isfinite(re).all())
    ne = (layer.node_edge_n.support_values(), layer.node_edge_e.support_values())
    for S in todo:
        case = '%s S=%d chunk %d' % (name, S, _lib.fused_chunk(S, tiles))
        xs, es = nan_in(x_all[:S], dev), nan_in(e_all[:S], dev)
        if trained:
            # the remainder rows of all S snapshots are computed once; the single-snapshot launches get their slices (the remainder
            # GEMM's own bits depend on S)
            assert ne[0][1] is not None and ne[1][1] is not None
            rem_n, rem_e = layer._remainders(ne, xs, es)
            pr = layer._params(ne, 64, 64)
            launch = lambda lo, hi: layer._launch(net, pr, xs[lo:hi], es[lo:hi], rem_x=rem_n[lo:hi], rem_e=rem_e[lo:hi])
        else:
            launch = lambda lo, hi: layer._fused(ne, xs[lo:hi], es[lo:hi], None, None)
        taken, _ = layer.route(64, 0, 64, 0, S, lambda fx, fe: net.fused_bits(fx, fe), remainder=trained)
        if taken == route:                      # 1: the layer itself takes the route and makes this launch
            out = layer(xs, es)
            assert layer.last_route == route, (case, layer.last_route)
            assert same_bits(launch(0, S), out), case
        else:                                   # a small network at S >= 16 x pack_factor: see the docstring
            assert taken == 'fused-tiled' and S not in SHORT_S, (case, taken)
            out = launch(0, S)
        assert net.fused_launches(64, 64, 64) == launches
        parity(case, out, (rx[:S], re[:S]))                                             # 2
        one = [launch(s, s + 1) for s in range(S)]                                      # 3: every snapshot alone, the same bits
        assert same_bits((torch.cat([o[0] for o in one]), torch.cat([o[1] for o in one])), out), case
        assert same_bits(launch(0, S), out), case                                       # 4: repeatable


def test_waves_without_work(dev):
    run_case(dev, ISOLATED)


def test_partly_filled_block(dev):
    run_case(dev, 'astlingen')


def test_full_and_short_tiles(dev):
    run_case(dev, '600/720')


def test_star_long_rows_and_overflow_gather(dev):
    run_case(dev, STAR)


def test_trained_bias_remainder_rows(dev):
    run_case(dev, '600/720', trained=True)
