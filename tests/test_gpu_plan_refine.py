"""GPU parity of the fused d = 64 spatial layer on REFINED tile plans (csrc/tile_plan.hpp: TileRefiner).

The refinement moves single rows between tiles after the agglomeration, so tiles are no longer unions of subtree clusters: own
rows of one tile may lie apart, halos are what the boundary moves left.  The kernel must not care -- per-row arithmetic follows
the row's own CSR lists -- and this is checked where the plan has several tiles per side and where the refinement did something:

  400/480      synthetic, 4 node + 5 link tiles at the headline limits (128 own / 128 primary / 208 secondary rows)
  RedChicoSur  the largest shipped network (443 / 444 rows), 4 + 4 tiles

One SpatialLayer forward at d = 64 with S = 3 and S = 5 snapshots each: the launch is k_fused_ws, every element is finite and
within TOL_BF16X3 of the fp64 oracle (inputs are views inside NaN-filled allocations), and a second run gives the same bits.
No shape of the benchmark is used."""
import functools
import json
import os

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
SNAPSHOTS = (3, 5)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    _lib.load()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def graph(name):
    if '/' in name:
        return FC.graph(name)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'networks.json')) as fh:
        net = json.load(fh)[name]
    return U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])


@functools.lru_cache(maxsize=None)
def case(name):
    """Graph, parameters, inputs of the longest S and their fp64 reference: computed once, shared by both S."""
    g = graph(name)
    p = FC.params(g, 64, 64, 64)
    x, e = FC.inputs(g, 64, 64, max(SNAPSHOTS))
    rx, re = FC.reference(g, p, x, e, 'relu')
    assert bool(torch.isfinite(rx).all()) and bool(torch.isfinite(re).all())
    return g, p, x, e, rx, re


@pytest.mark.parametrize('S', SNAPSHOTS)
@pytest.mark.parametrize('name', ['400/480', 'RedChicoSur'])
def test_layer_on_refined_plan(dev, name, S):
    g, p, x, e, rx, re = case(name)
    hdr, _, caps = _lib.tile_plan(g, 128, 128, 128, 208)
    assert min((hdr[:, 6] == 0).sum(), (hdr[:, 6] == 1).sum()) >= 3             # several tiles per side
    assert caps['refine']['fill'] + caps['refine']['move'] > 0                  # ... which the refinement has touched
    net = _lib.NetworkHandle(g)
    layer = load_spatial_layer(U.SpatialLayer(g, 64, 'relu', fx=64, fe=64, sparse_params=True, net=net, precision='bf16x3'), p, dev)
    launches = net.fused_launches(64, 64, 64)
    assert [(l['kernel'], l['fp'], l['fs'], l['side_mask']) for l in launches] == [('k_fused_ws', 64, 64, 3)], launches
    assert launches[0]['n_tiles'] == len(hdr)                                   # the layer runs the plan checked above
    xs, es = nan_in(x[:S], dev), nan_in(e[:S], dev)
    out = layer(xs, es)
    assert layer.last_route == 'fused', layer.last_route
    for side, o, ref in zip(('nodes', 'links'), out, (rx[:S], re[:S])):
        assert bool(torch.isfinite(o).all()), '%s S=%d %s: non-finite output' % (name, S, side)
        err = float((o.double().cpu() - ref).abs().max())
        print('plan-refine %s S=%d %s: observed / allowed = %.3f' % (name, S, side, err / (TOL * max(1.0, float(ref.abs().max())))))
        util.close(o, ref, TOL)
    again = layer(xs, es)
    assert all(torch.equal(a, b) for a, b in zip(again, out))
