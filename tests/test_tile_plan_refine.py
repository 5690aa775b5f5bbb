"""The row-by-row refinement of the tile plans (csrc/tile_plan.hpp: TileRefiner), checked on the host (no GPU).

After the agglomeration the planner moves single rows between tiles (fill / boundary moves) and dissolves the smallest tiles
into their neighbours.  Every plan must still be what the kernels rely on -- check_plan of tests/test_tile_plan.py: each row
owned once, halo = exactly the outside neighbours, secondary rows = exactly the incident ones, own rows by descending degree,
local indices that resolve -- within the limits it was given, and it must never have MORE tiles than the planner had before the
refinement existed.  Those earlier counts are the constants below (a run of the parent commit)."""
import numpy as np
import pytest

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from tests.test_tile_plan import check_plan

# (t_node, t_link, p_limit, q_limit) of tests/test_tile_plan.py::test_plan_on_real_networks, then the limits the d = 64 and the
# d = 128 kernels plan with
LIMITS = ((128, 120, 0, 0), (48, 48, 64, 80), (16, 12, 0, 0), (1, 1, 0, 0), (40, 40, 16, 16), (128, 128, 128, 208), (64, 64, 64, 128))
PARENT_TILES = {
    'astlingen': (2, 2, 6, 59, 6, 2, 2),
    'shunqing': (4, 6, 24, 244, 50, 3, 5),
    'chaohu': (4, 8, 29, 281, 29, 4, 6),
    'hague': (5, 10, 43, 420, 47, 4, 8),
    'RedChicoSur': (10, 21, 87, 887, 89, 8, 16),
}
# synthetic networks (nodes, links): tiles of the parent at (128, 128, 128, 208) and at (64, 64, 64, 128)
PARENT_SYNTHETIC = {(10000, 12000): (202, 445), (2000, 2500): (43, 94)}
HEADLINE_TILES = 191      # 85 node + 106 link tiles (parent: 89 + 113)


def within_limits(hdr, p_lim, q_lim):
    multi = hdr[:, 0] > 1                                    # a single row that exceeds the limits on its own stays as it is
    return bool((hdr[multi, 1] <= p_lim).all() and (hdr[multi, 2] <= q_lim).all())


@pytest.mark.parametrize('name', sorted(PARENT_TILES))
def test_shipped_networks(networks, name):
    net = networks[name]
    g = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    for (t_node, t_link, p_lim, q_lim), parent in zip(LIMITS, PARENT_TILES[name]):
        hdr, pool, caps = _lib.tile_plan(g, t_node, t_link, p_lim, q_lim)
        check_plan(g, hdr, pool, caps, t_node, t_link)
        assert len(hdr) <= parent, (name, t_node, t_link, p_lim, q_lim, len(hdr), parent)
        if p_lim:
            assert within_limits(hdr, p_lim, q_lim)
        else:
            assert caps['refine'] == dict(fill=0, move=0, dissolve=0)      # no limits, no agglomeration: nothing to refine


def test_isolated_rows_and_self_loop_link():
    e = np.array([[0, 1], [1, 1], [1, 2], [4, 2]])
    g = U.DrainageGraph.from_edges(e, n_node=6)            # nodes 3 and 5 isolated, link 1 self-referential
    for lim in ((4, 4, 0, 0), (4, 4, 4, 4), (3, 3, 4, 4)):
        hdr, pool, caps = _lib.tile_plan(g, *lim)
        check_plan(g, hdr, pool, caps, lim[0], lim[1])
        if lim[2]:
            assert within_limits(hdr, lim[2], lim[3])


def test_small_tiles_fill_move_and_dissolve_all_fire():
    """600 nodes / 720 links at limits (32, 48): about sixty tiles of about twenty rows, small enough for every step to act."""
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(600, 720, 0))
    hdr, pool, caps = _lib.tile_plan(g, 32, 32, 32, 48)
    check_plan(g, hdr, pool, caps, 32, 32)
    assert within_limits(hdr, 32, 48)
    assert caps['refine']['fill'] > 0 and caps['refine']['move'] > 0 and caps['refine']['dissolve'] > 0, caps['refine']
    assert len(hdr) <= 61                                   # the parent's count
    again = _lib.tile_plan(g, 32, 32, 32, 48)
    assert np.array_equal(again[0], hdr) and np.array_equal(again[1], pool) and again[2] == caps      # deterministic


@pytest.mark.parametrize('size', sorted(PARENT_SYNTHETIC))
def test_synthetic_networks_never_more_tiles(size):
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(size[0], size[1], 0))
    for (t, p_lim, q_lim), parent in zip(((128, 128, 208), (64, 64, 128)), PARENT_SYNTHETIC[size]):
        hdr, pool, caps = _lib.tile_plan(g, t, t, p_lim, q_lim)
        assert len(hdr) <= parent, (size, t, len(hdr), parent)
        assert within_limits(hdr, p_lim, q_lim) and (hdr[:, 0] <= t).all()
        for side, n in ((0, g.n_node), (1, g.n_edge)):
            assert hdr[hdr[:, 6] == side, 0].sum() == n


def test_headline_plan_crosses_the_three_round_cliff():
    """At most 192 tiles: uds_fused_chunk then picks chunks of 15 snapshots for S = 60, 4 x tiles <= 768 workgroups, three rounds
    of 256 instead of four."""
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(10000, 12000, 0))
    hdr, pool, caps = _lib.tile_plan(g, 128, 128, 128, 208)
    check_plan(g, hdr, pool, caps, 128, 128)
    assert within_limits(hdr, 128, 208)
    assert len(hdr) == HEADLINE_TILES
    assert ((hdr[:, 6] == 0).sum(), (hdr[:, 6] == 1).sum()) == (85, 106)
    assert _lib.fused_chunk(60, len(hdr)) == 15
    assert 4 * len(hdr) <= 3 * 256
