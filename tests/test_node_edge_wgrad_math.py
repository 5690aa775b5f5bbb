"""CPU checks of the uds_node_edge_wgrad cases (tests/node_edge_wgrad_util.py): the Python restatement of the plan is the library's
host plan, every instantiation and both padded and unpadded h are reached, the pieces cover 0..S exactly once, and the fp64
references carry signal.  No GPU: the plan and the workspace size are host functions."""
import pytest

from gnn_uds_amd import _lib
from tests import node_edge_wgrad_util as NU


@pytest.mark.parametrize('case', NU.CASES, ids=NU.case_id)
def test_restatement_is_the_library_plan(case):
    R, M, S, h = case
    p = NU.plan(*case)
    assert _lib.node_edge_wgrad_plan(*case) == p and p['ksteps'] in (1, 2)
    assert _lib.load().uds_node_edge_wgrad_workspace_bytes(*case) == 4 * p['pieces'] * R * M


def test_plan_over_a_grid_of_shapes():
    for R in (1, 63, 64, 65, 444, 5000):
        for M in (1, 29, 128, 443):
            for S in (0, 1, 7, 8, 9, 16, 17, 640, 16384):
                for h in (4, 28, 32, 36, 64):
                    assert _lib.node_edge_wgrad_plan(R, M, S, h) == NU.plan(R, M, S, h), (R, M, S, h)


@pytest.mark.parametrize('case', NU.REFUSALS + [(3, 0, 1, 32), (3, 3, -1, 32), (3, 3, 1, 0), (3, 3, (1 << 24) + 1, 32), (1 << 25, 1, 1, 32),
                                                (1 << 16, 1 << 17, 1, 32)])
def test_refused_shapes(case):
    assert NU.plan(*case) == NU.REFUSED == _lib.node_edge_wgrad_plan(*case)
    assert _lib.load().uds_node_edge_wgrad_workspace_bytes(*case) == 0
    assert not _lib.node_edge_wgrad_supported(6) and not _lib.node_edge_wgrad_supported(68) and _lib.node_edge_wgrad_supported(32)


def test_every_route_is_reached():
    plans = [NU.plan(*c) for c in NU.CASES]
    assert {(p['ksteps'], p['padded']) for p in plans} == {(1, False), (1, True), (2, False), (2, True)}
    assert {min(p['pieces'], 2) for p in plans} == {1, 2}                        # one piece, and a split reduction
    assert any(p['spp'] > NU.MIN_SPP for p in plans)                              # a piece length set by S, not by the minimum
    assert any(-(-c[0] // NU.TILE) > 1 and -(-c[1] // NU.TILE) > 1 for c in NU.CASES)      # several tiles both ways
    assert any(c[0] % 16 and c[1] % 16 for c in NU.CASES)                        # ragged 16-row blocks both ways


def test_split_cases_are_what_they_claim():
    R, M, S, h = NU.CASES[7]
    assert NU.plan(R, M, S, h)['pieces'] == 2 and NU.plan(R, M, S - 1, h)['pieces'] == 1
    for c, n in ((NU.CASES[8], 3), (NU.CASES[9], 2)):
        pc = NU.pieces_of(*c)
        assert len(pc) == n and pc[-1][1] - pc[-1][0] == 1


@pytest.mark.parametrize('case', NU.CASES, ids=NU.case_id)
def test_pieces_cover_the_snapshots_once(case):
    S = case[2]
    covered = [s for a, b in NU.pieces_of(*case) for s in range(a, b)]
    assert covered == list(range(S))
    assert all(b > a for a, b in NU.pieces_of(*case))


@pytest.mark.parametrize('case', NU.CASES, ids=NU.case_id)
def test_references_carry_signal(case):
    p = NU.inputs(case)
    R, M, S, h = case
    assert p['ref'].shape == (R, M)
    # EVERY element's sum stands at least fifty times above the allowed error (the smallest of the 196 692 sums of 64 terms of
    # the RedChicoSur case is 93 x); the terms have mean 1/16, so where there are enough of them the sums sit near S h / 16
    # and a dropped snapshot or k-step (1 / (2 S) of that or more) shows
    allowed = NU.wtol(S * h) * max(1.0, float(p['ref'].abs().max()))
    assert float(p['ref'].abs().min()) > 50 * allowed
    if R * M >= 100:
        assert float(p['ref'].mean()) > 0.9 * S * h / 16 and S * h / 16 / (2 * S) > 100 * allowed
        assert float(p['inci'].abs().max()) > 1.5 and float(p['inci'].min()) < -1.5      # values other than 0 / 1
    assert float(p['inci'].abs().min()) > 0 and not bool((p['inci'] == 1).any())
