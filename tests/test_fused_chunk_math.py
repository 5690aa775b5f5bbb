"""CPU checks behind tests/test_gpu_fused_chunks.py: the library's chunk function is the arithmetic the cases are derived from,
and the references of tests/fused_chunk_util.py would see what a broken snapshot pipeline computes.

A stale double buffer or a miscounted wait makes a kernel read a row of the wrong snapshot.  Each such mistake is planted in the
fp64 reference, on the node side and on the link side separately, and has to move every affected snapshot by at least 100 x
the bound the GPU tests allow: a kernel that made it could not pass them.  (On the 600 / 720 network the smallest move is 6 x
that requirement for secondary rows, 16 x for the remainder and 140 x for primary rows; relu leaves 42 % of a snapshot's node
outputs and 53 % of its link outputs non-zero.)"""
import pytest
import torch

from gnn_uds_amd import _lib
from tests import fused_chunk_util as FC

TILES = list(range(1, 41)) + [41, 42, 57, 64, 77, 125, 128, 129, 172, 255, 256, 257, 300, 600, 900]


def pick_chunk(S, tiles):
    """Restatement of the launch rule: workgroups = chunks * tiles run in rounds of 256, a workgroup costs 3 + 2 c half snapshots;
    the chunk length with the cheapest launch, the shorter one on a tie."""
    best = None
    for c in range(1, S + 1):
        cost = -(-(-(-S // c) * tiles) // 256) * (3 + 2 * c)
        if best is None or cost < best[0]:
            best = (cost, c)
    return best[1]


def test_chunk_entry_is_the_launch_rule():
    for tiles in TILES:
        for S in range(1, 129):
            c = _lib.fused_chunk(S, tiles)
            assert c == pick_chunk(S, tiles), (S, tiles, c)
            # one snapshot per workgroup exactly when the launch fits one round of 256 workgroups (a single snapshot has no
            # other chunk length, however many tiles)
            assert (c == 1) == (S * tiles <= 256 or S == 1), (S, tiles, c)


def test_chunk_entry_checks_its_arguments():
    lib = _lib.load()
    for S, tiles, text in ((0, 5, 'S=0 tiles=5'), (5, 0, 'S=5 tiles=0'), (-1, 5, 'S=-1 tiles=5'), (1 << 31, 5, 'S=2147483648 tiles=5'),
                           (5, 1 << 31, 'S=5 tiles=2147483648')):
        with pytest.raises(_lib.UdsError, match='uds_fused_chunk: bad sizes ' + text):
            _lib.fused_chunk(S, tiles)
    assert lib.uds_fused_chunk(4, 4, None) == -22 and lib.uds_last_error().decode().startswith('uds_fused_chunk: NULL argument')


def test_cases_exist_where_the_issue_found_them():
    """42 tiles: the (chunk, tail) cases at S = 8, 7, 13, 14, 19, 26; find_S returns the smallest S and respects its cap."""
    assert [FC.find_S(42, c, t) for c, t in ((2, 0), (2, 1), (3, 1), (3, 2), (4, 3), (5, 1))] == [8, 7, 13, 14, 19, 26]
    assert FC.find_S(42, 5, 1, cap=25) is None and FC.find_S(1, 2, 0, cap=256) is None
    for tiles in (2, 13, 26, 58):
        for case in FC.cases_for(tiles, cap=4096):
            S, chunk, tail = case
            assert _lib.fused_chunk(S, tiles) == chunk and S % chunk == tail and chunk > 1
        S, chunk, tail = FC.find_long(tiles, 8, cap=4096)
        assert chunk >= 8 and tail and _lib.fused_chunk(S, tiles) == chunk and S % chunk == tail


S_REF = 5      # snapshots of the planted-mistake references: s - 2 and s + 1 exist for some of them


@pytest.fixture(scope='module')
def case():
    """600 / 720, d = 64, relu, a trained NodeEdge bias on both sides: every operand of a side is there to get wrong."""
    g = FC.graph('600/720')
    p = FC.params(g, 64, 64, 64, dense=True, trained=True)
    x, e = FC.inputs(g, 64, 64, S_REF)
    return g, p, x, e, FC.layer_ref(g, p, x, e)


def test_layer_ref_is_the_oracle(case):
    g, p, x, e, (rx, re) = case
    ox, oe = FC.reference(g, p, x, e)
    assert float((rx - ox).abs().max()) < 1e-12 and float((re - oe).abs().max()) < 1e-12
    a = FC.graph('astlingen')
    q = FC.params(a, 64, 64, 64, dense=True, trained=True)
    xa, ea = FC.inputs(a, 64, 64, 3)
    for got, want in zip(FC.layer_ref(a, q, xa, ea, 'tanh'), FC.reference(a, q, xa, ea, 'tanh', dense_oracle=True)):
        assert float((got - want).abs().max()) < 1e-12
    s = FC.params(g, 96, 64, 64)             # values on the support, mixed widths
    xs, es = FC.inputs(g, 96, 64, 2)
    for got, want in zip(FC.layer_ref(g, s, xs, es), FC.reference(g, s, xs, es)):
        assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize('side', ['node', 'link'])
@pytest.mark.parametrize('part,offset', FC.MISTAKES, ids=['%s%+d' % m for m in FC.MISTAKES])
def test_a_row_of_the_wrong_snapshot_shows(case, side, part, offset):
    g, p, x, e, ref = case
    i = 0 if side == 'node' else 1
    bad = FC.layer_ref(g, p, x, e, wrong=(side, part, offset))
    assert torch.equal(bad[1 - i], ref[1 - i])                    # the other side reads its own operands
    hit = FC.affected(S_REF, offset)
    assert len(hit) == S_REF - abs(offset)
    need = 100 * FC.TOL_BF16X3 * max(1.0, float(ref[i].abs().max()))
    for s in range(S_REF):
        moved = float((bad[i][s] - ref[i][s]).abs().max())
        assert (moved >= need) if s in hit else (moved == 0.0), (s, moved, need)


def test_relu_leaves_signal_in_every_snapshot(case):
    """Signed inputs under relu: at least 30 % of each snapshot's outputs on each side are non-zero (a zero compares equal to
    anything relu clamps)."""
    g, p, x, e, ref = case
    plain = FC.params(g, 64, 64, 64)          # no remainder: rows a-c
    for outs in (ref, FC.reference(g, plain, x, e)):
        for o in outs:
            share = (o != 0).double().mean(dim=(1, 2))
            assert float(share.min()) >= 0.30, share
