"""CPU checks behind tests/test_gpu_remainder_routes.py: every case of tests/remainder_util.py reaches the route it claims, every
route the launch code can select (k_remainder_gemm; k_remainder_gemm2 with whole tiles; with tiles cut in ks = 2 .. 8; both
k_dense_split_planes instantiations) is reached, the route mirror agrees with the library's two byte counts -- which answer
without a device -- on every case and on a few thousand other shapes, and the references carry signal: a kernel that makes one
of the mistakes below moves some case's result by more than the GPU bound.

The CPU model alone (test_emulation_stays_within_the_gpu_bound): the split-bf16 product hi hi + lo hi + hi lo in fp64 differs from
the fp64 product of the fp32 values by up to 0.579 of TOL_GEMM = 1e-5 x max(1, max|ref|) over GEMM_CASES (R128M65S7h36: 1.01e-5
against 1.75e-5; 0.41 - 0.58 at every case of 63 links or more).  hi + lo keeps a value to 2^-16 and the inputs are signed, so
error and result both grow like sqrt(M): the arithmetic itself takes half of the project's bound, whatever the kernel.  What a
kernel adds to that -- its fp32 accumulation -- is 0.005 of the bound in the same model (fp32 matmuls of the planes).
"""
import random

import pytest
import torch

from gnn_uds_amd import _lib
from tests import remainder_util as RU
from tests.remainder_util import TOL_GEMM, case_id, emulate, gemm_inputs, gemm_ref, pad_k, piece_starts, plan, route

CUT_CASES = [c for c in RU.GEMM_CASES if c['claims'][0] == 'v2' and c['claims'][3] > 1 and c is not RU.MIXED_CASE]


# ---- tables and routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RU.GEMM_CASES, ids=case_id)
def test_case_reaches_the_route_it_claims(case):
    assert route(case) == case['claims']
    print(case_id(case), route(case))


@pytest.mark.parametrize('case', RU.DENSE_CASES, ids=case_id)
def test_dense_case_reaches_the_route_it_claims(case):
    assert RU.dense_route(case) == case['claims']


@pytest.mark.parametrize('case', RU.FN_CASES, ids=case_id)
def test_fn_case_reaches_the_routes_it_claims(case):
    R, M, S, h = case['R'], case['M'], case['S'], case['h']
    assert (plan(R, M, S, h)[:4], plan(M, R, S, h)[:4]) == case['claims']


def test_case_ids_are_unique():
    for table in (RU.GEMM_CASES, RU.DENSE_CASES, RU.FN_CASES):
        ids = [case_id(c) for c in table]
        assert len(ids) == len(set(ids))


def test_every_route_is_reached():
    routes = [route(c) for c in RU.GEMM_CASES]
    assert any(r[0] == 'v1' for r in routes)
    v2 = [r for r in routes if r[0] == 'v2']
    assert {r[3] for r in v2} == set(range(1, 9))                    # whole tiles and every ks
    assert all((r[2] == 0) == (r[3] == 1) for r in v2)
    assert any(r[1] and r[2] for r in v2)                            # whole and cut tiles in one launch
    assert sum(r[1] + r[2] >= 257 for r in v2) == 1                  # ... once: the only case of that size
    assert any(r[2] > 1 and r[1] == 0 for r in v2)
    # pieces of unequal length that start on an odd absolute k-step: the LDS double buffer goes by that parity
    odd = [r for r in v2 if len(set(r[4])) > 1 and any(s % 2 for s in piece_starts(r[4]))]
    assert len(odd) >= 2
    assert all(min(r[4]) >= 8 for r in v2 if r[3] > 1)               # the planner's promise: a piece is 8 k-steps or more
    dense = [RU.dense_route(c) for c in RU.DENSE_CASES]
    assert {r[0] for r in dense} == {2, 4}                           # k_dense_split_planes<2>, <4>
    assert {r[1] for r in dense} == {'v1', 'v2'} and {r[4] > 1 for r in dense if r[1] == 'v2'} == {False, True}
    fn = [c['claims'] for c in RU.FN_CASES]
    assert {f[0][0] for f in fn} == {'v1', 'v2'} and {f[1][0] for f in fn} == {'v1', 'v2'}


def test_xcd_order_is_a_permutation():
    """Every tile is computed once whatever the grid: 1 .. 600 workgroups, the whole part and the cut part of every case; the
    tables hold grids below 8, multiples of 8 and grids that leave a rest, for both kernels."""
    for nblk in range(1, 601):
        assert sorted(RU.xcd_order(nblk)) == list(range(nblk)), nblk
    o = RU.xcd_order(22)
    assert [o[b] for b in range(0, 22, 8)] == [0, 1, 2] and [o[b] for b in range(7, 22, 8)] == [20, 21]
    v1 = {r[1] for r in map(route, RU.GEMM_CASES) if r[0] == 'v1'}
    assert any(t < 8 for t in v1) and any(t > 8 and t % 8 for t in v1)
    cut = {r[2] * r[3] for r in map(route, RU.GEMM_CASES) if r[0] == 'v2' and r[3] > 1}
    assert any(t < 8 for t in cut) and any(t % 8 == 0 for t in cut) and any(t > 8 and t % 8 for t in cut)
    # a table with square tile grids only could not tell w % n_ctile from w % n_rtile
    assert any(c['claims'][0] == 'v2' and c['claims'][3] > 1 and -(-c['S'] * c['h'] // 256) not in (1, -(-c['R'] // 256)) for c in RU.GEMM_CASES)


def test_gemm_table_covers_the_edges_the_issue_lists():
    cs = RU.GEMM_CASES
    v1 = [c for c in cs if c['claims'][0] == 'v1']
    nc = lambda c: c['S'] * c['h']
    assert any(c['R'] == 1 for c in v1) and any(c['M'] == 1 for c in v1) and any(nc(c) == 4 for c in v1)
    assert any(c['R'] == 127 and nc(c) >= 256 for c in v1) and any(nc(c) == 252 and c['R'] >= 128 for c in v1)
    assert {c['R'] for c in v1} >= {128, 129} and {nc(c) for c in v1} >= {128, 132}
    assert {c['M'] for c in v1} >= {63, 64, 65}
    whole = [c for c in cs if c['claims'][0] == 'v2' and c['claims'][3] == 1]
    assert any(c['R'] == 128 and nc(c) == 256 for c in whole)
    assert {c['R'] for c in whole} >= {255, 256, 257}
    assert any(nc(c) == 260 for c in whole)
    assert {pad_k(c['M']) for c in whole} >= {64, 448}
    assert plan(256, 449, 13, 20)[3] == 2                            # one k-step of 64 more and the same shape is cut
    assert {c['h'] for c in cs} >= {4, 12, 20, 32, 36, 64}
    assert any(c['S'] == 1 for c in cs) and any(c['lead'] for c in v1) and any(c['lead'] for c in whole)
    assert any(c['M'] % 64 == 0 for c in cs) and sum(c['M'] % 64 != 0 for c in cs) >= 15


def test_dense_table_covers_the_edges_the_issue_lists():
    cs = RU.DENSE_CASES
    assert {(c['F'], c['h']) for c in cs} == {(F, h) for F in (64, 128) for h in (32, 64)}
    assert {c['act'] for c in cs} == set(RU.ACTS) == set(k for k in _lib.ACT if k)
    assert sum(not c['bias'] for c in cs) == 1
    assert any(c['M'] < 64 for c in cs) and any(c['M'] == 64 for c in cs) and any(c['M'] > 64 and c['M'] % 64 for c in cs)


# ---- the mirror against the library -----------------------------------------------------------------------------------------
def _sweep():
    rng = random.Random(5)
    for c in RU.GEMM_CASES + RU.DENSE_CASES + RU.FN_CASES:
        yield c['R'], c['M'], c['S'], c['h']
        yield c['M'], c['R'], c['S'], c['h']
    for _ in range(3000):
        yield rng.randint(1, 9000), rng.randint(1, 3000), rng.randint(1, 80), 4 * rng.randint(1, 16)
    for R in (128, 255, 4096, 8192, 8704, 20000, 70000):            # 257 tiles and more: whole rounds and a cut rest
        for M in (100, 255, 256, 300, 512, 1000, 2048, 5000):
            for S in (8, 64, 68, 200, 1000):
                for h in (32, 64):
                    yield R, M, S, h
    yield 128, 600, 60000, 64                                        # the activation image reaches 4 GiB: k_remainder_gemm
    yield 3000000, 1000, 8, 32                                       # the image of rest does


def test_mirror_agrees_with_the_library():
    lib = _lib.load()
    seen = set()
    for R, M, S, h in _sweep():
        q = plan(R, M, S, h)
        t_rest, ks = (q[2], q[3]) if q[0] == 'v2' else (0, 1)
        Kp = pad_k(M)
        assert lib.uds_remainder_workspace_bytes(R, M, S, h) == 2 * S * h * Kp * 2 + t_rest * ks * 262144, (R, M, S, h)
        assert lib.uds_remainder_packed_bytes(R, M) == 2 * R * Kp * 2, (R, M)
        assert RU.workspace_bytes(R, M, S, h) == 2 * S * h * Kp * 2 + t_rest * ks * 262144 and RU.packed_bytes(R, M) == 2 * R * Kp * 2
        seen.add((q[0], ks, q[0] == 'v2' and q[1] > 0))
    assert {('v1', 1, False)} | {('v2', k, False) for k in range(2, 9)} | {('v2', k, True) for k in range(1, 9)} <= seen
    assert lib.uds_remainder_workspace_bytes(0, 5, 1, 4) == 0 and lib.uds_remainder_packed_bytes(3, 0) == 0


# ---- the references -------------------------------------------------------------------------------------------------------
def _lim(ref, tol=TOL_GEMM):
    return tol * max(1.0, float(ref.abs().max()))


def _moved(wrong, ref, tol=TOL_GEMM):
    return float((wrong - ref).abs().max()) > _lim(ref, tol)


_DATA = {}


def data(c):
    if id(c) not in _DATA:
        p = gemm_inputs(c)
        _DATA[id(c)] = (p, gemm_ref(p['rest'], p['x']))
    return _DATA[id(c)]


def test_inputs_are_signed_and_of_the_stated_scale():
    for c in RU.GEMM_CASES[3:8]:
        p, ref = data(c)
        assert abs(float(p['x'].mean())) < 0.05 and abs(float(p['x'].std()) - 1) < 0.05
        assert abs(float(p['rest'].mean())) < 0.005 and abs(float(p['rest'].std()) - 0.05) < 0.005
        assert float(ref.abs().max()) < 0.05 * c['M'] ** 0.5 * 6          # a random walk, not a sum of positive terms
    c = RU.DENSE_CASES[0]
    p = RU.dense_inputs(c)
    assert p['rest'].dtype == p['e'].dtype == p['W'].dtype == torch.float32 and float(RU.dense_act_ref(c, p).min()) == 0.0


def test_split_is_the_documented_one():
    v = torch.tensor([1.0, 1.00390625, 1.01171875, -3.3, 0.05, 2.0 ** -20, 0.0, 1.0 + 2.0 ** -8 + 2.0 ** -20])
    hi, lo = RU.split_bf16(v)
    h, l = hi.view(torch.bfloat16).float(), lo.view(torch.bfloat16).float()
    assert h[1] == 1.0 and l[1] == 0.00390625                        # a tie goes to the even mantissa ...
    assert h[2] == 1.015625 and l[2] == -0.00390625                  # ... up as well as down
    assert float(lo[0]) == 0 and float(hi[6]) == 0 and float(lo[6]) == 0
    assert bool(((v - (h + l)).abs() <= 2.0 ** -16 * v.abs()).all())
    x = gemm_inputs(RU.GEMM_CASES[6])['x']
    img = RU.x_planes(x)
    assert img.shape == (2, 132, 64) and bool((img[:, :, 63:] == 0).all())
    assert torch.equal(img[0, 12 * 3 + 5, :63], RU.split_bf16(x[3, :, 5])[0])


def test_emulation_stays_within_the_gpu_bound():
    worst = (0.0, None, 0.0, 0.0)
    for c in RU.GEMM_CASES:
        p, ref = data(c)
        err = float((emulate(p['rest'], p['x']) - ref).abs().max())
        if err / _lim(ref) > worst[0]:
            worst = (err / _lim(ref), case_id(c), err, _lim(ref))
    print('the CPU model alone: ratio %.4f at %s (err %.3e allowed %.3e)' % worst)
    assert worst[0] <= 0.6


# ---- signal: a kernel with the same mistake cannot pass -------------------------------------------------------------------
def _piece_product(c, p, piece):
    """What K piece `piece` of the case's cut contributes (links past M are the zero padding)."""
    pieces = c['claims'][4]
    k0 = piece_starts(pieces)[piece] * 32
    k1 = min(k0 + pieces[piece] * 32, c['M'])
    assert k0 < k1
    return gemm_ref(p['rest'][:, k0:k1], p['x'][:, k0:k1])


@pytest.mark.parametrize('case', CUT_CASES, ids=case_id)
def test_signal_k_pieces(case):
    """The last K piece dropped; one piece added twice (each of them in turn)."""
    p, ref = data(case)
    ks = case['claims'][3]
    assert _moved(ref - _piece_product(case, p, ks - 1), ref)
    for piece in range(ks):
        assert _moved(ref + _piece_product(case, p, piece), ref), piece


def test_signal_low_plane_term():
    """hi hi + hi lo without lo hi: 2^-9 of a product, three orders above the bound."""
    for c in RU.GEMM_CASES[:-1]:
        p, ref = data(c)
        rl = RU.planes64(p['rest'])[1]
        xh = RU.planes64(p['x'])[0]
        assert _moved(emulate(p['rest'], p['x']) - torch.matmul(rl, xh), ref), case_id(c)


def test_signal_k_padding():
    """Both operand images padded with 2^-7 instead of zero: (Kp - M) 2^-14 on every element."""
    n = 0
    for c in RU.GEMM_CASES:
        p, ref = data(c)
        pad = pad_k(c['M']) - c['M']
        if pad:
            n += 1
            assert _moved(ref + pad * 2.0 ** -14, ref), case_id(c)
    assert n >= 15


def test_signal_column_mapping():
    """Result column c belongs to (snapshot c / h, feature c % h); with 16 in the place of h the element lands elsewhere (every h
    of the table but 16 itself, which the table does not hold)."""
    for c in RU.GEMM_CASES[:-1]:
        p, ref = data(c)
        S, R, h = ref.shape
        if S * h <= 16:
            continue
        cols = torch.arange(S * h)
        mat = ref.permute(1, 0, 2).reshape(R, S * h)                 # [r][c]
        off = ((cols // 16)[None, :] * R + torch.arange(R)[:, None]) * h + (cols % 16)[None, :]
        wrong = torch.zeros(ref.numel(), dtype=ref.dtype)             # (an element nobody writes keeps the pre-fill)
        ok = off < wrong.numel()
        wrong[off[ok]] = mat[ok]
        assert _moved(wrong.reshape(ref.shape), ref), case_id(c)


def test_signal_row_clamp():
    """Loads clamp the rows past R to row R - 1 and the stores skip them.  A store that does not skip puts row R - 1 of snapshot s
    where row 0 of snapshot s + 1 belongs (the element after (s, R - 1, h - 1)); a clamp taken one row low stores the product of
    row R - 2 into row R - 1."""
    for c in RU.GEMM_CASES[:-1]:
        p, ref = data(c)
        S, R, h = ref.shape
        if S > 1:
            wrong = ref.clone()
            wrong[1:, 0] = ref[:-1, R - 1]
            assert _moved(wrong, ref), case_id(c)
        if R > 1:
            wrong = ref.clone()
            wrong[:, R - 1] = ref[:, R - 2]
            assert _moved(wrong, ref), case_id(c)


def test_signal_dense_in_front():
    """uds_remainder_forward_dense: the bias left out, the activation left out, rows past M of the planes not zeroed (act(b)
    instead: what the kernel computes from a clamped row when it forgets `live`)."""
    from oracle import spektral_dense as OD
    for c in RU.DENSE_CASES:
        p = RU.dense_inputs(c)
        a = RU.dense_act_ref(c, p)
        ref = torch.matmul(p['rest'].double(), a)
        z = p['e'].double() @ p['W'].double()
        if c['bias']:
            assert _moved(torch.matmul(p['rest'].double(), OD.activation(c['act'])(z)), ref, RU.TOL_DENSE), case_id(c)
        if c['act'] != 'linear':
            assert _moved(torch.matmul(p['rest'].double(), z + (p['b'].double() if c['bias'] else 0)), ref, RU.TOL_DENSE), case_id(c)


def test_fn_reference_is_the_derivative():
    c = RU.FN_CASES[0]
    p = RU.fn_inputs(c)
    out, d_rest, d_xs = RU.fn_ref(p)
    g, rest, x = p['g'].double(), p['rest'].double(), p['x'].double()
    assert float((d_xs - torch.matmul(rest.t(), g)).abs().max()) <= 1e-12
    assert float((d_rest - torch.einsum('srf,smf->rm', g, x)).abs().max()) <= 1e-11
    # the transposed GEMM of the backward is another problem: a forward-shaped mistake there is seen
    assert _moved(torch.matmul(rest.t()[:, :-1], g[:, :-1]), d_xs, RU.TOL_DXS)
