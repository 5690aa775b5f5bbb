"""uds_node_edge_wgrad: the cases, a Python restatement of the host plan (kernels_node_edge_wgrad.hpp: node_edge_wgrad_plan) that
says which instantiation a case runs and how the reduction over S is cut, and the seeded inputs.  Shared by
tests/test_node_edge_wgrad_math.py (CPU: the restatement is the library's plan, every route is reached, the references carry
signal) and tests/test_gpu_node_edge_wgrad.py (GPU parity with the fp64 product)."""
import numpy as np
import torch

TILE, MIN_SPP, TARGET_WG = 64, 8, 512
REFUSED = dict(ksteps=0, pieces=0, spp=0, padded=False)


def plan(R, M, S, h):
    """dict(ksteps, pieces, spp, padded) as _lib.node_edge_wgrad_plan reports it."""
    lim = 1 << 24
    if h < 4 or h > 64 or h % 4 or R < 1 or M < 1 or S < 0 or S > lim or R > lim or M > lim:
        return dict(REFUSED)
    tiles = -(-R // TILE) * -(-M // TILE)
    if tiles > 1 << 20:
        return dict(REFUSED)
    want = max(1, TARGET_WG // tiles)
    spp = max(MIN_SPP, -(-S // want))
    return dict(ksteps=1 if h <= 32 else 2, pieces=-(-S // spp), spp=spp, padded=h % 32 != 0)


def pieces_of(R, M, S, h):
    """[(first snapshot, end)] of every piece."""
    p = plan(R, M, S, h)
    return [(i * p['spp'], min(S, (i + 1) * p['spp'])) for i in range(p['pieces'])]


def first_split(R, M, h):
    """The smallest S for which the plan takes two pieces."""
    S = 1
    while plan(R, M, S, h)['pieces'] < 2:
        S += 1
    return S


def one_past_a_boundary(R, M, h, pieces=3):
    """The smallest S cut into `pieces` pieces whose last piece holds one snapshot."""
    S = 1
    while True:
        p = plan(R, M, S, h)
        if p['pieces'] == pieces and S - (pieces - 1) * p['spp'] == 1:
            return S
        S += 1


# (R, M, S, h): the issue's table, then the two S values read from the plan, then a piece length above the minimum
CASES = [
    (1, 1, 1, 4),                                          # smallest accepted shape
    (30, 29, 3, 32),                                       # astlingen, ragged tiles
    (29, 30, 1, 64),                                       # ragged tiles, widest h
    (65, 33, 5, 12),                                       # padded K, two row tiles
    (70, 50, 3, 20),                                       # padded K
    (443, 444, 2, 32),                                     # RedChicoSur
    (444, 443, 2, 64),                                     # RedChicoSur, transposed roles
    (30, 29, first_split(30, 29, 32), 32),                 # split reduction: the smallest S with two pieces
    (65, 33, one_past_a_boundary(65, 33, 64), 64),         # ragged last piece (one snapshot), two tiles, two k-steps
    (33, 65, one_past_a_boundary(33, 65, 40, 2), 40),      # padded second k-step across a split
    (449, 449, 65, 32),                                    # 8 x 8 tiles: 8 workgroups wanted per tile, pieces of 9 snapshots
]
REFUSALS = [(5, 7, 2, 6), (5, 7, 2, 68), (0, 7, 2, 32)]    # h = 6, h = 68, R = 0


def case_id(c):
    return 'R%d-M%d-S%d-h%d' % c


_CACHE = {}


def inputs(c):
    """dict(g (S, R, h), x (S, M, h), inci (R, M), ref (R, M)): fp64 tensors of fp32 values (the device sees the same numbers),
    g and x uniform in [-0.25, 0.75) so that no sum is near zero, inci uniform in +-2; ref = einsum('srk,smk->rm') in fp64.
    Computed once per case and shared: do not modify."""
    if c not in _CACHE:
        R, M, S, h = c
        gen = torch.Generator().manual_seed(7000 + CASES.index(c) if c in CASES else 6999)
        u = lambda *shape: (torch.rand(*shape, generator=gen, dtype=torch.float64) - 0.25).float().double()
        g, x = u(S, R, h), u(S, M, h)
        inci = ((torch.rand(R, M, generator=gen, dtype=torch.float64) - 0.5) * 4).float().double()
        _CACHE[c] = dict(g=g, x=x, inci=inci, ref=torch.einsum('srk,smk->rm', g, x))
    return _CACHE[c]


def wtol(K):
    """The project's weight-gradient bound (tests/test_gpu_wgrad_wide.py) for a reduction of length K = S * h."""
    return 3e-5 * max(1.0, (K / 1000.0) ** 0.5)


def incidence(R, M, seed=0):
    """(R, M) fp64 incidence of fp32 values with three entries per row, values from {-1, 0.5, 2, -0.25}: not a 0/1 matrix."""
    rng = np.random.default_rng(seed + 31 * R + M)
    a = np.zeros((R, M))
    for r in range(R):
        cols = rng.choice(M, min(3, M), replace=False)
        a[r, cols] = rng.choice([-1.0, 0.5, 2.0, -0.25], len(cols))
    return torch.as_tensor(a)
