"""uds_ce_draw / uds_ce_update on the MI355X against the fp64 restatements of tests/mpc_util.py (tests/test_mpc_solver_math.py
holds those to known answers).

Draw.  The restatement takes the same Philox words and the same fp32 uniforms and evaluates Box-Muller in fp64, so what is
left is the kernel's fp32 arithmetic: logf, sqrtf, the rounded argument 2 pi u2 of cosf, the product and the fused
mean + std z.  Where the restatement clips, the kernel's value is exactly 0 or 1.  Elsewhere the worst |out - ref| measured on
an MI355X over the three cases below (std up to 0.6) is 5.07e-7 (128 x 37 draws; 2.42e-7 at 2048 x 3, 3.82e-7 at 4 x 1024);
DRAW_TOL allows 4 x that for other inputs' logf / cosf rounding.  (1e-5 or more would be a defect, not a tolerance.)

Update.  Elite membership, best_y, best_obj and status are exact; mean and std are held to CE_MEAN_BOUND / CE_STD_BOUND, which
tests/mpc_util.py derives from the 10-level trees of the kernel (both below 1e-5; the std bound for a reference std >= 0.01)."""
import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from tests import mpc_util as MU
from tests.window_util import guards_intact, nan_view

pytestmark = pytest.mark.gpu
DRAW_TOL = 4 * 5.07e-7
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _f32(a, dev):
    return nan_view(torch.as_tensor(np.asarray(a), dtype=torch.float32), dev)[0]


@pytest.mark.parametrize('pop,n_var,seed', [(64, 37, 0x1234567890ABCDEF), (1024, 3, 7), (2, 1024, 1 << 63)])
def test_draw(dev, pop, n_var, seed):
    rng = np.random.default_rng(n_var)
    mean = MU.f32_exact(rng.uniform(0, 1, n_var))
    std = MU.f32_exact(rng.uniform(0.05, 0.6, n_var))
    std[0], mean[-1] = 0.0, 0.97                                     # a variable that never moves, one that clips at 1 often
    mean_d, std_d = _f32(mean, dev), _f32(std, dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    first, parent = nan_view(torch.full((pop, n_var), NAN, device=dev))
    _lib.ce_draw(mean_d, std_d, seed, count, pop, out=first)
    second = _lib.ce_draw(mean_d, std_d, seed, count, pop)
    assert int(count) == 2 * pop and guards_intact(parent, pop * n_var)
    ref, raw = MU.ce_draw_ref(mean, std, seed, 0, 2 * pop)
    out = torch.cat([first, second]).double().cpu().numpy()
    clipped = (raw <= 0) | (raw >= 1)
    assert clipped.any() and (~clipped).any()
    assert (out[clipped] == ref[clipped]).all()                      # exactly 0 / 1 where the restatement clips
    err = float(np.abs(out - ref).max())
    print('draw pop %d n_var %d: max |out - ref| %.3e' % (pop, n_var, err))
    assert err < 1e-5, 'a defect, not a tolerance: %.3e' % err
    assert err <= DRAW_TOL, err
    assert (out[:, 0] == mean[0]).all() and out.min() >= 0 and out.max() <= 1
    # two calls of pop rows are one call of 2 pop rows (where the size allows it), from a fresh count
    if 2 * pop <= _lib.CE_MAX:
        count.zero_()
        whole = _lib.ce_draw(mean_d, std_d, seed, count, 2 * pop)
        assert torch.equal(whole, torch.cat([first, second])) and int(count) == 2 * pop


def _run_update(dev, y, obj, n_elite, smooth, std_min, mean, std, best_y, best_obj):
    views = {k: nan_view(torch.as_tensor(np.asarray(v, dtype=np.float64), dtype=torch.float32).reshape(np.shape(v) or (1,)), dev)
             for k, v in dict(mean=mean, std=std, best_y=best_y, best_obj=best_obj).items()}
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    _lib.ce_update(_f32(y, dev), _f32(obj, dev), n_elite, smooth, std_min, views['mean'][0], views['std'][0], views['best_y'][0],
                   views['best_obj'][0], status)
    for k, (view, parent) in views.items():
        assert guards_intact(parent, view.numel()), k
    got = {k: v[0].double().cpu().numpy() for k, v in views.items()}
    got['status'] = status.tolist()
    return got


def _check_update(dev, y, obj, n_elite, smooth=0.3, std_min=1e-3, best_obj=INF, seed=0):
    rng = np.random.default_rng(seed)
    n_var = y.shape[1]
    mean, std, best_y = MU.f32_exact(rng.uniform(0, 1, n_var)), MU.f32_exact(rng.uniform(0.05, 0.5, n_var)), MU.f32_exact(rng.uniform(0, 1, n_var))
    ref = MU.ce_update_ref(y, obj, n_elite, smooth, std_min, mean, std, best_y, best_obj)
    got = _run_update(dev, y, obj, n_elite, smooth, std_min, mean, std, best_y, best_obj)
    assert got['status'] == [ref['status'], 0, 0, 0]
    assert (got['best_y'] == ref['best_y']).all() and float(got['best_obj'][0]) == ref['best_obj']      # exact
    if not ref['elites']:
        assert (got['mean'] == mean).all() and (got['std'] == std).all()                                # K = 0: nothing moves
        return ref, got
    assert np.abs(got['mean'] - ref['mean']).max() <= MU.CE_MEAN_BOUND, float(np.abs(got['mean'] - ref['mean']).max())
    serr = np.abs(got['std'] - ref['std'])
    assert (serr <= MU.ce_std_bound(y, ref['elites'])).all(), float(serr.max())
    return ref, got


def _candidates(pop, n_var, seed):
    rng = np.random.default_rng(seed)
    return MU.f32_exact(rng.uniform(0, 1, (pop, n_var))), MU.f32_exact(rng.normal(0, 3, pop))


@pytest.mark.parametrize('pop,n_var,n_elite', [(50, 7, 10), (16, 4, 1), (16, 4, 16), (257, 33, 64), (1024, 5, 1024), (3, 1024, 2)])
def test_update_mean_std_and_best(dev, pop, n_var, n_elite):
    y, obj = _candidates(pop, n_var, pop + n_var)
    for smooth in (0.0, 0.3, 1.0):
        ref, _ = _check_update(dev, y, obj, n_elite, smooth=smooth, seed=n_elite)
        assert len(ref['elites']) == n_elite and ref['best_obj'] == obj.min()
    ref, _ = _check_update(dev, y, obj, n_elite, best_obj=float(obj.min()))          # not strictly lower: best_y, best_obj stay
    assert ref['best_obj'] == obj.min()
    ref, _ = _check_update(dev, y, obj, n_elite, std_min=0.45)                        # the floor binds on some variable
    assert (ref['std'] == float(np.float32(0.45))).any()


def _membership(dev, obj, n_elite):
    """Who was elite, read off the kernel's own output: candidate p is the only one with y[p, p] = 1, so with smooth = 0 the new
    mean of variable p is 1 / K when p is elite and exactly 0 otherwise."""
    pop = len(obj)
    got = _run_update(dev, np.eye(pop), obj, n_elite, 0.0, 0.0, np.zeros(pop), np.zeros(pop), np.zeros(pop), INF)
    return sorted(np.nonzero(got['mean'])[0].tolist()), got


def test_update_elite_membership_ties_and_non_finite(dev):
    cases = [
        ([3.0, 1.0, 2.0, 1.0, 1.0, 5.0], 2),                       # a tie across the elite boundary: the lower index wins
        ([3.0, 1.0, 2.0, 1.0, 1.0, 5.0], 4),
        ([0.0, -0.0, 1.0, -0.0], 2),                               # -0 == +0
        ([NAN, 2.0, INF, -INF, 1.0, NAN], 4),                      # non-finite values rank last and are never elite
        ([NAN, 2.0, INF, -INF, 1.0, NAN], 1),
        ([-INF, 7.0], 2),
        ([1e-45, 0.0, -1e-45, 3.4e38, -3.4e38], 3),                # denormals and the ends of the range order as floats do
    ]
    rng = np.random.default_rng(3)
    big = MU.f32_exact(np.round(rng.normal(0, 2, 1024), 1))        # many ties at pop = 1024
    big[rng.choice(1024, 100, replace=False)] = NAN
    cases.append((big.tolist(), 300))
    for obj, n_elite in cases:
        obj = np.asarray(obj, dtype=np.float32).astype(np.float64)
        want = MU.ce_elites(obj, n_elite)
        who, got = _membership(dev, obj, n_elite)
        assert who == sorted(want), (obj[:8], n_elite)
        assert got['status'] == [0, 0, 0, 0] and float(got['best_obj'][0]) == obj[want[0]]
        assert got['best_y'].tolist() == np.eye(len(obj))[want[0]].tolist()


def test_update_without_a_finite_candidate_changes_nothing_and_raises_status(dev):
    y, _ = _candidates(8, 5, 1)
    for obj in ([NAN] * 8, [INF, -INF, NAN, INF, NAN, -INF, INF, NAN]):
        ref, got = _check_update(dev, y, np.asarray(obj), 3, best_obj=2.5)
        assert ref['status'] == 1 and got['status'][0] == 1 and float(got['best_obj'][0]) == 2.5
    # status is raised, never cleared: a good iteration after a bad one leaves it set
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    mean, std, best_y, best_obj = t(np.full(5, 0.5)), t(np.full(5, 0.3)), t(np.zeros(5)), t([INF])
    _lib.ce_update(t(y), t([NAN] * 8), 3, 0.3, 1e-3, mean, std, best_y, best_obj, status)
    _lib.ce_update(t(y), t(np.arange(8.0)), 3, 0.3, 1e-3, mean, std, best_y, best_obj, status)
    assert status.tolist() == [1, 0, 0, 0] and float(best_obj) == 0.0
