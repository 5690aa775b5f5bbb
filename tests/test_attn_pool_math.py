"""The closed-form reference of the two-block GlobalAttnSumPool (tests/pool_util.py) on the CPU: it is the gradient of the softmax
form (torch autograd in fp64), and a plain fp32 evaluation of the same formulas stays within a quarter of the bounds the GPU
kernels are held to (tests/test_gpu_attn_pool_train.py) -- the reference alone leaves the kernels three quarters of each bound.

Measured over POOL_CASES with torch's fp32 CPU kernels against fp64, relative to max(1, max|ref|): out 4.7e-7, (M, L) 8.5e-7, dx / de
1.3e-6 (of 2.5e-6 allowed here), dk 1.1e-6 at most; the wide-score case below 5e-8 on every tensor (one row carries the whole
weight)."""
import pytest
import torch

from tests.pool_util import POOL_CASES, TOL_BWD, TOL_FWD, case_id, pool_autograd, pool_closed_form, pool_ref, rel_err


@pytest.mark.parametrize('case', POOL_CASES, ids=case_id)
def test_closed_form_is_the_gradient_of_the_softmax_form(case):
    (x, e, k, g), ref = pool_ref(case)
    B, Rx, Re, F, _ = case
    assert tuple(x.shape) == (B, Rx, F) and (e is None) == (Re == 0) and tuple(k.shape) == (F, 1) and tuple(g.shape) == (B, F)
    ag = pool_autograd(x, e, k, g)
    for name in ('out', 'dx', 'de', 'dk'):
        if ref[name] is None:
            assert ag[name] is None
            continue
        assert ref[name].shape == ag[name].shape
        assert rel_err(ref[name], ag[name]) < 1e-13, name
    M, L = ref['stat'][:, 0], ref['stat'][:, 1]
    rows = x if e is None else torch.cat([x, e], dim=-2)
    assert torch.equal(M, (rows @ k).squeeze(-1).max(dim=-1).values) and bool((L >= 1).all()) and bool((L <= Rx + Re).all())
    big = {name: float(ref[name].abs().max()) for name in ('dx', 'de', 'dk') if ref[name] is not None}
    print(case_id(case), big)
    assert max(big.get('dx', 0.0), big.get('de', 0.0)) > 1e-3      # the gradients carry signal
    if Rx + Re == 1:
        assert big['dk'] == 0.0                                  # a single row: alpha = 1 whatever k is
    elif case[4] == 1:                                           # (the wide-score case puts nearly all weight on one row: a small dk)
        assert big['dk'] > 1e-3


def test_the_wide_case_needs_the_running_maximum():
    (x, e, k, g), ref = pool_ref(POOL_CASES[-1])
    s = (torch.cat([x, e], dim=-2) @ k).squeeze(-1)
    assert float(s.max()) > 89 and float(s.min()) < -89          # exp(89) is not an fp32 number
    assert not bool(torch.isfinite(torch.exp(s.float())).all())


@pytest.mark.parametrize('case', POOL_CASES, ids=case_id)
def test_plain_fp32_stays_within_a_quarter_of_the_gpu_bounds(case):
    (x, e, k, g), ref = pool_ref(case)
    f = lambda t: None if t is None else t.float()
    got = pool_closed_form(f(x), f(e), f(k), f(g))
    assert got['out'].dtype == torch.float32
    for name, tol in (('out', TOL_FWD), ('stat', TOL_FWD), ('dx', TOL_BWD), ('de', TOL_BWD), ('dk', TOL_BWD)):
        if ref[name] is None:
            continue
        err = rel_err(got[name], ref[name])
        print('%s %s: fp32 / fp64 %.2e of %.2e' % (case_id(case), name, err, tol))
        assert err <= 0.25 * tol, (name, err)


def test_entries_refuse_bad_arguments_before_any_launch():
    """UDS_EINVAL (-22) for a NULL x, a width that is no power of two and link rows without their tensor: argument checks come
    before the launch, so this needs no device (the pointers are never followed)."""
    from gnn_uds_amd import _lib
    lib = _lib.load()
    p = 4096                                                      # any 16-byte aligned non-NULL address
    assert lib.uds_attn_sum_pool_pair(None, 5, p, 4, p, 2, 16, p, p, None) == -22
    assert lib.uds_attn_sum_pool_pair(p, 5, p, 4, p, 2, 12, p, p, None) == -22
    assert lib.uds_attn_sum_pool_pair(p, 5, None, 4, p, 2, 16, p, None, None) == -22
    assert lib.uds_attn_sum_pool_pair(p + 4, 5, p, 4, p, 2, 16, p, None, None) == -22 and b'aligned' in lib.uds_last_error()
    bwd = lambda x, e, F, ws=p: lib.uds_attn_sum_pool_backward(x, 5, e, 4, p, p, p, p, 2, F, p, p, ws, p, None)
    assert bwd(None, p, 16) == -22 and bwd(p, p, 12) == -22 and bwd(p, None, 16) == -22
    assert bwd(p, p, 16, None) == -22 and b'dk_ws' in lib.uds_last_error()
