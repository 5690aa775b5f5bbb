"""uds_attn_sum_pool_pair / uds_attn_sum_pool_backward (GlobalAttnSumPool over node rows followed by link rows, never
concatenated, and its one-pass backward) on the GPU against the closed-form fp64 reference of tests/pool_util.py, whose cases
and formulas tests/test_attn_pool_math.py checks on the CPU.

Bounds (relative to max(1, max|ref|) through tests.util.close), the project's own:
  out, (M, L)   5e-6   tests/test_gpu_emulator.py test_attn_sum_pool_kernel
  dx, de, dk    1e-5   the sparse backward bound (tests/test_gpu_sparse_widths.py)
The forward is also held to the bits of uds_attn_sum_pool on the concatenated tensor.  Inputs live in NaN-filled allocations,
outputs and the dk workspace in sentinel-guarded ones.

Worst observed / allowed on an MI355X (UDS_TOL_REPORT=1), per test:
  test_pair_forward                          0.125  (out, B6-Rx443-Re444-F128: 7.7e-6 of 6.1e-5; (M, L) 0.116 at the same case)
  test_pool_backward                         0.076  (dx, B5-Rx30-Re29-F128; de 0.050, dk 0.067; the wide-score case 0.005: 4.6e-8)
  test_module_paths                          0.055 on the HIP path (out); 0.387 on the torch path (dk at F = 512)
  test_module_takes_a_misaligned_gradient    0.043  (dk)
No bound was raised.  (The first build let the compiler fuse the backward's score product, an ulp off the forward's: de of the
wide-score case then sat at 2.0 of its bound; uds::dot4 fixes the arithmetic, not the bound.)
"""
import pytest
import torch

from gnn_uds_amd import _lib
from gnn_uds_amd.agent import GlobalAttnSumPool
from tests.pool_util import POOL_CASES, TOL_BWD, TOL_FWD, case_id, pool_autograd, pool_ref
from tests.util import Guarded, close, nan_in

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def device_inputs(case, dev):
    (x, e, k, g), ref = pool_ref(case)
    f = lambda t: None if t is None else nan_in(t.float(), dev)
    return f(x), f(e), f(k.reshape(-1)), f(g), ref


def forward_guarded(x, e, k, dev, want_stat):
    """uds_attn_sum_pool_pair straight through the C entry, into guarded out / stat."""
    B, Rx, F = x.shape
    out, stat = Guarded((B, F), dev), Guarded((B, 2), dev) if want_stat else None
    rc = _lib.load().uds_attn_sum_pool_pair(x.data_ptr(), Rx, None if e is None else e.data_ptr(), 0 if e is None else e.shape[1], k.data_ptr(), B, F,
                                            out.view.data_ptr(), stat.view.data_ptr() if want_stat else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.load().uds_last_error()
    out.check('out')
    if want_stat:
        stat.check('stat')
    return out.view, stat.view if want_stat else None


@pytest.mark.parametrize('case', POOL_CASES, ids=case_id)
def test_pair_forward(dev, case):
    """Bit for bit uds_attn_sum_pool on the concatenated rows, with and without stat; (M, L) and out against fp64."""
    x, e, k, _, ref = device_inputs(case, dev)
    cat = x if e is None else nan_in(torch.cat([x, e], dim=-2), dev)
    one_block = _lib.attn_sum_pool(cat, k)
    out, _ = forward_guarded(x, e, k, dev, False)
    out_s, stat = forward_guarded(x, e, k, dev, True)
    assert torch.equal(out, one_block) and torch.equal(out_s, one_block)
    assert torch.equal(_lib.attn_sum_pool_pair(x, e, k), one_block)
    assert torch.equal(_lib.attn_sum_pool_pair(cat, None, k), one_block)                  # e = None: the one-block call
    o2, s2 = _lib.attn_sum_pool_pair(x, e, k, want_stat=True)
    assert torch.equal(o2, one_block) and torch.equal(s2, stat)
    close(out, ref['out'], TOL_FWD)
    close(stat, ref['stat'], TOL_FWD)


def backward_guarded(x, e, k, out, stat, g, dev, want=(True, True, True)):
    B, Rx, F = x.shape
    want_dx, want_de, want_dk = want[0], want[1] and e is not None, want[2]
    bufs = {'dx': Guarded((B, Rx, F), dev) if want_dx else None, 'de': Guarded((B, e.shape[1], F), dev) if want_de else None,
            'dk': Guarded((F,), dev) if want_dk else None, 'dk_ws': Guarded((B, F), dev) if want_dk else None}
    v = lambda n: None if bufs[n] is None else bufs[n].view
    dx, de, dk = _lib.attn_sum_pool_backward(x, e, k, out, stat, g, want_dx=want_dx, want_de=want_de, want_dk=want_dk, dx=v('dx'), de=v('de'),
                                             dk=v('dk'), dk_ws=v('dk_ws'))
    for n, b in bufs.items():
        if b is not None:
            b.check(n)
    assert (dx is None) == (not want_dx) and (de is None) == (not want_de) and (dk is None) == (not want_dk)
    return dx, de, dk


@pytest.mark.parametrize('case', POOL_CASES, ids=case_id)
def test_pool_backward(dev, case):
    x, e, k, g, ref = device_inputs(case, dev)
    out, stat = _lib.attn_sum_pool_pair(x, e, k, want_stat=True)
    out, stat = nan_in(out, dev), nan_in(stat, dev)
    dx, de, dk = backward_guarded(x, e, k, out, stat, g, dev)
    close(dx, ref['dx'], TOL_BWD)
    if e is not None:
        close(de, ref['de'], TOL_BWD)
    close(dk, ref['dk'].reshape(-1), TOL_BWD)
    same = lambda a, b: (a is None and b is None) or torch.equal(a, b)
    dx2, de2, dk2 = backward_guarded(x, e, k, out, stat, g, dev)                           # a second call: the same bits
    assert same(dx, dx2) and same(de, de2) and same(dk, dk2)
    for i in range(3):                                                                     # each output NULL: the others unchanged
        want = tuple(j != i for j in range(3))
        got = backward_guarded(x, e, k, out, stat, g, dev, want)
        for j, (a, b) in enumerate(zip((dx, de, dk), got)):
            assert b is None if (j == i or a is None) else torch.equal(a, b), (i, j)


def _module_case(dev, B, Rx, Re, F, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    x, e, k, g = r(B, Rx, F) * 4 - 2, r(B, Re, F) * 4 - 2, r(F, 1) - 0.5, r(B, F) * 2 - 1
    pool = GlobalAttnSumPool(F).to(dev)
    pool.attn_kernel.data = k.float().to(dev)
    pool.requires_grad_(True)
    return pool, x, e, k, g, pool_autograd(x, e, k, g)


@pytest.mark.parametrize('F,path', [(64, 'hip-train'), (12, 'torch'), (512, 'torch')])
def test_module_paths(dev, F, path):
    """GlobalAttnSumPool: HIP forward and backward at a supported width, the torch composition at F = 12 and F = 512; the values
    and the gradients of the softmax form either way."""
    pool, x, e, k, g, ref = _module_case(dev, 3, 30, 29, F, 5)
    xd, ed = x.float().to(dev).requires_grad_(True), e.float().to(dev).requires_grad_(True)
    out = pool(xd, ed)
    assert pool.last_path == path
    (out * g.float().to(dev)).sum().backward()
    close(out, ref['out'], TOL_FWD)
    close(xd.grad, ref['dx'], TOL_BWD)
    close(ed.grad, ref['de'], TOL_BWD)
    close(pool.attn_kernel.grad, ref['dk'], TOL_BWD)
    with torch.no_grad():
        out2 = pool(xd, ed)
        assert pool.last_path == ('hip' if path == 'hip-train' else 'torch')
        one = pool(torch.cat([xd, ed], dim=-2))                                           # the one-argument call keeps working
    close(out2, ref['out'], TOL_FWD)
    assert torch.equal(one, out2) if path == 'hip-train' else bool((one - out2).abs().max() <= 1e-6)
    if path == 'hip-train':
        assert torch.equal(out2, out)
        # only the rows need a gradient: no kernel gradient comes back, and x.grad carries the same bits
        pool.attn_kernel.requires_grad_(False)
        x2 = x.float().to(dev).requires_grad_(True)
        (pool(x2, ed.detach()) * g.float().to(dev)).sum().backward()
        assert pool.last_path == 'hip-train' and torch.equal(x2.grad, xd.grad)


def test_module_takes_a_misaligned_gradient(dev):
    """The upstream gradient as a view at an odd offset (AttnSumPoolFn clones it: the kernel reads 16-byte vectors)."""
    pool, x, e, k, g, ref = _module_case(dev, 3, 30, 29, 64, 6)
    xd, ed = x.float().to(dev).requires_grad_(True), e.float().to(dev).requires_grad_(True)
    out = pool(xd, ed)
    gbuf = torch.zeros(3 * 64 + 1, device=dev)
    gview = gbuf[1:].view(3, 64)
    gview.copy_(g.float())
    assert gview.data_ptr() % 16
    out.backward(gview)
    close(xd.grad, ref['dx'], TOL_BWD); close(ed.grad, ref['de'], TOL_BWD); close(pool.attn_kernel.grad, ref['dk'], TOL_BWD)


def test_refusals(dev):
    """Bad arguments return UDS_EINVAL (-22) and launch nothing."""
    lib = _lib.load()
    B, Rx, Re, F = 2, 5, 4, 16
    t = lambda *s: torch.zeros(*s, device=dev)
    x, e, k, out, stat, g = t(B, Rx, F), t(B, Re, F), t(F), t(B, F), t(B, 2), t(B, F)
    dx, de, dk, ws = t(B, Rx, F), t(B, Re, F), t(F), t(B, F)
    p = lambda a: a.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.uds_attn_sum_pool_pair(p(x), Rx, p(e), Re, p(k), B, F, p(out), p(stat), st) == 0
    assert lib.uds_attn_sum_pool_pair(None, Rx, p(e), Re, p(k), B, F, p(out), p(stat), st) == -22             # NULL x
    assert lib.uds_attn_sum_pool_pair(p(x), Rx, p(e), Re, p(k), B, 12, p(out), p(stat), st) == -22            # F = 12
    assert lib.uds_attn_sum_pool_pair(p(x), Rx, None, Re, p(k), B, F, p(out), p(stat), st) == -22             # Re > 0, e NULL
    assert b'uds_attn_sum_pool_pair' in lib.uds_last_error()
    bwd = lambda xx, ee, ff, w=p(ws): lib.uds_attn_sum_pool_backward(xx, Rx, ee, Re, p(k), p(out), p(stat), p(g), B, ff, p(dx), p(de), w, p(dk), st)
    assert bwd(p(x), p(e), F) == 0
    assert bwd(None, p(e), F) == -22
    assert bwd(p(x), p(e), 12) == -22
    assert bwd(p(x), None, F) == -22
    assert bwd(p(x), p(e), F, None) == -22                                                                    # dk without its workspace
    assert b'uds_attn_sum_pool_backward' in lib.uds_last_error()
    torch.cuda.synchronize()
