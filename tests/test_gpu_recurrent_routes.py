"""fp64 parity of the GRU / LSTM C entries at every kernel route: uds_recurrent_forward[_train] (k_recurrent<G> with U in LDS up to
116 / 100 units, k_recurrent_stream<G> above, thread counts that are no multiple of 64), uds_recurrent_fused (k_recurrent_mfma<3,0>,
<3,2>, <3,4>, <4,0>, <4,2>: 16-row block edges, idle waves, the prologue of the one-step-ahead x pipeline, 96 steps) and
uds_recurrent_backward[_h] (k_recurrent_bwd<G>, k_recurrent_bwd_h<G, H> at every width, the packed image staged or read in place),
plus saturated gates through every forward kernel and the backward ones.  tests/recurrent_util.py holds the cases, the Python
restatement of the host routing, the fp64 references and the CPU model of the split-bf16 arithmetic the backward bound comes from;
tests/test_recurrent_route_math.py checks on the CPU that the cases run what they claim, that the bounds hold for the reference
alone and that wrong kernels cannot pass.

Every input -- the packed weights and the saved forward states included -- is a view inside a NaN-filled allocation; every output
is a view inside a sentinel-filled allocation, checked on both sides and for finiteness.  Plain allocations, shapes the entries
accept: nothing here is meant to fault.

Bounds, the measure always the fp64 reference (none was raised):
  exact fp32 forward (h and the LSTM's c)   TOL_FP32 = 5e-6 * max(1, max|ref|)       (tests/test_gpu_parity.py: TOL)
  one-launch forward                        TOL_BF16X3 = 2e-5 * max(1, max|ref|)     (tests/test_gpu_emulator.py: TOL_FWD['bf16x3'])
  backward, dxp and darec each              3 x max|split-bf16 CPU model - ref| of that case and tensor: 0.00016 .. 0.0058 of the
                                            project's 1e-3 * max|ref gradient| (tests/test_recurrent_route_math.py)
Bitwise: uds_recurrent_forward gives the h of uds_recurrent_forward_train, the binding's own call gives the same, a batch gives
what its elements give alone, two runs give the same.

MEASURED on an MI355X (every case prints its figures; UDS_TOL_REPORT=1 lists them sorted), worst observed / allowed per test [case]:
  test_exact_forward, h            0.044  [exact-GRU-B2T9R37-H200]                 err 2.18e-7; T = 96 at 128 units: 0.044
  test_exact_forward, c            0.035  [exact-LSTM-B2T9R37-H256]                err 2.20e-7
  test_one_launch_forward          0.286  [fused-GRU-B3T96R17-H64-F64-norb]        err 5.72e-6 (the CPU model alone: 0.288)
      per form: <3,0> 0.132, <3,2> 0.286, <3,4> 0.174 (inputs +-0.5), <4,0> 0.051, <4,2> 0.146; T = 9 and T = 96 alike
  test_backward, dxp               0.747  [bwd-GRU-B1T1R1-H48]                     err 9.63e-8 against 3 x 4.30e-8
  test_backward, darec             0.668  [bwd-GRU-B1T1R1-H32]                     err 4.28e-8 against 3 x 2.13e-8
      the worst are all one step from the zero state, where the model's error is fp32 rounding alone and the kernels' v_exp_f32 /
      v_rcp_f32 gates use up the margin; from T = 2 on every case stays below 0.46
  test_saturated_forward           0.041 (exact h), 0.012 (exact c), 0.107 (<3,0>), 0.047 (<4,0>); carried and replaced states exact
  test_saturated_backward          0.364  [bwd-LSTM-B2T5R19-H64-norb-sat]          err 7.14e-7
test_lds_limit_is_raised_on_every_device needs two visible devices; it has only run where one was, and skipped.
Nothing failed on the commit before this file: the kernels were right at every route, horizon and saturation tried here.
"""
import pytest
import torch

from gnn_uds_amd import _lib
from tests import recurrent_util as RU
from tests.recurrent_util import GATES, case_id, forward_ref, inputs
from tests.util import Guarded, close, nan_in

pytestmark = pytest.mark.gpu

KIND = {'GRU': 0, 'LSTM': 1}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sl(t, b):
    return t if t is None or b is None else t[b:b + 1]


def _report(what, c, got, ref, tol):
    """close() against tol * max(1, max|ref|), the observed / allowed ratio printed first."""
    err, lim = float((got.double().cpu() - ref).abs().max()), RU.bound(ref, tol)
    print('%-9s %-40s err %.3e allowed %.3e ratio %.3f' % (what, case_id(c), err, lim, err / lim))
    close(got, ref, tol, _depth=2)


# ---- uds_recurrent_forward[_train] ------------------------------------------------------------------------------------------
def run_exact(dev, c, p, train=True, b=None):
    """The case (batch element b alone, if given) through uds_recurrent_forward_train / uds_recurrent_forward on guarded memory."""
    kind, H = c['kind'], c['H']
    xp, U, rb = nan_in(_sl(p['x'], b), dev), nan_in(p['U'], dev), nan_in(p['rb'], dev)
    B, T, R, _ = xp.shape
    out = Guarded((B, T, R, H), dev)
    cst = Guarded((B, T, R, H), dev) if train and kind == 'LSTM' else None
    lib = _lib.load()
    if train:
        rc = lib.uds_recurrent_forward_train(xp.data_ptr(), U.data_ptr(), _ptr(rb), B, T, R, H, KIND[kind], out.view.data_ptr(),
                                             _ptr(cst.view) if cst else None, _stream())
    else:
        rc = lib.uds_recurrent_forward(xp.data_ptr(), U.data_ptr(), _ptr(rb), B, T, R, H, KIND[kind], out.view.data_ptr(), _stream())
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    out.check(case_id(c) + ' h')
    if cst:
        cst.check(case_id(c) + ' c')
    return out.view, cst.view if cst else None


def exact_parity(dev, c):
    p = inputs(c)
    ref_h, ref_c = forward_ref(c, p)
    h, cs = run_exact(dev, c, p)
    _report('exact h', c, h, ref_h, RU.TOL_FP32)
    if c['kind'] == 'LSTM':
        _report('exact c', c, cs, ref_c, RU.TOL_FP32)
    assert torch.equal(run_exact(dev, c, p, train=False)[0], h)              # the inference entry: the same bits
    f = lambda t: None if t is None else t.float().to(dev)
    assert torch.equal(_lib.recurrent_forward(f(p['x']), f(p['U']), f(p['rb']), c['kind']), h)
    h2, c2 = run_exact(dev, c, p)
    assert torch.equal(h2, h) and (cs is None or torch.equal(c2, cs))        # two runs
    for b in range(c['B'] if c['B'] > 1 else 0):                             # a batch element alone
        hb, cb = run_exact(dev, c, p, b=b)
        assert torch.equal(hb[0], h[b]) and (cs is None or torch.equal(cb[0], cs[b])), 'batch element %d' % b
    return p, h, ref_h


@pytest.mark.parametrize('case', RU.EXACT_CASES, ids=case_id)
def test_exact_forward(dev, case):
    exact_parity(dev, case)


# ---- uds_recurrent_fused ----------------------------------------------------------------------------------------------------
def run_fused(dev, c, p, packed, b=None):
    x, b_in, rb = nan_in(_sl(p['x'], b), dev), nan_in(p['b_in'], dev), nan_in(p['rb'], dev)
    B, T, R, _ = x.shape
    out = Guarded((B, T, R, 64), dev)
    lib = _lib.load()
    rc = lib.uds_recurrent_fused(x.data_ptr(), c['F'], packed.data_ptr(), _ptr(b_in), _ptr(rb), B, T, R, KIND[c['kind']], out.view.data_ptr(),
                                 _stream())
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    out.check(case_id(c))
    return out.view


def fused_parity(dev, c):
    p = inputs(c)
    ref, _ = forward_ref(c, p)
    f = lambda t: None if t is None else t.float().to(dev)
    packed = nan_in(_lib.recurrent_pack(f(p['W']), f(p['U'])), dev)
    assert packed.numel() * 4 == RU.recurrent_mfma_lds(GATES[c['kind']], c['F'] // 32)
    out = run_fused(dev, c, p, packed)
    _report('fused', c, out, ref, RU.TOL_BF16X3)
    assert torch.equal(_lib.recurrent_fused(f(p['x']), packed, f(p['b_in']), f(p['rb']), c['kind'], projected=c['F'] == 0), out)
    assert torch.equal(run_fused(dev, c, p, packed), out)
    for b in range(c['B'] if c['B'] > 1 else 0):
        assert torch.equal(run_fused(dev, c, p, packed, b=b)[0], out[b]), 'batch element %d' % b
    return p, out, ref


@pytest.mark.parametrize('case', RU.FUSED_CASES, ids=case_id)
def test_one_launch_forward(dev, case):
    fused_parity(dev, case)


# ---- uds_recurrent_backward[_h] ---------------------------------------------------------------------------------------------
def run_backward(dev, c, p, h, cs, packed, b=None):
    kind, H, G = c['kind'], c['H'], GATES[c['kind']]
    xp, rb, gh = nan_in(_sl(p['x'], b), dev), nan_in(p['rb'], dev), nan_in(_sl(p['gh'], b), dev)
    hd, cd = nan_in(_sl(h, b), dev), nan_in(_sl(cs, b), dev)
    B, T, R, _ = xp.shape
    dxp, darec = Guarded((B, T, R, G * H), dev), Guarded((G, B, T, R, H), dev)
    lib = _lib.load()
    entry = _lib.recurrent_bwd_route(H)
    assert entry == ('uds_recurrent_backward' if c['claims'][0] == 'bwd64' else 'uds_recurrent_backward_h')
    width = [] if entry == 'uds_recurrent_backward' else [H]
    rc = getattr(lib, entry)(xp.data_ptr(), packed.data_ptr(), _ptr(rb), hd.data_ptr(), _ptr(cd), gh.data_ptr(), B, T, R, *width, KIND[kind],
                             dxp.view.data_ptr(), darec.view.data_ptr(), _stream())
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    dxp.check(case_id(c) + ' dxp')
    darec.check(case_id(c) + ' darec')
    return dxp.view, darec.view


def backward_parity(dev, c):
    p = inputs(c)
    ref_dxp, ref_darec, a_dxp, a_darec, _ = RU.backward_bounds(c, p)
    f = lambda t: None if t is None else t.float().to(dev)
    h, cs = _lib.recurrent_forward_train(f(p['x']), f(p['U']), f(p['rb']), c['kind'])      # the states the backward pass is given
    packed = nan_in(_lib.recurrent_pack_bwd(f(p['U'])), dev)
    assert packed.numel() * 4 == RU.recurrent_bwd_packed_bytes(GATES[c['kind']], c['H'])
    dxp, darec = run_backward(dev, c, p, h, cs, packed)
    for what, got, ref, allowed in (('dxp', dxp, ref_dxp, a_dxp), ('darec', darec, ref_darec, a_darec)):
        err = float((got.double().cpu() - ref).abs().max())
        print('bwd %-5s %-36s err %.3e allowed %.3e ratio %.3f  (1e-3 * max|ref| = %.3e)'
              % (what, case_id(c), err, allowed, err / allowed, RU.TOL_GRAD * float(ref.abs().max())))
    for got, ref, allowed in ((dxp, ref_dxp, a_dxp), (darec, ref_darec, a_darec)):
        close(got, ref, allowed / max(1.0, float(ref.abs().max())))          # = an absolute bound of `allowed`
    dxp2, darec2 = run_backward(dev, c, p, h, cs, packed)
    assert torch.equal(dxp2, dxp) and torch.equal(darec2, darec)
    for b in range(c['B'] if c['B'] > 1 else 0):
        dxb, dab = run_backward(dev, c, p, h, cs, packed, b=b)
        assert torch.equal(dxb[0], dxp[b]) and torch.equal(dab[:, 0], darec[:, b]), 'batch element %d' % b


@pytest.mark.parametrize('case', RU.BWD_CASES, ids=case_id)
def test_backward(dev, case):
    backward_parity(dev, case)


# ---- saturated gates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RU.SAT_CASES, ids=case_id)
def test_saturated_forward(dev, case):
    """Pre-activations of +-60 and +-100 through k_recurrent, k_recurrent_stream and k_recurrent_mfma<G, 0>: exp(100) is inf in
    fp32, the quotient must come out 0.  Finite everywhere (the guards check), within the route's bound everywhere; where the GRU's
    update gate is saturated the state is carried bit for bit (z = 1) or replaced by exactly +-1 (z = 0, saturated candidate)."""
    p, out, ref = (exact_parity if case['fam'] == 'exact' else fused_parity)(dev, case)
    if case['kind'] == 'GRU':
        carry, fresh, sign = RU.sat_gru_masks(case, p)
        got = out.cpu()
        before = torch.cat([torch.zeros_like(got[:, :1]), got[:, :-1]], dim=1)
        assert torch.equal(got[carry], before[carry])
        assert torch.equal(got[fresh].double(), sign[fresh])


@pytest.mark.parametrize('case', RU.SAT_CASES, ids=case_id)
def test_saturated_backward(dev, case):
    """The backward kernel of the same width on the same inputs: finite everywhere (the guards check), every gradient -- those of
    the saturated elements are zero to 1e-24 in the reference -- within the case's bound."""
    backward_parity(dev, RU.sat_bwd_case(case))


# ---- the dynamic-LDS limit is a per-device attribute ------------------------------------------------------------------------
def test_lds_limit_is_raised_on_every_device(dev):
    """A GRU of 96 units needs 109 KiB of dynamic LDS for k_recurrent: above the 64 KiB default, so the limit has to be raised on
    each device the process launches on, not once per process."""
    if torch.cuda.device_count() < 2:
        pytest.skip('one device visible')
    c = RU.TWO_DEVICE_CASE
    p = inputs(c)
    ref, _ = forward_ref(c, p)
    for d in (0, 1):
        with torch.cuda.device(d):
            h, _ = run_exact(torch.device('cuda', d), c, p)
            close(h, ref, RU.TOL_FP32)
