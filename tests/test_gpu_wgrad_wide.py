"""fp64 parity of uds_wgrad_wide (k_wgrad_wide<MT, NT> + k_wgrad_reduce), the weight gradient of the layers uds_wgrad refuses: up
to 256 input rows plus the bias, up to 256 columns.  tests/wgrad_wide_util.py holds the cases, the Python restatement of the host
routing that says which instantiation and block grid each case runs, and the seeded inputs; tests/test_wgrad_wide_math.py checks on
the CPU that every case reaches what it claims, that every instantiation is reached and that the references carry signal.

Every input is a view inside a NaN-filled allocation; the workspace, d_kernel and d_bias are views inside sentinel-filled
allocations, pre-filled with NaN, checked on both sides and for finiteness (the WHOLE workspace: an element of a partial the
kernel does not write shows).  Plain allocations, valid shapes: nothing here is meant to fault; refusals are return codes.

Tolerances, relative to max(1, max|ref|) through tests.util.close, the measure always the fp64 reference:
  uds_wgrad_wide, d_kernel and d_bias      WGRAD_TOL = 3e-5 * max(1, sqrt(rows / 1000)), the bound of tests/test_gpu_rowgemm_routes.py
                                           for uds_wgrad (the same three bf16 products, fp32 sums in a fixed order)
  through autograd, linear activation      dW, db: the same bound (dZ is then the upstream gradient itself, the weight gradient the
                                           kernel's work alone); dX: 4e-5, the row GEMM's bound of tests/test_gpu_train.py
  GatFn at 'bf16x3'                        d kernel, d a_self, d a_nbr (the wide entry's three calls): the weight-gradient bound;
                                           d xa, d xb, d bias: 1e-4, the project's row-GEMM bound (TOL_ROWGEMM): d_hx is computed
                                           from an hx that carries the row GEMM's error
  a model step, switch on against off      WGRAD_TOL relative to each gradient's own maximum
uds_wgrad and uds_wgrad_wide agree on the shapes both take through the shared reference, never bitwise (different summation
orders; the wide entry sums d_bias in plain fp32).  Every call is repeated: torch.equal.

MEASURED on an MI355X (UDS_TOL_REPORT=1), worst observed / allowed per test over all its cases [case]:
  test_wgrad_wide, d_kernel                              0.180  [B2T3R33-F128-H64-s1]          err 1.80e-5
  test_wgrad_wide, d_bias                                0.004  [B1T1R40-F20-H16-s0]           err 4.82e-7 (plain fp32 sums)
  test_wide_entry_on_the_shapes_uds_wgrad_takes          0.165  [B1T1R77-F127-H32-s0]          err 1.25e-5, uds_wgrad beside it the same;
                                                         d_bias 0.005 wide, 0.216 uds_wgrad [B1T1R128-F16-H1-s0]
  test_dense_backward_at_the_default_widths   dW 0.145 [64-128], db 0.004, dX 0.107 [128-64]
  test_conv1d_backward_at_the_default_widths  dW 0.141 [dil 1], db 0.002, dX 0.011
  test_gat_backward_at_the_default_widths     d kernel 0.162 (err 1.50e-5), d a_self 0.157, d a_nbr 0.165 of the weight-gradient
                                              bound; d xb 0.044, d bias 0.001 of 1e-4
  test_default_size_model_step                           0.763  [Conv1D, block1.layers.1.gat_x.attn_kernel_self], 0.588 [GRU,
                                                         block1.layers.0.gat_x.attn_kernel_self]: the 2 x 128 `da` gradient, whose own
                                                         maximum is small beside the products it sums
No bound was raised.

The step of the default-size model counts 6 library-route calls with the switch on, not 0: the embedding layers (embed_x 5 -> 128,
embed_e 4 -> 128, embed_b and embed_ae 1 -> 64) are exact-fp32 layers at every model size, and the routing keeps 'fp32' layers on
the library GEMM as before.  test_default_size_model_step asserts that these six are the only ones and that no 'bf16x3' layer's
weight gradient takes the library route.
"""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import autograd as AG
from oracle import emulator_ref as OE
from oracle import sparse_csr as OS
from oracle import spektral_dense as OD
from tests import rowgemm_util as RU
from tests import wgrad_wide_util as WU
from tests.rowgemm_util import wgrad_inputs, wgrad_ref
from tests.util import Guarded, close, emulator_args, emulator_norms, load_emulator, nan_in
from tests.wgrad_wide_util import case_id, wide_inputs

pytestmark = pytest.mark.gpu

WGRAD_TOL = 3e-5
TOL_DX = 4e-5
TOL_GAT = 1e-4


def wtol(rows):
    return WGRAD_TOL * max(1.0, (rows / 1000.0) ** 0.5)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture()
def counts():
    """autograd.ROUTE_COUNTS reset to zero."""
    for k in AG.ROUTE_COUNTS:
        AG.ROUTE_COUNTS[k] = 0
    return AG.ROUTE_COUNTS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_wide(dev, c, a, g):
    B, T, R, F, H = c['B'], c['T'], c['R'], c['F'], c['H']
    lib = _lib.load()
    n_ws = lib.uds_wgrad_wide_workspace_floats(B * T * R, F, H, int(c['bias']))
    assert n_ws == WU.workspace_floats(B * T * R, F, H) > 0
    nan = lambda *shape: torch.full(shape, float('nan'), device=dev)
    ws, dk = Guarded((n_ws,), dev, nan(n_ws)), Guarded((F, H), dev, nan(F, H))
    db = Guarded((H,), dev, nan(H)) if c['bias'] else None
    rc = lib.uds_wgrad_wide(a.data_ptr(), g.data_ptr(), B, T, R, F, H, c['shift'], int(c['bias']), ws.view.data_ptr(), dk.view.data_ptr(),
                            db.view.data_ptr() if db else None, _stream())
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    ws.check('workspace')
    dk.check('d_kernel')
    if db:
        db.check('d_bias')
    return dk.view, db.view if db else None


def check_wide(dev, case, p):
    a, g = nan_in(p['a'], dev), nan_in(p['g'], dev)
    ref_k, ref_b = wgrad_ref(p['a'], p['g'], case['shift'])
    dk, db = run_wide(dev, case, a, g)
    tol = wtol(case['B'] * case['T'] * case['R'])
    ek = float((dk.double().cpu() - ref_k).abs().max())
    print('wide %-40s d_kernel err %.3e allowed %.3e' % (case_id(case), ek, tol * max(1.0, float(ref_k.abs().max()))))
    if case['shift'] >= case['T']:
        assert torch.equal(dk.cpu(), torch.zeros(case['F'], case['H']))
    close(dk, ref_k, tol)
    if case['bias']:
        eb = float((db.double().cpu() - ref_b).abs().max())
        print('wide %-40s d_bias   err %.3e allowed %.3e' % (case_id(case), eb, tol * max(1.0, float(ref_b.abs().max()))))
        close(db, ref_b, tol)
    dk2, db2 = run_wide(dev, case, a, g)
    assert torch.equal(dk, dk2) and (db is None or torch.equal(db, db2))
    return a, g


# ---- the C entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WU.WIDE_CASES, ids=case_id)
def test_wgrad_wide(dev, case):
    check_wide(dev, case, wide_inputs(case))


@pytest.mark.parametrize('case', [c for c in RU.WGRAD_CASES if c['B'] * c['T'] * c['R'] <= 5000], ids=RU.case_id)
def test_wide_entry_on_the_shapes_uds_wgrad_takes(dev, case):
    """The wide entry on uds_wgrad's own cases and data, and uds_wgrad beside it: both within the bound of the one reference."""
    p = wgrad_inputs(case)
    a, g = check_wide(dev, case, p)
    ref_k, ref_b = wgrad_ref(p['a'], p['g'], case['shift'])
    dk, db = _lib.wgrad(a, g, case['shift'], case['bias'])
    tol = wtol(case['B'] * case['T'] * case['R'])
    close(dk, ref_k, tol)
    if case['bias']:
        close(db, ref_b, tol)


def test_zero_rows_give_zeros(dev):
    ws, dk, db = Guarded((4,), dev), Guarded((130, 70), dev), Guarded((70,), dev)
    nan = torch.full((4,), float('nan'), device=dev)
    rc = _lib.load().uds_wgrad_wide(nan.data_ptr(), nan.data_ptr(), 0, 3, 5, 130, 70, 1, 1, ws.view.data_ptr(), dk.view.data_ptr(),
                                    db.view.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    dk.check('d_kernel')
    db.check('d_bias')
    assert not dk.view.any() and not db.view.any()


@pytest.mark.parametrize('F,H,with_bias', WU.WIDE_REFUSED)
def test_refusals_launch_nothing(dev, F, H, with_bias):
    from tests.util import SENTINEL
    lib = _lib.load()
    a, g = torch.zeros(1, 1, 4, F, device=dev), torch.zeros(1, 1, 4, H, device=dev)
    ws, dk, db = Guarded((4096,), dev), Guarded((F, H), dev), Guarded((H,), dev)
    rc = lib.uds_wgrad_wide(a.data_ptr(), g.data_ptr(), 1, 1, 4, F, H, 0, int(with_bias), ws.view.data_ptr(), dk.view.data_ptr(),
                            db.view.data_ptr(), _stream())
    assert rc == -22 and lib.uds_last_error().startswith(b'uds_wgrad_wide:')
    with pytest.raises(_lib.UdsError):
        _lib.wgrad_wide(a, g, 0, with_bias)
    torch.cuda.synchronize()
    for t in (ws, dk, db):
        assert bool((t.buf.view(torch.int32) == SENTINEL).all())


# ---- through autograd at the default widths ---------------------------------------------------------------------------------
def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float().double()      # fp32 values: the device sees the same numbers


def leaf(t):
    return t.clone().requires_grad_(True)


def dev_leaf(t, dev):
    return t.float().to(dev).requires_grad_(True)


class _Mod:
    """the attributes the Functions read from a module"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize('rows,fi,fo', [(150, 128, 64), (150, 64, 128), (150, 128, 192)], ids=['128-64', '64-128', 'gru-projection-128-192'])
def test_dense_backward_at_the_default_widths(dev, counts, rows, fi, fo):
    g = torch.Generator().manual_seed(rows + fi + fo)
    lim = (6.0 / (fi + fo)) ** 0.5
    x, k, b, gy = rnd(g, 2, rows, fi) - 0.5, (rnd(g, fi, fo) * 2 - 1) * lim, rnd(g, fo) - 0.5, rnd(g, 2, rows, fo) - 0.5
    xr, kr, br = leaf(x), leaf(k), leaf(b)
    (OD.dense(xr, kr, br, 'linear') * gy).sum().backward()
    xd, kd, bd = dev_leaf(x, dev), dev_leaf(k, dev), dev_leaf(b, dev)
    m = _Mod(precision='bf16x3', units=fo, kernel=kd)
    (AG.DenseFn.apply(xd, kd, bd, m, 'linear') * gy.float().to(dev)).sum().backward()
    assert counts == {'wgrad': 0, 'wgrad_wide': 1, 'library': 0}
    close(xd.grad, xr.grad, TOL_DX)
    close(kd.grad, kr.grad, wtol(2 * rows))
    close(bd.grad, br.grad, wtol(2 * rows))


@pytest.mark.parametrize('dil', [1, 2])
def test_conv1d_backward_at_the_default_widths(dev, counts, dil):
    B, T, R, F, H = 2, 7, 9, 128, 64
    g = torch.Generator().manual_seed(T + R + dil)
    lim = (6.0 / (3 * F + 3 * H)) ** 0.5
    x, k, b, gy = rnd(g, B, T, R, F) - 0.5, (rnd(g, 3, F, H) * 2 - 1) * lim, rnd(g, H) - 0.5, rnd(g, B, T, R, H) - 0.5
    xr, kr, br = leaf(x), leaf(k), leaf(b)
    ref = OE.conv1d_causal(xr.permute(0, 2, 1, 3).reshape(B * R, T, F), kr, br, dil, 'linear').reshape(B, R, T, H).permute(0, 2, 1, 3)
    (ref * gy).sum().backward()
    xd, kd, bd = dev_leaf(x, dev), dev_leaf(k, dev), dev_leaf(b, dev)
    m = _Mod(precision='bf16x3', activation='linear', dilation_rate=dil, kernel=kd)
    (AG.Conv1DFn.apply(xd, kd, bd, m) * gy.float().to(dev)).sum().backward()
    # two taps without the bias row (128 x 64: uds_wgrad takes them), the bias-carrying tap is 129 rows
    assert counts == {'wgrad': 2, 'wgrad_wide': 1, 'library': 0}
    close(xd.grad, xr.grad, TOL_DX)
    close(kd.grad, kr.grad, wtol(B * T * R))
    close(bd.grad, br.grad, wtol(B * T * R))


def test_gat_backward_at_the_default_widths(dev, counts):
    """GatFn on a 40-node network, xa 128 and xb 64 wide, d = 128: d kernel = [xa | xb]^T d_hx (128 x 128 and 64 x 128) and the
    attention vectors' gradient (2 x 128) all come from the wide entry."""
    n, S, fa, fb, d = 40, 3, 128, 64, 128
    edges = U.synthetic_drainage_network(n, 44, seed=3)
    csr = U.DrainageGraph.from_edges(edges, n).adj
    g = torch.Generator().manual_seed(n + d)
    lim = (6.0 / (fa + fb + d)) ** 0.5
    xa, xb = rnd(g, S, n, fa) - 0.5, rnd(g, S, n, fb) - 0.5
    k, a_s, a_n, b = (rnd(g, fa + fb, 1, d) * 2 - 1) * lim, rnd(g, d, 1, 1) - 0.5, rnd(g, d, 1, 1) - 0.5, rnd(g, d) - 0.5
    gy = rnd(g, S, n, d) - 0.5
    ref_in = [leaf(t) for t in (xa, k, a_s, a_n, b, xb)]
    z = torch.cat([ref_in[0], ref_in[5]], dim=-1)
    (OS.gat_conv_csr(z, csr.rowptr, csr.col, ref_in[1], ref_in[2], ref_in[3], ref_in[4], 'linear') * gy).sum().backward()
    dv = [dev_leaf(t, dev) for t in (xa, k, a_s, a_n, b, xb)]
    out = AG.GatFn.apply(dv[0], dv[5], dv[1], dv[2], dv[3], dv[4], 'linear', _lib.CsrHandle(csr), 'bf16x3')
    (out * gy.float().to(dev)).sum().backward()
    assert counts['library'] == 0 and counts['wgrad_wide'] == 3
    names = ('xa', 'kernel', 'a_self', 'a_nbr', 'bias', 'xb')
    for name, got, ref in zip(names, dv, ref_in):
        # the three weight gradients are the wide entry's work: its own bound; the others inherit the row GEMM's error through hx
        tol = wtol(S * n) if name in ('kernel', 'a_self', 'a_nbr') else TOL_GAT
        err = float((got.grad.double().cpu() - ref.grad).abs().max())
        print('gat %-7s err %.3e allowed %.3e' % (name, err, tol * max(1.0, float(ref.grad.abs().max()))))
        close(got.grad, ref.grad, tol)


def test_shift_beyond_int32_drops_every_term(dev):
    """A shift that does not fit 32 bits is a shift past T: d_kernel exactly zero, d_bias the full column sum."""
    case = WU.SHIFT_CASES[4]
    p = wide_inputs(case)
    a, g = nan_in(p['a'], dev), nan_in(p['g'], dev)
    dk, db = run_wide(dev, dict(case, shift=(1 << 32) + 1), a, g)
    assert not dk.any()
    close(db, wgrad_ref(p['a'], p['g'], case['T'])[1], wtol(case['B'] * case['T'] * case['R']))


# ---- a default-size model: one training step per temporal net ---------------------------------------------------------------
def _step(emul, dev_in):
    xd, ad, bd, yd, exd, eyd = dev_in
    emul.zero_grad(set_to_none=True)
    ae = emul.get_edge_action(ad, True)
    preds, edge_preds = emul._model(xd, ad, bd, exd, ae, None, True)
    lw = emul._loss_setup(preds.device)
    (emul.get_node_loss(yd, bd, preds) + emul.get_flood_loss(yd, preds) + emul._mse(eyd, edge_preds, lw['ewei'])).backward()
    return {name: p.grad.detach().clone() for name, p in emul.named_parameters()}


@pytest.mark.parametrize('recurrent', ['Conv1D', 'GRU'])
def test_default_size_model_step(dev, counts, monkeypatch, recurrent):
    """embed_size 128, hidden_dim 64, 2 + 2 layers, 60 nodes / 66 links, T = 6, flood channel: with the switch on no weight
    gradient of a 'bf16x3' layer takes the library route (the exact-fp32 embedding layers keep it: see the header), and every
    parameter's gradient is the one of the same step with the switch off within the weight-gradient bound."""
    n, B, T = 60, 2, 6
    edges = U.synthetic_drainage_network(n, 66, seed=5)
    args = emulator_args(edges, n, embed_size=128, hidden_dim=64, seq_in=T, seq_out=T, n_sp_layer=2, n_tp_layer=2, recurrent=recurrent)
    norms = emulator_norms(args)
    c = OE.config(args)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, precision='bf16x3')
    load_emulator(emul, OE.init_params(args, seed=1), dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    emul.requires_grad_(True)
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.rand(*s, generator=g)
    x, b, ex, a = r(B, T, n, c.n_in), r(B, T, n, c.b_in) * 0.1, r(B, T, len(edges), c.e_in), r(B, T, len(args.act_edges))
    y, ey = r(B, T, n, 5), r(B, T, len(edges), 3)
    y[..., -2] = (y[..., -2] > 0.7).float()
    dev_in = tuple(t.to(dev) for t in (x, a, b, y, ex, ey))
    seen, route = [], AG.weight_grad_route
    monkeypatch.setattr(AG, 'weight_grad_route', lambda F, H, wb, prec: seen.append((route(F, H, wb, prec), F, H, prec)) or seen[-1][0])
    on = _step(emul, dev_in)
    moved = dict(counts)
    # The embedding layers (embed_x 5 -> 128, embed_e 4 -> 128, embed_b and embed_ae 1 -> 64) are exact-fp32 layers at every model
    # size: the routing rules keep 'fp32' on the library, as it was.  Every other weight gradient of the step is off it.
    assert [s for s in seen if s[0] == 'library' and s[3] == 'bf16x3'] == []
    assert sorted(s[1:] for s in seen if s[0] == 'library') == [(1, 64, 'fp32')] * 2 + [(4, 128, 'fp32')] * 2 + [(5, 128, 'fp32')] * 2
    assert moved['library'] == 6 and moved['wgrad_wide'] > 0 and sum(moved.values()) == len(seen)
    monkeypatch.setattr(AG, 'WIDE_WGRAD', False)
    off = _step(emul, dev_in)
    assert counts['library'] == 12 + moved['wgrad_wide'] and counts['wgrad_wide'] == moved['wgrad_wide']      # exactly those calls moved
    print('%s: %r' % (recurrent, moved))
    tol = wtol(B * T * max(n, len(edges)))
    worst = (0.0, '')
    for name, ref in off.items():
        scale = float(ref.abs().max())
        err = float((on[name] - ref).abs().max())
        if scale > 0:
            worst = max(worst, (err / (tol * scale), name))
    print('%s: worst observed / allowed %.3f [%s]' % (recurrent, worst[0], worst[1]))
    for name, ref in off.items():
        err = float((on[name] - ref).abs().max())
        assert err <= tol * float(ref.abs().max()), '%s: %.3e vs max|grad| %.3e' % (name, err, float(ref.abs().max()))
