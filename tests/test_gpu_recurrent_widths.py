"""GRU / LSTM temporal layers at hidden_dim 16 .. 128 (multiples of 16): inference at 128 units (uds_recurrent_forward with the
recurrent kernel streamed from global memory), back-propagation through time at every width (uds_recurrent_backward_h), the
whole Emulator's gradients and Adam steps -- against torch autograd over the fp64 oracle (oracle.emulator_ref.gru_sequence /
lstm_sequence, oracle.train_ref.grads / Adam).

The bounds are those of tests/test_gpu_train.py, every entry of every tensor compared (sigmoid / tanh gates: no kink):
  layer forward                        1e-5 * max(1, max|ref|)            (`close`)
  layer gradients (x, kernel, recurrent_kernel, bias)   1e-3 * max|reference gradient of that tensor|
  whole-model gradients                1e-3 * max|grad of that tensor| + 1e-7 * max|grad of any tensor|, losses 2e-5, every parameter
  three Adam steps                     losses rtol 2e-3 / atol 1e-5, parameters 3e-4
(UDS_TOL_REPORT=1 prints observed / allowed for every check.)
"""
import os

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from oracle import train_ref as OT
from tests.util import OBSERVED, close, emulator_param_pairs
from tests.test_gpu_train import GRAD_TOL, _problem

pytestmark = pytest.mark.gpu

WIDTHS = [16, 32, 48, 80, 96, 112, 128]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _report(name, err, lim):
    if os.environ.get('UDS_TOL_REPORT') and lim > 0:      # (an exactly-zero reference gradient has no ratio to report)
        OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0] + ':' + name, 0, err, lim))


def _layer(kind, H, F, dev, seed=7):
    from gnn_uds_amd.emulator import GRU, LSTM
    g = torch.Generator().manual_seed(seed)
    mod = (GRU if kind == 'GRU' else LSTM)(H, in_features=F, generator=g, precision='bf16x3').to(dev)
    with torch.no_grad():
        mod.bias.add_(torch.randn(mod.bias.shape, generator=g).to(dev) * 0.1)          # non-zero input and recurrent biases
    return mod, g


def _oracle(kind, mod, x, gy=None):
    """fp64 reference of the layer on x (B, T, R, F): rows are independent series -> (B*R, T, F); with gy, the gradients too."""
    B, T, R, F = x.shape
    H = mod.units
    ref_p = [p.detach().double().cpu().requires_grad_(gy is not None) for p in (mod.kernel, mod.recurrent_kernel, mod.bias)]
    xr = x.clone().requires_grad_(gy is not None)
    fn = OE.gru_sequence if kind == 'GRU' else OE.lstm_sequence
    yr = fn(xr.permute(0, 2, 1, 3).reshape(B * R, T, F), *ref_p).reshape(B, R, T, H).permute(0, 2, 1, 3)
    if gy is not None:
        (yr * gy).sum().backward()
    return yr.detach(), xr, ref_p


def _check_layer_gradients(dev, kind, H, F, B, T, R):
    mod, g = _layer(kind, H, F, dev)
    x = torch.randn(B, T, R, F, generator=g, dtype=torch.float64)
    gy = torch.randn(B, T, R, H, generator=g, dtype=torch.float64)
    yr, xr, ref_p = _oracle(kind, mod, x, gy)
    xd = x.float().to(dev).requires_grad_(True)
    mod.requires_grad_(True)
    yd = mod(xd)
    close(yd, yr, 1e-5)
    (yd * gy.float().to(dev)).sum().backward()
    for name, got, ref in (('x', xd.grad, xr.grad), ('kernel', mod.kernel.grad, ref_p[0].grad),
                           ('recurrent_kernel', mod.recurrent_kernel.grad, ref_p[1].grad), ('bias', mod.bias.grad, ref_p[2].grad)):
        assert got is not None and tuple(got.shape) == tuple(ref.shape), name
        err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
        assert scale > 0 or (T == 1 and name == 'recurrent_kernel'), name      # one step from the zero state: d U is exactly zero
        print('%s H=%d F=%d T=%d R=%d %s: grad err %.3e, allowed %.3e' % (kind, H, F, T, R, name, err, 1e-3 * scale))
        _report(name, err, 1e-3 * scale)
        assert err <= 1e-3 * scale, '%s H=%d %s: grad err %.3e vs max|grad| %.3e' % (kind, H, name, err, scale)


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
@pytest.mark.parametrize('H,F', [(h, 64) for h in WIDTHS] + [(32, 32), (128, 128)])
def test_recurrent_backward_matches_autograd_of_the_oracle_at_every_width(dev, kind, H, F):
    """test_gpu_train.test_recurrent_backward_matches_autograd_of_the_oracle at the other widths: ragged row count (37 = 2
    blocks + 5), T = 9, two batch elements, non-zero biases; F = H is a second temporal layer's input."""
    _check_layer_gradients(dev, kind, H, F, B=2, T=9, R=37)


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
@pytest.mark.parametrize('H,T,R', [(48, 1, 37), (128, 1, 37), (48, 9, 32), (128, 9, 48)])
def test_recurrent_backward_single_step_and_whole_row_blocks(dev, kind, H, T, R):
    """T = 1 (the zero initial state only: no recurrent product reaches dh) and R = 16 k exactly (no ragged last block)."""
    _check_layer_gradients(dev, kind, H, 64, B=2, T=T, R=R)


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
def test_inference_at_128_units(dev, kind):
    """GRU(128) / LSTM(128) without gradients: the recurrent kernel (128 x 384 / 512 floats) does not fit the LDS."""
    mod, g = _layer(kind, 128, 64, dev)
    x = torch.randn(2, 9, 37, 64, generator=g, dtype=torch.float64)
    yr, _, _ = _oracle(kind, mod, x)
    with torch.no_grad():
        yd = mod(x.float().to(dev))
    close(yd, yr, 1e-5)
    # and the LSTM's cell states, which the backward pass reads
    if kind == 'LSTM':
        xp = (x @ mod.kernel.detach().double().cpu() + mod.bias.detach().double().cpu()).float().to(dev)
        h, c = _lib.recurrent_forward_train(xp, mod.recurrent_kernel, None, 'LSTM')
        assert torch.equal(h, _lib.recurrent_forward(xp, mod.recurrent_kernel, None, 'LSTM'))
        k, u, b = (p.detach().double().cpu() for p in (mod.kernel, mod.recurrent_kernel, mod.bias))
        seq = x.permute(0, 2, 1, 3).reshape(2 * 37, 9, 64)
        hs, cs = torch.zeros(74, 128, dtype=torch.float64), torch.zeros(74, 128, dtype=torch.float64)
        for t in range(9):
            a = seq[:, t] @ k + hs @ u + b
            i, f, gg, o = (a[:, 128 * j:128 * (j + 1)] for j in range(4))
            cs = torch.sigmoid(f) * cs + torch.sigmoid(i) * torch.tanh(gg)
            hs = torch.sigmoid(o) * torch.tanh(cs)
            close(c[:, t].reshape(74, 128), cs, 1e-5)


@pytest.mark.parametrize('over', [dict(recurrent='GRU', n_sp_layer=1, n_tp_layer=2, hidden_dim=32),
                                  dict(recurrent='GRU', n_sp_layer=1, n_tp_layer=2, hidden_dim=128),
                                  dict(recurrent='LSTM', n_sp_layer=1, n_tp_layer=1, if_flood=0, hidden_dim=128),
                                  dict(recurrent='LSTM', n_sp_layer=1, n_tp_layer=1, if_flood=0, hidden_dim=48)])
def test_emulator_gradients_at_other_widths(dev, networks, over):
    """test_gpu_train.test_emulator_gradients' procedure on astlingen with GRU / LSTM temporal nets of 32, 48 and 128 units."""
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, **over)
    x, a, b, y, ex, ey = cpu_in
    ref_losses, ref_grads = OT.grads(args, params, norms, x, a, b, y, ex, ey)
    emul.requires_grad_(True)
    xd, ad, bd, yd, exd, eyd = dev_in
    ae = emul.get_edge_action(ad, True) if emul.act else None
    preds, edge_preds = emul._model(xd, ad, bd, exd, ae, None, True)
    lw = emul._loss_setup(dev)
    ls = [emul.get_node_loss(yd, bd, preds)] + ([emul.get_flood_loss(yd, preds)] if emul.if_flood else []) + [emul._mse(eyd, edge_preds, lw['ewei'])]
    for got, ref in zip(ls, ref_losses):
        close(got, ref, 2e-5)
    sum(ls).backward()
    n_checked = 0
    gmax = max(float(t.abs().max()) for t in ref_grads.values())
    for pname, p, ref in emulator_param_pairs(emul, ref_grads):
        got = p.grad.detach().double().cpu() if p.grad is not None else torch.zeros_like(ref)
        assert got.numel() == ref.numel()
        ref = ref.reshape(got.shape)
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        lim = GRAD_TOL[args.conv] * scale + 1e-7 * gmax
        print('%s: grad err %.3e, allowed %.3e' % (pname, err, lim))
        _report(pname, err, lim)
        assert err <= lim, '%s: grad err %.3e vs max|grad| %.3e' % (pname, err, scale)
        n_checked += 1
    assert n_checked == len(list(emul.parameters()))


def test_fit_eval_steps_match_oracle_adam_gru_128(dev, networks):
    """Three fit_eval Adam steps of the GRU hidden_dim = 128 model against OT.Adam over OT.grads
    (test_gpu_train.test_fit_eval_steps_match_oracle_adam's procedure and bounds)."""
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, recurrent='GRU', n_sp_layer=1, n_tp_layer=2, hidden_dim=128,
                                                         learning_rate=1e-3)
    x, a, b, y, ex, ey = cpu_in
    opt = OT.Adam(lr=1e-3)
    leaves = list(OT.tree_leaves(params))
    ref_hist = []
    for _ in range(3):
        ls, gr = OT.grads(args, params, norms, x, a, b, y, ex, ey)
        ref_hist.append([float(l) for l in ls])
        opt.step(leaves, gr)
    hist = [[float(l) for l in emul.fit_eval(*dev_in)] for _ in range(3)]
    for h, r in zip(hist, ref_hist):
        assert np.allclose(h, r, rtol=2e-3, atol=1e-5), (hist, ref_hist)
    after = dict(OT.tree_leaves(params))
    n_checked = 0
    for pname, p, ref in emulator_param_pairs(emul, after):
        err = float((p.detach().double().cpu() - ref.reshape(p.shape)).abs().max())
        print('%s: parameter after 3 Adam steps differs by %.3e, allowed 3.0e-04' % (pname, err))
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)       # each step moves <= lr = 1e-3
        n_checked += 1
    assert n_checked == len(list(emul.parameters()))
    ev = emul.fit_eval(*dev_in, fit=False)
    assert len(ev) == 3 and all(np.isfinite(float(v)) for v in ev)


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
def test_width_64_through_the_new_entry_is_the_old_kernel(dev, kind):
    """uds_recurrent_backward_h at H = 64 and uds_recurrent_backward: bitwise-equal dxp and darec on the same seeded input."""
    g = torch.Generator().manual_seed(11)
    B, T, R, H, G = 2, 9, 37, 64, 3 if kind == 'GRU' else 4
    f = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(dev)
    xp, U, gh = f(B, T, R, G * H), f(H, G * H), f(B, T, R, H)
    rb = f(G * H) if kind == 'GRU' else None
    h, c = _lib.recurrent_forward_train(xp, U, rb, kind)
    packed = _lib.recurrent_pack_bwd(U)
    dxp, darec = _lib.recurrent_backward(xp, packed, rb, h, c, gh, kind)            # routed to uds_recurrent_backward
    lib = _lib.load()
    dxp2, darec2 = torch.full_like(dxp, float('nan')), torch.full_like(darec, float('nan'))
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.uds_recurrent_backward_h(ptr(xp), ptr(packed), ptr(rb), ptr(h), ptr(c), ptr(gh), B, T, R, H, G - 3, ptr(dxp2), ptr(darec2),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.uds_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dxp, dxp2) and torch.equal(darec, darec2)
    # the library's own packing of a 64-unit kernel is the image the old entry takes
    n = lib.uds_recurrent_bwd_packed_bytes(64, G - 3)
    assert n == packed.numel() * 4
    own = torch.empty(n // 4, device=dev)
    assert lib.uds_recurrent_pack_bwd(ptr(U), 64, G - 3, ptr(own), torch.cuda.current_stream().cuda_stream) == 0, lib.uds_last_error()
    assert torch.equal(own.view(torch.int32), packed.view(torch.int32))


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
@pytest.mark.parametrize('H', [32, 128])
def test_recurrent_fn_is_bitwise_repeatable(dev, kind, H):
    """Two runs of RecurrentFn (forward + backward) on the same input give the same bits: nothing depends on arrival order."""
    from gnn_uds_amd import autograd as AG
    g = torch.Generator().manual_seed(H)
    B, T, R, G = 2, 9, 300, 3 if kind == 'GRU' else 4
    f = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(dev)
    xp0, U0, gh = f(B, T, R, G * H), f(H, G * H) * 0.3, f(B, T, R, H)
    rb0 = f(G * H) if kind == 'GRU' else None
    runs = []
    for _ in range(2):
        xp, U = xp0.clone().requires_grad_(True), U0.clone().requires_grad_(True)
        rb = None if rb0 is None else rb0.clone().requires_grad_(True)
        y = AG.RecurrentFn.apply(xp, U, rb, kind, 'bf16x3')
        (y * gh).sum().backward()
        runs.append([y.detach(), xp.grad, U.grad] + ([rb.grad] if rb is not None else []))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_unsupported_width_is_refused_under_gradients(dev):
    from gnn_uds_amd.emulator import GRU
    mod = GRU(24, in_features=64, generator=torch.Generator().manual_seed(1)).to(dev)
    x = torch.zeros(1, 3, 5, 64, device=dev)
    with torch.no_grad():
        assert tuple(mod(x).shape) == (1, 3, 5, 24)            # inference keeps running where the fp32 kernel fits
    mod.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r'16, 32, 48, 64, 80, 96, 112, 128'):
        mod(x)


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
@pytest.mark.parametrize('H', [16, 48, 64, 112, 128])
def test_packed_image_matches_the_host_restatement(dev, kind, H):
    """uds_recurrent_pack_bwd against the NumPy / torch restatement of the layout (tests/test_recurrent_width_plan.py), bit for bit."""
    from tests.test_recurrent_width_plan import reference_pack
    G = 3 if kind == 'GRU' else 4
    U = torch.randn(H, G * H, generator=torch.Generator().manual_seed(H + G))
    got = _lib.recurrent_pack_bwd(U.to(dev))
    assert got.numel() * 4 == _lib.recurrent_bwd_packed_bytes(H, G)
    assert torch.equal(got.cpu().view(torch.int16), reference_pack(U, G).reshape(-1))
