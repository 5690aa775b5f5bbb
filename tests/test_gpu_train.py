"""GPU parity of the reverse-mode path (`fit_eval`, emulator.py:440-484) against torch autograd over the
fp64 CPU oracle: every autograd Function of gnn_uds_amd/autograd.py on its own (RemainderFn: tests/test_gpu_remainder_routes.py,
beside the GEMM it runs forward and transposed), the gradients of all Emulator
parameters, and the parameters after Adam steps.  The oracle is "parity unpinned" (oracle/__init__.py): the reference
holds no gradients or trained weights to pin it.

Stated tolerances (relative to max(1, max|reference tensor|) unless said otherwise):
  exact-fp32 kernels ('fp32')         5e-6 per operator   (measured <= 4e-7)
  split-bf16 MFMA kernels ('bf16x3')  4e-5 per operator   (measured <= 2.2e-5)
  whole-model gradients               GRAD_TOL * max|grad of that tensor| + 1e-7 * max|grad of any tensor|: 1e-3 for the GAT models
                                      (measured <= 4e-4), 5e-3 for conv = GCN (measured <= 2.3e-3: the NodeEdge / Dense gradients there
                                      are 1e-6 of the largest gradient, i.e. at the split-bf16 noise floor of the sums they come from)
(UDS_TOL_REPORT=1 prints observed / allowed for every check.)
"""
import os

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import autograd as AG
from oracle import emulator_ref as OE
from oracle import sparse_csr as OS
from oracle import spektral_dense as OD
from oracle import train_ref as OT
from tests.util import close, emulator_args, emulator_norms, emulator_param_pairs, load_emulator

pytestmark = pytest.mark.gpu
GRAD_TOL = {'GAT': 1e-3, 'GCN': 5e-3, 'False': 1e-3}      # whole-model gradients, relative to the tensor's largest gradient


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)




def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def leaf(t):
    return t.clone().requires_grad_(True)


def dev_leaf(t, dev):
    return t.float().to(dev).requires_grad_(True)


class _Mod:
    """the attributes the Functions read from a module"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize('rows,fi,fo,act,prec', [(70, 64, 32, 'relu', 'bf16x3'), (70, 64, 64, 'tanh', 'bf16x3'), (33, 5, 64, 'linear', 'fp32'),
                                                 (50, 96, 32, 'relu', 'bf16x3'), (41, 32, 1, 'sigmoid', 'bf16x3'),
                                                 (20, 64, 3, 'hard_sigmoid', 'fp32')])
def test_dense_backward(dev, rows, fi, fo, act, prec):
    g = torch.Generator().manual_seed(rows + fo)
    x, k, b, gy = rnd(g, 2, rows, fi) - 0.5, rnd(g, fi, fo) - 0.5, rnd(g, fo) - 0.5, rnd(g, 2, rows, fo) - 0.5
    xr, kr, br = leaf(x), leaf(k), leaf(b)
    (OD.dense(xr, kr, br, act) * gy).sum().backward()
    xd, kd, bd = dev_leaf(x, dev), dev_leaf(k, dev), dev_leaf(b, dev)
    m = _Mod(precision=prec, units=fo, kernel=kd)
    (AG.DenseFn.apply(xd, kd, bd, m, act) * gy.float().to(dev)).sum().backward()
    tol = 5e-6 if prec == 'fp32' else 4e-5
    close(xd.grad, xr.grad, tol)
    close(kd.grad, kr.grad, tol)
    close(bd.grad, br.grad, tol)


@pytest.mark.parametrize('B,T,R,F,H,shift,bias', [(1, 1, 1000, 64, 32, 0, True), (1, 1, 77, 5, 64, 0, True), (1, 1, 300, 96, 64, 0, True),
                                                  (1, 1, 4000, 128, 64, 0, False), (2, 9, 40, 64, 64, 2, False), (1, 5, 33, 64, 3, 4, True),
                                                  (1, 1, 31, 1, 32, 0, True), (1, 3, 20000, 32, 16, 1, True)])
def test_wgrad_kernel(dev, B, T, R, F, H, shift, bias):
    """Split-K MFMA weight gradient (split-bf16, 3 products): 4e-5 * max(1, max|ref|) * sqrt(rows / 1000) (fp32 sums over rows)."""
    g = torch.Generator().manual_seed(R + F)
    a, gz = rnd(g, B, T, R, F) - 0.5, rnd(g, B, T, R, H) - 0.5
    ref = a[:, :T - shift].reshape(-1, F).t() @ gz[:, shift:].reshape(-1, H) if shift < T else torch.zeros(F, H, dtype=torch.float64)
    dk, db = _lib.wgrad(a.float().to(dev), gz.float().to(dev), shift, bias)
    tol = 4e-5 * max(1.0, (B * T * R / 1000) ** 0.5)
    close(dk, ref, tol)
    if bias:
        close(db, gz.reshape(-1, H).sum(0), tol)
    else:
        assert db is None
    dk2, _ = _lib.wgrad(a.float().to(dev), gz.float().to(dev), shift, bias)
    assert torch.equal(dk, dk2)                                   # fixed summation order: bitwise reproducible


@pytest.mark.parametrize('B,T,R,F,H,dil,act,prec', [(2, 7, 5, 64, 64, 1, 'relu', 'bf16x3'), (1, 12, 3, 64, 64, 4, 'relu', 'bf16x3'),
                                                    (2, 6, 4, 10, 6, 2, 'tanh', 'fp32'), (1, 9, 4200, 32, 32, 2, 'relu', 'bf16x3'),
                                                    (1, 23, 4100, 64, 64, 4, 'tanh', 'bf16x3'), (1, 30, 4100, 64, 64, 1, 'tanh', 'bf16x3')])    # smooth activation: 6M outputs always hold a few |y| < 1e-5 whose relu mask would flip
def test_conv1d_backward(dev, B, T, R, F, H, dil, act, prec):
    g = torch.Generator().manual_seed(T + R)
    x, k, b, gy = rnd(g, B, T, R, F) - 0.5, rnd(g, 3, F, H) - 0.5, rnd(g, H) - 0.5, rnd(g, B, T, R, H) - 0.5
    xr, kr, br = leaf(x), leaf(k), leaf(b)
    ref = OE.conv1d_causal(xr.permute(0, 2, 1, 3).reshape(B * R, T, F), kr, br, dil, act).reshape(B, R, T, H).permute(0, 2, 1, 3)
    (ref * gy).sum().backward()
    xd, kd, bd = dev_leaf(x, dev), dev_leaf(k, dev), dev_leaf(b, dev)
    m = _Mod(precision=prec, activation=act, dilation_rate=dil, kernel=kd)
    (AG.Conv1DFn.apply(xd, kd, bd, m) * gy.float().to(dev)).sum().backward()
    tol = 5e-6 if prec == 'fp32' else 4e-5
    close(xd.grad, xr.grad, tol)
    close(kd.grad, kr.grad, tol * (10 if R > 1000 else 1))       # sums over B*T*R rows
    close(bd.grad, br.grad, tol * (10 if R > 1000 else 1))


@pytest.mark.parametrize('name,d,fb,act', [('chaohu', 8, 0, 'relu'), ('shunqing', 64, 32, 'relu'), ('astlingen', 16, 4, 'tanh'),
                                           ('hub', 64, 0, 'linear')])
def test_gat_backward(dev, networks, name, d, fb, act):
    if name == 'hub':      # a junction with 30 conduits plus a chain: rows with more than 16 neighbours
        edges = np.array([[0, i] for i in range(1, 31)] + [[i, i + 1] for i in range(30, 45)])
        gph = U.DrainageGraph.from_edges(edges, 46)
    else:
        net = networks[name]
        gph = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    for csr in (gph.adj, gph.edge_adj):
        n, S, fa = csr.n_rows, 3, 12
        g = torch.Generator().manual_seed(n + d)
        xa, xb = rnd(g, S, n, fa) - 0.5, (rnd(g, S, n, fb) - 0.5 if fb else None)
        k, a_s, a_n, b = rnd(g, fa + fb, 1, d) - 0.5, rnd(g, d, 1, 1) - 0.5, rnd(g, d, 1, 1) - 0.5, rnd(g, d) - 0.5
        gy = rnd(g, S, n, d) - 0.5
        ref_in = [leaf(t) for t in (xa, k, a_s, a_n, b)] + ([leaf(xb)] if fb else [])
        z = ref_in[0] if not fb else torch.cat([ref_in[0], ref_in[5]], dim=-1)
        (OS.gat_conv_csr(z, csr.rowptr, csr.col, ref_in[1], ref_in[2], ref_in[3], ref_in[4], act) * gy).sum().backward()
        dv = [dev_leaf(t, dev) for t in (xa, k, a_s, a_n, b)] + ([dev_leaf(xb, dev)] if fb else [])
        h = _lib.CsrHandle(csr)
        out = AG.GatFn.apply(dv[0], dv[5] if fb else None, dv[1], dv[2], dv[3], dv[4], act, h, 'fp32')
        (out * gy.float().to(dev)).sum().backward()
        for got, ref in zip(dv, ref_in):
            close(got.grad, ref.grad, 1e-5)


def test_gat_backward_transposed_pattern_directed(dev):
    """A non-symmetric pattern (directed adjacency): the column pass must walk the true transpose."""
    rowptr = np.array([0, 2, 3, 6, 7], dtype=np.int32)
    col = np.array([0, 2, 1, 0, 1, 2, 3], dtype=np.int32)
    csr = U.graph.CSR(rowptr, col, 4, 4)
    g = torch.Generator().manual_seed(5)
    S, f, d = 2, 8, 8
    x, k, a_s, a_n, b, gy = (rnd(g, S, 4, f) - 0.5, rnd(g, f, 1, d) - 0.5, rnd(g, d, 1, 1) - 0.5, rnd(g, d, 1, 1) - 0.5, rnd(g, d) - 0.5,
                             rnd(g, S, 4, d) - 0.5)
    ref_in = [leaf(t) for t in (x, k, a_s, a_n, b)]
    (OS.gat_conv_csr(*ref_in[:1], rowptr, col, *ref_in[1:], 'relu') * gy).sum().backward()
    dv = [dev_leaf(t, dev) for t in (x, k, a_s, a_n, b)]
    h = _lib.CsrHandle(csr)
    ht, perm = h.transposed(dev)
    assert ht.n_rows == 4 and perm.cpu().tolist() == [0, 3, 2, 4, 1, 5, 6]       # column-major walk of the entries
    (AG.GatFn.apply(dv[0], None, dv[1], dv[2], dv[3], dv[4], 'relu', h, 'fp32') * gy.float().to(dev)).sum().backward()
    for got, ref in zip(dv, ref_in):
        close(got.grad, ref.grad, 1e-5)


@pytest.mark.parametrize('name,F', [('chaohu', 32), ('hague', 8)])
def test_spmm_backward_and_sddmm(dev, networks, name, F):
    net = networks[name]
    gph = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    for csr in (gph.inc_n, gph.inc_e):
        g = torch.Generator().manual_seed(csr.n_rows)
        S = 4
        val, x, gy = rnd(g, csr.nnz) - 0.5, rnd(g, S, csr.n_cols, F) - 0.5, rnd(g, S, csr.n_rows, F) - 0.5
        vr, xr = leaf(val), leaf(x)
        (OS.incidence_aggregate_csr(xr, csr.rowptr, csr.col, vr, csr.n_rows) * gy).sum().backward()
        vd, xd = dev_leaf(val, dev), dev_leaf(x, dev)
        h = _lib.CsrHandle(csr)
        (AG.SpmmFn.apply(vd, xd, h) * gy.float().to(dev)).sum().backward()
        close(xd.grad, xr.grad, 5e-6)
        close(vd.grad, vr.grad, 5e-6)


def test_cumsum_and_flow_balance_backward(dev, networks):
    g = torch.Generator().manual_seed(1)
    x, res, gy = rnd(g, 2, 6, 9, 8) - 0.5, rnd(g, 2, 1, 9, 8) - 0.5, rnd(g, 2, 6, 9, 8) - 0.5
    xr, rr = leaf(x), leaf(res)
    (torch.relu(torch.cumsum(xr, 1) + rr) * gy).sum().backward()
    xd, rd = dev_leaf(x, dev), dev_leaf(res, dev)
    (AG.CumsumActFn.apply(xd, rd, 'relu') * gy.float().to(dev)).sum().backward()
    close(xd.grad, xr.grad, 2e-6)
    close(rd.grad, rr.grad, 2e-6)

    net = networks['chaohu']
    edges = np.array(net['edges'])
    gph = U.DrainageGraph.from_edges(edges, net['n_node'])
    ne = torch.from_numpy(gph.inc_n.to_dense())
    flow = rnd(g, 4, gph.n_edge) - 0.5
    s_in, s_out = rnd(g, gph.n_node), rnd(g, gph.n_node)
    g_in, g_out = rnd(g, 4, gph.n_node) - 0.5, rnd(g, 4, gph.n_node) - 0.5
    fr = leaf(flow)
    pos, neg = ne.clamp(0, 1), ne.clamp(-1, 0).abs()
    fp, fn = fr.clamp(min=0).unsqueeze(-1), (-fr.clamp(max=0)).unsqueeze(-1)
    q_out, q_in = (pos @ fp + neg @ fn)[..., 0] * s_out, (neg @ fp + pos @ fn)[..., 0] * s_in
    ((q_in * g_in).sum() + (q_out * g_out).sum()).backward()
    f32 = lambda t: t.float().to(dev)
    fd = dev_leaf(flow, dev)
    qi, qo = AG.FlowBalanceFn.apply(fd, _lib.CsrHandle(gph.inc_n), f32(torch.as_tensor(gph.inc_n.val)), f32(s_in), f32(s_out),
                                    torch.as_tensor(edges, dtype=torch.int64, device=dev))
    ((qi * f32(g_in)).sum() + (qo * f32(g_out)).sum()).backward()
    close(fd.grad, fr.grad, 2e-6)


def _problem(networks, name, dev, seed=3, B=2, **over):
    net = networks[name]
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, **over)
    norms = emulator_norms(args)
    params = OE.init_params(args, seed=1)
    c = OE.config(args)
    g = torch.Generator().manual_seed(seed)
    T_out = c.seq_out * max(c.roll, 1)
    x, b, ex = rnd(g, B, c.seq_in, n, c.n_in), rnd(g, B, T_out, n, c.b_in) * 0.1, rnd(g, B, c.seq_in, len(edges), c.e_in)
    a = rnd(g, B, T_out, len(args.act_edges)) if c.act else None
    y = rnd(g, B, T_out, n, 5)
    y[..., -2] = (y[..., -2] > 0.7).double()
    ey = rnd(g, B, T_out, len(edges), 3)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, precision=over.get('precision', 'bf16x3'))
    load_emulator(emul, params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    f32 = lambda t: None if t is None else t.float().to(dev)
    return args, norms, params, emul, (x, a, b, y, ex, ey), tuple(f32(t) for t in (x, a, b, y, ex, ey))


@pytest.mark.parametrize('kind', ['GRU', 'LSTM'])
def test_recurrent_backward_matches_autograd_of_the_oracle(dev, kind):
    """Back-propagation through time of a 64-unit GRU / LSTM (uds_recurrent_backward + uds_wgrad with a time shift) against
    torch autograd over the fp64 step-by-step oracle (oracle.emulator_ref.gru_sequence / lstm_sequence, themselves pinned
    against torch.nn.GRU / LSTM in tests/test_oracle_emulator.py): ragged row count (37 = 2 blocks + 5), T = 9, two batch
    elements; gradients of the input, kernel, recurrent kernel and both biases, 1e-3 of each tensor's largest gradient."""
    from gnn_uds_amd.emulator import GRU, LSTM
    g = torch.Generator().manual_seed(7)
    B, T, R, F, H = 2, 9, 37, 64, 64
    G = 3 if kind == 'GRU' else 4
    mod = (GRU if kind == 'GRU' else LSTM)(H, in_features=F, generator=g, precision='bf16x3').to(dev)
    with torch.no_grad():
        mod.bias.add_(torch.randn(mod.bias.shape, generator=g).to(dev) * 0.1)
    x = torch.randn(B, T, R, F, generator=g, dtype=torch.float64)
    gy = torch.randn(B, T, R, H, generator=g, dtype=torch.float64)
    # fp64 reference: rows are independent series -> (B*R, T, F)
    ref_p = [p.detach().double().cpu().requires_grad_(True) for p in (mod.kernel, mod.recurrent_kernel, mod.bias)]
    xr = x.clone().requires_grad_(True)
    seq = xr.permute(0, 2, 1, 3).reshape(B * R, T, F)
    fn = OE.gru_sequence if kind == 'GRU' else OE.lstm_sequence
    yr = fn(seq, *ref_p).reshape(B, R, T, H).permute(0, 2, 1, 3)
    (yr * gy).sum().backward()
    xd = x.float().to(dev).requires_grad_(True)
    mod.requires_grad_(True)
    yd = mod(xd)
    close(yd, yr.detach(), 1e-5)
    (yd * gy.float().to(dev)).sum().backward()
    for name, got, ref in (('x', xd.grad, xr.grad), ('kernel', mod.kernel.grad, ref_p[0].grad),
                           ('recurrent_kernel', mod.recurrent_kernel.grad, ref_p[1].grad), ('bias', mod.bias.grad, ref_p[2].grad)):
        err = float((got.double().cpu() - ref).abs().max())
        assert err <= 1e-3 * float(ref.abs().max()), '%s %s: grad err %.3e vs max|grad| %.3e' % (kind, name, err, float(ref.abs().max()))


@pytest.mark.parametrize('name,over', [('astlingen', dict(recurrent='GRU', n_sp_layer=1, n_tp_layer=2)),      # the reference's default temporal net
                                       ('astlingen', dict(recurrent='LSTM', n_sp_layer=1, n_tp_layer=1, if_flood=0)),
                                       ('astlingen', dict(embed_size=8, hidden_dim=8, n_sp_layer=1, n_tp_layer=1, if_flood=1)),
                                       ('shunqing', dict()),
                                       ('hague', dict(act=False, if_flood=0, edge_fusion=False, resnet=False, n_sp_layer=1)),
                                       ('astlingen', dict(roll=2, seq_in=4, seq_out=2, n_sp_layer=1)),
                                       ('astlingen', dict(conv='GCN', act=False, if_flood=0, resnet=False, n_sp_layer=1)),
                                       ('astlingen', dict(conv='False', seq_in=5, seq_out=5, n_sp_layer=2)),      # the non-graph baseline
                                       ('astlingen', dict(activation='tanh', n_sp_layer=1)),      # args.activation other than relu
                                       ('astlingen', dict(activation='sigmoid', n_sp_layer=1, n_tp_layer=1))])
def test_emulator_gradients(dev, networks, name, over):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, name, dev, **over)
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
        ref = ref.reshape(got.shape)             # GCNConv kernels are (F, C), the oracle's parameter tree keeps (F, 1, C)
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        # relative to the tensor's own largest gradient; the absolute floor (fp32 epsilon of the LARGEST gradient of the model)
        # matters for attn_kernel_self, whose gradient is ~1e-24 (softmax is shift-invariant in s_self: exactly zero where
        # leaky_relu is linear), and for the NodeEdge weights under GCN (1e-6 of the largest gradient: split-bf16 noise)
        if os.environ.get('UDS_TOL_REPORT'):
            from tests.util import OBSERVED
            OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0] + ':' + pname, 0, err, GRAD_TOL[args.conv] * scale + 1e-7 * gmax))
        assert err <= GRAD_TOL[args.conv] * scale + 1e-7 * gmax, '%s: grad err %.3e vs max|grad| %.3e' % (pname, err, scale)
        n_checked += 1
    assert n_checked == len(list(emul.parameters()))


def test_fit_eval_steps_match_oracle_adam(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, embed_size=64, n_sp_layer=1, learning_rate=1e-3)
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
    for pname, p, ref in emulator_param_pairs(emul, after):
        err = float((p.detach().double().cpu() - ref).abs().max())
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)       # each step moves <= lr = 1e-3
    ev = emul.fit_eval(*dev_in, fit=False)
    assert len(ev) == 3 and all(np.isfinite(float(v)) for v in ev)


def test_grad_norm_task_weights_match_the_oracle(dev, networks):
    """GradNorm (`fit_grad_norm`, emulator.py:486-519): two updates of [alpha_reg, alpha_cls] against the fp64 restatement
    (oracle.train_ref.grad_norm_step); the weights stay at sum 2 and the weighted training step still runs."""
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, embed_size=64, n_sp_layer=1, gradnorm=True)
    x, a, b, y, ex, ey = cpu_in
    ini_ref = [float(l) for l in OT.losses(args, params, norms, x, a, b, y, ex, ey)]
    ini = [float(l) for l in emul.fit_eval(*dev_in, fit=False)]
    assert np.allclose(ini, ini_ref, rtol=2e-3, atol=1e-6)
    alpha = torch.ones(2, dtype=torch.float64)
    opt = OT.Adam(lr=1e-4, clipnorm=None)
    for _ in range(2):
        ref_loss = OT.grad_norm_step(args, params, norms, x, a, b, y, ex, ey, ini_ref, alpha, opt)
        got_loss = emul.fit_grad_norm(*dev_in, ini_ref)
        assert abs(float(got_loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)) + 1e-9
        got = emul._alphas(dev).detach().double().cpu()
        assert abs(float(got.sum()) - 2.0) < 1e-6 and torch.allclose(got, alpha, rtol=0, atol=2e-6), (got, alpha)
    ls = emul.fit_eval(*dev_in)                                  # the alpha-weighted step
    assert len(ls) == 3 and all(np.isfinite(float(v)) for v in ls)


def test_save_load_retrain_resumes_training(dev, networks, tmp_path):
    """`save` / `load(retrain=True)` (emulator.py:814-852) keep the optimizer moments + step count and the GradNorm task
    weights with their optimizer: two steps, save, two more -- against two steps, save, load into a FRESH emulator, two
    more.  The resumed run must retrace the uninterrupted one (same kernels, same inputs: the same numbers); without the
    optimizer state it would restart Adam's bias correction and differ in the first digit."""
    over = dict(embed_size=64, n_sp_layer=1, learning_rate=1e-3, gradnorm=True)
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, **over)
    ini = [float(l) for l in emul.fit_eval(*dev_in, fit=False)]
    for _ in range(2):
        emul.fit_eval(*dev_in)
        emul.fit_grad_norm(*dev_in, ini)
    emul.save(str(tmp_path))
    for name in ('model.pt', 'optim.pt', 'gradnorm.pt', 'norm_x.npy', 'norm_e.npy'):
        assert (tmp_path / name).exists(), name
    cont = []
    for _ in range(2):
        cont.append([float(l) for l in emul.fit_eval(*dev_in)])
        emul.fit_grad_norm(*dev_in, ini)
    _, _, _, fresh, _, _ = _problem(networks, 'astlingen', dev, **over)
    fresh.load(str(tmp_path), retrain=True)
    assert fresh._optimizer.t == 2 and fresh._alpha_optimizer.t == 2
    resumed = []
    for _ in range(2):
        resumed.append([float(l) for l in fresh.fit_eval(*dev_in)])
        fresh.fit_grad_norm(*dev_in, ini)
    assert np.allclose(resumed, cont, rtol=1e-6, atol=1e-9), (resumed, cont)
    for (n1, p1), (n2, p2) in zip(emul.named_parameters(), fresh.named_parameters()):
        assert torch.allclose(p1, p2, rtol=0, atol=1e-7), n1
    assert torch.allclose(emul._alphas(dev), fresh._alphas(dev), rtol=0, atol=1e-7)
    cold = _problem(networks, 'astlingen', dev, **over)[3]
    cold.load(str(tmp_path))                                     # weights and norms only: a fresh optimizer
    assert cold._optimizer is None
    with pytest.raises(FileNotFoundError):                          # a Keras weight file is read (tests/test_h5.py); none is here
        cold.load(str(tmp_path / 'model.h5'))


def test_fit_eval_reduces_the_loss(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'hague', dev, n_sp_layer=2, learning_rate=2e-3)
    first = sum(float(v) for v in emul.fit_eval(*dev_in))
    for _ in range(25):
        last = sum(float(v) for v in emul.fit_eval(*dev_in))
    assert last < 0.8 * first, (first, last)


def test_training_uses_no_cpu_fallback(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, n_sp_layer=1)
    emul.requires_grad_(True)
    with pytest.raises(_lib.UdsError):
        emul.forward(cpu_in[0].float().requires_grad_(True), cpu_in[2].float(), cpu_in[4].float(),
                     torch.ones(2, 5, emul.n_edge, 1))


@pytest.mark.parametrize('chunks', [1, 2])
def test_mpc_objective_and_gradient(dev, networks, chunks):
    """`gnn_uds_amd.mpc` (mpc.py:551-612 + astlingen.py:75-99): objective of a population of control sequences and its
    gradient with respect to the decision vector, one and two prediction chunks; against autograd over the fp64 oracle.
    Tolerances: objective 5e-4 relative, gradient 1e-2 * max|grad| (reverse mode through ~10 split-bf16 layers and the
    de-normalised post-processing; hard gates keep their oracle value on this input)."""
    from gnn_uds_amd import mpc as M
    net = networks['astlingen']
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, seq_in=4, seq_out=2, n_sp_layer=1, if_flood=1, epsilon=0.0)
    norms = emulator_norms(args)
    params = OE.init_params(args, seed=3)
    c = OE.config(args)
    g = torch.Generator().manual_seed(11)
    T = c.seq_out * chunks
    state, runoff, edge_state = rnd(g, c.seq_in, n, 5), rnd(g, T, n, 1) * 0.05, rnd(g, c.seq_in, len(edges), 4)
    state[..., 3] = (state[..., 3] > 0.8).double()
    pop, n_step, n_act, r_step = 3, chunks, len(args.act_edges), 2
    y = 0.2 + 0.6 * rnd(g, pop, n_step * n_act)
    tg = dict(flood_idx=torch.tensor([3, 7, 11]), flood_w=torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64),
              outflow_idx=torch.tensor([0]), outflow_w=torch.tensor([0.3], dtype=torch.float64),
              smooth_idx=torch.tensor([5, 9]), smooth_w=torch.tensor([0.7, 0.2], dtype=torch.float64))
    gamma = torch.tensor([1.0, 0.9, 0.8, 0.7][:T], dtype=torch.float64)
    yr = y.clone().requires_grad_(True)
    ref = OE.mpc_objective(args, params, norms, yr, state, runoff, edge_state, n_step, n_act, r_step, tg, gamma)
    (gref,) = torch.autograd.grad(ref.sum(), yr)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    f = lambda t: t.float().to(dev)
    tgd = {k: (v.to(dev) if v.dtype == torch.int64 else f(v)) for k, v in tg.items()}
    obj, grad = M.objective_and_gradient(emul, f(y), f(state), f(runoff), f(edge_state), n_step, n_act, r_step, tgd, f(gamma))
    assert tuple(obj.shape) == (pop,) and tuple(grad.shape) == tuple(y.shape)
    close(obj, ref.detach(), 2e-5)
    gmax = float(gref.abs().max())
    assert gmax > 0
    err = float((grad.double().cpu() - gref).abs().max())
    if os.environ.get('UDS_TOL_REPORT'):
        from tests.util import OBSERVED
        OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0] + ':gradient', 0, err, 2e-3 * gmax))
    assert err <= 2e-3 * gmax, 'gradient err %.3e vs max|grad| %.3e' % (err, gmax)
    # Hessian-vector product (mpc.py:616-624): central difference of the HIP gradient against the SAME difference of the fp64
    # oracle's gradient (the scheme is the definition here; the exact product differs from both by O(eps^2) away from kinks)
    pvec = rnd(g, pop, n_step * n_act) - 0.5
    eps = 1e-2 / float(pvec.abs().max())

    def oracle_grad(yy):
        yy = yy.clone().requires_grad_(True)
        return torch.autograd.grad(OE.mpc_objective(args, params, norms, yy, state, runoff, edge_state, n_step, n_act, r_step, tg, gamma).sum(), yy)[0]
    href = (oracle_grad(y + eps * pvec) - oracle_grad(y - eps * pvec)) / (2 * eps)
    hp = M.hessp(emul, f(y), f(pvec), f(state), f(runoff), f(edge_state), n_step, n_act, r_step, tgd, f(gamma))
    assert tuple(hp.shape) == tuple(y.shape)
    herr = float((hp.double().cpu() - href).abs().max())
    # the difference quotient divides the gradient's own error (<= 2e-3 gmax, measured ~2e-4) by 2 eps
    assert herr <= 2e-3 * gmax / eps, 'hessp err %.3e vs max|Hp| %.3e (max|grad| %.3e, eps %.3e)' % (herr, float(href.abs().max()), gmax, eps)


def test_c5_block_diagonal_batch_forward_backward(dev):
    """BASELINE.json config 5 in its own form -- G mini-graphs as ONE block-diagonal network, training forward + backward of the
    L-layer spatial block (what `bench.py --workload c5` times, there with 1000 x 2000-node graphs) -- against autograd over the
    fp64 sparse oracle on the batched network, plus the property the batching rests on: every mini-graph's rows equal those of
    that graph run alone (no leakage across the diagonal blocks)."""
    G, n1, e1, d, L = 12, 300, 360, 64, 2
    nets = [U.synthetic_drainage_network(n1, e1, seed=k) for k in range(G)]
    g = U.DrainageGraph.from_edges(np.concatenate([ed + n1 * k for k, ed in enumerate(nets)]), n1 * G)
    assert g.n_node == n1 * G and g.n_edge == e1 * G
    block = U.SpatialBlock(g, d, L, 'relu', sparse_params=True, generator=torch.Generator().manual_seed(1)).to(dev)
    block.requires_grad_(True)
    gen = torch.Generator().manual_seed(2)
    x, e = torch.rand(1, g.n_node, d, generator=gen), torch.rand(1, g.n_edge, d, generator=gen)
    tx, te = torch.rand(1, g.n_node, d, generator=gen), torch.rand(1, g.n_edge, d, generator=gen)
    ox, oe = block(x.to(dev), e.to(dev))
    loss = torch.nn.functional.mse_loss(ox, tx.to(dev)) + torch.nn.functional.mse_loss(oe, te.to(dev))
    loss.backward()
    # fp64 oracle with autograd on the same batched network
    csr = lambda c: (c.rowptr, c.col)
    ps = []
    for ly in block.layers:
        p = {k: (v.double().clone().requires_grad_(True) if v is not None else None) for k, v in ly.export_params().items()}
        ps.append(p)
    rx, re = x.double(), e.double()
    for p in ps:
        rx, re = OS.spatial_layer_csr(rx, re, p, csr(g.adj), csr(g.edge_adj), csr(g.inc_n), csr(g.inc_e))
    rloss = torch.nn.functional.mse_loss(rx, tx.double()) + torch.nn.functional.mse_loss(re, te.double())
    rloss.backward()
    close(ox.detach(), rx.detach(), 4e-5)
    assert abs(float(loss.detach()) - float(rloss.detach())) <= 4e-5 * max(1.0, abs(float(rloss.detach())))
    names = {'xe_k': ('dense_xe', 'kernel'), 'xe_b': ('dense_xe', 'bias'), 'ex_k': ('dense_ex', 'kernel'), 'gx_k': ('gat_x', 'kernel'),
             'gx_as': ('gat_x', 'attn_kernel_self'), 'ge_an': ('gat_e', 'attn_kernel_neighs'), 'ge_b': ('gat_e', 'bias'),
             'ne_n_v': ('node_edge_n', 'weight'), 'ne_e_v': ('node_edge_e', 'weight')}
    worst = max(float(p[k].grad.abs().max()) for p in ps for k in names)
    for ly, p in zip(block.layers, ps):
        for k, (mod, attr) in names.items():
            got, want = getattr(getattr(ly, mod), attr).grad.double().cpu().reshape(p[k].grad.shape), p[k].grad
            lim = GRAD_TOL['GAT'] * float(want.abs().max()) + 1e-7 * worst
            assert float((got - want).abs().max()) <= lim, (k, float((got - want).abs().max()), lim)
    # one mini-graph alone: same rows (forward)
    k = 5
    g1 = U.DrainageGraph.from_edges(nets[k], n1)
    b1 = U.SpatialBlock(g1, d, L, 'relu', sparse_params=True).to(dev)
    for l1, lb in zip(b1.layers, block.layers):
        for m in ('dense_xe', 'dense_ex', 'gat_x', 'gat_e'):
            getattr(l1, m).load_state_dict(getattr(lb, m).state_dict())
        sel = lambda csr_b, lo, hi: torch.as_tensor(np.nonzero((csr_b.rows() >= lo) & (csr_b.rows() < hi))[0], device=dev)
        l1.node_edge_n.weight.data = lb.node_edge_n.weight.data[sel(g.inc_n, n1 * k, n1 * (k + 1))].clone()
        l1.node_edge_e.weight.data = lb.node_edge_e.weight.data[sel(g.inc_e, e1 * k, e1 * (k + 1))].clone()
        l1.node_edge_n.bias.data = torch.zeros_like(l1.node_edge_n.weight.data)
        l1.node_edge_e.bias.data = torch.zeros_like(l1.node_edge_e.weight.data)
    with torch.no_grad():
        sx, se = b1(x[:, n1 * k:n1 * (k + 1)].to(dev).contiguous(), e[:, e1 * k:e1 * (k + 1)].to(dev).contiguous())
    assert float((sx - ox[:, n1 * k:n1 * (k + 1)].detach()).abs().max()) <= 4e-5 * max(1.0, float(sx.abs().max()))
    assert float((se - oe[:, e1 * k:e1 * (k + 1)].detach()).abs().max()) <= 4e-5 * max(1.0, float(se.abs().max()))


def test_c5_at_size_100_minigraphs_of_2000_nodes(dev):
    """BASELINE.json config 5 at a tenth of its stated batch and its stated graph size: 100 mini-graphs x (2 000 nodes,
    2 500 links) = 200 000 / 250 000 rows as ONE block-diagonal network, 3-layer block, training forward + backward.  The
    oracle at that size is the fp64 sparse restatement with autograd on two SAMPLED mini-graphs: block-diagonal batching
    means a mini-graph's outputs and input gradients are those of the graph run alone with its slice of the parameters.
    Activation tanh: among the 38 M relu outputs of this batch a few lie within rounding of zero, where the fp32 and the fp64
    masks differ and a gradient entry is off by a whole term (observed: 3.8e-6 on a largest gradient of 6.7e-4) -- a property
    of the kink, not of the kernels (test_conv1d_backward makes the same choice at 6 M outputs)."""
    G, n1, e1, d, L, ACT = 100, 2000, 2500, 64, 3, 'tanh'
    nets = [U.synthetic_drainage_network(n1, e1, seed=k) for k in range(G)]
    g = U.DrainageGraph.from_edges(np.concatenate([ed + n1 * k for k, ed in enumerate(nets)]), n1 * G)
    block = U.SpatialBlock(g, d, L, ACT, sparse_params=True, generator=torch.Generator().manual_seed(1)).to(dev)
    block.requires_grad_(True)
    gen = torch.Generator().manual_seed(2)
    x, e = torch.rand(1, g.n_node, d, generator=gen), torch.rand(1, g.n_edge, d, generator=gen)
    gx, ge = torch.rand(1, g.n_node, d, generator=gen) - 0.5, torch.rand(1, g.n_edge, d, generator=gen) - 0.5
    xd, ed_ = x.to(dev).requires_grad_(True), e.to(dev).requires_grad_(True)
    ox, oe = block(xd, ed_)
    ((ox * gx.to(dev)).sum() + (oe * ge.to(dev)).sum()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in block.parameters())
    csr = lambda c: (c.rowptr, c.col)
    for k in (7, 93):
        g1 = U.DrainageGraph.from_edges(nets[k], n1)
        ns, es = slice(n1 * k, n1 * (k + 1)), slice(e1 * k, e1 * (k + 1))
        sel = lambda c, lo, hi: torch.as_tensor(np.nonzero((c.rows() >= lo) & (c.rows() < hi))[0])
        ps = []
        for ly in block.layers:
            p = {kk: (v.double() if v is not None else None) for kk, v in ly.export_params().items()}
            p['ne_n_v'] = p['ne_n_v'][sel(g.inc_n, n1 * k, n1 * (k + 1))]
            p['ne_e_v'] = p['ne_e_v'][sel(g.inc_e, e1 * k, e1 * (k + 1))]
            ps.append(p)
        rx, re = x[:, ns].double().requires_grad_(True), e[:, es].double().requires_grad_(True)
        hx, he = rx, re
        for p in ps:
            hx, he = OS.spatial_layer_csr(hx, he, p, csr(g1.adj), csr(g1.edge_adj), csr(g1.inc_n), csr(g1.inc_e), act=ACT)
        ((hx * gx[:, ns].double()).sum() + (he * ge[:, es].double()).sum()).backward()
        close(ox[:, ns].detach(), hx.detach(), 4e-5)
        close(oe[:, es].detach(), he.detach(), 4e-5)
        for got, want in ((xd.grad[:, ns], rx.grad), (ed_.grad[:, es], re.grad)):
            err = float((got.double().cpu() - want).abs().max())
            assert err <= GRAD_TOL['GAT'] * float(want.abs().max()), (k, err, float(want.abs().max()))
