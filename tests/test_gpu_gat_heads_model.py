"""Multi-head GATConv through the layers and models, on the GPU, against the fp64 CPU oracle (oracle.spektral_dense.gat_conv_dense
is written for a (F, H, C) kernel; oracle.emulator_ref / oracle.train_ref run on parameters reshaped from the oracle's (F, 1, d) /
(d, 1, 1) to (F, H, C) / (C, H, 1) -- a relabelling of the same numbers).  Networks: astlingen (30 nodes / 29 links) and one
300-node synthetic network; n_sp_layer = 1 where a whole model is involved.

Bounds, those of the single-head counterparts (relative to max(1, max|ref|) through tests.util.close unless said otherwise):
  GATConv forward and coefficients   5e-6   tests/test_gpu_parity.py TOL (test_gat_forward_vs_dense_masked_oracle)
  GATConv gradients                  1e-5   tests/test_gpu_train.py test_gat_backward
  SpatialLayer                       5e-6 'fp32', 1e-5 'bf16x3'   tests/test_gpu_parity.py PREC_TOL
  Emulator / ConvNet forward         2e-5   tests/test_gpu_emulator.py TOL_FWD['bf16x3'] (5e-6 for an 'fp32' model)
  Emulator losses and gradients      2e-5 and 1e-3 * max|grad of the tensor| + 1e-7 * max|grad of any tensor|   tests/test_gpu_train.py
                                     GRAD_TOL['GAT'] (through tests/test_gpu_use_adj_train.py _check_model_grads)
  attention dropout at the layer     2e-5 forward, 1e-4 * max|grad| + 1e-7 gradients   tests/test_gpu_dropout.py
"""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import dist as D
from gnn_uds_amd.layers import DropoutStream
from oracle import dropout_ref as DR
from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from oracle import train_ref as OT
from tests.test_gpu_use_adj_train import _check_model_grads, _mask_moves_the_gradients, _ref_grads
from tests.util import cast, close, emulator_args, emulator_norms, load_emulator, load_spatial_layer, spatial_params

pytestmark = pytest.mark.gpu

TOL = 5e-6
TOL_GRAD = 1e-5
PREC_TOL = {'fp32': 5e-6, 'bf16x3': 1e-5}
TOL_FWD = {'fp32': 5e-6, 'bf16x3': 2e-5}
NETS = ['astlingen', 'syn300']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def nets(networks):
    return {'astlingen': (np.array(networks['astlingen']['edges']), networks['astlingen']['n_node']),
            'syn300': (np.asarray(U.synthetic_drainage_network(300, 360, 0)), 300)}


def rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def to_heads(kernel, a_self, a_nbr, H):
    """(F, 1, d), (d, 1, 1), (d, 1, 1) -> (F, H, C), (C, H, 1), (C, H, 1): the same numbers, relabelled."""
    F, _, d = kernel.shape
    return kernel.reshape(F, H, d // H).contiguous(), a_self.reshape(d // H, H, 1).contiguous(), a_nbr.reshape(d // H, H, 1).contiguous()


def reshape_tree(params, H):
    for key in ('block1', 'block2', 'block'):
        for q in params.get(key, []):
            for name in ('gat_x', 'gat_e', 'gat'):
                if name in q:
                    c = q[name]
                    c['kernel'], c['attn_kernel_self'], c['attn_kernel_neighs'] = to_heads(c['kernel'], c['attn_kernel_self'], c['attn_kernel_neighs'], H)
    return params


def entries(coef, csr):
    """The oracle's dense coefficients (..., N, H, N) at the entries of the pattern: (..., H, nnz)."""
    rows, cols = torch.as_tensor(csr.rows()), torch.as_tensor(np.asarray(csr.col, dtype=np.int64))
    return coef.transpose(-3, -2)[..., rows, cols]


# ---- GATConv ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('concat', [True, False], ids=['concat', 'mean'])
@pytest.mark.parametrize('H,C', [(2, 32), (4, 16), (3, 12)])
@pytest.mark.parametrize('name', NETS)
def test_gatconv_heads_against_the_dense_layer(dev, nets, name, H, C, concat):
    edges, n = nets[name]
    gph = U.DrainageGraph.from_edges(edges, n)
    g = torch.Generator().manual_seed(10 * H + C)
    S, F = 3, 20
    x = rnd(g, S, n, F) - 0.3
    k, a_s, a_n = rnd(g, F, H, C) - 0.5, rnd(g, C, H, 1) - 0.5, rnd(g, C, H, 1) - 0.5
    b = rnd(g, H * C if concat else C) - 0.5
    filt = torch.from_numpy(gph.adj.to_dense())
    filt[torch.arange(n), torch.arange(n)] = 0                                  # the layer must force the diagonal itself
    leaves = [t.clone().requires_grad_(True) for t in (x, k, a_s, a_n, b)]
    ref, coef = OD.gat_conv_dense(leaves[0], filt, *leaves[1:], act='tanh', concat_heads=concat, return_attn=True)
    gy = rnd(g, *ref.shape) - 0.5
    (ref * gy).sum().backward()

    layer = U.GATConv(C, attn_heads=H, concat_heads=concat, return_attn_coef=True, activation='tanh', in_channels=F).to(dev)
    assert tuple(layer.kernel.shape) == (F, H, C) and tuple(layer.attn_kernel_self.shape) == (C, H, 1) and tuple(layer.bias.shape) == tuple(b.shape)
    f = lambda t: t.float().to(dev)
    layer.kernel.data, layer.attn_kernel_self.data, layer.attn_kernel_neighs.data, layer.bias.data = f(k), f(a_s), f(a_n), f(b)
    a = filt.numpy()
    out, attn = layer([f(x), a])                                                # inference: no autograd
    close(out, ref.detach(), TOL)
    assert tuple(attn.shape) == (S, H, gph.adj.nnz)
    close(layer.dense_attn_coef(attn, a), coef.detach(), TOL)
    assert float((attn.sum(-1) - n).abs().max()) < 1e-3                          # every row's coefficients sum to one
    x4 = f(x).reshape(1, S, n, F)                                               # leading dims are preserved
    o4, a4 = layer([x4, a])
    assert o4.shape == (1,) + tuple(out.shape) and a4.shape == (1,) + tuple(attn.shape)
    assert torch.equal(layer([f(x), a], return_attn_coef=False), out)           # asking for the coefficients changes nothing

    layer.requires_grad_(True)
    xd = f(x).requires_grad_(True)
    out_t, attn_t = layer([xd, a])
    assert torch.equal(out_t.detach(), out) and torch.equal(attn_t, attn) and not attn_t.requires_grad
    (out_t * f(gy)).sum().backward()
    for got, want in zip((xd, layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias), leaves):
        assert float(want.grad.abs().max()) > 1e-3
        close(got.grad, want.grad, TOL_GRAD)


def test_gatconv_heads_attention_dropout(dev, nets):
    """Keras' training mode: one multiplier per (snapshot, head, pattern entry), S * H * nnz positions of the stream; the dense
    restatement is fed the same (S, H, nnz) mask through oracle.spektral_dense.ATTN_DROPOUT."""
    edges, n = nets['syn300']
    gph = U.DrainageGraph.from_edges(edges, n)
    csr = gph.adj
    g = torch.Generator().manual_seed(4)
    S, F, H, C = 3, 24, 4, 8
    x = torch.randn(S, n, F, generator=g, dtype=torch.float64)
    layer = U.GATConv(C, attn_heads=H, activation='tanh', in_channels=F, generator=g).to(dev)
    with torch.no_grad():
        layer.bias.normal_(0.0, 0.1)
    st = DropoutStream(seed=99)
    xd = x.float().to(dev).requires_grad_(True)
    layer.requires_grad_(True)
    out = layer([xd, csr], attn_dropout=st)
    assert st.offset == (S * H * csr.nnz + 3) // 4 * 4
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gy.float().to(dev)).sum().backward()
    mask = DR.dropout_mask(S * H * csr.nnz, 0.5, 99, 0).astype(np.float64).reshape(S, H, csr.nnz) * 2.0
    dense = np.zeros((S, H, n, n))
    dense[..., csr.rows(), np.asarray(csr.col, dtype=np.int64)] = mask
    dense = torch.from_numpy(dense).permute(0, 2, 1, 3)                         # (S, N, H, N)
    ref_p = [p.detach().double().cpu().requires_grad_(True) for p in (layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias)]
    xr = x.clone().requires_grad_(True)
    OD.ATTN_DROPOUT = lambda cf, a: cf * dense
    try:
        ref = OD.gat_conv_dense(xr, torch.from_numpy(csr.to_dense()), *ref_p, 'tanh')
    finally:
        OD.ATTN_DROPOUT = None
    (ref * gy).sum().backward()
    close(out.detach(), ref.detach(), 2e-5)
    with torch.no_grad():
        plain = layer([xd.detach(), csr])
    assert float((plain - out.detach()).abs().max()) > 1e-2                      # the mask does something
    for got, want in [(xd.grad, xr.grad)] + [(p.grad, r.grad) for p, r in zip((layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias), ref_p)]:
        err, scale = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        assert err <= 1e-4 * scale + 1e-7, (err, scale)


# ---- SpatialLayer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', NETS)
def test_spatial_layer_heads(dev, nets, name, precision):
    edges, n = nets[name]
    gph = U.DrainageGraph.from_edges(edges, n)
    d, H, S = 64, 4, 3
    p = spatial_params(gph.n_node, gph.n_edge, d, d, d, seed=7)
    for side in ('gx', 'ge'):
        p[side + '_k'], p[side + '_as'], p[side + '_an'] = to_heads(p[side + '_k'], p[side + '_as'], p[side + '_an'], H)
    g = torch.Generator().manual_seed(8)
    x, e = rnd(g, S, gph.n_node, d), rnd(g, S, gph.n_edge, d)
    ne = torch.from_numpy(gph.inc_n.to_dense())
    rx, re = OD.spatial_layer_dense(x, e, p, torch.from_numpy(gph.adj.to_dense()), torch.from_numpy(gph.edge_adj.to_dense()), ne)
    layer = U.SpatialLayer(gph, d, 'relu', sparse_params=False, precision=precision, attn_heads=H)
    assert tuple(layer.gat_x.kernel.shape) == (d + d // 2, H, d // H)
    load_spatial_layer(layer, p, dev)
    ox, oe = layer(x.float().to(dev), e.float().to(dev))
    assert layer.last_path == 'unfused'
    close(ox, rx, PREC_TOL[precision]); close(oe, re, PREC_TOL[precision])
    one = U.SpatialLayer(gph, d, 'relu', sparse_params=False, precision=precision)      # the single-head layer is what it was
    assert tuple(one.gat_x.kernel.shape) == (d + d // 2, 1, d) and one.attn_heads == 1


# ---- Emulator -------------------------------------------------------------------------------------------------------------------
def _problem(nets, name, dev, H, seed=3, B=2, use_adj=False, precision='bf16x3', **over):
    """tests/test_gpu_train.py's _problem (tests/test_gpu_use_adj_train.py's _adj_problem with use_adj) for args.attn_heads = H."""
    edges, n = nets[name]
    if use_adj:
        over.update(use_adj=True, act_edges=edges[::2])
    args = emulator_args(edges, n, attn_heads=H, n_sp_layer=1, **over)
    norms = emulator_norms(args)
    params = reshape_tree(OE.init_params(args, seed=1), H)
    c = OE.config(args)
    g = torch.Generator().manual_seed(seed)
    T_out = c.seq_out
    x, b, ex = rnd(g, B, c.seq_in, n, c.n_in), rnd(g, B, T_out, n, c.b_in) * 0.1, rnd(g, B, c.seq_in, len(edges), c.e_in)
    if use_adj:
        a = (rnd(g, B, T_out, len(args.act_edges)) > 0.4).double() * (0.5 + rnd(g, B, T_out, len(args.act_edges)))
    else:
        a = rnd(g, B, T_out, len(args.act_edges))
    y = rnd(g, B, T_out, n, 5)
    y[..., -2] = (y[..., -2] > 0.7).double()
    ey = rnd(g, B, T_out, len(edges), 3)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, precision=precision)
    load_emulator(emul, params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    cpu_in = (x, a, b, y, ex, ey)
    return args, norms, params, emul, cpu_in, tuple(t.float().to(dev) for t in cpu_in)


@pytest.mark.parametrize('name', NETS)
def test_emulator_heads_forward_and_gradients(dev, nets, name):
    args, norms, params, emul, cpu_in, dev_in = _problem(nets, name, dev, H=2)
    assert emul.attn_heads == 2 and tuple(emul.block1.layers[0].gat_x.kernel.shape)[1:] == (2, 32)
    x, a, b, y, ex, ey = cpu_in
    xd, ad, bd, yd, exd, eyd = dev_in
    c = OE.config(args)
    ry, rey = OE.forward(args, params, x, b, ex, OE.get_edge_action(c, a))
    with torch.no_grad():
        oy, oey = emul(xd, bd, exd, emul.get_edge_action(ad))
    assert emul.block1.layers[0].last_path == emul.block2.layers[0].last_path == 'unfused'
    close(oy, ry, TOL_FWD['bf16x3']); close(oey, rey, TOL_FWD['bf16x3'])
    assert reference_moves_by(args, params, norms, cpu_in, OT.grads, probes=2) < 0.1
    ref_losses, ref_grads = OT.grads(args, params, norms, x, a, b, y, ex, ey)
    _check_model_grads(emul, args, dev_in, ref_losses, ref_grads)


def reference_moves_by(args, params, norms, cpu_in, grads_fn, rel=1e-6, probes=4):
    """How far the fp64 reference gradients move, in units of the GRAD_TOL['GAT'] bound, when every parameter is perturbed by
    `rel` relative Gaussian noise (the order of the split-bf16 forward's error per product, 2^-16 ~ 1.5e-5 at most): a draw
    whose reference sits on a relu kink at that scale has no reference value to hold the kernels to.  Oracle only, ~0.1 s a probe."""
    import copy
    x, a, b, y, ex, ey = cpu_in
    _, g0 = grads_fn(args, params, norms, x, a, b, y, ex, ey)
    gmax = max(float(t.abs().max()) for t in g0.values())
    worst = 0.0
    for k in range(probes):
        gn = torch.Generator().manual_seed(k)
        q = copy.deepcopy(params)
        for _, t in OT.tree_leaves(q):
            t.data = t.data * (1 + rel * torch.randn(t.shape, generator=gn, dtype=torch.float64))
        _, g1 = grads_fn(args, q, norms, x, a, b, y, ex, ey)
        worst = max(worst, max(float((g0[n] - g1[n]).abs().max()) / (1e-3 * float(g0[n].abs().max()) + 1e-7 * gmax) for n in g0))
    return worst


def test_emulator_heads_use_adj(dev, nets):
    """use_adj: block 2's node side sees the per-time-step adjacency, one mask shared by the heads.

    Inputs from seed 4, not the 3 of tests/test_gpu_use_adj_train.py: with the parameters relabelled to two heads the fp64
    REFERENCE of the seed-3 draw sits on a relu kink of the last link-side temporal layer -- perturbing its parameters by 1e-6
    relative (noise seed 1 of reference_moves_by) moves block1.0.gat_e.bias by 3.07, block1.0.gat_e.kernel by 2.57 and tem2_e.1 by
    2.47 / 2.34 bounds, which is to the digit what the split-bf16 model showed against it on an MI355X (3.07, 2.57, 2.47, 2.33; the
    same model at precision='fp32': 0.001 of the bound; the single-head model on that draw: 0.010, its reference moving by 0.022).
    So the draw is chosen on the reference alone: the first seed from 3 upwards whose reference moves by less than a tenth of the
    bound under four such probes, and the test asserts that property before it compares anything.  Bounds unchanged."""
    args, norms, params, emul, cpu_in, dev_in = _problem(nets, 'astlingen', dev, H=2, seed=4, use_adj=True)
    assert emul.use_adj
    assert reference_moves_by(args, params, norms, cpu_in, _ref_grads) < 0.1
    x, a, b, y, ex, ey = cpu_in
    c = OE.config(args)
    ry, rey = OE.forward(args, params, x, b, ex, OE.get_edge_action(c, a), OE.get_adj_action(c, a))
    xd, ad, bd = dev_in[0], dev_in[1], dev_in[2]
    with torch.no_grad():
        oy, oey = emul(xd, bd, dev_in[4], emul.get_edge_action(ad), emul.get_adj_action(ad))
    close(oy, ry, TOL_FWD['bf16x3']); close(oey, rey, TOL_FWD['bf16x3'])
    ref_losses, ref_grads = _ref_grads(args, params, norms, x, a, b, y, ex, ey)
    _, free_grads = _ref_grads(args, params, norms, x, a, b, y, ex, ey, use_adj=False)
    assert _mask_moves_the_gradients(ref_grads, free_grads) > 10.0               # the check could not pass ignoring the mask
    _check_model_grads(emul, args, dev_in, ref_losses, ref_grads)


# ---- ConvNet --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,graph_base', [('astlingen', 0), ('astlingen', 1), ('syn300', 0)])
def test_convnet_heads(dev, nets, name, graph_base):
    edges, n = nets[name]
    H, d, h = 2, 64, 32
    args = emulator_args(edges, n, graph_base=graph_base, n_sp_layer=2, conv_dim=d, use_pred=False, if_flood=0, activation='relu', attn_heads=H)
    args.edge_state_shape = (len(edges), 3)
    gen = torch.Generator().manual_seed(7)
    gl = lambda *s: OE._glorot(gen, s)
    dense = lambda fi, fo: {'kernel': gl(fi, fo), 'bias': torch.randn(fo, generator=gen, dtype=torch.float64) * 0.05}
    conv = lambda f: {'kernel': gl(f, 1, d), 'attn_kernel_self': gl(d, 1, 1), 'attn_kernel_neighs': gl(d, 1, 1),
                      'bias': torch.randn(d, generator=gen, dtype=torch.float64) * 0.05}
    ne = lambda r, m: {'weight': torch.randn(r, m, generator=gen, dtype=torch.float64) * 0.05, 'bias': torch.zeros(r, m, dtype=torch.float64)}
    if graph_base:
        layers = [{'gat': conv(d)} for _ in range(2)]
    else:
        layers = [{'dense_xe': dense(d, h), 'dense_ex': dense(d, h), 'node_edge_n': ne(n, len(edges)), 'node_edge_e': ne(len(edges), n),
                   'gat_x': conv(d + h), 'gat_e': conv(d + h)} for _ in range(2)]
    params = reshape_tree({'embed_x': dense(4, d), 'embed_e': dense(3, d), 'block': layers, 'pool': {'attn_kernel': gl(d, 1)}}, H)
    X, E = rnd(gen, 6, n, 4), rnd(gen, 6, len(edges), 3)
    ref = OE.convnet_forward(args, params, X, E)
    m = U.ConvNet(args, 'GAT').to(dev)
    assert m.attn_heads == H
    f32 = lambda t: t.float().to(dev).contiguous()
    m.embed_x.kernel.data, m.embed_x.bias.data = f32(params['embed_x']['kernel']), f32(params['embed_x']['bias'])
    m.embed_e.kernel.data, m.embed_e.bias.data = f32(params['embed_e']['kernel']), f32(params['embed_e']['bias'])
    m.pool.attn_kernel.data = f32(params['pool']['attn_kernel'])

    def load_gat(mod, q):
        assert tuple(mod.kernel.shape) == tuple(q['kernel'].shape) and mod.kernel.shape[1] == H
        mod.kernel.data, mod.bias.data = f32(q['kernel']), f32(q['bias'])
        mod.attn_kernel_self.data, mod.attn_kernel_neighs.data = f32(q['attn_kernel_self']), f32(q['attn_kernel_neighs'])
    for ly, q in zip(m.block.layers, layers):
        if graph_base:
            load_gat(ly, q['gat'])
            continue
        for mod, key in ((ly.dense_xe, 'dense_xe'), (ly.dense_ex, 'dense_ex')):
            mod.kernel.data, mod.bias.data = f32(q[key]['kernel']), f32(q[key]['bias'])
        for mod, key in ((ly.node_edge_n, 'node_edge_n'), (ly.node_edge_e, 'node_edge_e')):
            mod.weight.data, mod.bias.data = f32(q[key]['weight']), f32(q[key]['bias'])
        load_gat(ly.gat_x, q['gat_x'])
        load_gat(ly.gat_e, q['gat_e'])
    close(m(f32(X), f32(E)), ref, TOL_FWD['bf16x3'])


# ---- Emulator.attention_coefficients --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,graph_base,precision', [(1, 0, 'bf16x3'), (1, 0, 'fp32'), (2, 0, 'bf16x3'), (1, 1, 'bf16x3')])
def test_attention_coefficients(dev, nets, monkeypatch, H, graph_base, precision):
    """A stock single-head model (and a two-head one, and graph_base) hands out what the oracle's layers return with return_attn,
    layer by layer; the model's ordinary forward is bit for bit what it was before the call."""
    args, norms, params, emul, cpu_in, dev_in = _problem(nets, 'astlingen', dev, H=H, precision=precision, graph_base=graph_base)
    x, a, b, y, ex, ey = cpu_in
    xd, ad, bd, exd = dev_in[0], dev_in[1], dev_in[2], dev_in[4]
    seen = []
    real = OD.gat_conv_dense

    def recording(*pos, **kw):
        out, coef = real(*pos, **dict(kw, return_attn=True))
        seen.append(coef.detach())
        return out
    c = OE.config(args)
    monkeypatch.setattr(OD, 'gat_conv_dense', recording)
    OE.forward(args, params, x, b, ex, OE.get_edge_action(c, a))
    monkeypatch.setattr(OD, 'gat_conv_dense', real)
    aed = emul.get_edge_action(ad)
    with torch.no_grad():
        before = emul(xd, bd, exd, aed)
        got = emul.attention_coefficients(xd, bd, exd, aed)
        after = emul(xd, bd, exd, aed)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    if H == 1 and not graph_base and precision == 'bf16x3':
        assert emul.block1.layers[0].last_path != 'unfused'                       # the ordinary forward is back on the fused kernel
    assert sorted(got) == ['block1', 'block2'] and len(got['block1']) == len(got['block2']) == 1
    B, tol = x.shape[0], TOL_FWD[precision]
    if graph_base:
        csr = emul._base_filter
        for blk, ref, T in (('block1', seen[0], c.seq_in), ('block2', seen[1], c.seq_out)):
            alpha = got[blk][0]
            assert tuple(alpha.shape) == (B, T, H, csr.nnz)
            close(alpha, entries(ref, csr).reshape(alpha.shape), tol)
        return
    assert len(seen) == 4                                                         # gat_x, gat_e of block 1, then of block 2
    for blk, refs, T in (('block1', seen[0:2], c.seq_in), ('block2', seen[2:4], c.seq_out)):
        ax, ae = got[blk][0]
        assert tuple(ax.shape) == (B, T, H, emul.graph.adj.nnz) and tuple(ae.shape) == (B, T, H, emul.graph.edge_adj.nnz)
        close(ax, entries(refs[0], emul.graph.adj).reshape(ax.shape), tol)
        close(ae, entries(refs[1], emul.graph.edge_adj).reshape(ae.shape), tol)
        assert float((ax.sum(-1) - emul.graph.adj.n_rows).abs().max()) < 1e-3


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, nets):
    edges, n = nets['astlingen']
    gph = U.DrainageGraph.from_edges(edges, n)
    with pytest.raises(ValueError, match='attn_heads'):
        U.SpatialLayer(gph, 64, 'relu', attn_heads=3)                            # 64 % 12
    with pytest.raises(ValueError, match='attn_heads'):
        U.SpatialBlock(gph, 40, 1, attn_heads=4)                                 # 40 % 16
    with pytest.raises(ValueError, match='attn_heads'):
        a = emulator_args(edges, n, attn_heads=3, n_sp_layer=1)
        U.Emulator(a.conv, a.resnet, a.recurrent, a)
    with pytest.raises(NotImplementedError, match='attn_heads'):
        U.SpatialLayer(gph, 64, 'relu', attn_heads=2).export_params()
    a = emulator_args(edges, n, attn_heads=2, n_sp_layer=1)
    emul = U.Emulator(a.conv, a.resnet, a.recurrent, a)
    with pytest.raises(NotImplementedError, match='attn_heads'):
        D.shard_emulator(emul, D.build_partition_plan(emul.graph, 2)[0], 'cpu')
    with pytest.raises(NotImplementedError, match='GAT'):
        g = emulator_args(edges, n, conv='GCN', act=False, if_flood=0, resnet=False, n_sp_layer=1)
        U.Emulator(g.conv, g.resnet, g.recurrent, g).to(dev).attention_coefficients(None, None, None)
