"""The RL agents' graph encoder `ConvNet` under training, and its Diffusion model, on the GPU against the fp64 CPU oracle.

Forward of ConvNet(args, 'Diffusion'): oracle.emulator_ref.convnet_forward (graph_base = 0); with graph_base = 1, where that
function only knows GAT, the same composition written out here from the oracle's Dense / DiffusionConv / softmax pool.
Bound: TOL_FWD['bf16x3'] of tests/test_gpu_emulator.py.

Gradients of the whole encoder: loss = (out * W).sum() for a fixed random W, fp64 autograd of the same reference, every
parameter plus the inputs X and E.  Bound per tensor, the project's (tests/test_gpu_train.py):
    GRAD_TOL[conv] * max|grad of the tensor| + 1e-7 * max|grad of any tensor|      (DIFF_GRAD_TOL for Diffusion)
B = 6, n_sp_layer = 2, conv_dim = 64, astlingen (30 nodes / 29 links).  As tests/test_gpu_gat_heads_model.py does, each case
first asserts on the fp64 reference ALONE that its gradients move by less than 0.1 of that bound when every parameter is
perturbed by 1e-6 relative noise: a draw on a relu kink has no reference value to hold the kernels to.  SEEDS holds the
seed of each configuration: 7, that of test_rl_convnet_encoder, has the property for all six (the reference moves by 0.0009 to
0.006 of the bound), so no configuration had to move on to the next seed.

Worst observed / allowed on an MI355X (UDS_TOL_REPORT=1):
  test_convnet_diffusion_forward   0.010 (shunqing)
  test_convnet_gradients           GAT 0.033 (one head) / 0.043 (two heads) at block.1.dense_ex.bias, 0.012 with graph_base = 1
                                   (pool.attn_kernel), GCN 0.003, Diffusion 0.002 / 0.006 (graph_base = 1); the forward under
                                   autograd at most 0.006 of TOL_FWD
"""
import copy
import math
import os

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from oracle import train_ref as OT
from tests.test_gpu_diffusion_train import DIFF_GRAD_TOL, THETA_SCALE
from tests.test_gpu_emulator import TOL_FWD
from tests.test_gpu_gat_heads_model import reshape_tree
from tests.test_gpu_train import GRAD_TOL
from tests.util import OBSERVED, close, emulator_args

pytestmark = pytest.mark.gpu

TOL = {'GAT': GRAD_TOL['GAT'], 'GCN': GRAD_TOL['GCN'], 'Diffusion': DIFF_GRAD_TOL}
# (conv, heads, graph_base) -> seed of the draw (parameters, inputs, W)
SEEDS = {('GAT', 1, 0): 7, ('GAT', 2, 0): 7, ('GCN', 1, 0): 7, ('Diffusion', 1, 0): 7, ('GAT', 1, 1): 7, ('Diffusion', 1, 1): 7}
D, HALF = 64, 32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def problem(networks, name, conv, heads, graph_base, seed, B=6):
    """args, oracle parameters (Keras shapes; (F, H, C) kernels for heads > 1) and fp64 inputs X, E, W."""
    edges, n = np.array(networks[name]['edges']), networks[name]['n_node']
    ne_ = len(edges)
    args = emulator_args(edges, n, graph_base=graph_base, n_sp_layer=2, conv_dim=D, use_pred=False, if_flood=0, activation='relu', conv=conv,
                         attn_heads=heads)
    args.edge_state_shape = (ne_, 3)
    gen = torch.Generator().manual_seed(seed)
    gl = lambda *s: OE._glorot(gen, s)
    bias = lambda k: torch.randn(k, generator=gen, dtype=torch.float64) * 0.05
    dense = lambda fi, fo: {'kernel': gl(fi, fo), 'bias': bias(fo)}
    if conv == 'Diffusion':
        # glorot-sized coefficients saturate the activation: shrunk as in tests/test_gpu_diffusion_train.py
        cv = lambda f: {'theta': (torch.rand(D, 7, generator=gen, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / 14) * THETA_SCALE}
    else:
        cv = lambda f: {'kernel': gl(f, 1, D), 'attn_kernel_self': gl(D, 1, 1), 'attn_kernel_neighs': gl(D, 1, 1), 'bias': bias(D)}
    nel = lambda r, m: {'weight': torch.randn(r, m, generator=gen, dtype=torch.float64) * 0.05, 'bias': torch.zeros(r, m, dtype=torch.float64)}
    if graph_base:
        layers = [{'gat': cv(D)} for _ in range(2)]
    else:
        layers = [{'dense_xe': dense(D, HALF), 'dense_ex': dense(D, HALF), 'node_edge_n': nel(n, ne_), 'node_edge_e': nel(ne_, n),
                   'gat_x': cv(D + HALF), 'gat_e': cv(D + HALF)} for _ in range(2)]
    params = {'embed_x': dense(4, D), 'embed_e': dense(3, D), 'block': layers, 'pool': {'attn_kernel': gl(D, 1)}}
    if heads > 1:
        params = reshape_tree(params, heads)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    return args, params, r(B, n, 4), r(B, ne_, 3), r(B, D) * 2 - 1


def reference(args, params, X, E):
    """fp64 ConvNet forward: the oracle's, or for graph_base Diffusion (which it does not build) the same composition."""
    if not (args.graph_base and args.conv == 'Diffusion'):
        return OE.convnet_forward(args, params, X, E)
    a = args.activation
    x = OD.dense(X, params['embed_x']['kernel'], params['embed_x']['bias'], a)
    e = OD.dense(E, params['embed_e']['kernel'], params['embed_e']['bias'], a)
    filt = OD.diffusion_preprocess(torch.from_numpy(np.asarray(args.adj, dtype=np.float64)))
    z = torch.cat([x, e], dim=-2)
    for p in params['block']:
        z = OD.diffusion_conv_dense(z, filt, p['gat']['theta'], a)
    alpha = torch.softmax((z @ params['pool']['attn_kernel']).squeeze(-1), dim=-1)
    return (alpha.unsqueeze(-2) @ z).squeeze(-2)


def load(m, params, conv, dev):
    """Copy the oracle parameters into the module; returns {oracle leaf name: module parameter} for every module parameter."""
    pairs = {}

    def put(p, name, t):
        p.data = t.float().to(dev).reshape(p.shape).contiguous()
        pairs[name] = p

    def put_conv(mod, q, prefix):
        if conv == 'Diffusion':
            put(mod.kernel, prefix + '.theta', q['theta'])
            return
        put(mod.kernel, prefix + '.kernel', q['kernel'])               # GCN: (F, 1, d) -> (F, d)
        put(mod.bias, prefix + '.bias', q['bias'])
        if conv == 'GAT':
            put(mod.attn_kernel_self, prefix + '.attn_kernel_self', q['attn_kernel_self'])
            put(mod.attn_kernel_neighs, prefix + '.attn_kernel_neighs', q['attn_kernel_neighs'])
    for key in ('embed_x', 'embed_e'):
        put(getattr(m, key).kernel, key + '.kernel', params[key]['kernel'])
        put(getattr(m, key).bias, key + '.bias', params[key]['bias'])
    put(m.pool.attn_kernel, 'pool.attn_kernel', params['pool']['attn_kernel'])
    for i, (ly, q) in enumerate(zip(m.block.layers, params['block'])):
        pre = 'block.%d.' % i
        if 'gat' in q:
            put_conv(ly, q['gat'], pre + 'gat')
            continue
        for key in ('dense_xe', 'dense_ex'):
            put(getattr(ly, key).kernel, pre + key + '.kernel', q[key]['kernel'])
            put(getattr(ly, key).bias, pre + key + '.bias', q[key]['bias'])
        for key in ('node_edge_n', 'node_edge_e'):
            put(getattr(ly, key).weight, pre + key + '.weight', q[key]['weight'])
            put(getattr(ly, key).bias, pre + key + '.bias', q[key]['bias'])
        cx, ce = (ly.gat_x, ly.gat_e) if conv == 'GAT' else (ly.gcn_x, ly.gcn_e)
        put_conv(cx, q['gat_x'], pre + 'gat_x')
        put_conv(ce, q['gat_e'], pre + 'gat_e')
    assert len(pairs) == len(list(m.parameters())), (sorted(pairs), [n for n, _ in m.named_parameters()])
    return pairs


def reference_grads(args, params, X, E, W):
    """d (reference(..) * W).sum() / d every leaf of params, X and E: {name: tensor}."""
    leaves = list(OT.tree_leaves(params)) + [('X', X), ('E', E)]
    ts = [t.detach().clone().requires_grad_(True) for _, t in leaves]
    tree = copy.deepcopy(params)
    for (name, _), t in zip(leaves[:-2], ts):
        node, parts = tree, name.split('.')
        for part in parts[:-1]:
            node = node[int(part)] if part.isdigit() else node[part]
        node[parts[-1]] = t
    out = reference(args, tree, ts[-2], ts[-1])
    gs = torch.autograd.grad((out * W).sum(), ts, allow_unused=True)
    return out.detach(), {name: (torch.zeros_like(t) if g is None else g) for (name, t), g in zip(leaves, gs)}


def bound(tol, ref, gmax):
    return tol * float(ref.abs().max()) + 1e-7 * gmax


def reference_moves_by(args, params, X, E, W, tol, names, rel=1e-6, probes=2):
    """The largest move of a compared reference gradient, in units of its bound, under `rel` relative Gaussian parameter noise."""
    _, g0 = reference_grads(args, params, X, E, W)
    gmax = max(float(g0[n].abs().max()) for n in names)
    worst = 0.0
    for k in range(probes):
        gn = torch.Generator().manual_seed(k)
        q = copy.deepcopy(params)
        for _, t in OT.tree_leaves(q):
            t.mul_(1 + rel * torch.randn(t.shape, generator=gn, dtype=torch.float64))
        _, g1 = reference_grads(args, q, X, E, W)
        worst = max(worst, max(float((g0[n] - g1[n]).abs().max()) / bound(tol, g0[n], gmax) for n in names))
    return worst


@pytest.mark.parametrize('name,graph_base', [('astlingen', 0), ('shunqing', 0), ('astlingen', 1)])
def test_convnet_diffusion_forward(dev, networks, name, graph_base):
    args, params, X, E, _ = problem(networks, name, 'Diffusion', 1, graph_base, 7)
    m = U.ConvNet(args, 'Diffusion').to(dev)
    load(m, params, 'Diffusion', dev)
    with torch.no_grad():
        out = m(X.float().to(dev), E.float().to(dev))
    assert m.pool.last_path == 'hip' and tuple(out.shape) == (6, D)
    close(out, reference(args, params, X, E), TOL_FWD['bf16x3'])


def test_convnet_names_what_is_built(networks):
    args = problem(networks, 'astlingen', 'GAT', 1, 0, 7)[0]
    with pytest.raises(NotImplementedError, match='GAT, GCN and Diffusion'):
        U.ConvNet(args, 'General')


@pytest.mark.parametrize('conv,heads,graph_base', sorted(SEEDS), ids=lambda v: str(v))
def test_convnet_gradients(dev, networks, conv, heads, graph_base):
    tol = TOL[conv]
    args, params, X, E, W = problem(networks, 'astlingen', conv, heads, graph_base, SEEDS[(conv, heads, graph_base)])
    m = U.ConvNet(args, conv).to(dev)
    pairs = load(m, params, conv, dev)
    names = sorted(pairs) + ['X', 'E']
    assert reference_moves_by(args, params, X, E, W, tol, names) < 0.1
    ref_out, ref = reference_grads(args, params, X, E, W)
    m.requires_grad_(True)
    Xd, Ed = X.float().to(dev).requires_grad_(True), E.float().to(dev).requires_grad_(True)
    out = m(Xd, Ed)
    assert m.pool.last_path == 'hip-train'
    close(out, ref_out, TOL_FWD['bf16x3'])
    (out * W.float().to(dev)).sum().backward()
    got = {n: p.grad for n, p in pairs.items()}
    got.update(X=Xd.grad, E=Ed.grad)
    gmax = max(float(ref[n].abs().max()) for n in names)
    assert float(ref['pool.attn_kernel'].abs().max()) > 0 and float(ref['X'].abs().max()) > 0 and float(ref['E'].abs().max()) > 0
    for n in names:
        assert got[n] is not None, n
        g, r = got[n].detach().double().cpu(), ref[n]
        r = r.reshape(g.shape)
        err, lim = float((g - r).abs().max()), bound(tol, r, gmax)
        if os.environ.get('UDS_TOL_REPORT'):
            OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0] + ':' + n, 0, err, lim))
        assert err <= lim, '%s: grad err %.3e vs max|grad| %.3e (bound %.3e)' % (n, err, float(r.abs().max()), lim)


def test_convnet_forward_is_the_pool_of_the_stack(dev, networks):
    """The GAT configuration of test_rl_convnet_encoder (shunqing, graph_base = 0): ConvNet.forward, which never concatenates, gives
    the bits of the pool over torch.cat([x, e], -2) of the same block outputs."""
    net = networks['shunqing']
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, graph_base=0, n_sp_layer=2, conv_dim=D, use_pred=False, if_flood=0, activation='relu')
    args.edge_state_shape = (len(edges), 3)
    m = U.ConvNet(args, 'GAT', generator=torch.Generator().manual_seed(7)).to(dev)
    gen = torch.Generator().manual_seed(8)
    X, E = torch.rand(6, n, 4, generator=gen).to(dev), torch.rand(6, len(edges), 3, generator=gen).to(dev)
    with torch.no_grad():
        out = m(X, E)
        assert m.pool.last_path == 'hip'
        x, e = m.block(m.embed_x(X), m.embed_e(E))
        assert torch.equal(out, m.pool(torch.cat([x, e], dim=-2)))
        assert torch.equal(out, _lib.attn_sum_pool(torch.cat([x, e], dim=-2).contiguous(), m.pool.attn_kernel))
