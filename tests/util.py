"""Shared helpers for the tests: seeded parameters in the oracle's (Keras-shaped) format."""
import inspect
import os

import numpy as np
import torch

# (test name, observed max abs error, allowed) of every close() call of the session: tests/conftest.py prints the largest
# observed / allowed ratios when UDS_TOL_REPORT is set, so that tolerances can be kept a stated factor above what the
# kernels actually achieve instead of orders of magnitude above it
OBSERVED = []


def close(out, ref, tol, _depth=1):
    """max|out - ref| <= tol * max(1, max|ref|); returns the observed error."""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = float((out - ref).abs().max()) if ref.numel() else 0.0
    lim = tol * max(1.0, float(ref.abs().max()) if ref.numel() else 1.0)
    if os.environ.get('UDS_TOL_REPORT'):
        fr = inspect.stack()[_depth]
        OBSERVED.append((os.environ.get('PYTEST_CURRENT_TEST', fr.function).split(' ')[0], fr.lineno, err, lim))
    assert err <= lim, 'max abs err %.3e > %.3e' % (err, lim)
    return err


def glorot(gen, shape, dtype):
    if len(shape) == 2:
        fan_in, fan_out = shape
    else:
        rf = int(np.prod(shape[:-2]))
        fan_in, fan_out = shape[-2] * rf, shape[-1] * rf
    lim = (6.0 / (fan_in + fan_out)) ** 0.5
    return ((torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1) * lim).to(dtype)


def spatial_params(n_node, n_edge, fx, fe, d, seed=1, dtype=torch.float64, bias_scale=0.1, dense_ne=True,
                   nnz_n=None, nnz_e=None):
    """Random parameters of one spatial layer (`emulator.py:225-230`), Keras shapes.  Biases are
    non-zero (trained-like) so bias handling is exercised."""
    g = torch.Generator().manual_seed(seed)
    h = d // 2
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype)
    p = {
        'xe_k': glorot(g, (fe, h), dtype), 'xe_b': rn(h) * bias_scale,
        'ex_k': glorot(g, (fx, h), dtype), 'ex_b': rn(h) * bias_scale,
        'gx_k': glorot(g, (fx + h, 1, d), dtype), 'gx_as': glorot(g, (d, 1, 1), dtype),
        'gx_an': glorot(g, (d, 1, 1), dtype), 'gx_b': rn(d) * bias_scale,
        'ge_k': glorot(g, (fe + h, 1, d), dtype), 'ge_as': glorot(g, (d, 1, 1), dtype),
        'ge_an': glorot(g, (d, 1, 1), dtype), 'ge_b': rn(d) * bias_scale,
    }
    if dense_ne:
        p.update({'ne_n_w': rn(n_node, n_edge) * 0.05, 'ne_n_b': torch.zeros(n_node, n_edge, dtype=dtype),
                  'ne_e_w': rn(n_edge, n_node) * 0.05, 'ne_e_b': torch.zeros(n_edge, n_node, dtype=dtype)})
    else:
        p.update({'ne_n_v': rn(nnz_n) * 0.05 + 0.3, 'ne_e_v': rn(nnz_e) * 0.05 + 0.3})
    return p


def cast(p, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in p.items()}


def load_spatial_layer(layer, p, device):
    """Copy oracle-format parameters into a gnn_uds_amd.layers.SpatialLayer."""
    f32 = lambda t: t.to(torch.float32).to(device).contiguous()
    layer.to(device)
    layer.dense_xe.kernel.data = f32(p['xe_k']); layer.dense_xe.bias.data = f32(p['xe_b'])
    layer.dense_ex.kernel.data = f32(p['ex_k']); layer.dense_ex.bias.data = f32(p['ex_b'])
    if 'ne_n_w' in p:
        layer.node_edge_n.weight.data = f32(p['ne_n_w']); layer.node_edge_n.bias.data = f32(p['ne_n_b'])
        layer.node_edge_e.weight.data = f32(p['ne_e_w']); layer.node_edge_e.bias.data = f32(p['ne_e_b'])
    else:
        layer.node_edge_n.weight.data = f32(p['ne_n_v']); layer.node_edge_n.bias.data = torch.zeros_like(layer.node_edge_n.weight.data)
        layer.node_edge_e.weight.data = f32(p['ne_e_v']); layer.node_edge_e.bias.data = torch.zeros_like(layer.node_edge_e.weight.data)
    layer.gat_x.kernel.data = f32(p['gx_k']); layer.gat_x.attn_kernel_self.data = f32(p['gx_as'])
    layer.gat_x.attn_kernel_neighs.data = f32(p['gx_an']); layer.gat_x.bias.data = f32(p['gx_b'])
    layer.gat_e.kernel.data = f32(p['ge_k']); layer.gat_e.attn_kernel_self.data = f32(p['ge_as'])
    layer.gat_e.attn_kernel_neighs.data = f32(p['ge_an']); layer.gat_e.bias.data = f32(p['ge_b'])
    return layer


# ---------------------------------------------------------------------------------------------------------------
# whole-emulator helpers
# ---------------------------------------------------------------------------------------------------------------
def emulator_args(edges, n_node, seed=0, **over):
    """A reference-style `args` namespace (attribute names of Emulator.__init__, emulator.py:48-127) for a link list."""
    from types import SimpleNamespace
    from oracle import graphs as OG
    edges = np.asarray(edges)
    rng = np.random.default_rng(seed)
    n_edge = len(edges)
    a = dict(state_shape=(n_node, 4), edge_state_shape=(n_edge, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=64,
             kernel_size=3, n_sp_layer=2, n_tp_layer=2, activation='relu', if_flood=3, epsilon=-1.0, edge_fusion=True,
             edges=edges, adj=over['adj'] if 'adj' in over else OG.adjacency(edges),
             edge_adj=over['edge_adj'] if 'edge_adj' in over else OG.edge_adjacency(edges),      # (networkx refuses chaohu's parallel link)
             node_edge=OG.node_edge_incidence(n_node, edges),
             act=True, act_edges=edges[[1, 4]], conv='GAT', resnet=True, recurrent='Conv1D', roll=0, model_dir='/tmp/uds_model',
             is_outfall=(np.arange(n_node) == 0).astype(float), hmax=1.0 + rng.random(n_node), hmin=np.zeros(n_node),
             area=np.zeros(n_node), pump=np.zeros(n_edge), pump_in=np.zeros(n_node), pump_out=np.zeros(n_node),
             offset=np.zeros(n_edge), ehmax=0.3 + rng.random(n_edge), tide=False)
    a.update(over)
    if a.get('graph_base'):                  # the reference passes the combined (N+E)^2 adjacency as `adj` (base.py:320-323)
        build = OG.node_based_adjacency if a['graph_base'] == 1 else OG.edge_based_adjacency
        a['adj'] = build(edges, a.get('directed', False), a.get('order', 1))
    return SimpleNamespace(**a)


def emulator_norms(args, seed=0, dtype=torch.float64):
    """[max, min] per node / link and channel (dataloader.py:224-266 layout): min = 0, max random positive."""
    g = torch.Generator().manual_seed(seed)
    n, e = args.state_shape[0], args.edge_state_shape[0]
    n_in = args.state_shape[1] + (1 if args.if_flood else 0)
    mk = lambda rows, c: torch.stack([0.5 + torch.rand(rows, c, generator=g, dtype=torch.float64),
                                      torch.zeros(rows, c, dtype=torch.float64)]).to(dtype)
    return {'x': mk(n, n_in), 'b': mk(n, 2 if args.tide else 1), 'y': mk(n, 5), 'r': mk(n, 1), 'e': mk(e, 4)}


def load_emulator(emul, p, device):
    """Copy oracle.emulator_ref.init_params parameters into a gnn_uds_amd.Emulator."""
    f32 = lambda t: t.to(torch.float32).to(device).contiguous()
    emul.to(device)

    def dense(m, q):
        m.kernel.data, m.bias.data = f32(q['kernel']), f32(q['bias'])

    def spatial(block, layers):
        if not emul.conv:                           # conv=False: the blocks are lists of Dense(2 d) layers
            for layer, q in zip(block, layers):
                dense(layer, q)
            return
        for layer, q in zip(block.layers, layers):
            if 'gat' in q:                      # graph_base: one conv over the stacked node + link rows
                if 'theta' in q['gat']:
                    layer.kernel.data = f32(q['gat']['theta'])
                    continue
                layer.kernel.data = f32(q['gat']['kernel'])
                layer.attn_kernel_self.data, layer.attn_kernel_neighs.data = f32(q['gat']['attn_kernel_self']), f32(q['gat']['attn_kernel_neighs'])
                layer.bias.data = f32(q['gat']['bias'])
                continue
            dense(layer.dense_xe, q['dense_xe']); dense(layer.dense_ex, q['dense_ex'])
            for ne, key in ((layer.node_edge_n, 'node_edge_n'), (layer.node_edge_e, 'node_edge_e')):
                ne.weight.data, ne.bias.data = f32(q[key]['weight']), f32(q[key]['bias'])
            convs = (layer.gat_x, layer.gat_e) if layer.conv == 'GAT' else (layer.gcn_x, layer.gcn_e)
            for m, key in zip(convs, ('gat_x', 'gat_e')):
                if layer.conv == 'Diffusion':
                    m.kernel.data = f32(q[key]['theta'])
                    continue
                if layer.conv == 'GAT':
                    m.kernel.data = f32(q[key]['kernel'])
                    m.attn_kernel_self.data, m.attn_kernel_neighs.data = f32(q[key]['attn_kernel_self']), f32(q[key]['attn_kernel_neighs'])
                else:
                    m.kernel.data = f32(q[key]['kernel'][:, 0, :])
                m.bias.data = f32(q[key]['bias'])

    dense(emul.embed_x, p['embed_x']); dense(emul.embed_b, p['embed_b']); dense(emul.embed_e, p['embed_e'])
    if emul.act:
        dense(emul.embed_ae, p['embed_ae'])
    spatial(emul.block1, p['block1']); spatial(emul.block2, p['block2'])
    for mods, key in ((emul.tem1_x, 'tem1_x'), (emul.tem1_e, 'tem1_e'), (emul.tem2_x, 'tem2_x'), (emul.tem2_e, 'tem2_e')):
        assert len(mods) == len(p[key])
        for m, q in zip(mods, p[key]):
            dense(m, q)
            if 'recurrent_kernel' in q:
                m.recurrent_kernel.data = f32(q['recurrent_kernel'])
    dense(emul.res_x, p['res_x']); dense(emul.res_e, p['res_e']); dense(emul.out, p['out'])
    for m, q in zip(emul.flood, p['flood']):
        dense(m, q)
    if emul.if_flood:
        dense(emul.flood_out, p['flood_out'])
    dense(emul.e_out_layer, p['e_out'])
    return emul


def emulator_param_pairs(emul, flat):
    """(name, module parameter, tensor) for every entry of `flat` -- a name -> tensor dict keyed like
    oracle.train_ref.tree_leaves(oracle params) ('block1.0.gat_x.kernel', 'tem1_x.1.bias', 'e_out.kernel', ...)."""
    out = []
    for name, t in flat.items():
        parts = name.split('.')
        m = emul
        for i, part in enumerate(parts[:-1]):
            if part == 'e_out':
                m = m.e_out_layer
            elif part in ('block1', 'block2'):
                m = getattr(m, part).layers if emul.conv else getattr(m, part)      # conv = False: a plain list of Dense layers
            elif part.isdigit():
                m = m[int(part)]
            elif part == 'gat' and not hasattr(m, 'gat'):
                pass                              # graph_base: the layer IS the conv
            elif part in ('gat_x', 'gat_e') and not hasattr(m, part):
                m = getattr(m, part.replace('gat', 'gcn'))      # conv = GCN: the oracle keeps the key, the module is gcn_x / gcn_e
            else:
                m = getattr(m, part)
        if parts[-1].startswith('attn_kernel') and not hasattr(m, parts[-1]):
            continue                              # conv = GCN: the oracle's parameter tree keeps the (unused) attention vectors
        out.append((name, getattr(m, parts[-1]), t))
    return out


# ---------------------------------------------------------------------------------------------------------------
# uds_dense_cumsum_heads: the cases and seeded inputs shared by tests/test_tail_ref_math.py (CPU: the cases can see a
# failure) and tests/test_gpu_tail_entries.py (GPU parity with oracle.tail_ref.dense_cumsum_heads_ref)
# ---------------------------------------------------------------------------------------------------------------
def _heads_case(B, R, T, n_a, n_hidden, act, act_a, act_h=None, act_f=None, res=True, bias=True, no_bias=()):
    """no_bias: the head layers whose bias is None -- 'a', 'h0' .. 'h4', 'f'."""
    assert (n_hidden > 0) == (act_h is not None) == (act_f is not None)
    assert n_hidden <= 1 or act_h not in ('sigmoid', 'hard_sigmoid')      # deeper, the flood output loses its signal
    return dict(B=B, R=R, T=T, n_a=n_a, n_hidden=n_hidden, act=act, act_a=act_a, act_h=act_h, act_f=act_f, res=res, bias=bias,
                no_bias=tuple(no_bias))


# (B, R) in {(1,1), (1,15), (1,16), (3,17), (2,33), (1,70)}: one row, a ragged single block, one full block, 6 units on 4-wave
# workgroups (the last workgroup half empty), a ragged third block, two workgroups; T in {1, 2, 3, 4, 7} round the input ring
# of 3; n_hidden 0..5 (4 and 5 at B > 1 and R no multiple of 16), n_a 1..4, every activation in every role
HEADS_CASES = [
    _heads_case(1, 1, 1, 1, 0, 'linear', 'hard_sigmoid'),
    _heads_case(1, 1, 3, 2, 1, 'relu', 'tanh', 'sigmoid', 'sigmoid'),
    _heads_case(1, 1, 7, 3, 5, 'relu', 'linear', 'relu', 'tanh'),
    _heads_case(1, 15, 2, 3, 2, 'tanh', 'linear', 'relu', 'hard_sigmoid'),
    _heads_case(1, 15, 7, 4, 3, 'relu', 'sigmoid', 'tanh', 'tanh'),
    _heads_case(1, 15, 3, 1, 4, 'hard_sigmoid', 'linear', 'tanh', 'tanh'),
    _heads_case(1, 16, 4, 1, 1, 'sigmoid', 'relu', 'hard_sigmoid', 'linear'),
    _heads_case(1, 16, 3, 3, 0, 'hard_sigmoid', 'tanh', res=False),
    _heads_case(1, 16, 7, 2, 5, 'tanh', 'tanh', 'relu', 'tanh', no_bias=('h3',)),
    _heads_case(1, 16, 1, 4, 1, 'relu', 'relu', 'tanh', 'relu'),
    _heads_case(3, 17, 7, 3, 4, 'relu', 'hard_sigmoid', 'relu', 'tanh'),
    _heads_case(3, 17, 4, 2, 5, 'linear', 'linear', 'tanh', 'relu'),
    _heads_case(3, 17, 1, 1, 3, 'relu', 'tanh', 'relu', 'linear', no_bias=('h1', 'f')),
    _heads_case(3, 17, 2, 4, 2, 'sigmoid', 'hard_sigmoid', 'tanh', 'linear', res=False, bias=False),
    _heads_case(3, 17, 3, 1, 0, 'tanh', 'sigmoid'),
    _heads_case(2, 33, 3, 4, 5, 'relu', 'hard_sigmoid', 'relu', 'linear', bias=False),
    _heads_case(2, 33, 2, 1, 4, 'tanh', 'sigmoid', 'tanh', 'hard_sigmoid', res=False),
    _heads_case(2, 33, 4, 3, 1, 'linear', 'sigmoid', 'relu', 'sigmoid', no_bias=('a',)),
    _heads_case(2, 33, 7, 2, 3, 'relu', 'hard_sigmoid', 'relu', 'sigmoid'),
    _heads_case(2, 33, 1, 2, 2, 'hard_sigmoid', 'relu', 'linear', 'linear', no_bias=('h0',)),
    _heads_case(1, 70, 1, 2, 2, 'linear', 'relu', 'linear', 'tanh'),
    _heads_case(1, 70, 7, 4, 0, 'relu', 'hard_sigmoid', no_bias=('a',)),
    _heads_case(1, 70, 4, 3, 4, 'linear', 'tanh', 'tanh', 'hard_sigmoid'),
    _heads_case(1, 70, 2, 1, 5, 'relu', 'sigmoid', 'tanh', 'relu', no_bias=('h4', 'a')),
]


def heads_case_id(c):
    s = 'B%dR%dT%d-a%d%s-h%d' % (c['B'], c['R'], c['T'], c['n_a'], c['act_a'], c['n_hidden'])
    if c['n_hidden']:
        s += '%s-f%s' % (c['act_h'], c['act_f'])
    return s + '-' + c['act'] + ('' if c['res'] else '-nores') + ('' if c['bias'] else '-nobias') + ''.join('-no_' + n for n in c['no_bias'])


def heads_inputs(c):
    """fp64 inputs of one case, every value exactly representable in fp32 (the GPU sees the same numbers): x, res uniform in
    +-0.5 (res differs between batch elements), Glorot kernels, every bias non-zero, uniform in +-0.1 and different per layer.
    Keys: x, W, b, res, A, a_bias, hidden [(H_i, hb_i)], Fk, f_bias; None where the case has no such tensor."""
    g = torch.Generator().manual_seed(1000 + HEADS_CASES.index(c))
    r32 = lambda t: t.float().double()
    uni = lambda lim, *shape: r32((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * lim)
    B, R, T = c['B'], c['R'], c['T']
    bias = lambda name, n: None if name in c['no_bias'] else uni(0.1, n)
    p = {'x': uni(0.5, B, T, R, 64), 'res': uni(0.5, B, 1, R, 64) if c['res'] else None,
         'W': r32(glorot(g, (64, 64), torch.float64)), 'b': uni(0.1, 64) if c['bias'] else None,
         'A': r32(glorot(g, (64, c['n_a']), torch.float64)), 'a_bias': bias('a', c['n_a']), 'hidden': [], 'Fk': None, 'f_bias': None}
    for i in range(c['n_hidden']):
        p['hidden'].append((r32(glorot(g, (64 if i == 0 else 32, 32), torch.float64)), bias('h%d' % i, 32)))
    if c['n_hidden']:
        p['Fk'], p['f_bias'] = r32(glorot(g, (32, 1), torch.float64)), bias('f', 1)
    return p


def heads_ref(c, p):
    from oracle.tail_ref import dense_cumsum_heads_ref
    return dense_cumsum_heads_ref(p['x'], p['W'], p['b'], p['res'], c['act'], p['A'], p['a_bias'], c['act_a'], p['hidden'], c['act_h'] or 'linear',
                                  p['Fk'], p['f_bias'], c['act_f'] or 'linear')


# Measured on an MI355X over HEADS_CASES (UDS_TOL_REPORT=1): the largest max|out - ref| / max(1, max|ref|) is 1.70e-5 (1.86e-5
# absolute), reached at T = 1 by a chain of linear layers -- no trend in T or in the number of chained split-bf16
# layers (2 to 8), so one constant: 4.7 x the observed maximum, inside the project's 3-6 x convention.
HEADS_TOL = 8e-5


def heads_tol(c):
    """Tolerance of a heads case for close() (relative to max(1, max|ref|)); the header of tests/test_gpu_tail_entries.py lists
    the measurements it is set from."""
    return HEADS_TOL


# ---------------------------------------------------------------------------------------------------------------
# guarded device memory (tests/test_gpu_tail_entries.py, tests/test_gpu_sparse_widths.py): plain allocations, nothing here
# is meant to fault
# ---------------------------------------------------------------------------------------------------------------
SENTINEL = 0x4B5A5A5A      # int32 bits of the guard floats (1.43e7 as a float: nothing a kernel here computes)
PAD = 1024                 # guard floats on each side of a view (a multiple of 4: the view stays 16-byte aligned)


class Guarded:
    """A contiguous fp32 view of `shape` in the middle of a sentinel-filled allocation."""

    def __init__(self, shape, dev, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.view = self.buf[PAD:PAD + self.n].view(shape)
        if init is not None:
            self.view.copy_(init)

    def check(self, what):
        bits = self.buf.view(torch.int32)
        assert bool((bits[:PAD] == SENTINEL).all()), '%s: written before its first element' % what
        assert bool((bits[PAD + self.n:] == SENTINEL).all()), '%s: written past its last element' % what
        assert bool(torch.isfinite(self.view).all()), '%s: non-finite output (an input was read outside its tensor?)' % what


def nan_in(t, dev):
    """`t` as a contiguous fp32 device view inside a NaN-filled allocation (None stays None)."""
    if t is None:
        return None
    buf = torch.full((t.numel() + 2 * PAD,), float('nan'), dtype=torch.float32, device=dev)
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---------------------------------------------------------------------------------------------------------------
# the degree ladder: patterns and operands shared by tests/test_sparse_ref_math.py (CPU: the cases are what they claim to
# be and the references carry signal) and tests/test_gpu_sparse_widths.py (GPU parity at every lane-group shape)
# ---------------------------------------------------------------------------------------------------------------
LADDER_DEGREES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)      # G - 1, G, G + 1, 2 G, 2 G + 1 for G = 2, 4, 8, 16
HUB_DEGREE = 49                                                        # more than three chunks of 16
LADDER_NO_DIAG = 40                                                    # the row without its diagonal
SPARSE_WIDTHS = [4, 8, 12, 16, 32, 64, 96, 128, 256]


def sparse_lanes(d):
    """(G, NC) of kernels_sparse.hpp's group_shape for a row of d floats, (0, 1) for the widths that walk."""
    return {2: (2, 1), 4: (4, 1), 8: (8, 1), 16: (16, 1), 32: (16, 2)}.get(d // 4, (0, 1))


def ladder(n, seed=0):
    """Square directed pattern of n >= 67 nodes, columns ascending, every row but one holding its diagonal:
      row r = 1 .. 14       LADDER_DEGREES[r - 1] entries (its diagonal plus random columns)
      row n - 1             the hub row: HUB_DEGREE = 49 entries; no other row holds column n - 1 (its targets do not point back)
      column c = 15 .. 28   LADDER_DEGREES[c - 15] entries (its diagonal plus random rows): the ladder of the transposed pattern
      column 0              the hub column: rows 30 .. 65 all point at node 0 (37 entries or more)
      row LADDER_NO_DIAG    lacks its diagonal (it keeps (40, 0) and whatever the ladder columns drew)
      every other row       its diagonal plus what the ladder columns and the hub column put there.
    Ladder rows and the hub row draw their columns outside 15 .. 28 and n - 1, ladder columns draw their rows outside 1 .. 14 and
    n - 1, so both ladders hold exactly."""
    assert n >= 67
    rng = np.random.default_rng(100 * seed + n)
    hub, lrows, lcols = n - 1, range(1, 15), range(15, 29)
    free_cols = [c for c in range(n) if c not in lcols and c != hub]
    free_rows = [r for r in range(n) if r not in lrows and r != hub]
    pairs = {(r, r) for r in range(n)}
    for r, deg in zip(lrows, LADDER_DEGREES):
        pairs |= {(r, int(c)) for c in rng.choice([c for c in free_cols if c != r], deg - 1, replace=False)}
    pairs |= {(hub, int(c)) for c in rng.choice(free_cols, HUB_DEGREE - 1, replace=False)}
    for c, deg in zip(lcols, LADDER_DEGREES):
        pairs |= {(int(r), c) for r in rng.choice([r for r in free_rows if r != c], deg - 1, replace=False)}
    pairs |= {(r, 0) for r in range(30, 66)}
    pairs.discard((LADDER_NO_DIAG, LADDER_NO_DIAG))
    return _pairs_csr(pairs, n, n)


def thick(n=67):
    """Square directed pattern whose every row is multi-chunk at every G: row i holds columns i, i + 1, .. (mod n), 33 + i % 17 of
    them.  The degree-sorted schedule runs by DESCENDING degree, so the row that comes last in order[] -- the one surplus groups
    of the ordered kernels shadow -- is the lowest-degree row; here that is row 51 with 33 entries (three chunks of 16)."""
    pairs = {(i, (i + k) % n) for i in range(n) for k in range(33 + i % 17)}
    return _pairs_csr(pairs, n, n)


def ladder_rect(seed=0):
    """67 x 41 pattern with values (SpMM / SDDMM): rows 0, 33 and 66 are empty -- 66 comes last in order[] --, row r = 1 .. 14 holds
    LADDER_DEGREES[r - 1] entries, row 65 all 41 columns (chunks of 16, 16, 9), the others 1 .. 6; values uniform in +-0.5."""
    rng = np.random.default_rng(7 + seed)
    n_rows, n_cols = 67, 41
    pairs = set()
    for r in range(n_rows):
        if r in (0, 33, 66):
            continue
        deg = LADDER_DEGREES[r - 1] if 1 <= r <= 14 else n_cols if r == 65 else int(rng.integers(1, 7))
        pairs |= {(r, int(c)) for c in rng.choice(n_cols, deg, replace=False)}
    csr = _pairs_csr(pairs, n_rows, n_cols)
    csr.val = f32_exact(rng.uniform(-0.5, 0.5, csr.nnz))
    return csr


def _pairs_csr(pairs, n_rows, n_cols):
    from gnn_uds_amd.graph import CSR
    rc = np.array(sorted(pairs), dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rc[:, 0], minlength=n_rows))])
    return CSR(rowptr.astype(np.int32), rc[:, 1].astype(np.int32), n_rows, n_cols)


def f32_exact(a):
    """fp64 array whose every value is an fp32 number: the device sees the same values."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def ladder_scores(csr, seed=0):
    """(s_self, s_nbr), each (3, n) fp64 of fp32 values.  Snapshots 0 and 1: s_nbr uniform in +-2 and s_self of a multi-entry row
    placed so that -s_self lies strictly between the smallest and the largest s_nbr of the row: both leaky slopes occur in it.
    Snapshot 2, the overflow snapshot: multiples of 0.25 in [-48, 48] (fp32 forms s_self + s_nbr exactly) with the last row's
    largest logit set to 48 + 44 = 92: exp(92) is not an fp32 number, only the row-maximum shift keeps expf finite."""
    rng = np.random.default_rng(1000 + seed + csr.n_rows)
    n, rp, col = csr.n_rows, csr.rowptr, csr.col
    ss, sn = np.empty((3, n)), np.empty((3, n))
    for s in range(2):
        sn[s] = f32_exact(rng.uniform(-2.0, 2.0, n))
        for i in range(n):
            v = sn[s, col[rp[i]:rp[i + 1]]]
            ss[s, i] = f32_exact(-(v.min() + rng.uniform(0.25, 0.75) * (v.max() - v.min())) if len(v) > 1 else rng.uniform(-2.0, 2.0))
    ss[2], sn[2] = rng.integers(-192, 193, n) * 0.25, rng.integers(-192, 193, n) * 0.25
    ss[2, n - 1], sn[2, col[rp[n - 1] + 5]] = 48.0, 44.0
    return ss, sn


def ladder_mask(csr, seed=0):
    """(3, nnz) 0/1 fp64: every entry -- the diagonal ones too, the kernels must keep those -- is off with probability 1/3; in
    snapshot 0 the last row (the 49-entry hub of a ladder), row 11 (17 entries there) and every row without a diagonal lose all
    their off-diagonal entries; in snapshot 1 the last row has its odd entries off and its even entries on, so every chunk of two
    or more entries is partly masked at every G."""
    rng = np.random.default_rng(2000 + seed + csr.n_rows)
    rows, col, rp, n = csr.rows(), csr.col.astype(np.int64), csr.rowptr, csr.n_rows
    mask = (rng.random((3, csr.nnz)) > 1.0 / 3.0).astype(np.float64)
    no_diag = [i for i in range(n) if i not in col[rp[i]:rp[i + 1]]]
    for r in [n - 1, 11] + no_diag:
        mask[0, (rows == r) & (col != r)] = 0.0
    k = np.arange(rp[n - 1], rp[n])
    mask[1, k] = ((k - rp[n - 1]) % 2 == 0).astype(np.float64)
    return mask


def ladder_coef(nnz, seed=11):
    """(3, nnz) fp64 attention-dropout multiplier, 0 or 2: the CPU restatement of _lib.dropout(ones, 0.5, seed, 0)."""
    from oracle.dropout_ref import dropout
    return dropout(np.ones((3, nnz)), 0.5, seed, 0)


def ladder_operands(n, d, seed=0):
    """hx, grad (3, n, d) and bias, a_self, a_nbr (d,): uniform in +-0.5, fp64 arrays of fp32 values."""
    rng = np.random.default_rng(3000 + seed + 1000 * n + d)
    u = lambda *shape: f32_exact(rng.uniform(-0.5, 0.5, shape))
    return dict(hx=u(3, n, d), grad=u(3, n, d), bias=u(d), a_self=u(d), a_nbr=u(d))


def gat_ref(csr, ss, sn, mask, coef, op):
    """fp64 reference of one (pattern, width, mask, coef) case from oracle.gat_csr_ref: pre (the aggregation before bias and
    activation), d_hx, ds_self, ds_nbr (the reverse mode of `pre` for the upstream gradient op['grad']).  mask / coef None = ones."""
    from oracle.gat_csr_ref import masked_backward, masked_forward
    rp, col = csr.rowptr.astype(np.int64), csr.col.astype(np.int64)
    ones = np.ones((ss.shape[0], csr.nnz))
    mk, cf = ones if mask is None else mask, ones if coef is None else coef
    pre, alpha = masked_forward(rp, col, mk, cf, op['hx'], ss, sn, np.zeros(op['hx'].shape[-1]), 'linear')
    d_hx, ds_self, ds_nbr, _ = masked_backward(rp, col, mk, cf, op['hx'], ss, sn, op['a_self'], op['a_nbr'], alpha, pre, op['grad'], 'linear')
    return dict(pre=pre, alpha=alpha, d_hx=d_hx, ds_self=ds_self, ds_nbr=ds_nbr)
