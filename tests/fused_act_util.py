"""Parameters, rows, per-epilogue fp64 references and planted mistakes shared by tests/test_fused_act_math.py (CPU: the inputs
reach every region of every activation and a wrong epilogue shows) and tests/test_gpu_fused_acts.py (GPU parity of the fused
spatial kernels, the C entry and the unfused chain at every activation).

A fused spatial kernel applies the layer activation in two epilogues per side: the secondary Dense (x_e = act(e W + b),
e_x = act(x W + b)) and the GAT output (act(acc * inv + bias)).  relu is compiled in; every other activation runs a separate
instantiation of every kernel (ACT = -1) that decides at run time.  With the parameters of tests/fused_chunk_util.py the Dense
pre-activations lie within +-1.71 and the GAT pre-activations within +-0.39: hard_sigmoid never clamps, and tanh and sigmoid stay
in their nearly linear part.  act_params replaces the four biases by values spread over +-LIM, so the pre-activations of both
epilogues cover +-4.6.  The bias is added in fp32 in both epilogues, so the split-bf16 error of the products stays what the
rows of tests/test_gpu_fused_chunks.py measured."""
import functools

import torch

from oracle import sparse_csr as OS
from oracle import spektral_dense as OD
from tests import fused_chunk_util as FC

ACTS = ('relu', 'linear', 'tanh', 'sigmoid', 'hard_sigmoid')      # relu: the control, the compiled-in instantiation on the new inputs
LIM = 4.0                                                         # the biases span [-LIM, LIM]
CLAMP = 2.5                                                       # hard_sigmoid is 0 below -CLAMP and 1 above CLAMP
BIASES = ('xe_b', 'ex_b', 'gx_b', 'ge_b')
# bias i is permuted with seed BIAS_SEED + i.  The smallest move of a planted mistake (leaky relu in the Dense epilogue, a link
# output) is 40-62 x the GPU bound over the seeds 0..39, depending on which GAT columns the most negative Dense biases meet;
# 18 is the seed with the largest smallest move, 62 x
BIAS_SEED = 18
# FC.params draws dense NodeEdge weights as 0.05 N(0, 1) but support-only values as 0.3 + 0.05 N(0, 1).  With the former the
# aggregate of the Dense outputs has a random sign per entry and a sixth of the size, and leaky relu in the Dense epilogue of a
# trained row moves an output by 23-55 x the GPU bound: over 400 bias seeds the smallest move of rows a-h was 44 x at best, never
# the 50 x that tests/test_fused_act_math.py asks of every row.  So the dense weights get the mean of the support-only values:
# every row then aggregates alike, with the product sizes rows a-c of tests/test_gpu_fused_chunks.py measured.
NE_MEAN = 0.3
NET = '600/720'                                                   # rows a-h and n
S_ROW = 3                                                         # snapshots of a GPU case on NET: chunk 1 for every launch there

WS = ('k_fused_ws', 64, 64, 3)
TILE96 = ('k_fused_tile', 96, 96, 3)
CS128 = ('k_fused_cs', 128, 128, 3)


def _row(fx, fe, d, route, expect, trained=False, ws_rem_ok=None, query=None):
    return dict(fx=fx, fe=fe, d=d, route=route, expect=expect, trained=trained, ws_rem_ok=ws_rem_ok, query=query or (fx, fe, d))


# rows a-h: the letters, constructor arguments and expected (kernel, fp, fs, side_mask) keys of tests/test_gpu_fused_chunks.py
ROWS = {
    'a': _row(64, 64, 64, 'fused', [WS]),
    'b': _row(96, 96, 64, 'fused', [TILE96]),
    'c': _row(96, 64, 64, 'fused', [('k_fused_tile', 96, 64, 1), ('k_fused_tile', 64, 96, 2)]),
    'd': _row(64, 64, 64, 'rem-ws', [WS], trained=True),
    'e': _row(64, 64, 64, 'rem-split96', [TILE96], trained=True, ws_rem_ok=False, query=(96, 96, 64)),
    'f': _row(128, 128, 128, 'fused', [CS128]),
    'g': _row(128, 64, 128, 'fused', [('k_fused_cs', 128, 64, 1), ('k_fused_cs', 64, 128, 2)]),
    'h': _row(128, 128, 128, 'rem-d128', [CS128], trained=True),
}
# j: astlingen 64 / 64 / 64, dense untrained NodeEdge parameters, pack_factor() == 4 and S = 4 * 16 + 3 -> 'fused-tiled'
# s: astlingen d = 64 and 128, trained, snapshot_remainder = True -> last_remainder == ('snapshot', 'snapshot')
# n: NET, 64 / 64 / 64 and 8 / 8 / 8, precision = 'fp32' -> 'entry', no fused launch
S_PACKED = 4 * 16 + 3
SHAPES = sorted({(r['fx'], r['fe'], r['d'], r['trained']) for r in ROWS.values()})      # the distinct layers of rows a-h


def act_params(g, fx, fe, d, trained=False, dense=False, seed=BIAS_SEED):
    """FC.params with the four biases replaced: each a seeded permutation of linspace(-LIM, LIM, n), rounded to fp32.  The Dense and
    GAT kernels and the inputs stay as they are.  dense: (N, E) NodeEdge matrices without a trained bias (row j); trained implies
    dense.  Dense NodeEdge weights are raised by NE_MEAN, see there."""
    p = FC.params(g, fx, fe, d, dense=dense or trained, trained=trained)
    for i, key in enumerate(BIASES):
        n = p[key].numel()
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + i))
        p[key] = torch.linspace(-LIM, LIM, n, dtype=torch.float64)[perm].float().double()
    for key in ('ne_n_w', 'ne_e_w'):
        if key in p:
            p[key] = (p[key] + NE_MEAN).float().double()
    return p


def _fn(act):
    return OD.activation(act) if act is None or isinstance(act, str) else act


def _sides(g, x, e):
    return (('node', x, e, 'xe', 'gx', 'ne_n', g.adj, g.inc_n, g.n_node), ('link', e, x, 'ex', 'ge', 'ne_e', g.edge_adj, g.inc_e, g.n_edge))


def pre_activations(g, p, x, e, act_dense):
    """What the two epilogues of each side see -> [(Dense pre-activation, GAT pre-activation)] for nodes, links.  From the pieces
    FC.layer_ref is built from; the GAT pre-activation is what gat_conv_csr returns with act 'linear'.  act_dense (a name or a
    function) is applied to the Dense pre-activation on the way to the GAT."""
    out = []
    for side, prim, sec, dn, gat, ne, adj, inc, rows in _sides(g, x, e):
        pre_d = OD.dense(sec, p[dn + '_k'], p[dn + '_b'], 'linear')
        sec_out = _fn(act_dense)(pre_d)
        if ne + '_v' in p:
            agg = OS.incidence_aggregate_csr(sec_out, inc.rowptr, inc.col, p[ne + '_v'], rows)
        else:
            inci = torch.from_numpy(g.inc_n.to_dense()).abs()
            rowptr, col, val, rest = OS.node_edge_support(inci if side == 'node' else inci.T, p[ne + '_w'], p[ne + '_b'])
            agg = OS.incidence_aggregate_csr(sec_out, rowptr, col, val, rows)
            if rest is not None:
                agg = agg + rest @ sec_out
        cat = torch.cat([prim, agg], dim=-1)
        out.append((pre_d, OS.gat_conv_csr(cat, adj.rowptr, adj.col, p[gat + '_k'], p[gat + '_as'], p[gat + '_an'], p[gat + '_b'], 'linear')))
    return out


def epilogue_ref(g, p, x, e, act_dense, act_gat):
    """The layer with one activation in the Dense epilogue and another in the GAT epilogue (names or functions) -> fp64 (nodes,
    links).  With both equal to one name it is FC.reference, bit for bit."""
    return tuple(_fn(act_gat)(pre_g) for _, pre_g in pre_activations(g, p, x, e, act_dense))


@functools.lru_cache(maxsize=None)
def case(name, fx, fe, d, trained, dense, act, S):
    """(graph, parameters, x, e, fp64 reference) of one GPU case, computed once and shared: treat as read-only."""
    g = FC.graph(name)
    p = act_params(g, fx, fe, d, trained=trained, dense=dense)
    x, e = FC.inputs(g, fx, fe, S)
    with torch.no_grad():
        ref = epilogue_ref(g, p, x, e, act, act)
    return g, p, x, e, ref


# what a wrong epilogue would compute, per activation
_clip = torch.clamp
MUTANTS = {
    'hard_sigmoid': (('no upper clamp', lambda t: _clip(0.2 * t + 0.5, min=0.0)), ('no lower clamp', lambda t: _clip(0.2 * t + 0.5, max=1.0)),
                     ('sigmoid', torch.sigmoid), ('slope 1/6', lambda t: _clip(t / 6.0 + 0.5, 0.0, 1.0))),
    'sigmoid': (('hard_sigmoid', OD.activation('hard_sigmoid')),),
    'tanh': (('clamp to [-1, 1]', lambda t: _clip(t, -1.0, 1.0)), ('linear', lambda t: t), ('sigmoid', torch.sigmoid)),
    'linear': (('relu', torch.relu), ('tanh', torch.tanh)),
    'relu': (('linear', lambda t: t), ('leaky 0.01', lambda t: torch.nn.functional.leaky_relu(t, 0.01))),
}
