"""Cases, seeded signed inputs and fp64 references shared by tests/test_fused_chunk_math.py (CPU: the chunk arithmetic and the
signal the references carry) and tests/test_gpu_fused_chunks.py (GPU parity of the fused spatial kernels at every snapshot-chunk
length).

A fused launch cuts its S snapshots into chunks and one workgroup handles one (tile, chunk) pair; the kernels pipeline over the
snapshots of a chunk, so a chunk of 1, 2, 3 and 4 or more snapshots runs different code, and a ragged last chunk adds a
shorter one to the same launch.  A case is a (chunk, tail) pair; the S that gives it is derived from the tile count of the
launch (find_S / find_long ask the library's own chunk function), never written down."""
import functools
import json
import os

import numpy as np
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from oracle import sparse_csr as OS
from oracle import spektral_dense as OD
from tests.util import spatial_params

TOL_BF16X3 = 1e-5                                   # the project's bound for the fused split-bf16 kernels, relative to max(1, max|ref|)
SHAPES = ((2, 0), (2, 1), (3, 1), (3, 2))           # (chunk, tail) of rows a-h; plus one chunk >= LONG_CHUNK with a non-zero tail
LONG_CHUNK = 4
S_CAP = 64                                          # rows a-h: a network whose plan needs more snapshots than this is too small
SIZES = ((600, 720), (1200, 1500), (2400, 3000))    # synthetic networks, smallest first


def find_S(tiles, chunk, tail, cap=S_CAP):
    """The smallest S <= cap whose launch over `tiles` tiles runs chunks of `chunk` snapshots with S % chunk == tail; None if none."""
    for S in range(1, cap + 1):
        if _lib.fused_chunk(S, tiles) == chunk and S % chunk == tail:
            return S
    return None


def find_long(tiles, min_chunk, cap=S_CAP):
    """The smallest S <= cap with a chunk of at least min_chunk snapshots and a non-zero tail -> (S, chunk, tail) or None."""
    for S in range(1, cap + 1):
        c = _lib.fused_chunk(S, tiles)
        if c >= min_chunk and S % c:
            return S, c, S % c
    return None


def cases_for(tiles, cap=S_CAP):
    """[(S, chunk, tail)] of SHAPES and the long chunk for a launch over `tiles` tiles; None in place of a case that needs S > cap."""
    out = []
    for chunk, tail in SHAPES:
        S = find_S(tiles, chunk, tail, cap)
        out.append(None if S is None else (S, chunk, tail))
    return out + [find_long(tiles, LONG_CHUNK, cap)]


@functools.lru_cache(maxsize=None)
def graph(name):
    """'astlingen' (tests/golden/networks.json) or a synthetic 'N/E'."""
    if name == 'astlingen':
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'networks.json')) as fh:
            net = json.load(fh)['astlingen']
        return U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    n, e = (int(v) for v in name.split('/'))
    return U.DrainageGraph.from_edges(U.synthetic_drainage_network(n, e, 0))


def signed(seed, *shape):
    """Uniform in [-0.5, 0.5), fp64 tensor of fp32 values (the device sees the same numbers); every snapshot differs."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float32) - 0.5).double()


def inputs(g, fx, fe, S, seed=31):
    """x (S, N, fx), e (S, E, fe): the extra 32 columns of a 96-wide side are its last 32."""
    return signed(seed, S, g.n_node, fx), signed(seed + 1, S, g.n_edge, fe)


def params(g, fx, fe, d, seed=33, dense=False, trained=False):
    """tests.util.spatial_params rounded to fp32 values; dense: (N, E) NodeEdge matrices, else values on the support; trained: a
    dense NodeEdge bias on both sides, non-zero off the support (as test_spatial_layer_vs_dense_masked_oracle)."""
    assert dense or not trained
    p = spatial_params(g.n_node, g.n_edge, fx, fe, d, seed=seed, dense_ne=dense, nnz_n=g.inc_n.nnz, nnz_e=g.inc_e.nnz)
    if trained:
        gen = torch.Generator().manual_seed(seed + 1)
        p['ne_n_b'] = torch.randn(p['ne_n_b'].shape, generator=gen, dtype=torch.float64) * 0.01
        p['ne_e_b'] = torch.randn(p['ne_e_b'].shape, generator=gen, dtype=torch.float64) * 0.01
    return {k: v.float().double() for k, v in p.items()}


def _csr(c):
    return c.rowptr, c.col


def reference(g, p, x, e, act='relu', dense_oracle=False):
    """fp64 outputs (S, N, d), (S, E, d): oracle.spektral_dense.spatial_layer_dense (small networks, dense NodeEdge parameters) or
    oracle.sparse_csr.spatial_layer_csr."""
    ne = torch.from_numpy(g.inc_n.to_dense()) if 'ne_n_w' in p else None
    if dense_oracle:
        return OD.spatial_layer_dense(x, e, p, torch.from_numpy(g.adj.to_dense()), torch.from_numpy(g.edge_adj.to_dense()), ne, act=act)
    return OS.spatial_layer_csr(x, e, p, _csr(g.adj), _csr(g.edge_adj), _csr(g.inc_n), _csr(g.inc_e), node_edge=ne, act=act)


# ---------------------------------------------------------------------------------------------------------------
# the reference with one operand of one side taken from the wrong snapshot: what a broken pipeline would compute
# ---------------------------------------------------------------------------------------------------------------
# (part, snapshot offset): secondary rows from s - 1 and from s - 2 (the wrong half of a `k & 1` buffer), primary rows from
# s - 1 and from s + 1 (a prefetch consumed early), the remainder from s - 1
MISTAKES = (('secondary', -1), ('secondary', -2), ('primary', -1), ('primary', 1), ('remainder', -1))


def affected(S, offset):
    """The snapshots whose operand exists at s + offset (the others keep their own: nothing stale to read)."""
    return [s for s in range(S) if 0 <= s + offset < S]


def layer_ref(g, p, x, e, act='relu', wrong=None):
    """The layer from the oracles' pieces, per side: primary rows (own and neighbouring rows of the side's GAT), secondary rows (the
    other side's rows under the Dense and the NodeEdge support) and the remainder (the NodeEdge bias off the support times the same
    Dense) as separate operands.  wrong = (side, part, offset): snapshot s of side 'node' / 'link' reads that part from snapshot
    s + offset (its own where that does not exist).  wrong = None is spatial_layer_csr / spatial_layer_dense."""
    S = x.shape[0]

    def take(t, side, part):
        if wrong is None or wrong[:2] != (side, part):
            return t
        idx = torch.arange(S)
        src = idx + wrong[2]
        return t[torch.where((src >= 0) & (src < S), src, idx)]

    out = []
    sides = (('node', x, e, 'xe', 'gx', 'ne_n', g.adj, g.inc_n, g.n_node), ('link', e, x, 'ex', 'ge', 'ne_e', g.edge_adj, g.inc_e, g.n_edge))
    for side, prim, sec, dn, gat, ne, adj, inc, rows in sides:
        if ne + '_v' in p:
            val, rest = p[ne + '_v'], None
        else:
            inci = torch.from_numpy(g.inc_n.to_dense()).abs()
            _, _, val, rest = OS.node_edge_support(inci if side == 'node' else inci.T, p[ne + '_w'], p[ne + '_b'])
        agg = OS.incidence_aggregate_csr(OD.dense(take(sec, side, 'secondary'), p[dn + '_k'], p[dn + '_b'], act), inc.rowptr, inc.col, val, rows)
        if rest is not None:
            agg = agg + rest @ OD.dense(take(sec, side, 'remainder'), p[dn + '_k'], p[dn + '_b'], act)
        cat = torch.cat([take(prim, side, 'primary'), agg], dim=-1)
        out.append(OS.gat_conv_csr(cat, adj.rowptr, adj.col, p[gat + '_k'], p[gat + '_as'], p[gat + '_an'], p[gat + '_b'], act))
    return tuple(out)
