"""Graph-sharded spatial block: node-cut partition of one big drainage network over the GPUs of a node, with the
boundary rows exchanged once per message-passing layer (one process per GPU, `torch.distributed` over RCCL / xGMI).

The reference has nothing like this (whole graph = one dense matrix on one device); it exists for the
200k-node case of BASELINE.json (`configs[3]`).  Snapshots of the headline-size network do NOT use it -- they shard
by snapshot with no collective (bench.py).

Dependency radius of one spatial layer (`emulator.py:225-230`): the outputs of a rank's own nodes / links need
  hx of   A1 = adj-neighbours of own nodes        -> x of A1 and e of L1 = links incident to A1
  he of   B1 = edge_adj-neighbours of own links   -> e of B1 and x of M1 = end nodes of B1
so every rank computes the layer on the sub-network induced by (A1 u M1, L1 u B1): rows it owns come out exact, the
halo rows are recomputed redundantly where needed (halo hx / he) and otherwise ignored; after the layer every rank
sends the exact outputs of the own rows its peers hold as halo.  Near-tree networks cut into P connected parts have
O(P) cut links, so a message is a few dozen rows: latency-bound, hence ONE message per peer per layer (node rows and
link rows packed together), posted as grouped isend/irecv (ncclSend/ncclRecv on RCCL, each peer pair on its own
xGMI link).

All index bookkeeping here is host-side numpy and deterministic: every rank derives the same plan from the same
network, nothing is negotiated at run time.  Tested with world_size-2 gloo processes on CPU (tests/test_dist.py).
"""
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from .emulator import Emulator
from .graph import CSR, DrainageGraph

I32 = np.int32


def _link_matrix(graph):
    """Symmetric 0/1 node x node matrix of the LINKS themselves (not the `order`-hop GAT pattern): what a node cut cuts."""
    import scipy.sparse as sp
    n = graph.n_node
    e = np.asarray(graph.edges, dtype=np.int64)
    e = e[e[:, 0] != e[:, 1]]
    a = sp.coo_matrix((np.ones(2 * len(e), dtype=np.int8), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                      shape=(n, n)).tocsr()
    a.data[:] = 1                                                      # parallel links count once
    return a


def _bfs_level_order(a, graph):
    """Breadth-first order of every connected component, started at its outfall (a node no link leaves; the lowest-numbered
    node where a component has none): a range of it is a band of tree levels, whose boundary is one level wide."""
    from scipy.sparse.csgraph import breadth_first_order, connected_components
    n = a.shape[0]
    _, label = connected_components(a, directed=False)
    has_out = np.zeros(n, dtype=bool)
    has_out[np.asarray(graph.edges, dtype=np.int64)[:, 0]] = True
    first = np.full(label.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, label, np.arange(n))
    sink = np.full(label.max() + 1, n, dtype=np.int64)
    idx = np.nonzero(~has_out)[0]
    np.minimum.at(sink, label[idx], idx)
    roots = np.where(sink < n, sink, first)
    return np.concatenate([breadth_first_order(a, int(r), directed=False, return_predecessors=False) for r in roots])


def _cut_links(graph, part):
    e = np.asarray(graph.edges, dtype=np.int64)
    return int((part[e[:, 0]] != part[e[:, 1]]).sum())


def _refine_boundary(a, part, n_parts, slack, passes=4):
    """Greedy boundary refinement (one Kernighan-Lin style sweep per pass): a boundary node moves to the neighbouring part
    that holds MORE of its links than its own part does, as long as no part leaves [n/P - slack, n/P + slack] nodes.  Nodes are
    visited in ascending id, gains are re-evaluated at visit time: deterministic, every rank derives the same result."""
    indptr, indices = a.indptr, a.indices
    n = a.shape[0]
    size = np.bincount(part, minlength=n_parts).astype(np.int64)
    lo, hi = n // n_parts - slack, -(-n // n_parts) + slack
    for _ in range(passes):
        src = np.repeat(np.arange(n), np.diff(indptr))
        boundary = np.unique(src[part[src] != part[indices]])
        moved = 0
        for v in boundary:
            nb = part[indices[indptr[v]:indptr[v + 1]]]
            own = part[v]
            cnt = np.bincount(nb, minlength=n_parts)
            best = int(np.argmax(cnt))                               # lowest part id among ties
            if best != own and cnt[best] > cnt[own] and size[own] - 1 >= lo and size[best] + 1 <= hi:
                part[v] = best
                size[own] -= 1
                size[best] += 1
                moved += 1
        if not moved:
            break
    return part


def partition_nodes(graph, n_parts, return_info=False):
    """Node -> part (int32), a node cut into `n_parts` parts of n/P nodes (+- 2 %).

    Three candidate orders are cut into equal contiguous ranges -- the node ids as given (SWMM files and the synthetic
    generator number a network roughly upstream -> downstream, so an id range is already a band of the tree), breadth-first
    levels from the outfalls, and reverse Cuthill-McKee -- and the one that cuts the fewest links is kept, then improved by a
    greedy boundary refinement.  (Round 2 used ranges of a DEPTH-first pre-order: on a deep narrow tree such a range cuts
    about one link per level -- 5 382 cut links 8-way on the 200k-node network against 463 for the plain id ranges.)
    All of it is deterministic host-side integer work; every rank derives the same partition from the same network."""
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    n = graph.n_node
    a = _link_matrix(graph)
    ranges = (np.arange(n, dtype=np.int64) * n_parts // n).astype(I32)
    orders = {'id': np.arange(n, dtype=np.int64), 'bfs': _bfs_level_order(a, graph),
              'rcm': np.asarray(reverse_cuthill_mckee(a, symmetric_mode=True), dtype=np.int64)}
    best, info = None, {}
    for name, order in orders.items():
        part = np.empty(n, dtype=I32)
        part[order] = ranges
        info[name] = _cut_links(graph, part)
        if best is None or info[name] < info[best[0]]:
            best = (name, part)
    part = _refine_boundary(a, best[1].copy(), n_parts, slack=max(1, n // n_parts // 50))
    info['refined'] = _cut_links(graph, part)
    info['kept'] = best[0]
    if info['refined'] > info[best[0]]:                              # never worse than the best plain range split
        part, info['refined'] = best[1], info[best[0]]
    return (part, info) if return_info else part


def _rows_union(csr, rows):
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64)
    rp = csr.rowptr.astype(np.int64)
    cnt = rp[rows + 1] - rp[rows]
    idx = np.repeat(rp[rows], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return np.unique(csr.col[idx].astype(np.int64))


def _induced(csr, rows, col_map, n_cols_local):
    """Sub-CSR on `rows` with columns restricted to the local set (col_map: global -> local or -1); also returns the
    global position of every kept entry (to gather per-entry parameters such as the NodeEdge support values)."""
    rp = csr.rowptr.astype(np.int64)
    cnt = rp[rows + 1] - rp[rows]
    pos = np.repeat(rp[rows], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    lcol = col_map[csr.col[pos].astype(np.int64)]
    keep = lcol >= 0
    row_of = np.repeat(np.arange(len(rows)), cnt)[keep]
    lcol, pos = lcol[keep], pos[keep]
    o = np.lexsort((lcol, row_of))
    row_of, lcol, pos = row_of[o], lcol[o], pos[o]
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.add.at(rowptr, row_of + 1, 1)
    val = None if csr.val is None else csr.val[pos]
    return CSR(np.cumsum(rowptr).astype(I32), lcol.astype(I32), len(rows), n_cols_local, val), pos


@dataclass
class LocalProblem:
    """What one rank computes and exchanges.  Local row order: own rows first (ascending id), then halo rows."""
    rank: int
    own_nodes: np.ndarray
    own_links: np.ndarray
    nodes: np.ndarray                 # local node list (global ids)
    links: np.ndarray
    graph: DrainageGraph              # induced sub-network on (nodes, links)
    inc_n_pos: np.ndarray             # global inc_n / inc_e entry of every local entry
    inc_e_pos: np.ndarray
    send_nodes: Dict[int, np.ndarray] = field(default_factory=dict)   # peer -> LOCAL indices of own rows it needs
    send_links: Dict[int, np.ndarray] = field(default_factory=dict)
    recv_nodes: Dict[int, np.ndarray] = field(default_factory=dict)   # peer -> LOCAL indices of halo rows it owns
    recv_links: Dict[int, np.ndarray] = field(default_factory=dict)


def build_partition_plan(graph, n_parts, part=None):
    """Deterministic plan for all ranks: List[LocalProblem]."""
    if part is None:
        part = partition_nodes(graph, n_parts)
    part = np.asarray(part, dtype=np.int64)
    link_part = part[graph.edges[:, 0].astype(np.int64)]            # a link belongs to the part of its from-node
    probs: List[LocalProblem] = []
    for r in range(n_parts):
        own_n = np.nonzero(part == r)[0]
        own_e = np.nonzero(link_part == r)[0]
        a1 = _rows_union(graph.adj, own_n)
        l1 = _rows_union(graph.inc_n, a1)
        b1 = _rows_union(graph.edge_adj, own_e)
        m1 = _rows_union(graph.inc_e, b1)
        nodes = np.concatenate([own_n, np.setdiff1d(np.union1d(a1, m1), own_n)])
        links = np.concatenate([own_e, np.setdiff1d(np.union1d(l1, b1), own_e)])
        nmap = np.full(graph.n_node, -1, dtype=np.int64)
        nmap[nodes] = np.arange(len(nodes))
        lmap = np.full(graph.n_edge, -1, dtype=np.int64)
        lmap[links] = np.arange(len(links))
        adj, _ = _induced(graph.adj, nodes, nmap, len(nodes))
        eadj, _ = _induced(graph.edge_adj, links, lmap, len(links))
        inc_n, pos_n = _induced(graph.inc_n, nodes, lmap, len(links))
        inc_e, pos_e = _induced(graph.inc_e, links, nmap, len(nodes))
        edges = np.stack([nmap[graph.edges[links, 0].astype(np.int64)], nmap[graph.edges[links, 1].astype(np.int64)]], axis=1)
        sub = DrainageGraph(len(nodes), len(links), edges.astype(I32), adj, eadj, inc_n, inc_e, dict(part=r, n_parts=n_parts))
        probs.append(LocalProblem(r, own_n, own_e, nodes, links, sub, pos_n, pos_e))
    for p in probs:                                                   # who needs what from whom
        halo_n, halo_e = p.nodes[len(p.own_nodes):], p.links[len(p.own_links):]
        for q in range(n_parts):
            if q == p.rank:
                continue
            hn = np.nonzero(part[halo_n] == q)[0]
            he = np.nonzero(link_part[halo_e] == q)[0]
            if len(hn) == 0 and len(he) == 0:
                continue
            p.recv_nodes[q] = (len(p.own_nodes) + hn).astype(np.int64)
            p.recv_links[q] = (len(p.own_links) + he).astype(np.int64)
            peer = probs[q]
            p_n = np.searchsorted(peer.own_nodes, halo_n[hn])        # own rows are sorted and come first locally
            p_e = np.searchsorted(peer.own_links, halo_e[he])
            peer.send_nodes[p.rank] = p_n.astype(np.int64)
            peer.send_links[p.rank] = p_e.astype(np.int64)
    return probs


class HaloExchange:
    """One message per peer: [node rows | link rows] of width F, posted as grouped isend / irecv."""

    def __init__(self, prob, device, group=None):
        self.prob, self.group = prob, group
        t = lambda a: torch.as_tensor(a, dtype=torch.int64, device=device)
        self.peers = sorted(set(prob.send_nodes) | set(prob.recv_nodes))
        self.send_n = {q: t(prob.send_nodes.get(q, np.zeros(0, np.int64))) for q in self.peers}
        self.send_e = {q: t(prob.send_links.get(q, np.zeros(0, np.int64))) for q in self.peers}
        self.recv_n = {q: t(prob.recv_nodes.get(q, np.zeros(0, np.int64))) for q in self.peers}
        self.recv_e = {q: t(prob.recv_links.get(q, np.zeros(0, np.int64))) for q in self.peers}
        # on the GPU a message is packed / unpacked by ONE launch (uds_halo_pack / uds_halo_unpack) with int32 row lists
        self.on_gpu = torch.device(device).type == 'cuda'
        if self.on_gpu:
            i32 = lambda d: {q: v.to(torch.int32) for q, v in d.items()}
            self._i32 = (i32(self.send_n), i32(self.send_e), i32(self.recv_n), i32(self.recv_e))

    def bytes_per_layer(self, S, F):
        return sum((len(self.send_n[q]) + len(self.send_e[q])) * S * F * 4 for q in self.peers)

    def __call__(self, x, e):
        """x (S, n_local_nodes, F), e (S, n_local_links, F): overwrite the halo rows with the owners' exact rows.  Everything
        is enqueued on the CURRENT stream (RCCL: the send / receive kernels are ordered after the stream's earlier work and
        `wait()` blocks the stream, not the host), so a caller that runs this under a side stream overlaps it with compute."""
        if not self.peers:
            return x, e
        ops, recvs, keep = [], [], []
        for q in self.peers:
            nn_, ne_ = len(self.recv_n[q]), len(self.recv_e[q])
            if nn_ + ne_:
                buf = torch.empty((x.shape[0], nn_ + ne_, x.shape[-1]), device=x.device, dtype=x.dtype)
                recvs.append((q, buf, nn_))
                ops.append(dist.P2POp(dist.irecv, buf, q, self.group))
            sn, se = self.send_n[q], self.send_e[q]
            if len(sn) + len(se):
                out = self.pack(x, e, q)
                keep.append(out)
                ops.append(dist.P2POp(dist.isend, out, q, self.group))
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        for q, buf, nn_ in recvs:
            self.unpack(buf, x, e, q)
        return x, e

    def pack(self, x, e, q):
        """The message for peer q: [own node rows it holds as halo | own link rows], (S, n, F)."""
        if self.on_gpu and x.is_cuda and x.shape[-1] % 4 == 0 and x.is_contiguous() and e.is_contiguous():
            from . import _lib
            return _lib.halo_pack(x, e, self._i32[0][q], self._i32[1][q])
        return torch.cat([x.index_select(1, self.send_n[q]), e.index_select(1, self.send_e[q])], dim=1).contiguous()

    def unpack(self, buf, x, e, q):
        """Scatter peer q's message into the halo rows it owns (in place)."""
        if self.on_gpu and x.is_cuda and x.shape[-1] % 4 == 0 and x.is_contiguous() and e.is_contiguous():
            from . import _lib
            _lib.halo_unpack(buf, x, e, self._i32[2][q], self._i32[3][q])
            return
        nn_ = len(self.recv_n[q])
        x.index_copy_(1, self.recv_n[q], buf[:, :nn_])
        e.index_copy_(1, self.recv_e[q], buf[:, nn_:])


class ShardedSpatialBlock:
    """The L-layer spatial block of one rank of a graph-sharded run.

    layer_fn(prob, layer_index, x_local, e_local) -> (x', e') computes one spatial layer on the rank's sub-network
    (exact on own rows).  The product passes HIP `SpatialLayer`s built on `prob.graph` (see `hip_layers`); the CPU
    tests pass the oracle."""

    def __init__(self, prob, n_layers, layer_fn, device, group=None):
        self.prob, self.n_layers, self.layer_fn = prob, n_layers, layer_fn
        self.exchange = HaloExchange(prob, device, group)
        self._side = None                     # side stream of the pipelined exchange, created on first use

    def scatter_inputs(self, x_global, e_global):
        """Local buffers from replicated global inputs (own + halo rows are simply read)."""
        dev = x_global.device
        ni = torch.as_tensor(self.prob.nodes, dtype=torch.int64, device=dev)
        li = torch.as_tensor(self.prob.links, dtype=torch.int64, device=dev)
        return x_global.index_select(1, ni).contiguous(), e_global.index_select(1, li).contiguous()

    def forward(self, x_local, e_local, stages=2):
        """x_local (S, n_local_nodes, F), e_local likewise, halo rows valid.  Returns the own rows of the block output.

        The snapshots are independent, so the exchange is hidden by PIPELINING OVER SNAPSHOT GROUPS: the S snapshots are cut
        into `stages` groups; as soon as a group's layer is computed its boundary rows are packed, sent and the received
        halo rows scattered on a side stream, while the main stream computes the same layer of the next group (and then the
        next layer of the first group, whose halo has arrived by then).  Only a group whose exchange is slower than one
        group-layer of compute leaves the main stream waiting.  The fused kernel is launched per group (it takes any S); no
        kernel needs a boundary / interior split of its tiles.  stages=1 (or one snapshot, or no peers): compute, then
        exchange, in order on one stream."""
        S = x_local.shape[0]
        L, ex = self.n_layers, self.exchange
        G = max(1, min(int(stages), S)) if ex.peers else 1
        if G == 1:
            for i in range(L):
                x_local, e_local = self.layer_fn(self.prob, i, x_local, e_local)
                if i + 1 < L:
                    x_local, e_local = ex(x_local, e_local)
            return x_local[:, :len(self.prob.own_nodes)], e_local[:, :len(self.prob.own_links)]
        cuts = [g * S // G for g in range(G + 1)]
        xs = [x_local[cuts[g]:cuts[g + 1]] for g in range(G)]
        es = [e_local[cuts[g]:cuts[g + 1]] for g in range(G)]
        on_gpu = x_local.is_cuda
        if on_gpu:
            if self._side is None:
                self._side = torch.cuda.Stream(device=x_local.device)
            main, side = torch.cuda.current_stream(x_local.device), self._side
        ready = [None] * G                    # event: the halo rows of group g hold the previous layer's exchanged values
        for i in range(L):
            for g in range(G):
                if ready[g] is not None:
                    main.wait_event(ready[g])
                xs[g], es[g] = self.layer_fn(self.prob, i, xs[g], es[g])
                if i + 1 == L:
                    continue
                if not on_gpu:                # CPU tensors (gloo tests): same order of messages, no streams
                    ex(xs[g], es[g])
                    continue
                computed = torch.cuda.Event()
                computed.record(main)
                with torch.cuda.stream(side):
                    side.wait_event(computed)
                    ex(xs[g], es[g])          # pack, send / receive, scatter: all ordered on the side stream
                    ready[g] = torch.cuda.Event()
                    ready[g].record(side)
                xs[g].record_stream(side)
                es[g].record_stream(side)
        no, lo = len(self.prob.own_nodes), len(self.prob.own_links)
        return torch.cat([t[:, :no] for t in xs], dim=0), torch.cat([t[:, :lo] for t in es], dim=0)


def hip_layers(prob, global_params, embed_size, activation='relu', precision='bf16x3', device='cuda'):
    """HIP `SpatialLayer`s for a rank's sub-network from GLOBAL per-layer parameters (dicts with the keys of
    `SpatialLayer.export_params()` in sparse form: 'ne_n_v' / 'ne_e_v' are indexed by global support entry)."""
    from .layers import SpatialLayer
    layers = []
    for p in global_params:
        if p['gx_k'].dim() == 3 and p['gx_k'].shape[1] != 1:
            raise NotImplementedError('hip_layers: attn_heads=%d -- the sharded layers are single-head' % p['gx_k'].shape[1])
        fx, fe = p['ex_k'].shape[0], p['xe_k'].shape[0]
        ly = SpatialLayer(prob.graph, embed_size, activation, fx=fx, fe=fe, sparse_params=True, precision=precision).to(device)
        f = lambda t: None if t is None else t.to(torch.float32).to(device).contiguous()
        ly.dense_xe.kernel.data, ly.dense_xe.bias.data = f(p['xe_k']), f(p['xe_b'])
        ly.dense_ex.kernel.data, ly.dense_ex.bias.data = f(p['ex_k']), f(p['ex_b'])
        ly.node_edge_n.weight.data = f(p['ne_n_v'][torch.as_tensor(prob.inc_n_pos)])
        ly.node_edge_e.weight.data = f(p['ne_e_v'][torch.as_tensor(prob.inc_e_pos)])
        ly.node_edge_n.bias.data = torch.zeros_like(ly.node_edge_n.weight.data)
        ly.node_edge_e.bias.data = torch.zeros_like(ly.node_edge_e.weight.data)
        for m, k in ((ly.gat_x, 'gx'), (ly.gat_e, 'ge')):
            m.kernel.data, m.bias.data = f(p[k + '_k']), f(p[k + '_b'])
            m.attn_kernel_self.data, m.attn_kernel_neighs.data = f(p[k + '_as']), f(p[k + '_an'])
        layers.append(ly)
    return layers


def all_ranks_finite(value, group=None):
    """True only when `value` (a tensor) is finite on EVERY rank: a MIN all-reduce of the local 0/1 flag, so that all ranks
    take the same branch -- a rank that raised on its own non-finite loss would leave its peers waiting in the gradient
    all-reduce.  The local test alone when torch.distributed is not initialised or the world has one rank."""
    ok = torch.isfinite(value).all()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        flag = ok.to(torch.float32).reshape(1)
        if dist.get_backend(group) == 'gloo':
            flag = flag.cpu()
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        return bool(flag.item() > 0.5)
    return bool(ok)


def allreduce_gradients(params, group=None, bucket_bytes=64 << 20):
    """Data-parallel training (snapshot / scenario sharding adds ONE gradient all-reduce per step): average
    the `.grad` of `params` over the ranks.  Gradients are packed into flat fp32 buckets (one bucket for a whole emulator:
    a few MB) so the ring all-reduce over xGMI runs once on a large message instead of once per tensor; parameters a rank
    did not touch count as zero.  No-op when torch.distributed is not initialised or the world has one rank."""
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    world = dist.get_world_size(group)
    if world == 1:
        return 0
    params = [p for p in params if p.requires_grad]
    n_calls, i = 0, 0
    while i < len(params):
        j, size = i, 0
        while j < len(params) and (j == i or (size + params[j].numel()) * 4 <= bucket_bytes):
            size += params[j].numel()
            j += 1
        flat = torch.zeros(size, dtype=torch.float32, device=params[i].device)
        off = 0
        for p in params[i:j]:
            if p.grad is not None:
                flat[off:off + p.numel()] = p.grad.reshape(-1)
            off += p.numel()
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat /= world
        off = 0
        for p in params[i:j]:
            p.grad = flat[off:off + p.numel()].reshape(p.shape).clone()
            off += p.numel()
        n_calls += 1
        i = j
    return n_calls


# ---------------------------------------------------------------------------------------------------------------------
# The whole Emulator on a graph-sharded network ("whole-forward schedule")
# ---------------------------------------------------------------------------------------------------------------------
def flow_rows(prob):
    """The `rows=` subset of the post-processing's flow exchange: the halo LINKS incident to own nodes (the only flows the
    link -> node balance of an own node reads that the rank does not own), no node rows.  Both ends agree without talking:
    a link belongs to its from-node's part, so the receiver keeps the halo links whose to-node it owns and the sender keeps
    the own links whose to-node the receiver owns -- in the plan's order, which the two lists share."""
    edges = np.asarray(prob.graph.edges, dtype=np.int64)
    n_own = len(prob.own_nodes)
    recv_links = {q: idx[(edges[idx, 1] >= 0) & (edges[idx, 1] < n_own)] for q, idx in prob.recv_links.items()}
    send_links = {}
    for q, idx in prob.send_links.items():
        theirs = prob.recv_nodes.get(q, np.zeros(0, np.int64))
        send_links[q] = idx[np.isin(edges[idx, 1], theirs)]
    return dict(send_links=send_links, recv_links=recv_links)


class HaloExchangeAll:
    """`HaloExchange` with ONE pack launch and ONE unpack launch per exchange, whatever the number of peers
    (uds_halo_pack_all / uds_halo_unpack_all): the per-peer row lists are concatenated (int32, with P + 1 offsets) and all
    messages live in one send buffer and one receive buffer, peer q's message the contiguous (S, nx_q + ne_q, F) block at
    S F (off_x[q] + off_e[q]) -- a plain slice for `batch_isend_irecv`.  Any row width F >= 1.

    rows: a subset of the plan's lists, a dict with any of 'send_nodes', 'send_links', 'recv_nodes', 'recv_links' (peer ->
    LOCAL indices, as in LocalProblem); a list the dict does not name is empty (`flow_rows`).  None: the plan's lists.

    `adjoint` is the transpose of `__call__` (graph-sharded training): the roles of the lists swap, halo rows return their
    gradient to the owner and keep none (uds_halo_pack_clear_all over the receive lists), owners add what comes back
    (uds_halo_accumulate_all over the send lists, in ascending peer order, no atomics).  Both directions post their messages
    through `transport`, the one method an in-process test transport overrides."""

    def __init__(self, prob, device, group=None, rows=None):
        self.prob, self.group = prob, group
        if rows is None:
            rows = dict(send_nodes=prob.send_nodes, send_links=prob.send_links, recv_nodes=prob.recv_nodes, recv_links=prob.recv_links)
        get = lambda key, q: np.asarray(rows.get(key, {}).get(q, np.zeros(0, np.int64)), dtype=np.int64)
        peers = sorted(set(prob.send_nodes) | set(prob.recv_nodes))
        lists = {k: [get(k, q) for q in peers] for k in ('send_nodes', 'send_links', 'recv_nodes', 'recv_links')}
        n_n, n_e = len(prob.nodes), len(prob.links)
        for k, bound in (('send_nodes', len(prob.own_nodes)), ('send_links', len(prob.own_links)), ('recv_nodes', n_n), ('recv_links', n_e)):
            lo = len(prob.own_nodes) if k == 'recv_nodes' else len(prob.own_links) if k == 'recv_links' else 0
            for a in lists[k]:        # the kernels do not check rows on the device: every row is checked here, once
                if len(a) and (a.min() < lo or a.max() >= bound):
                    raise ValueError('HaloExchangeAll: %s rows outside [%d, %d)' % (k, lo, bound))
        keep = [i for i in range(len(peers)) if sum(len(lists[k][i]) for k in lists)]
        self.peers = [peers[i] for i in keep]
        t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=device)
        self.dev = {}
        self.n_send, self.n_recv = {}, {}             # peer -> message rows
        for side in ('send', 'recv'):
            xs = [lists[side + '_nodes'][i] for i in keep]
            es = [lists[side + '_links'][i] for i in keep]
            off_x = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.int64)
            off_e = np.concatenate([[0], np.cumsum([len(a) for a in es])]).astype(np.int64)
            cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
            self.dev[side] = dict(idx_x=t(cat(xs), torch.int64), idx_e=t(cat(es), torch.int64), off_x=off_x, off_e=off_e,
                                  idx_x32=t(cat(xs), torch.int32), idx_e32=t(cat(es), torch.int32),
                                  off_x32=t(off_x, torch.int32), off_e32=t(off_e, torch.int32))
            for k, q in enumerate(self.peers):
                (self.n_send if side == 'send' else self.n_recv)[q] = (int(off_x[k] + off_e[k]), int(off_x[k + 1] + off_e[k + 1]))
        # the adjoint zeroes the received rows after packing them and adds the returned messages into the sent rows: the
        # received rows must be distinct across peers, the sent rows distinct within a peer (checked once, here)
        for k in ('recv_nodes', 'recv_links'):
            allrows = np.concatenate([lists[k][i] for i in keep]) if keep else np.zeros(0, np.int64)
            if len(np.unique(allrows)) != len(allrows):
                raise ValueError('HaloExchangeAll: %s rows repeat across peers' % k)
        for k in ('send_nodes', 'send_links'):
            if any(len(np.unique(lists[k][i])) != len(lists[k][i]) for i in keep):
                raise ValueError('HaloExchangeAll: %s rows repeat within a peer' % k)
        self.dev['acc'] = self._accumulate_plan(t)
        self.adjoint_calls = 0

    def _accumulate_plan(self, t):
        """Targets of the adjoint's accumulation -- the distinct own rows in the send lists, node rows first -- and the CSR of
        the message rows (numbered across peers, as the buffer) that each one adds, in ascending peer order."""
        d = self.dev['send']
        off_x, off_e = d['off_x'], d['off_e']
        P = len(self.peers)
        sx, se = d['idx_x'].cpu().numpy(), d['idx_e'].cpu().numpy()
        peer_x = np.repeat(np.arange(P), np.diff(off_x)).astype(np.int64)
        peer_e = np.repeat(np.arange(P), np.diff(off_e)).astype(np.int64)
        msg_x = np.arange(len(sx), dtype=np.int64) + off_e[peer_x]          # message row of send-list entry k: r_q + j
        msg_e = np.arange(len(se), dtype=np.int64) + off_x[peer_e + 1]
        tgts, ptr, src = [], [0], []
        for rows, msg in ((sx, msg_x), (se, msg_e)):
            o = np.argsort(rows, kind='stable')                              # entries are in peer order: stable keeps it
            tgt, cnt = np.unique(rows[o], return_counts=True)
            tgts.append(tgt)
            ptr.extend((ptr[-1] + np.cumsum(cnt)).tolist())
            src.append(msg[o])
        tgt_x, tgt_e, ptr, src = tgts[0], tgts[1], np.asarray(ptr, np.int64), np.concatenate(src)
        return dict(tgt_x=t(tgt_x, torch.int64), tgt_e=t(tgt_e, torch.int64), ptr=ptr, src=src,
                    tgt_x32=t(tgt_x, torch.int32), tgt_e32=t(tgt_e, torch.int32), ptr32=t(ptr, torch.int32), src32=t(src, torch.int32))

    def rows(self, side):
        """(node rows, link rows) of all messages of `side` ('send' / 'recv'), int64 on the device, peers concatenated."""
        d = self.dev[side]
        return d['idx_x'], d['idx_e']

    def pack(self, x, e):
        """All outgoing messages in one flat buffer (one launch on the GPU)."""
        d = self.dev['send']
        if x.is_cuda:
            from . import _lib
            return _lib.halo_pack_all(x, e, d['idx_x32'], d['idx_e32'], d['off_x32'], d['off_e32'])
        S, F = e.shape[0], e.shape[-1]        # CPU tensors (gloo): the same layout with index ops
        parts = []
        for k in range(len(self.peers)):
            sx = d['idx_x'][int(d['off_x'][k]):int(d['off_x'][k + 1])]
            se = d['idx_e'][int(d['off_e'][k]):int(d['off_e'][k + 1])]
            parts.append(torch.cat([x.index_select(1, sx), e.index_select(1, se)], dim=1).reshape(-1))
        return torch.cat(parts) if parts else e.new_empty(0)

    def unpack(self, buf, x, e):
        """Scatter every received message into the halo rows (in place; one launch on the GPU)."""
        d = self.dev['recv']
        if x.is_cuda:
            from . import _lib
            _lib.halo_unpack_all(buf, x, e, d['idx_x32'], d['idx_e32'], d['off_x32'], d['off_e32'])
            return
        S, F = e.shape[0], e.shape[-1]
        for k in range(len(self.peers)):
            r0, r1 = int(d['off_x'][k] + d['off_e'][k]), int(d['off_x'][k + 1] + d['off_e'][k + 1])
            nx_ = int(d['off_x'][k + 1] - d['off_x'][k])
            msg = buf[S * F * r0:S * F * r1].reshape(S, r1 - r0, F)
            x.index_copy_(1, d['idx_x'][int(d['off_x'][k]):int(d['off_x'][k + 1])], msg[:, :nx_])
            e.index_copy_(1, d['idx_e'][int(d['off_e'][k]):int(d['off_e'][k + 1])], msg[:, nx_:])

    def pack_clear(self, gx, ge):
        """The adjoint's outgoing messages: the RECEIVE lists' rows packed as `unpack` reads them, each row then zeroed (in
        place; one launch on the GPU)."""
        d = self.dev['recv']
        if gx.is_cuda:
            from . import _lib
            return _lib.halo_pack_clear_all(gx, ge, d['idx_x32'], d['idx_e32'], d['off_x32'], d['off_e32'])
        parts = []
        for k in range(len(self.peers)):
            sx = d['idx_x'][int(d['off_x'][k]):int(d['off_x'][k + 1])]
            se = d['idx_e'][int(d['off_e'][k]):int(d['off_e'][k + 1])]
            parts.append(torch.cat([gx.index_select(1, sx), ge.index_select(1, se)], dim=1).reshape(-1))
        gx.index_fill_(1, d['idx_x'], 0)
        ge.index_fill_(1, d['idx_e'], 0)
        return torch.cat(parts) if parts else ge.new_empty(0)

    def accumulate(self, buf, gx, ge):
        """Add every returned message (laid out as the forward SEND buffer) into the sent rows, in place: the current value
        first, then the peers in ascending order (one launch on the GPU, no atomics)."""
        d, a = self.dev['send'], self.dev['acc']
        if gx.is_cuda:
            from . import _lib
            _lib.halo_accumulate_all(buf, gx, ge, d['off_x32'], d['off_e32'], a['tgt_x32'], a['tgt_e32'], a['ptr32'], a['src32'])
            return
        S, F = ge.shape[0], ge.shape[-1]        # CPU tensors (gloo): one index_add_ per peer and kind, each row added once
        for k in range(len(self.peers)):
            r0, r1 = int(d['off_x'][k] + d['off_e'][k]), int(d['off_x'][k + 1] + d['off_e'][k + 1])
            nx_ = int(d['off_x'][k + 1] - d['off_x'][k])
            msg = buf[S * F * r0:S * F * r1].reshape(S, r1 - r0, F)
            gx.index_add_(1, d['idx_x'][int(d['off_x'][k]):int(d['off_x'][k + 1])], msg[:, :nx_])
            ge.index_add_(1, d['idx_e'][int(d['off_e'][k]):int(d['off_e'][k + 1])], msg[:, nx_:])

    def message(self, buf, q, side, S, F):
        """Peer q's slice of a send / receive buffer."""
        r0, r1 = (self.n_send if side == 'send' else self.n_recv)[q]
        return buf[S * F * r0:S * F * r1]

    def transport(self, msgs):
        """Move one exchange's messages: msgs lists (peer, outgoing slice or None, incoming slice or None) in ascending peer
        order; grouped isend / irecv (ncclSend / ncclRecv on RCCL), waited for on the current stream."""
        ops = []
        for q, out, inc in msgs:
            if inc is not None:
                ops.append(dist.P2POp(dist.irecv, inc, q, self.group))
            if out is not None:
                ops.append(dist.P2POp(dist.isend, out, q, self.group))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()

    def __call__(self, x, e):
        """x (S, n_local_nodes, F) or None (a link-only exchange), e (S, n_local_links, F): overwrite the halo rows with the
        owners' exact rows; enqueued on the current stream, as `HaloExchange`."""
        if x is None:
            x = e.new_empty((e.shape[0], 0, e.shape[-1]))
        if not self.peers:
            return x, e
        S, F = e.shape[0], e.shape[-1]
        sbuf = self.pack(x, e)
        n_recv = self.n_recv[self.peers[-1]][1]
        rbuf = torch.empty(S * n_recv * F, device=e.device, dtype=e.dtype)
        some = lambda n, buf, q, side: self.message(buf, q, side, S, F) if n[q][1] > n[q][0] else None
        self.transport([(q, some(self.n_send, sbuf, q, 'send'), some(self.n_recv, rbuf, q, 'recv')) for q in self.peers])
        self.unpack(rbuf, x, e)
        return x, e

    def adjoint(self, gx, ge):
        """The transpose of `__call__`, in place on gradients shaped like its x (or None, link-only) and e: the gradient of
        every halo row the exchange overwrote goes to its owner and is zeroed here; every own row a peer holds as halo adds
        that peer's message.  The message to peer q is this rank's receive block from q; it lands in a buffer laid out as
        the forward send buffer.  Summed over ranks, <E(x), g> = <x, E^T(g)>."""
        if gx is None:
            gx = ge.new_empty((ge.shape[0], 0, ge.shape[-1]))
        self.adjoint_calls += 1
        if not self.peers:
            return gx, ge
        S, F = ge.shape[0], ge.shape[-1]
        sbuf = self.pack_clear(gx, ge)
        n_back = self.n_send[self.peers[-1]][1]
        rbuf = torch.empty(S * n_back * F, device=ge.device, dtype=ge.dtype)
        some = lambda n, buf, q, side: self.message(buf, q, side, S, F) if n[q][1] > n[q][0] else None
        self.transport([(q, some(self.n_recv, sbuf, q, 'recv'), some(self.n_send, rbuf, q, 'send')) for q in self.peers])
        self.accumulate(rbuf, gx, ge)
        return gx, ge


def _refuse_unsharded_configuration(emul):
    """Why `shard_emulator` cannot shard this model, or None."""
    if not emul.conv:
        return NotImplementedError, 'conv=False (the non-graph baseline flattens the whole network into one row per step)'
    if emul.conv_kind != 'GAT':
        return NotImplementedError, 'conv=%s: the sharded forward is built for GAT' % emul.conv_kind
    if emul.graph_base:
        return NotImplementedError, 'graph_base=%r: one graph over nodes and links has no node cut here' % emul.graph_base
    if emul.use_adj:
        return NotImplementedError, 'use_adj: the per-step adjacency of block 2 is not sharded'
    if emul.dropout:
        return NotImplementedError, 'dropout=%r: the sharded forward is inference only' % emul.dropout
    if getattr(emul, 'attn_heads', 1) > 1:
        return NotImplementedError, 'attn_heads=%d: the sharded layers and their halo backward are single-head' % emul.attn_heads
    for bi, block in enumerate((emul.block1, emul.block2)):
        for li, ly in enumerate(block.layers):
            for name in ('node_edge_n', 'node_edge_e'):
                ne = getattr(ly, name)
                if not ne.sparse and ne.support_values()[1] is not None:
                    return ValueError, ('block %d layer %d %s: the NodeEdge bias is non-zero off the incidence support -- every node then '
                                        'depends on every link and no halo of bounded radius exists' % (bi + 1, li, name))
    return None


class _ExchangedBlock(nn.Module):
    """A SpatialBlock run layer by layer on a rank's sub-network with a halo exchange after every layer but the last (and,
    for block 2, one exchange of its input first): exact on own rows, as `ShardedSpatialBlock`, same layers and kernels."""

    def __init__(self, block, exchange, exchange_input):
        super().__init__()
        self.block, self.exchange_input = block, exchange_input
        self._exchange = exchange

    def forward(self, x, e, xb=None, eb=None, adj_mask=None, dropout=None, attn_dropout=None):
        if adj_mask is not None or dropout is not None or attn_dropout is not None:
            raise NotImplementedError('the sharded forward runs without use_adj and dropout')
        ex = self._exchange
        if self.exchange_input:
            x, e = ex(x.contiguous(), e.contiguous())
        layers = self.block.layers
        net = layers[0].network()
        for i, layer in enumerate(layers):
            layer._net = net
            x, e = layer(x, e, xb if i == 0 else None, eb if i == 0 else None)
            if i + 1 < len(layers):
                x, e = ex(x.contiguous(), e.contiguous())
        return x, e


class _LocalEmulator(Emulator):
    """The Emulator of one rank: `Emulator` on the rank's sub-network whose action tables keep the GLOBAL columns and whose
    flow balance first receives the owners' gated flows of the halo links incident to own nodes."""

    def get_edge_action(self, a, g=True):
        table = torch.cat([torch.ones_like(a[..., :1]), a], dim=-1)
        return table[..., self._dev_index('edge_action', self._edge_act_cols, a.device)].unsqueeze(-1)

    def get_action(self, a, g=True):
        table = torch.cat([torch.ones_like(a[..., :1]), a], dim=-1)
        return (table[..., self._dev_index('act_out', self._node_act_cols[0], a.device)],
                table[..., self._dev_index('act_in', self._node_act_cols[1], a.device)])

    def _flow_balance(self, flow):
        f = flow.reshape(-1, self.n_edge, 1).contiguous()
        _, f = self._flow_exchange(None, f)        # in place; out of place (a new leaf) while a training step records its tape
        return super()._flow_balance(f.reshape(flow.shape))


def global_action_columns(emul):
    """Column (1-based, 0 = no actuator) of the action vector that drives every link, and every node as the from / to end of
    an actuated link -- the maps `Emulator.get_edge_action` / `get_action` build, over the WHOLE network."""
    n_act = len(emul._act_edge_index())
    link = np.zeros(emul.n_edge, dtype=np.int64)
    link[emul._act_edge_index()] = np.arange(1, n_act + 1)
    out_o, out_i = np.zeros(emul.n_node, dtype=np.int64), np.zeros(emul.n_node, dtype=np.int64)
    out_o[emul.act_edges[:, 0]] = np.arange(1, len(emul.act_edges) + 1)
    out_i[emul.act_edges[:, 1]] = np.arange(1, len(emul.act_edges) + 1)
    return link, out_o, out_i


def shard_emulator(emul, prob, device, group=None):
    """The `ShardedEmulator` of one rank: an `Emulator` on `prob.graph` (the `args.graph` CSR path, local rows own first)
    carrying the global model's state -- row-local parameters copied, NodeEdge parameters gathered onto the local support,
    per-row constants and norms sliced to the local rows, the `_has_*` flags and the action columns of the GLOBAL model.
    `emul` stays the rank's global replica (training: `ShardedEmulator.loss_and_grad` / `fit_eval`).  Refuses
    (NotImplementedError / ValueError) what has no bounded halo or is not built: conv=False, a conv other than GAT,
    graph_base, use_adj, dropout, and a NodeEdge bias that is non-zero off the incidence support."""
    why = _refuse_unsharded_configuration(emul)
    if why is not None:
        raise why[0]('shard_emulator: ' + why[1])
    from types import SimpleNamespace
    nodes, links = np.asarray(prob.nodes, dtype=np.int64), np.asarray(prob.links, dtype=np.int64)
    args = dict(vars(emul._args))
    nmap = np.full(emul.n_node, -1, dtype=np.int64)
    nmap[nodes] = np.arange(len(nodes))
    act_edges = None
    if emul.act:
        ae = nmap[np.asarray(emul.act_edges, dtype=np.int64)]
        act_edges = ae[(ae >= 0).all(1)]           # documentation only: the action maps below carry the global columns
    const = lambda name, idx: getattr(emul, name).detach().cpu().numpy()[idx].astype(np.float64)
    ly0 = emul.block1.layers[0]
    args.update(state_shape=(len(nodes), emul._args.state_shape[1]), edge_state_shape=(len(links), emul.e_in),
                edges=np.asarray(prob.graph.edges), graph=prob.graph, adj=None, edge_adj=None, node_edge=None,
                act_edges=act_edges, dropout=0.0, graph_base=0, use_adj=False, sparse_params=ly0.node_edge_n.sparse,
                **{k: const(k, nodes) for k in ('is_outfall', 'area', 'pump_in', 'pump_out', 'hmax', 'hmin')},
                **{k: const(k, links) for k in ('ehmax', 'pump', 'offset')})
    local = _LocalEmulator(emul.conv, emul.resnet, emul.recurrent, SimpleNamespace(**args), precision=ly0.precision)
    # parameters: row-local ones copied; NodeEdge gathered onto the local support (sparse) or sliced (dense (R, M))
    dev = torch.device(device)
    ti = lambda a: torch.as_tensor(a, dtype=torch.int64)
    gp = dict(emul.named_parameters())
    with torch.no_grad():
        for name, p in local.named_parameters():
            src = gp[name].detach().cpu()
            if '.node_edge_n.' in name or '.node_edge_e.' in name:
                rows_n = name.split('.')[-2] == 'node_edge_n'
                if src.dim() == 1:
                    src = src[ti(prob.inc_n_pos if rows_n else prob.inc_e_pos)]
                else:
                    src = src[ti(nodes)][:, ti(links)] if rows_n else src[ti(links)][:, ti(nodes)]
            if tuple(src.shape) != tuple(p.shape):
                raise ValueError('shard_emulator: parameter %s %r does not map onto the local %r' % (name, tuple(src.shape), tuple(p.shape)))
            p.copy_(src)
    local.requires_grad_(False)
    local.to(dev)
    # host-side facts of the WHOLE network (a part whose links are all pumped must not take the pump override on its own)
    for flag in ('_has_offset', '_has_pump', '_has_link_pump', '_has_any_pump'):
        setattr(local, flag, getattr(emul, flag))
    if emul.act:
        link, out_o, out_i = global_action_columns(emul)
        local._edge_act_cols, local._node_act_cols = link[links], (out_o[nodes], out_i[nodes])
    norms = {}
    for k, t in emul._norms.items():
        t = t.detach().cpu()
        norms[k] = (t[:, ti(links)] if k == 'e' else t[:, ti(nodes)]).numpy()
    local.set_norm(*(norms.get(k) for k in 'xbyre'))
    return ShardedEmulator(local, prob, dev, group, global_model=emul)


class ShardedEmulator:
    """One rank's share of a graph-sharded `Emulator` forward / `predict_tf` / `predict` (built by `shard_emulator`).

    Inputs are the rank's LOCAL rows (own rows first, then halo rows) of the replicated global tensors (`scatter_inputs`);
    actions `a` are the global (B, T, n_act) settings.  Schedule, L = n_sp_layer:
      embeddings on all local rows (inputs are exact on halo rows: no exchange);
      block 1 with an exchange after each layer but the last (L - 1, width d, S = B seq_in);
      temporal stack 1, the last seq_out steps, ONE exchange of them (width H, S = B seq_out);
      block 2 with L - 1 exchanges (its first layer reads the exact b / ae pieces); temporal stack 2 and heads (row-local);
      post-processing: link gates (exact on own links: a link's from-node has the link's owner), ONE link-only exchange of
      the gated flow column (`flow_rows`, edge_fusion only), the flow balance on the local incidence, node gates / pumped-
      storage depth / constrain_tf (row-local);
      predict_tf / predict: ONE exchange of the final (y, ey), so the returned local tensors are exact on ALL local rows
      and can be fed back as the next chunk's input without another scatter (mpc.predict_horizon).
    `forward` returns local tensors exact on OWN rows (`own`).  `exchange` / `flow_exchange` are attributes (defaults:
    `HaloExchangeAll` over the plan's lists / over `flow_rows`); anything with the same `__call__(x, e)` may replace them
    (training also needs their `adjoint(gx, ge)`).

    Training (`loss_and_grad`, `fit_eval`; DESIGN.md section 8, "training across the cut"): `global_model` is this rank's
    replica of the whole Emulator, which holds the authoritative parameters and the Adam state.  The forward records every
    exchange on a tape, out of place; the reverse schedule runs the adjoint exchanges on the calling thread; the loss is
    summed over own rows and divided by the global sample counts; the gradients go into the global layout and are summed over
    the ranks by `reduce` -- the one hook every cross-rank reduction goes through."""

    def __init__(self, local, prob, device, group=None, global_model=None):
        self.local, self.prob, self.device = local, prob, torch.device(device)
        self.group, self.global_model = group, global_model
        self.exchange = HaloExchangeAll(prob, device, group)
        self.flow_exchange = HaloExchangeAll(prob, device, group, rows=flow_rows(prob))
        self._tape = None                     # a list while a training forward runs: (exchange, pre, post) per exchange
        local.block1 = _ExchangedBlock(local.block1, lambda x, e: self._exchanged(self.exchange, x, e), False)
        local.block2 = _ExchangedBlock(local.block2, lambda x, e: self._exchanged(self.exchange, x, e), True)
        local._flow_exchange = lambda x, e: self._exchanged(self.flow_exchange, x, e)
        self.n_own_nodes, self.n_own_links = len(prob.own_nodes), len(prob.own_links)

    # model facts read by callers such as mpc.predict_horizon
    seq_in = property(lambda self: self.local.seq_in)
    seq_out = property(lambda self: self.local.seq_out)
    if_flood = property(lambda self: self.local.if_flood)
    act = property(lambda self: self.local.act)

    def get_edge_action(self, a, g=True):
        """(B, T, n_local_links, 1): the global settings spread over the local links (global action columns)."""
        return self.local.get_edge_action(a, g)

    def scatter_inputs(self, X, B, E, AE=None):
        """The local rows of replicated global inputs: X (B, T, N, C), B (B, T, N, b) node tensors, E (B, T, E, C), AE
        (B, T, E, 1) link tensors (None passes through); own + halo rows are simply read."""
        dev = X.device
        ni = self.local._dev_index('scatter_nodes', self.prob.nodes, dev)
        li = self.local._dev_index('scatter_links', self.prob.links, dev)
        pick = lambda t, idx: None if t is None else t.index_select(2, idx).contiguous()
        return pick(X, ni), pick(B, ni), pick(E, li), pick(AE, li)

    def own(self, y, ey=None):
        """The own rows of local node (..., n_local_nodes, C) / link tensors; one tensor in, one out."""
        oy = y[..., :self.n_own_nodes, :]
        return oy if ey is None else (oy, ey[..., :self.n_own_links, :])

    @staticmethod
    def _inference_only(*tensors):
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
            raise NotImplementedError('ShardedEmulator is inference only: no gradients across the cut')

    def forward(self, X, B, E, AE=None):
        """`Emulator.forward` on local rows: (B, T, n_local_nodes, n_out), (B, T, n_local_links, e_out), exact on own rows."""
        self._inference_only(X, B, E, AE)
        return self.local.forward(X, B, E, AE)

    __call__ = forward

    def predict_tf(self, states, b, a=None, edge_state=None):
        """`Emulator.predict_tf` on local rows; the result is exact on ALL local rows."""
        return self._predict(states, b, a, edge_state, False)

    def predict(self, states, b, a=None, edge_state=None):
        """`Emulator.predict` (NumPy-mode post-processing) on local rows; exact on ALL local rows."""
        return self._predict(states, b, a, edge_state, True)

    def _predict(self, states, b, a, edge_state, np_form):
        self._inference_only(states, b, a, edge_state)
        y, ey = self.local._predict(states, b, a, edge_state, np_form)
        # one exchange of the final outputs, both pieces padded to one width
        nb, T, cy, ce = y.shape[0], y.shape[1], y.shape[-1], ey.shape[-1]
        F = max(cy, ce)
        pad = lambda t, c: t if c == F else torch.cat([t, t.new_zeros(t.shape[:-1] + (F - c,))], dim=-1)
        xs = pad(y, cy).reshape(nb * T, y.shape[2], F).contiguous()
        es = pad(ey, ce).reshape(nb * T, ey.shape[2], F).contiguous()
        xs, es = self.exchange(xs, es)
        return xs.reshape(nb, T, -1, F)[..., :cy], es.reshape(nb, T, -1, F)[..., :ce]

    # ------------------------------------------------------------------ training across the cut
    def _exchanged(self, ex, x, e):
        """An exchange of the forward.  Inference: in place, `ex(x, e)`.  While a training step records its tape: out of place
        -- the segment outputs `pre` stay in the autograd graph, the exchange writes into detached copies `post` that become
        new leaves, and (ex, pre, post) goes on the tape for the reverse schedule."""
        if self._tape is None:
            return ex(x, e)
        px = None if x is None else x.detach().clone()
        pe = e.detach().clone()
        ex(px, pe)
        post = tuple(None if t is None else t.requires_grad_() for t in (px, pe))
        self._tape.append((ex, (x, e), post))
        return post

    def _reverse(self, loss):
        """The reverse schedule, on the calling thread (never inside the autograd engine, whose one worker thread per device
        would wait on a peer's message while holding every rank's backward): the loss first, then every tape entry from the
        last to the first -- adjoint exchange of the gradient that reached `post`, then on through `pre`.  In reverse order
        `post_k` has received all of its gradient (from the loss and from the later `pre_j`) when its turn comes; the graph is
        retained until the last call because the residual links the first segment straight to the heads."""
        tape, self._tape = self._tape, None
        loss.backward(retain_graph=bool(tape))
        for k in range(len(tape) - 1, -1, -1):
            ex, pre, post = tape[k]
            g = [None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)).contiguous() for t in post]
            ex.adjoint(g[0], g[1])
            outs = [(p, gp) for p, gp in zip(pre, g) if p is not None and p.requires_grad]
            if outs:
                torch.autograd.backward([p for p, _ in outs], [gp for _, gp in outs], retain_graph=k > 0)
        del tape

    def reduce(self, t):
        """Sum `t` over the ranks (in place where the backend allows; returns the summed tensor): `dist.all_reduce` SUM over
        `group` when torch.distributed is initialised with more than one rank, else `t`.  Every cross-rank reduction of a
        training step goes through here -- the loss parts with the non-finite flag, then the gradient buffer -- so an
        in-process test may replace it with a fixed-rank-order sum."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            if dist.get_backend(self.group) == 'gloo' and t.is_cuda:
                c = t.cpu()
                dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.group)
                return c.to(t.device)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def _check_trainable(self):
        g = self.global_model
        if g is None:
            raise ValueError('ShardedEmulator training needs the global model replica (build it with shard_emulator)')
        if g.gradnorm:
            raise NotImplementedError('sharded training without GradNorm: its task weights need per-task gradient norms at a '
                                      'shared layer, not built across the cut')
        if g.roll:
            raise NotImplementedError('sharded training with roll=%d: fed-back chunks would need the output exchange on the tape' % g.roll)
        if g.if_flood and g.balance:
            raise NotImplementedError('if_flood with balance: the reference leaves fl_loss undefined here (emulator.py:466,473)')
        for name, p in g.named_parameters():
            if ('.node_edge_n.' in name or '.node_edge_e.' in name) and p.dim() != 1:
                raise ValueError('sharded training needs sparse NodeEdge parameters (sparse_params=True): %s is a dense %r -- the '
                                 "reference's dense bias trains OFF the incidence support, every node then depends on every link and "
                                 'no halo of bounded radius exists' % (name, tuple(p.shape)))

    def own_loss_weights(self, device):
        """nwei / ewei / poswei of the OWN rows, sliced from the GLOBAL model's `_loss_setup` (its head-range reweighting uses
        statistics of all nodes, which a part cannot recompute)."""
        hit = getattr(self, '_lw_own', None)
        if hit is None or hit[0] != device:
            lw = self.global_model._loss_setup(device)
            ni = torch.as_tensor(self.prob.own_nodes, dtype=torch.int64, device=device)
            li = torch.as_tensor(self.prob.own_links, dtype=torch.int64, device=device)
            hit = self._lw_own = (device, dict(nwei=lw['nwei'].index_select(0, ni), ewei=lw['ewei'].index_select(0, li),
                                               poswei=lw['poswei'].index_select(0, ni)))
        return hit[1]

    def loss_parts(self, y, b, preds, ey, edge_preds):
        """This rank's share of [node_loss, (flood_loss,) edge_loss] of `Emulator.fit_eval`: the per-sample terms of the OWN
        rows summed and divided by the GLOBAL sample count (B T N for the node terms, B T E for the link term), so that the sum
        over ranks is the whole-network loss.  Local tensors (own rows first)."""
        g, lc = self.global_model, self.local
        lw = self.own_loss_weights(preds.device)
        no, lo = self.n_own_nodes, self.n_own_links
        nb, T = preds.shape[0], preds.shape[1]
        cn, ce = float(nb * T * g.n_node), float(nb * T * g.n_edge)
        mse = lambda t, p, w=None: (((p - t) ** 2).mean(dim=-1) * (1.0 if w is None else w)).sum()
        if g.balance:
            q_w, pr = lc.constrain_tf(lc.normalize(preds, 'y', True), lc.normalize(b, 'b', True)[..., :1])
            q_w = (q_w / lc._norm('y', preds.device)[0, :, -1]).unsqueeze(-1)
            pr = lc.normalize(pr, 'y').clamp(0, 1)
            true = torch.cat([y[..., :3], y[..., -1:]], dim=-1)[..., :no, :]
            node = mse(true * lw['nwei'], torch.cat([pr[..., :3], q_w], dim=-1)[..., :no, :] * lw['nwei']) / cn
        else:
            node = mse(y[..., :no, :3] * lw['nwei'], preds[..., :no, :3] * lw['nwei']) / cn
        parts = [node]
        if g.if_flood and not g.balance:
            yo = y[..., :no, :]
            weight = lw['poswei'] * yo[..., -2] + lw['nwei'][:, -1] * (1 - yo[..., -2])
            p = preds[..., :no, -1:].clamp(1e-7, 1 - 1e-7)
            t = yo[..., -2:-1]
            per = -(t * torch.log(p) + (1 - t) * torch.log(1 - p)).mean(dim=-1)
            parts.append((per * weight).sum() / cn)
        parts.append(mse(ey[..., :lo, :], edge_preds[..., :lo, :], lw['ewei']) / ce)
        return parts

    def _reduced_losses(self, parts, flag=None):
        vec = torch.stack([p.detach().float() for p in parts] + ([] if flag is None else [flag]))
        vec = self.reduce(vec)
        return [vec[i] for i in range(len(parts))], (None if flag is None else float(vec[-1]))

    def _global_layout(self):
        if getattr(self, '_layout', None) is None:
            lay, off = {}, 0
            for name, p in self.global_model.named_parameters():
                lay[name] = (off, tuple(p.shape))
                off += p.numel()
            pos = {True: torch.as_tensor(self.prob.inc_n_pos, dtype=torch.int64, device=self.device),
                   False: torch.as_tensor(self.prob.inc_e_pos, dtype=torch.int64, device=self.device)}
            self._layout = (lay, off, pos)
        return self._layout

    @staticmethod
    def _global_name(name):
        """The global model's name of a local parameter (the local spatial blocks are wrapped in `_ExchangedBlock`)."""
        for b in ('block1', 'block2'):
            if name.startswith(b + '.block.'):
                return b + name[len(b) + 6:]
        return name

    @staticmethod
    def _support_rows(name):
        """None for a row-local parameter, else True / False: a sparse NodeEdge parameter on the node / link rows."""
        if '.node_edge_n.' in name or '.node_edge_e.' in name:
            return name.split('.')[-2] == 'node_edge_n'
        return None

    def loss_and_grad(self, x, a, b, y, ex, ey):
        """The whole-network loss and gradient of one `fit_eval` step, computed on this rank's part.  Local rows of NORMALISED
        tensors: x, b, ex as `scatter_inputs` gives them, y (B, T, n_local_nodes, C), ey (B, T, n_local_links, C) picked the
        same way; a the global (B, T, n_act) settings.  Returns (losses, grads): `fit_eval`'s list of 0-d tensors with the
        GLOBAL values, and {global parameter name: gradient summed over the ranks}; every rank returns the same."""
        self._check_trainable()
        lc = self.local
        params = [(self._global_name(n), p) for n, p in lc.named_parameters()]
        for _, p in params:
            p.grad = None
            p.requires_grad_(True)
        self._tape = []
        try:
            with torch.enable_grad():
                ae = lc.get_edge_action(a, True) if lc.act else None
                preds, edge_preds = lc._model(x, a, b, ex, ae, None, True)
                parts = self.loss_parts(y, b, preds, ey, edge_preds)
                loss = sum(parts[1:], parts[0])
                losses, bad = self._reduced_losses(parts, (~torch.isfinite(loss.detach())).float())
                if bad > 0:                        # decided on all ranks together: all raise, none waits in an exchange
                    raise FloatingPointError('Loss contains NaN or Inf values.')
                self._reverse(loss)
        finally:
            self._tape = None
            for _, p in params:
                p.requires_grad_(False)
        lay, total, pos = self._global_layout()
        flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        for name, p in params:
            if p.grad is None:
                continue
            off, shape = lay[name]
            n = 1
            for v in shape:
                n *= v
            rows = self._support_rows(name)
            g = p.grad.reshape(-1).float()
            if rows is None:
                flat[off:off + n] = g
            else:                               # local support entries map to distinct global entries
                flat[off:off + n].index_copy_(0, pos[rows], g)
            p.grad = None
        flat = self.reduce(flat)
        grads = {}
        for name, (off, shape) in lay.items():
            n = 1
            for v in shape:
                n *= v
            grads[name] = flat[off:off + n].view(shape)
        return losses, grads

    def fit_eval(self, x, a, b, y, ex, ey, fit=True):
        """`Emulator.fit_eval` on a graph-sharded network (same tensors as `loss_and_grad`).  fit=True: the summed gradient
        steps the global replica's KerasAdam (per-variable clipnorm = 1 needs the whole gradient), then the local parameters
        are refreshed in place from it; the replicas stay the same bits on every rank.  fit=False: evaluation only.
        Returns the global [node_loss, (flood_loss,) edge_loss] as 0-d tensors."""
        self._check_trainable()
        if not fit:
            with torch.no_grad():
                lc = self.local
                ae = lc.get_edge_action(a, True) if lc.act else None
                preds, edge_preds = lc._model(x, a, b, ex, ae, None, False)
                return self._reduced_losses(self.loss_parts(y, b, preds, ey, edge_preds))[0]
        losses, grads = self.loss_and_grad(x, a, b, y, ex, ey)
        g = self.global_model
        gparams = list(g.named_parameters())
        for name, p in gparams:
            p.grad = grads[name].to(p.device)
        if g._optimizer is None:
            from .emulator import KerasAdam
            g._optimizer = KerasAdam([p for _, p in gparams], g.learning_rate, clipnorm=1.0)
        g._optimizer.step()
        for _, p in gparams:
            p.grad = None
        self.refresh()
        return losses

    @torch.no_grad()
    def refresh(self):
        """Copy the global replica's parameters into the local ones, in place (`copy_`: the versioned caches of packed
        weights and support values see the change)."""
        gp = dict(self.global_model.named_parameters())
        _, _, pos = self._global_layout()
        for name, p in self.local.named_parameters():
            name = self._global_name(name)
            src = gp[name].detach().to(p.device)
            rows = self._support_rows(name)
            p.copy_(src if rows is None else src.index_select(0, pos[rows].to(p.device)))
