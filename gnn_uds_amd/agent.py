"""The RL agents' graph encoder on the HIP engine: `ConvNet` of the reference
(`surrogate/agent.py:20-99`) -- Dense embeddings, the SAME spatial block as the emulator (fusion MLPs, NodeEdge, GAT on the
node graph and the line graph, or GCN / Diffusion with their normalised filters; or one conv over the combined graph for
`graph_base`), then Spektral's `GlobalAttnSumPool` over the node rows followed by the link rows (two row blocks, never concatenated;
forward and backward on HIP).  One snapshot per sample, the batch is large: the snapshots of
the fused kernel are the batch elements.

    ConvNet(args, conv)(X, E[, B]) -> (batch, conv_dim)

Weight names follow the Keras layers (`embed_x`, `embed_e`, `block.layers.i.*`, `pool.attn_kernel` (F, 1)).
`args.attn_heads` (default 1; NOT a reference key -- the reference's GATConv layers have one head) builds the GAT layers with H
heads of conv_dim / H channels each, concatenated.
"""
import numpy as np
import torch
from torch import nn

from . import _lib
from . import autograd as _ag
from .graph import DrainageGraph, csr_from_dense, edge_based_adj_csr, node_based_adj_csr
from .layers import Dense, DiffusionConv, GCNConv, GraphBaseBlock, SpatialBlock, _glorot_uniform, _param


class GlobalAttnSumPool(nn.Module):
    """spektral.layers.GlobalAttnSumPool in batch mode: alpha = softmax_n(x @ attn_kernel), out = sum_n alpha_n x_n.  With a
    width the kernels take (a power of two from 4 to 256) the pool runs on HIP, with and without autograd; `forward(x, e)` pools
    over the rows of x followed by those of e without concatenating them."""

    def __init__(self, in_features, generator=None):
        super().__init__()
        self.attn_kernel = _param(_glorot_uniform((int(in_features), 1), 'cpu', generator))
        self.hip = True             # False: the torch composition at every shape (tools/attn_pool_time.py measures against it)
        self.last_path = None       # 'hip' (uds_attn_sum_pool_pair), 'hip-train' (autograd.AttnSumPoolFn) or 'torch': what the last call ran

    def forward(self, x, e=None):
        """x (B, Rx, F)[, e (B, Re, F)]: the pool over the rows of x followed by those of e (the stack is not built on the HIP paths)."""
        if not x.is_cuda:
            raise _lib.UdsError('GlobalAttnSumPool input is on %s: gnn_uds_amd runs on the MI355X only' % x.device)
        F = x.shape[-1]
        if self.hip and x.dim() == 3 and (e is None or e.dim() == 3) and F >= 4 and F <= 256 and (F & (F - 1)) == 0:
            if _ag.grad_on(x, e, self.attn_kernel):                                       # RL training: forward + one-pass backward, no (B, R) tensor
                self.last_path = 'hip-train'
                return _ag.AttnSumPoolFn.apply(x, e, self.attn_kernel)
            self.last_path = 'hip'
            return _lib.attn_sum_pool_pair(x.contiguous(), None if e is None else e.contiguous(), self.attn_kernel)      # one HIP launch
        self.last_path = 'torch'
        if e is not None:
            x = torch.cat([x, e], dim=-2)
        alpha = torch.softmax(torch.matmul(x, self.attn_kernel).squeeze(-1), dim=-1)      # (B, N): every other shape, differentiable
        return torch.matmul(alpha.unsqueeze(-2), x).squeeze(-2)                          # (B, F)


class ConvNet(nn.Module):
    def __init__(self, args, conv='GAT', precision='bf16x3', generator=None):
        super().__init__()
        g = lambda k, d=None: getattr(args, k, d)
        self.conv_dim, self.n_sp_layer = int(g('conv_dim', 128)), int(g('n_sp_layer', 3))
        self.n_node, self.n_in = g('state_shape', (40, 4))
        if g('if_flood', False):
            self.n_in += 1
        self.use_pred = bool(g('use_pred', False))
        self.b_in = (2 if g('tide', False) else 1) if self.use_pred else 0
        self.graph_base = int(g('graph_base', 0))
        self.n_edge, self.e_in = g('edge_state_shape', (40, 3))
        self.activation = g('activation', None) or 'linear'
        self.attn_heads = int(g('attn_heads', 1) or 1)
        kind = 'GAT' if 'GAT' in conv else ('GCN' if 'GCN' in conv else ('Diffusion' if 'Diff' in conv else None))
        if kind is None:
            raise NotImplementedError('conv=%r is not built (GAT, GCN and Diffusion are)' % (conv,))
        pre = {'GAT': None, 'GCN': GCNConv.preprocess, 'Diffusion': DiffusionConv.preprocess}[kind]
        d, a, gen = self.conv_dim, self.activation, generator
        self.embed_x = Dense(d, a, in_features=self.n_in + self.b_in, generator=gen)       # agent.py:78
        self.embed_e = Dense(d, a, in_features=self.e_in, generator=gen)                   # agent.py:79
        graph = g('graph')
        if self.graph_base and isinstance(graph, DrainageGraph):
            # `args.graph`: the combined (N+E) x (N+E) matrix in CSR from the link list (never dense); GCN / Diffusion normalise it there
            build = node_based_adj_csr if self.graph_base == 1 else edge_based_adj_csr
            filt = build(graph.edges, graph.n_node, bool(g('directed', False)), int(g('order', 1)), g('length', 0), g('lengths', None))
            if kind != 'GAT':
                filt = pre(filt)                    # a pattern without values counts as ones
            self.block = GraphBaseBlock(self.n_node, self.n_edge, filt, d, self.n_sp_layer, a, generator=gen, conv=kind, precision=precision,
                                        attn_heads=self.attn_heads)
        elif self.graph_base:
            adj = np.asarray(g('adj'))
            filt = csr_from_dense((adj > 0).astype(int), add_self_loops=True) if kind == 'GAT' else pre(adj)
            self.block = GraphBaseBlock(self.n_node, self.n_edge, filt, d, self.n_sp_layer, a, generator=gen, conv=kind, precision=precision,
                                        attn_heads=self.attn_heads)
        else:
            if isinstance(graph, DrainageGraph):
                if kind != 'GAT' and (graph.raw_adj is None or graph.raw_edge_adj is None):
                    raise ValueError('conv=%r from args.graph needs the raw adjacency matrices (graph.raw_adj / raw_edge_adj): build '
                                     'the graph with DrainageGraph.from_edges or DrainageGraph.from_dense' % (conv,))
                filters = (None, None) if kind == 'GAT' else (pre(graph.raw_adj), pre(graph.raw_edge_adj))
            else:
                adj, edge_adj = np.asarray(g('adj', np.eye(self.n_node))), np.asarray(g('edge_adj', np.eye(self.n_edge)))
                graph = DrainageGraph.from_dense(adj, edge_adj, np.asarray(g('node_edge'), dtype=np.float64), g('edges'))
                filters = (None, None) if kind == 'GAT' else (pre(adj), pre(edge_adj))
            self.block = SpatialBlock(graph, d, self.n_sp_layer, a, generator=gen, precision=precision, conv=kind, filters=filters,
                                      attn_heads=self.attn_heads)
        self.pool = GlobalAttnSumPool(d, generator=gen)

    def forward(self, X, E, B=None):
        """X (batch, N, n_in), E (batch, E, e_in)[, B (batch, N, b_in) when use_pred] -> (batch, conv_dim)."""
        if self.use_pred:
            if B is None:
                raise ValueError('use_pred needs the boundary input B')
            X = torch.cat([X, B], dim=-1)
        x, e = self.embed_x(X.contiguous()), self.embed_e(E.contiguous())
        x, e = self.block(x, e)
        return self.pool(x, e)
