"""`Emulator`: the reference's surrogate model (`surrogate/emulator.py:47-852`) on the HIP engine.

Same constructor (`Emulator(conv, resnet, recurrent, args)`, attributes read from `args` with the reference's
names and defaults, emulator.py:48-127), same method names, positional order and tensor layouts
(`(B,T,N,C)` / `(B,T,E,C)`), re-expressed as a `torch.nn.Module`:

    forward / model          build_network                      emulator.py:166-341
    predict, predict_tf      raw states -> de-normalised (B,T,N,5), (B,T,E,3)        :566-641
    _model                   single chunk or `roll` autoregressive chunks            :400-438
    simulate                 sliding-window evaluation of an event                   :521-564
    post_proc_tf, constrain_tf, normalize, set_norm, get_edge_action, get_action     :364-398,680-810
    save / load              weights + norm_*.npy                                    :814-852

What runs where: every layer of the network (embedding / fusion / head Dense, NodeEdge, GAT / GCN / Diffusion, causal dilated
Conv1D, the resnet prefix sum) and the link->node flow balance of post_proc_tf are HIP kernels behind the C ABI.
The remaining post-processing is elementwise gating / clipping on tensors already in HBM and is written with torch
tensor ops (device plumbing).  Training (`fit_eval`, GradNorm) and `graph_base` 1 / 2 are built for GAT, GCN and
DiffusionConv (inference and training: `autograd.DiffusionFn` on `uds_diffusion_backward`).
`use_adj` (per-time-step adjacency rewritten by the control action) is built for GAT as a mask over the CSR entries, for
inference and training (`autograd.GatFn(edge_mask=)` on `uds_gat_aggregate_ex` / `uds_gat_backward_ex`).
GRU / LSTM temporal nets run (inference and, at 16 to 128 units in steps of 16, training).  Training-time dropout: `layers.Dropout` on `uds_dropout`.  Not built, each raises: `use_adj` with GCN / Diffusion,
GeneralConv (a sparse-mode-only Spektral layer the reference's dense call cannot run either).  conv = False -- the reference's non-graph
baseline, its shipped `*_nncat_*` models -- runs on the same Dense / temporal / cumsum kernels (`_forward_mlp`).
"""
import os
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from . import _lib
from .graph import DrainageGraph, csr_from_dense
from . import autograd as _ag
from .graph import csr_from_dense, edge_based_adj_csr, node_based_adj_csr
from .layers import Dense, DiffusionConv, Dropout, DropoutStream, GATConv, GCNConv, GraphBaseBlock, NodeEdge, PackCache, SpatialBlock, SpatialLayer, _glorot_uniform, _packed_kernel, _param


class Conv1D(nn.Module):
    """keras Conv1D(filters, kernel_size, padding='causal', dilation_rate, activation) along the time axis of
    x (B, T, R, F) -- the reference transposes to (B*R, T, F) first (emulator.py:244), this layout needs no transpose."""

    def __init__(self, filters, kernel_size, dilation_rate=1, activation=None, in_features=None, generator=None,
                 precision='fp32'):
        super().__init__()
        self.filters, self.kernel_size, self.dilation_rate = int(filters), int(kernel_size), int(dilation_rate)
        self.precision = precision
        self.activation = activation or 'linear'
        self.kernel = _param(_glorot_uniform((self.kernel_size, int(in_features), self.filters), 'cpu', generator))
        self.bias = _param(torch.zeros(self.filters))

    def forward(self, x):
        if _ag.grad_on(x, self.kernel, self.bias):
            return _ag.Conv1DFn.apply(x, self.kernel, self.bias, self)
        x = x.contiguous()
        k, f, h = self.kernel.shape
        if self.precision == 'bf16x3' and _lib.rowgemm_supported(k * f, f, h):     # matrix-core path (split-bf16, 3 products)
            return _lib.rowgemm_forward(x, _packed_kernel(self, self.kernel.reshape(k * f, h)), self.bias, h, self.activation,
                                        taps=k, dilation=self.dilation_rate)
        return _lib.conv1d_causal(x, self.kernel, self.bias, self.dilation_rate, self.activation)


# what `Emulator.temporal_route` reads of a temporal layer: is it a Conv1D, its kernel shape (k0, k1, k2), dilation and activation
# (None for GRU / LSTM), precision, output width
TemporalLayer = namedtuple('TemporalLayer', 'conv1d kernel dilation activation precision out')

# what `Emulator.decode` needs of the history (`Emulator.encode_history`): x (B, seq_out, N, H), e (B, seq_out, E, H) after the first
# temporal stage, and the last linear step of the two embeddings, (B, 1, N, d) and (B, 1, E, d) (the resnet residual)
History = namedtuple('History', 'x e x_lin_last e_lin_last')


class _DenseShim:
    """What DenseFn reads of its module, for a bare (kernel, bias) pair."""

    forward_precision = 'fp32'      # the recurrent layers' input projection is exact fp32 at every width (at 64 units its 192 / 256
                                    # columns never fitted the matrix-core row GEMM; a 16-unit GRU's 48 would)

    def __init__(self, precision, units):
        self.precision, self.units = precision, units


class _Recurrent(nn.Module):
    """keras GRU / LSTM(units, return_sequences=True) along the time axis of x (B, T, R, F) (emulator.py:158-161): the input
    projection of every time step is one Dense launch, the recurrence one streaming kernel (uds_recurrent_forward), exact
    fp32; a 64 -> 64 layer with precision='bf16x3' is ONE launch on the matrix cores (uds_recurrent_fused).  Parameters keep the Keras names and shapes -- `kernel` (F, G*units), `recurrent_kernel` (units, G*units), `bias`
    ((2, 3*units) for the TF2 GRU with reset_after=True: input and recurrent bias; (4*units,) for the LSTM) -- and the
    Keras initialisers (glorot_uniform, orthogonal, zeros with the LSTM's forget-gate bias at one).  Under autograd (training) the
    layer runs Dense + `RecurrentFn` (autograd.py): back-propagation through time is one HIP launch (uds_recurrent_backward at 64
    units, uds_recurrent_backward_h at every other multiple of 16 from 16 to 128; other widths raise NotImplementedError)."""
    KIND, G = None, 0

    def __init__(self, units, return_sequences=True, in_features=None, generator=None, precision='fp32'):
        super().__init__()
        self.precision, self._packs = precision, PackCache()
        if not return_sequences:
            raise NotImplementedError('the emulator uses return_sequences=True (emulator.py:159,161)')
        self.units = int(units)
        gh = self.G * self.units
        self.kernel = _param(_glorot_uniform((int(in_features), gh), 'cpu', generator))
        q, _ = torch.linalg.qr(torch.randn(gh, self.units, generator=generator))            # orthogonal initialiser
        self.recurrent_kernel = _param(q.T.contiguous())
        if self.KIND == 'GRU':
            self.bias = _param(torch.zeros(2, gh))
        else:
            b = torch.zeros(gh)
            b[self.units:2 * self.units] = 1.0                                              # unit_forget_bias
            self.bias = _param(b)

    def forward(self, x):
        if _ag.grad_on(x, self.kernel, self.recurrent_kernel, self.bias):
            # training (fit_eval, emulator.py:457-484): input projection through the Dense operator, the recurrence through
            # RecurrentFn (exact-fp32 forward, back-propagation through time on the matrix cores)
            if _lib.recurrent_bwd_route(self.units) is None:
                raise NotImplementedError('the %s backward kernels are built for %s units (hidden_dim a multiple of 16 from 16 to 128), not %d'
                                          % (self.KIND, ', '.join(str(w) for w in _lib.RECURRENT_TRAIN_WIDTHS), self.units))
            b_in, b_rec = (self.bias[0], self.bias[1]) if self.KIND == 'GRU' else (self.bias, None)
            xp = self._projection(x, b_in, True)
            return _ag.RecurrentFn.apply(xp, self.recurrent_kernel, None if b_rec is None else b_rec.contiguous(), self.KIND, self.precision)
        x = x.contiguous()
        b_in, b_rec = (self.bias[0].contiguous(), self.bias[1].contiguous()) if self.KIND == 'GRU' else (self.bias, None)
        F = x.shape[-1]
        if self.precision == 'bf16x3' and self.units == 64 and F % 32 == 0:
            direct = _lib.recurrent_fused_supported(F, self.KIND)

            def build():
                if direct:
                    return (_lib.recurrent_pack(self.kernel, self.recurrent_kernel),)
                # W + U do not fit the LDS together (LSTM at 128) or another width: the projection on the row-GEMM kernel
                fold = b_in.clone()
                if b_rec is not None:
                    fold[:2 * 64] += b_rec[:2 * 64]               # the z / r gates add both biases (the candidate's stays apart)
                return (_lib.recurrent_pack(None, self.recurrent_kernel),
                        [_lib.rowgemm_pack(self.kernel[:, 64 * g:64 * (g + 1)].contiguous()) for g in range(self.G)], fold)
            packed = self._packs.get('recurrent', (self.kernel, self.recurrent_kernel, self.bias), build)
            if direct:
                # the whole layer in one launch on the matrix cores (input projection never written out, state fed back in registers)
                return _lib.recurrent_fused(x, packed[0], b_in, b_rec, self.KIND)
            if _lib.rowgemm_supported(F, F, 64):
                packed_u, packed_w, fold = packed
                xp = torch.empty(x.shape[:-1] + (self.G * 64,), device=x.device, dtype=torch.float32)
                for g, pk in enumerate(packed_w):
                    _lib.rowgemm_cat(x, None, pk, fold[64 * g:64 * (g + 1)].contiguous(), 64, 'linear', out=xp, col0=64 * g)
                return _lib.recurrent_fused(xp, packed_u, None, b_rec, self.KIND, projected=True)
        return _lib.recurrent_forward(self._projection(x, b_in, False), self.recurrent_kernel, b_rec, self.KIND)

    def _projection(self, x, b_in, train):
        """x @ kernel + input bias for every time step, (B, T, R, G*units): one Dense launch up to 256 columns (what uds_dense_act
        takes: every width up to 80 units for the GRU, 64 for the LSTM), 256-column pieces above; train: through DenseFn."""
        gh = self.G * self.units
        pieces = []
        for c0 in range(0, gh, 256):
            k, b = (self.kernel, b_in) if gh <= 256 else (self.kernel[:, c0:c0 + 256], b_in[c0:c0 + 256])
            if train:
                k = k.contiguous()
                pieces.append(_ag.DenseFn.apply(x, k, b.contiguous(), _DenseShim(self.precision, k.shape[1]), 'linear'))
            else:
                pieces.append(_lib.dense_act(x, k.contiguous(), b.contiguous(), 'linear'))
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=-1)


class GRU(_Recurrent):
    KIND, G = 'GRU', 3


class LSTM(_Recurrent):
    KIND, G = 'LSTM', 4


class _AdamState:
    """The checkpoint format `KerasAdam` and `HipKerasAdam` share: one written by either loads into the other."""

    def state_dict(self):
        """Iteration count + first / second moments (what `optimizer.get_weights()` holds in Keras, emulator.py:826)."""
        return {'t': self.t, 'm': [t.detach().cpu() for t in self.m], 'v': [t.detach().cpu() for t in self.v]}

    def load_state_dict(self, sd):
        if len(sd['m']) != len(self.params) or any(tuple(a.shape) != tuple(p.shape) for a, p in zip(sd['m'], self.params)):
            raise ValueError('optimizer state does not match the model parameters')
        self.t = int(sd['t'])
        for dst, src in zip(self.m, sd['m']):
            dst.copy_(src)
        for dst, src in zip(self.v, sd['v']):
            dst.copy_(src)


class KerasAdam(_AdamState):
    """keras.optimizers.Adam(learning_rate, clipnorm) as TF 2.10 applies it (emulator.py:111): every gradient is clipped
    by ITS OWN norm (tf.clip_by_norm), then m, v are updated and var -= lr * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + 1e-7)."""

    def __init__(self, params, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None):
        self.params = list(params)
        self.lr, self.b1, self.b2, self.eps, self.clipnorm = learning_rate, beta_1, beta_2, epsilon, clipnorm
        self.t = 0
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]

    @torch.no_grad()
    def step(self):
        self.t += 1
        lr_t = self.lr * (1 - self.b2 ** self.t) ** 0.5 / (1 - self.b1 ** self.t)
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not idx:
            return
        ps, gs = [self.params[i] for i in idx], [self.params[i].grad for i in idx]
        ms, vs = [self.m[i] for i in idx], [self.v[i] for i in idx]
        norms = torch.stack(torch._foreach_norm(gs))                      # one launch group, one host sync below
        if not bool(torch.isfinite(norms).all()):
            raise FloatingPointError('grads contain NaN/Inf!')
        if self.clipnorm is not None:
            gs = torch._foreach_mul(gs, list((self.clipnorm / torch.clamp(norms, min=self.clipnorm)).unbind()))
        torch._foreach_mul_(ms, self.b1)
        torch._foreach_add_(ms, gs, alpha=1 - self.b1)
        torch._foreach_mul_(vs, self.b2)
        torch._foreach_addcmul_(vs, gs, gs, value=1 - self.b2)
        den = torch._foreach_sqrt(vs)
        torch._foreach_add_(den, self.eps)
        torch._foreach_addcdiv_(ps, ms, den, value=-lr_t)


class HipKerasAdam(_AdamState):
    """`KerasAdam` as ONE HIP operator (uds_adam_step: per-variable norms, clipping, moments and update in two passes over the
    whole parameter list) with the step count and a status word on the device, so that a captured graph can replay a step:
    nothing per step is computed on the host.  Same constructor and the same `state_dict` format as `KerasAdam` (a checkpoint
    written by either loads into the other); `step(loss)` never synchronises -- a non-finite loss or gradient norm leaves every
    parameter, moment and the step count as they were and is reported by `raise_if_not_finite()`, the one 4-byte read of a step."""

    def __init__(self, params, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None):
        self.params = list(params)
        self.lr, self.b1, self.b2, self.eps, self.clipnorm = learning_rate, beta_1, beta_2, epsilon, clipnorm
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.v = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        dev = self.params[0].device if self.params else torch.device('cpu')
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)        # [0] t, [1] status of the last step, [2..3] kernel scratch
        self._ws = torch.empty(_lib.adam_workspace_floats([p.numel() for p in self.params]), dtype=torch.float32, device=dev)

    @property
    def t(self):
        return int(self.state[0])

    @t.setter
    def t(self, value):
        self.state[0] = int(value)

    @torch.no_grad()
    def step(self, loss=None):
        """One update of every parameter that has a gradient (in place; gradients are only read).  loss: the step's 0-d loss
        tensor, tested for NaN / Inf on the device, or None."""
        idx = [i for i, p in enumerate(self.params) if p.grad is not None]
        for i in idx:
            if not self.params[i].is_contiguous():
                raise _lib.UdsError('HipKerasAdam: parameter %d is not contiguous' % i)
        _lib.adam_step([self.params[i] for i in idx], [self.params[i].grad.contiguous() for i in idx], [self.m[i] for i in idx],
                       [self.v[i] for i in idx], self.state, self._ws, None if loss is None else loss.detach().reshape(1), self.lr, self.b1,
                       self.b2, self.eps, self.clipnorm)
        for i in idx:           # the kernel wrote the parameters behind autograd's back: every PackCache must see a change
            torch.autograd.graph.increment_version(self.params[i])

    def raise_if_not_finite(self):
        """The exceptions of the eager step for the last `step`: `fit_eval`'s for a non-finite loss, `KerasAdam.step`'s for a
        non-finite gradient norm.  In either case that step changed nothing."""
        status = int(self.state[1])
        if status & 1:
            raise FloatingPointError('Loss contains NaN or Inf values.')
        if status & 2:
            raise FloatingPointError('grads contain NaN/Inf!')


def _numeric_suffix(name):
    tail = name.rsplit('_', 1)[-1]
    return int(tail) if tail.isdigit() else 0


def _find_keras_weight(weights, lname, kname):
    """The array Keras saved for weight `kname` of layer `lname`, or None.  Tried in turn: the exact names (`<layer>/<w>:0`,
    the HDF5 group path `<layer>/<layer>/<w>:0`, `<layer>/<w>`); for a weight nested in a recurrent cell (`<cell>/<w>`) ANY
    single `*_cell*` sub-group of the layer (the cell's auto-number depends on how many cells the Keras session had created
    before, which the checkpoint does not say); for a DiffusionConv kernel the `diffuse_features*` sub-layers' (K + 1,)
    kernels stacked in numeric order into the (channels, K + 1) array the module keeps."""
    for key in ('%s/%s:0' % (lname, kname), '%s/%s/%s:0' % (lname, lname, kname), '%s/%s' % (lname, kname)):
        if key in weights:
            return weights[key]
    mine = [k for k in weights if isinstance(k, str) and k.split('/')[0] == lname]
    if '/' in kname:                                   # '<cell>/<weight>': match the cell sub-group by suffix
        tail = '/' + kname.split('/', 1)[1]
        hits = [k for k in mine if '_cell' in k and (k.endswith(tail + ':0') or k.endswith(tail))]
        if len(hits) == 1:
            return weights[hits[0]]
        return None
    if kname == 'kernel':
        subs = [k for k in mine if 'diffuse_features' in k and (k.endswith('/kernel:0') or k.endswith('/kernel'))]
        if subs:
            subs.sort(key=lambda k: _numeric_suffix([p for p in k.split('/') if p.startswith('diffuse_features')][-1]))
            return np.stack([np.asarray(weights[k]).reshape(-1) for k in subs])
    return None


class Emulator(nn.Module):
    _snapshot_remainder = False
    _dense_node_edge_train = False
    _fused_gat_backward = False
    _graphed_fit = False
    FIT_GRAPHS = 4             # captured `fit_eval` graphs kept per model (least recently used out)
    last_fit_path = None       # 'graph' (replayed), 'graph-capture' (captured, then replayed) or 'eager' after a fit_eval call
    last_fit_refusal = None    # with graphed_fit: why the last fit_eval call ran eager (fit_graph_refusal), or None

    def __init__(self, conv=None, resnet=False, recurrent=None, args=None, precision='bf16x3', generator=None):
        super().__init__()
        g = lambda k, d=None: getattr(args, k, d)
        self.n_node, self.n_in = g('state_shape', (40, 4))
        self.tide = bool(g('tide', False))
        self.b_in = 2 if self.tide else 1
        act = g('act', False)
        self.act = bool(act and act != 'False')
        self.n_out = self.n_in - 1
        self.seq_in, self.seq_out = g('seq_in', 6), g('seq_out', 1)
        self.embed_size, self.hidden_dim = g('embed_size', 64), g('hidden_dim', 64)
        self.kernel_size, self.n_sp_layer, self.n_tp_layer = g('kernel_size', 3), g('n_sp_layer', 3), g('n_tp_layer', 2)
        self.dropout = g('dropout', 0.0)
        self.activation = g('activation', 'relu')
        # attention heads of the GATConv layers: NOT a reference key (the reference builds every GATConv with Spektral's default,
        # one head); H > 1 gives H heads of embed_size / H channels each, concatenated -- the same width and bytes per row
        self.attn_heads = int(g('attn_heads', 1) or 1)
        self.if_flood = int(g('if_flood', 0))
        if self.if_flood:
            self.n_in += 1
        self.epsilon = g('epsilon', -1.0)
        self.graph_base = g('graph_base', 0)
        self.edge_fusion = bool(g('edge_fusion', False))
        self.edges = np.asarray(g('edges'))
        self.n_edge, self.e_in = g('edge_state_shape', (40, 4))
        self.e_out = self.e_in - 1
        if self.edge_fusion:
            self.n_out -= 2
        self.use_adj = bool(g('use_adj', False)) if self.act else False
        self.act_edges = np.asarray(g('act_edges', np.zeros((0, 2), dtype=int))) if self.act else None
        self.roll = int(g('roll', 0))
        self.model_dir = g('model_dir')
        self.balance = bool(g('balance', False))
        self.gradnorm = bool(g('gradnorm', False))
        self.learning_rate = float(g('learning_rate', 1e-3))
        self._args, self._optimizer, self._lw = args, None, None
        self.resnet = bool(resnet)
        self.conv = False if conv in (None, 'None', 'False', 'NoneType', False) else conv
        self.recurrent = recurrent
        if not self.conv:
            # the reference's non-graph baseline (its shipped `*_nncat_*` models, `conv: 'False'`): node and link states flattened into
            # one vector per time step, Dense layers instead of graph convolutions (emulator.py:181-182,197-212,236-237); the graph
            # is still needed by the post-processing (link -> node flow balance)
            self.conv_kind = 'GAT'
        elif 'GAT' in self.conv:
            self.conv_kind = 'GAT'
        elif 'GCN' in self.conv:
            self.conv_kind = 'GCN'
        elif 'Diff' in self.conv:                      # emulator.py:135-138
            self.conv_kind = 'Diffusion'
        else:
            # GeneralConv (emulator.py:146-149) is a sparse-mode-only Spektral layer: the reference's dense mixed-mode call
            # does not run with it either
            raise NotImplementedError('conv=%r is not built (GAT, GCN and Diffusion are)' % (conv,))
        if self.use_adj and self.conv_kind != 'GAT':
            raise NotImplementedError('use_adj is built for conv=GAT (GCN / Diffusion re-normalise the rewritten adjacency per time step: '
                                      'emulator.py:355-358)')
        if self.graph_base not in (0, 1, 2):
            raise ValueError('graph_base must be 0, 1 (node-based) or 2 (edge-based), got %r' % (self.graph_base,))
        if recurrent not in ('Conv1D', 'GRU', 'LSTM', None, 'None', False):
            raise NotImplementedError('recurrent=%r: Conv1D, GRU, LSTM or none (emulator.py:154-163)' % (recurrent,))
        # keras Dropout layers (:199-213,234-235,287-288,314-318) and Spektral's attention dropout inside every GATConv (rate 0.5): active
        # only in `forward(..., training=True)` = `fit_eval(fit=True)` (`self.model(inp, training=fit)`, :411,434); one counter-based
        # stream for all of them (layers.Dropout, GATConv(attn_dropout=))
        self.dropout_stream = DropoutStream(generator=generator) if self.dropout else None
        self._drop02 = Dropout(0.2, self.dropout_stream) if self.dropout else None
        self._drop = Dropout(self.dropout, self.dropout_stream) if self.dropout else None

        graph = g('graph')
        self._base_filter = None
        if self.graph_base:
            # ONE graph over nodes and links (base.py:471-532); `args.adj` is then the combined (N+E) x (N+E) matrix
            # (base.py:320-323) -- or, with `args.graph`, the pattern is rebuilt in CSR from the link list
            self.graph = graph if isinstance(graph, DrainageGraph) else DrainageGraph.from_edges(self.edges, self.n_node)
            node_edge = None if isinstance(graph, DrainageGraph) else np.asarray(g('node_edge'), dtype=np.float64)
            if g('adj') is not None and not isinstance(graph, DrainageGraph):
                adj = np.asarray(g('adj'))
                if adj.shape != (self.n_node + self.n_edge,) * 2:
                    raise ValueError('graph_base needs the combined (N+E, N+E) adjacency, got %r' % (adj.shape,))
                if self.conv_kind != 'GAT':
                    self._base_filter = (GCNConv if self.conv_kind == 'GCN' else DiffusionConv).preprocess(adj)
                else:
                    self._base_filter = csr_from_dense((adj > 0).astype(int), add_self_loops=True)
            else:
                build = node_based_adj_csr if self.graph_base == 1 else edge_based_adj_csr
                self._base_filter = build(self.edges, self.n_node, bool(g('directed', False)), int(g('order', 1)), g('length', 0), g('lengths', None))
                if self.conv_kind != 'GAT':       # the builders carry their values (none = ones, or the Gaussian kernel): normalised on the CSR
                    self._base_filter = (GCNConv if self.conv_kind == 'GCN' else DiffusionConv).preprocess(self._base_filter)
            self.filter = self.edge_filter = None
        elif isinstance(graph, DrainageGraph):
            # large networks: `args.graph` (CSR, e.g. DrainageGraph.from_edges) instead of the dense (N,N) / (E,E) / (N,E)
            # matrices of `args.adj`, `args.edge_adj`, `args.node_edge`, which cannot exist at N >= 50k
            self.graph, self.filter, self.edge_filter, node_edge = graph, None, None, None
            if self.conv_kind != 'GAT':
                # GCN / Diffusion normalise the RAW matrices (values kept, no forced diagonal) on their CSR pattern; the Diffusion
                # layers then run their table-free form (layers.DiffusionConv)
                if graph.raw_adj is None or graph.raw_edge_adj is None:
                    raise ValueError('conv=%r from args.graph needs the raw adjacency matrices (graph.raw_adj / raw_edge_adj): build '
                                     'the graph with DrainageGraph.from_edges or DrainageGraph.from_dense' % (conv,))
                pre = (GCNConv if self.conv_kind == 'GCN' else DiffusionConv).preprocess
                self.filter, self.edge_filter = pre(graph.raw_adj), pre(graph.raw_edge_adj)
        else:
            adj = np.asarray(g('adj', np.eye(self.n_node)))
            edge_adj = np.asarray(g('edge_adj', np.eye(self.n_edge)))
            node_edge = np.asarray(g('node_edge'), dtype=np.float64)
            self.graph = DrainageGraph.from_dense(adj, edge_adj, node_edge, self.edges)
            if self.use_adj:
                # get_adj_action rewrites entries of the RAW adjacency and casts to int (emulator.py:343-361): with a weighted
                # adjacency (length > 0: Gaussian kernel values < 1) that cast removes every off-diagonal entry, actuated or
                # not -- kept as the reference has it: the raw values at the pattern's entries (the forced diagonal reads 0)
                ga = self.graph.adj
                rows = np.repeat(np.arange(ga.n_rows), np.diff(ga.rowptr))
                self._adj_raw = np.asarray(adj, dtype=np.float64)[rows, np.asarray(ga.col, dtype=np.int64)]
            if self.conv_kind != 'GAT':
                pre = (GCNConv if self.conv_kind == 'GCN' else DiffusionConv).preprocess
                self.filter, self.edge_filter = pre(adj), pre(edge_adj)                                   # emulator.py:133-134,137-138
            else:
                self.filter, self.edge_filter = (adj > 0).astype(int), (edge_adj > 0).astype(int)        # emulator.py:143-145

        # per-node / per-link physical constants (emulator.py:71-98), kept as float32 buffers
        vec = lambda k, n, d: torch.as_tensor(np.asarray(g(k, np.full(n, d)), dtype=np.float64), dtype=torch.float32)
        for name, n, d in (('is_outfall', self.n_node, 0.0), ('area', self.n_node, 0.0), ('pump_in', self.n_node, 0.0),
                           ('pump_out', self.n_node, 0.0), ('hmax', self.n_node, 1.5), ('hmin', self.n_node, 0.0),
                           ('ehmax', self.n_edge, 0.5), ('pump', self.n_edge, 0.0), ('offset', self.n_edge, 0.0)):
            self.register_buffer(name, vec(name, n, d), persistent=False)
        # dense signed incidence: only the offset / pump branches of post_proc_tf use it (small networks)
        self.register_buffer('node_edge', None if node_edge is None else torch.as_tensor(node_edge, dtype=torch.float32), persistent=False)
        self.register_buffer('_inc_sign', torch.as_tensor(self.graph.inc_n.val, dtype=torch.float32), persistent=False)
        self._inc_handle = None
        self._norms = {}
        # host-side facts about the constant buffers (the reference tests them per call, emulator.py:688,698,630): decided once,
        # so the forward path has no device -> host synchronisation (and can be captured into a HIP graph)
        self._has_offset = bool(float(self.offset.max()) > 0) if self.n_edge else False
        self._has_pump = bool(float(self.pump.min()) > 0) if self.n_edge else False             # `self.pump.min() > 0` (:698)
        self._has_link_pump = bool(float(self.pump.abs().max()) > 0) if self.n_edge else False   # any rated link pump (NumPy-mode override, :656-659)
        self._has_any_pump = bool(float(self.pump_in.sum() + self.pump_out.sum() + self.pump.sum()) > 0)
        self._idx_cache = {}
        self._norm_derived = {}
        self._graph = None

        d, h, H, L, gen = self.embed_size, self.embed_size // 2, self.hidden_dim, self.n_sp_layer, generator
        a = self.activation
        pr = precision
        if not (self.recurrent in ('Conv1D', 'GRU', 'LSTM') and self.n_tp_layer):
            H = d                                                                               # no temporal net: widths stay d
        if not self.conv:
            self._build_mlp(d, h, H, L, a, gen, pr)
            return
        self.embed_x = Dense(d, 'linear', in_features=self.n_in, generator=gen)                 # emulator.py:198
        self.embed_b = Dense(h, a, in_features=self.b_in, generator=gen)                        # :203
        self.embed_e = Dense(d, 'linear', in_features=self.e_in, generator=gen)                 # :206
        self.embed_ae = Dense(h, a, in_features=1, generator=gen) if self.act else None         # :212
        # NodeEdge parameters: the reference's dense (R, M) pair, or one (weight, bias) per support entry (`args.sparse_params`,
        # default: above 16M matrix entries) -- the latter cannot hold a bias trained off the support (load_keras_weights raises)
        sp = getattr(args, 'sparse_params', None)
        sp = self.n_node * self.n_edge > (1 << 24) if sp is None else bool(sp)
        if self.graph_base:
            self.block1 = GraphBaseBlock(self.n_node, self.n_edge, self._base_filter, d, L, a, generator=gen, conv=self.conv_kind,
                                         precision=precision, attn_heads=self.attn_heads)                              # :220-223
        else:
            self.block1 = SpatialBlock(self.graph, d, L, a, sparse_params=sp, generator=gen, precision=precision,
                                       conv=self.conv_kind, filters=(self.filter, self.edge_filter),
                                       attn_heads=self.attn_heads)                                                    # :219-235
        self.tem1_x, self.tem1_e = self._tem_net(d, H, gen, pr), self._tem_net(d, H, gen, pr)     # :247,254
        fx2, fe2 = H + h, H + (h if self.act else 0)
        if self.graph_base:
            if fx2 != fe2:
                raise ValueError('graph_base stacks node and link rows in block 2: needs act=True (equal widths %d / %d)' % (fx2, fe2))
            self.block2 = GraphBaseBlock(self.n_node, self.n_edge, self._base_filter, d, L, a, f_in=fx2, generator=gen,
                                         conv=self.conv_kind, precision=precision, attn_heads=self.attn_heads)         # :273-276
        else:
            self.block2 = SpatialBlock(self.graph, d, L, a, fx=fx2, fe=fe2, sparse_params=sp, generator=gen, precision=precision,
                                       conv=self.conv_kind, filters=(self.filter, self.edge_filter),
                                       attn_heads=self.attn_heads)                                                    # :272-288
        self.tem2_x, self.tem2_e = self._tem_net(d, H, gen, pr), self._tem_net(d, H, gen, pr)     # :302,308
        self._build_heads(d, h, H, a, gen, pr)

    def _tem_net(self, f, H, gen, pr):
        """`get_tem_nets` (:154-163) on an f-wide input: n_tp_layer causal Conv1D layers with dilation 2**i, or GRU / LSTM layers."""
        def layer(i):
            fi = f if i == 0 else H
            if self.recurrent == 'Conv1D':
                return Conv1D(H, self.kernel_size, 2 ** i, self.activation, in_features=fi, generator=gen, precision=pr)
            return (GRU if self.recurrent == 'GRU' else LSTM)(H, in_features=fi, generator=gen, precision=pr)
        return nn.ModuleList([layer(i) for i in range(self.n_tp_layer if self.recurrent in ('Conv1D', 'GRU', 'LSTM') else 0)])

    def _build_heads(self, d, h, H, a, gen, pr, N=1, E=1):
        """The output stage (:313-337).  N, E: the MLP model's heads emit all nodes / links of a step at once."""
        self.res_x = Dense(d, 'linear' if self.resnet else a, in_features=H, generator=gen, precision=pr)     # :313 'dense_resx'
        self.res_e = Dense(d, 'linear' if self.resnet else a, in_features=H, generator=gen, precision=pr)     # :317
        self.out = Dense(self.n_out * N, 'hard_sigmoid', in_features=d, generator=gen, precision=pr)          # :322-325
        fl, fi = [], d
        for _ in range(self.if_flood):
            fl.append(Dense(h, a, in_features=fi, generator=gen, precision=pr))                               # :329
            fi = h
        self.flood = nn.ModuleList(fl)
        self.flood_out = Dense(N, 'sigmoid', in_features=fi, generator=gen, precision=pr) if self.if_flood else None      # :327-330
        self.e_out_layer = Dense(self.e_out * E, 'tanh', in_features=d, generator=gen, precision=pr)          # :335-337

    @property
    def snapshot_remainder(self):
        """True: the SpatialLayers of both blocks compute the dense remainder of a trained NodeEdge bias with the one-launch snapshot
        kernel (SpatialLayer.snapshot_remainder) where the network's shape allows.  Default False: the tiled GEMM path."""
        return self._snapshot_remainder

    @snapshot_remainder.setter
    def snapshot_remainder(self, on):
        self._snapshot_remainder = bool(on)
        for m in self.modules():
            if isinstance(m, SpatialLayer):
                m.snapshot_remainder = self._snapshot_remainder

    @property
    def dense_node_edge_train(self):
        """True: every dense-parameter NodeEdge of the model trains as one autograd Function (NodeEdge.dense_train: the whole
        weight o inci + bias on the split-bf16 GEMM, d bias and d weight from uds_node_edge_wgrad).  Default False: the support
        on the exact-fp32 CSR kernels plus the off-support remainder."""
        return self._dense_node_edge_train

    @dense_node_edge_train.setter
    def dense_node_edge_train(self, on):
        self._dense_node_edge_train = bool(on)
        for m in self.modules():
            if isinstance(m, NodeEdge):
                m.dense_train = self._dense_node_edge_train

    @property
    def fused_gat_backward(self):
        """True: every single-head GATConv of the model -- both spatial blocks and the graph_base block -- takes its backward from
        one uds_gat_backward_act call (GATConv.fused_backward: activation, attention / aggregation, bias and attention-kernel
        gradients in three launches).  Default False: the chain of separate steps.  The forward pass is the same."""
        return self._fused_gat_backward

    @fused_gat_backward.setter
    def fused_gat_backward(self, on):
        self._fused_gat_backward = bool(on)
        for m in self.modules():
            if isinstance(m, GATConv):
                m.fused_backward = self._fused_gat_backward

    @property
    def graphed_fit(self):
        """True: `fit_eval` replays ONE captured HIP graph per step (forward, tail, backward and `HipKerasAdam` for fit=True;
        forward and tail for fit=False) where `fit_graph_refusal()` allows, and runs the eager step with the same
        `HipKerasAdam` where it does not.  Default False: the eager step with `KerasAdam`.  Switching converts an existing
        optimizer through its `state_dict`; switching off frees the graphs."""
        return self._graphed_fit

    @graphed_fit.setter
    def graphed_fit(self, on):
        on = bool(on)
        want = HipKerasAdam if on else KerasAdam
        if self._optimizer is not None and on != self._graphed_fit and type(self._optimizer) is not want:
            new = want(self._optimizer.params, self.learning_rate, clipnorm=1.0)
            new.load_state_dict(self._optimizer.state_dict())
            self._optimizer = new
        if not on:
            self.drop_fit_graphs()
        self._graphed_fit = on

    # ------------------------------------------------------------------ the non-graph baseline (conv False)
    def _build_mlp(self, d, h, H, L, a, gen, pr):
        """`build_network(conv=False)` (emulator.py:166-341 with `net = Dense`): every time step's node states (N * n_in values) and link
        states (E * e_in) are ONE row each; embeddings, `Dense(2 d)(concat([x, e]))` + split in place of the spatial layers, the same
        temporal nets / resnet head, and heads that emit all N (E) outputs of a step at once.  Same Dense / Conv1D / recurrent /
        cumsum kernels as the graph model, on (B, T, 1, F) rows."""
        if self.seq_in != self.seq_out:
            raise NotImplementedError('conv=False reshapes the boundary input with seq_in (emulator.py:202): it only runs with seq_in == seq_out')
        N, E = self.n_node, self.n_edge
        self.embed_x = Dense(d, 'linear', in_features=N * self.n_in, generator=gen)             # :197-198
        self.embed_b = Dense(h, a, in_features=N * self.b_in, generator=gen)                    # :202-203
        self.embed_e = Dense(d, 'linear', in_features=E * self.e_in, generator=gen)             # :205-206
        self.embed_ae = Dense(h, a, in_features=E, generator=gen) if self.act else None         # :211-212
        self.block1 = nn.ModuleList([Dense(2 * d, a, in_features=2 * d, generator=gen, precision=pr) for _ in range(L)])          # :236-237
        self.tem1_x, self.tem1_e = self._tem_net(d, H, gen, pr), self._tem_net(d, H, gen, pr)
        f2 = (H + h) + (H + (h if self.act else 0))
        self.block2 = nn.ModuleList([Dense(2 * d, a, in_features=(f2 if i == 0 else 2 * d), generator=gen, precision=pr) for i in range(L)])
        self.tem2_x, self.tem2_e = self._tem_net(d, H, gen, pr), self._tem_net(d, H, gen, pr)
        self._build_heads(d, h, H, a, gen, pr, N, E)

    def _forward_mlp(self, X, B, E, AE, drop):
        T = self.seq_out
        dr = (lambda t: self._drop(t, True)) if drop else (lambda t: t)
        flat = lambda t: t.reshape(t.shape[0], t.shape[1], 1, -1).contiguous()        # (B, T, N, c) -> one row of N * c per step
        x, e, b, ae, x_lin_last, e_lin_last = self._embed(X, B, E, AE, drop, flat)

        def spatial(layers, x, e):
            for ly in layers:
                z = ly(torch.cat([x, e], dim=-1))
                x, e = dr(z[..., :z.shape[-1] // 2].contiguous()), dr(z[..., z.shape[-1] // 2:].contiguous())
            return x, e

        x, e = spatial(self.block1, x, e)
        x, e = self._temporal(self.tem1_x, self.tem1_e, x, e, mlp=True)
        x = torch.cat([x[:, -T:], b], dim=-1)                                         # :260
        e = torch.cat([e[:, -T:], ae], dim=-1) if self.act else e[:, -T:]             # :262
        x, e = spatial(self.block2, x, e)
        x, e = self._temporal(self.tem2_x, self.tem2_e, x, e, mlp=True)
        pgrad = _ag.grad_on(*self.parameters())
        return (self._output(x, x_lin_last, self.res_x, self.out, list(self.flood), self.flood_out, drop, pgrad, self.n_node),     # :313-333
                self._output(e, e_lin_last, self.res_e, self.e_out_layer, [], None, drop, pgrad, self.n_edge))                     # :317-337

    # ------------------------------------------------------------------ network forward (build_network)
    def attention_coefficients(self, X, B, E, AE=None, ADJ=None):
        """What the GATConv layers attend to: inputs as `forward` takes them, run without autograd and without dropout.  Returns
        {'block1': [...], 'block2': [...]} with one (alpha_x, alpha_e) pair per spatial layer -- (B, T, H, nnz of the node
        adjacency) and (B, T, H, nnz of the link adjacency), in the entry order of `self.graph.adj` / `self.graph.edge_adj`
        (T = seq_in in block 1, seq_out in block 2) -- or, for `graph_base`, one (B, T, H, nnz) tensor per layer.  The softmax
        coefficients themselves (Spektral's return_attn_coef); works for single-head models too.  The layers run the unfused
        chain (uds_gat_aggregate_heads): the fused kernels never hold the coefficients."""
        if not self.conv or self.conv_kind != 'GAT':
            raise NotImplementedError('attention coefficients exist for conv=GAT models')
        self._attn_sink = sink = {}
        try:
            with torch.no_grad():
                self.forward(X, B, E, AE, ADJ, training=False)
        finally:
            self._attn_sink = None
        return sink

    def forward(self, X, B, E, AE=None, ADJ=None, training=False):
        """ADJ: the per-time-step node adjacency of `use_adj` (emulator.py:178-180,268-271; block 2 only): the edge mask
        (B, T_out, nnz) of `get_adj_action`, or the reference's dense (B, T_out, n, n) integer array (small networks).
        training: keras' `training=` flag -- switches the Dropout layers on when the model was built with `dropout` > 0."""
        drop = bool(self.dropout) and training
        self.last_temporal_route, self.last_head_route = [], []
        self.last_prefix_batch = X.shape[0]
        if not self.conv:
            return self._forward_mlp(X, B, E, AE, drop)
        adj_mask = self._adj_mask(ADJ, X.shape[0], X.device)
        # the four embeddings first, in the reference's order (the dropout masks are drawn in it); then the two halves
        x, e, b, ae, x_lin_last, e_lin_last = self._embed(X, B, E, AE, drop, lambda t: t.contiguous())
        history = self._history_stage(x, e, x_lin_last, e_lin_last, drop)
        return self._decode_stage(history, b, ae, adj_mask, drop)

    model = forward

    # ------------------------------------------------------------------ the two halves of the graph model's forward
    last_prefix_batch = None   # after a forward / predict_tf_shared: the batch the history half ran at (1 when a population shared it);
    #                            after `mpc.Problem.predict`: that of the horizon's first chunk

    def _adj_mask(self, ADJ, nb, device):
        if ADJ is None:
            return None
        if not (self.act and self.use_adj):
            raise ValueError('ADJ given but the model was built without act + use_adj')
        return self._adj_mask_from(ADJ, device).reshape(nb * self.seq_out, -1)

    def _spatial(self, block, x, e, xb=None, eb=None, mask=None, drop=False):
        """One spatial block on (nb, T, N, f) / (nb, T, E, f) rows; xb / eb: the second piece of the first layer's input."""
        nb, T = x.shape[:2]
        r = lambda t, n: None if t is None else t.reshape(nb * T, n, -1)
        kw = {} if mask is None else {'adj_mask': mask}
        if drop:
            kw['dropout'] = lambda t: self._drop(t, True)
            if self.conv_kind == 'GAT':      # training=True reaches the GATConv layers too: Spektral's attention dropout (rate 0.5)
                kw['attn_dropout'] = self.dropout_stream
        sink = getattr(self, '_attn_sink', None)
        if sink is not None:                 # attention_coefficients(): the layers run unfused and hand their coefficients out
            kw['attn_out'] = got = []
        xs, es = block(r(x, self.n_node), r(e, self.n_edge), r(xb, self.n_node), r(eb, self.n_edge), **kw)
        if sink is not None:
            bt = lambda t: t.reshape((nb, T) + t.shape[-2:])
            sink['block1' if block is self.block1 else 'block2'] = [bt(a) if isinstance(a, torch.Tensor) else (bt(a[0]), bt(a[1])) for a in got]
        return xs.reshape(nb, T, self.n_node, -1), es.reshape(nb, T, self.n_edge, -1)

    def _history_stage(self, x, e, x_lin_last, e_lin_last, drop):
        """Block 1 and the first temporal stage on the embedded history (:236-257) -> `History`: all a forward keeps of X and E."""
        x, e = self._spatial(self.block1, x, e, drop=drop)
        x, e = self._temporal(self.tem1_x, self.tem1_e, x, e)
        return History(x[:, -self.seq_out:], e[:, -self.seq_out:], x_lin_last, e_lin_last)             # :249,256

    def _decode_stage(self, history, b, ae, adj_mask, drop):
        """Block 2, the second temporal stage and the output stage (:260-337) on a `History` and the embedded B / AE."""
        # concat([x, b]) / concat([e, ae]) (:260-262) are not materialised: the first layer of block 2 reads both pieces
        x, e = self._spatial(self.block2, history.x.contiguous(), history.e.contiguous(), b, ae if self.act else None, adj_mask, drop)
        x, e = self._temporal(self.tem2_x, self.tem2_e, x, e)
        pgrad = _ag.grad_on(*self.parameters())
        return (self._output(x, history.x_lin_last, self.res_x, self.out, list(self.flood), self.flood_out, drop, pgrad),     # :313-333
                self._output(e, history.e_lin_last, self.res_e, self.e_out_layer, [], None, drop, pgrad))                     # :317-337

    def encode_history(self, X, E):
        """The half of `forward` that reads only the history: normalised X (B, seq_in, N, c), E (B, seq_in, E, c) -> `History`
        (x, e after the first temporal stage, cut to seq_out steps, and the last linear step of both embeddings).  Inference only
        (no dropout).  `decode` is the other half; forward(X, B, E, AE, ADJ) computes decode(encode_history(X, E), B, AE, ADJ)
        with the same kernels."""
        if not self.conv:
            raise NotImplementedError('encode_history / decode split the graph model; conv=False runs `forward`')
        self.last_temporal_route, self.last_head_route = [], []
        self.last_prefix_batch = X.shape[0]
        c = lambda t: t.contiguous()
        x_lin_last = self.embed_x(c(X[:, -1:]), 'linear')           # as `_embed`: the linear last step, then the activated embedding
        x = self.embed_x(c(X), self.activation)
        e_lin_last = self.embed_e(c(E[:, -1:]), 'linear')
        e = self.embed_e(c(E), self.activation)
        return self._history_stage(x, e, x_lin_last, e_lin_last, False)

    def decode(self, history, B, AE=None, ADJ=None, pop=None):
        """The half of `forward` after the history: embed_b, embed_ae, block 2, the second temporal stage, the output stage.
        pop: `history` and B have batch 1 and are shared by a population whose AE / ADJ have batch pop: the boundary embedding
        runs once, and the shared tensors are expanded to pop rows just before block 2 (one copy, the bytes block 2 reads)."""
        if not self.conv:
            raise NotImplementedError('encode_history / decode split the graph model; conv=False runs `forward`')
        c = lambda t: t.contiguous()
        b = self.embed_b(c(B))
        ae = self.embed_ae(c(AE)) if self.act else None
        nb = history.x.shape[0]
        if pop is not None:
            if nb != 1 or b.shape[0] != 1 or (ae is not None and ae.shape[0] != pop):
                raise ValueError('decode(pop=%d): the history and B must have batch 1 and AE batch pop' % pop)
            rows = lambda t: t.expand((pop,) + tuple(t.shape[1:])).contiguous()
            history, b, nb = History(*(rows(t) for t in history)), rows(b), pop
        return self._decode_stage(history, b, ae, self._adj_mask(ADJ, nb, history.x.device), False)

    def _embed(self, X, B, E, AE, drop, prep):
        """The four embeddings (:197-212) -> x, e, b, ae and the last linear step of x and e (the resnet residual).  prep: what
        makes a Dense input of a tensor (contiguous; the MLP model flattens a step into one row)."""
        if drop:      # Dense(linear) -> Dropout(0.2) -> residual slice -> activation (:198-201,206-209); masks drawn in the reference's order x, b, e, ae
            xl = self._drop02(self.embed_x(prep(X), 'linear'), True)
            b = self._drop02(self.embed_b(prep(B)), True)
            el = self._drop02(self.embed_e(prep(E), 'linear'), True)
            ae = self._drop02(self.embed_ae(prep(AE)), True) if self.act else None
            x_lin_last, e_lin_last = xl[:, -1:].contiguous(), el[:, -1:].contiguous()
            return _ag.apply_activation(xl, self.activation), _ag.apply_activation(el, self.activation), b, ae, x_lin_last, e_lin_last
        # the embedding is linear, its last step is kept as the residual, then the activation is applied (:198-201):
        # two launches of the same GEMM (same per-row arithmetic), one with and one without the activation
        x_lin_last = self.embed_x(prep(X[:, -1:]), 'linear')
        x = self.embed_x(prep(X), self.activation)
        e_lin_last = self.embed_e(prep(E[:, -1:]), 'linear')
        e = self.embed_e(prep(E), self.activation)
        return x, e, self.embed_b(prep(B)), self.embed_ae(prep(AE)) if self.act else None, x_lin_last, e_lin_last

    # ------------------------------------------------------------------ the temporal stage: route, then one method per route
    fused_temporal = False     # True: a side's Conv1D stack goes out as ONE uds_conv_stack_forward launch where `temporal_route` says 'stack'
    STACK_MIN_STREAMS = 256    # (batch element, 16-row block) streams below which the layers stay (they leave k_conv3_stream there too)
    last_temporal_route = None  # after a forward: [stage 1, stage 2], each what `temporal_route` returned
    last_temporal_path = None  # ... and its summary: 'stack' (a side took the one-launch kernel) or 'layers'
    TEMPORAL_ROUTES = {'stack': '_tem_stack', 'pair': '_tem_pair', 'layers': '_tem_layers'}

    @staticmethod
    def temporal_layer(m):
        """What `temporal_route` reads of one temporal layer."""
        if isinstance(m, Conv1D):
            return TemporalLayer(True, tuple(m.kernel.shape), m.dilation_rate, m.activation, m.precision, m.filters)
        return TemporalLayer(False, None, None, None, m.precision, m.units)

    def temporal_route(self, B, T, N, E, fx, fe, layers_x, layers_e, rowgemm_supported, grad_x=(), grad_e=(), mlp=False):
        """Which kernels the two stacks of one temporal stage (:244-257) run -> ('sides', (key of the node stack, key of the link
        stack)) or ('pairs', (one key per layer index)), keys of TEMPORAL_ROUTES.  Plain values in, no tensor, no launch, no side
        effect: the stacks read (B, T, N, fx) and (B, T, E, fe); layers_x / layers_e: one `TemporalLayer` per layer;
        rowgemm_supported: `_lib.rowgemm_supported`; grad_x / grad_e: whether autograd records for the stack input ([0]) and for a
        parameter of layer i ([i + 1]) -- "grad" at a layer is any of these up to its own.  First match wins:

          0   the MLP model (conv False: one row per step)                                         sides: layers, layers
          1   per side: fused_temporal, 2 or 3 layers, all Conv1D with kernel (3, 64, 64) on a 64-wide input, dilation 2**i at
              layer i, one activation, all bf16x3, B * ceil(rows / 16) >= STACK_MIN_STREAMS, no grad at any layer
                                                                                                   sides: stack there
          2   a side of row 1 next to one that is not                                              sides: layers on the other
          3   stacks of different lengths                                                          sides: layers, layers
          4   per layer index: both Conv1D of one kernel shape (k0, k1, k2), dilation and activation, both bf16x3, both inputs
              k1 wide, rowgemm_supported(k0 * k1, k1, k2), B * T * max(N, E) <= 16384, k0 * k1 // 32 in (2, 6), no grad at
              this layer on either side                                                            pairs: pair at that index
          5   every other layer index                                                              pairs: layers

        'stack' is uds_conv_stack_forward and 'pair' uds_rowgemm_forward_pair: each gives the bits of the layers it replaces."""
        if mlp:
            return 'sides', ('layers', 'layers')

        def stack(rows, f, layers, grad):
            return (self.fused_temporal and len(layers) in (2, 3) and f == 64 and all(ly.conv1d for ly in layers) and
                    all(ly.kernel == (3, 64, 64) and ly.dilation == 2 ** i and ly.activation == layers[0].activation and
                        ly.precision == 'bf16x3' for i, ly in enumerate(layers)) and
                    B * ((rows + 15) // 16) >= self.STACK_MIN_STREAMS and not any(grad))
        sides = tuple('stack' if stack(*side) else 'layers' for side in ((N, fx, layers_x, grad_x), (E, fe, layers_e, grad_e)))
        if 'stack' in sides or len(layers_x) != len(layers_e):
            return 'sides', sides
        keys = []
        for i, (lx, le) in enumerate(zip(layers_x, layers_e)):
            k = lx.kernel
            pair = (lx.conv1d and le.conv1d and le.kernel == k and lx.dilation == le.dilation and lx.activation == le.activation and
                    lx.precision == le.precision == 'bf16x3' and fx == fe == k[1] and rowgemm_supported(k[0] * k[1], k[1], k[2]) and
                    B * T * max(N, E) <= 16384 and k[0] * k[1] // 32 in (2, 6) and not any(grad_x[:i + 2]) and not any(grad_e[:i + 2]))
            keys.append('pair' if pair else 'layers')
            fx, fe = lx.out, le.out
        return 'pairs', tuple(keys)

    def _temporal(self, mods_x, mods_e, x, e, mlp=False):
        """One temporal stage: asks `temporal_route` once, runs what it says and records it."""
        grads = lambda t, mods: (_ag.grad_on(t),) + tuple(_ag.grad_on(*m.parameters()) for m in mods)
        route = form, keys = self.temporal_route(
            x.shape[0], x.shape[1], x.shape[2], e.shape[2], x.shape[-1], e.shape[-1], [self.temporal_layer(m) for m in mods_x],
            [self.temporal_layer(m) for m in mods_e], _lib.rowgemm_supported, grads(x, mods_x), grads(e, mods_e), mlp)
        self.last_temporal_route.append(route)
        self.last_temporal_path = 'stack' if any('stack' in k for _, k in self.last_temporal_route) else 'layers'
        if form == 'sides':
            return getattr(self, self.TEMPORAL_ROUTES[keys[0]])(mods_x, x), getattr(self, self.TEMPORAL_ROUTES[keys[1]])(mods_e, e)
        for key, lx, le in zip(keys, mods_x, mods_e):
            x, e = self._tem_pair(lx, le, x, e) if key == 'pair' else (self._tem_layers([lx], x), self._tem_layers([le], e))
        return x, e

    def _tem_layers(self, mods, t):
        for ly in mods:
            t = ly(t)
        return t

    def _tem_stack(self, mods, t):
        """One side's stack as ONE launch: the layers in between never reach memory."""
        return _lib.conv_stack_forward(t.contiguous(), [(_packed_kernel(m, m.kernel.reshape(192, 64)), m.bias) for m in mods], mods[0].activation)

    def _tem_pair(self, lx, le, x, e):
        """Two small Conv1D layers of one shape, one per side, as ONE launch."""
        k0, k1, k2 = lx.kernel.shape
        return _lib.rowgemm_forward_pair(x.contiguous(), _packed_kernel(lx, lx.kernel.reshape(k0 * k1, k2)), lx.bias,
                                         e.contiguous(), _packed_kernel(le, le.kernel.reshape(k0 * k1, k2)), le.bias, k2,
                                         lx.activation, taps=k0, dilation=lx.dilation_rate)

    # ------------------------------------------------------------------ the output stage: route, then one method per route
    last_head_route = None     # after a forward: [node side, link side], each a key of HEAD_ROUTES
    HEAD_ROUTES = {'heads': '_head_fused', 'dropout': '_head_dropout', 'plain': '_head_plain', 'dense-cumsum': '_head_dense_cumsum',
                   'cumsum': '_head_cumsum'}

    def head_route(self, B, rows, res, head_units, hidden, drop=False, grad_any=False, grad_own=False, mlp=False):
        """Which kernels one side of the output stage (:313-337) runs -> a key of HEAD_ROUTES.  Plain values in, no tensor, no
        launch, no side effect: the side reads (B, T, rows, F); res: (precision, units, F) of its res layer; head_units: units of
        its first head; hidden: [(units, input width)] of the layers between the res layer and its second head (the flood chain; none
        on the link side); drop: dropout is active; grad_any: autograd records for the input, the residual or ANY parameter of the
        model; grad_own: ... for the input, the residual or a parameter of the res layer.  First match wins:

          1   resnet, res = (bf16x3, 64, 64), head_units <= 4, at most 5 hidden layers, all 32 units, the first 64 wide,
              no dropout, no grad_any, not the MLP model                                           heads
          2   dropout active: the layer, Dropout, CumsumActFn if resnet                           dropout
          3   not resnet: the layer                                                                plain
          4   res = (bf16x3, 64, 64), B * rows >= 4096, no grad_own, not the MLP model             dense-cumsum
          5   the layer, then CumsumActFn under grad, else uds_cumsum_act                          cumsum

        'heads' (uds_dense_cumsum_heads) also runs the side's heads; after every other route they are launches of their own.
        The MLP model (one row per step, heads that emit all N or E outputs of a step) never takes 1 or 4."""
        wide = tuple(res) == ('bf16x3', 64, 64)
        if (not mlp and self.resnet and wide and head_units <= 4 and len(hidden) <= 5 and all(u == 32 for u, _ in hidden) and
                (not hidden or hidden[0][1] == 64) and not drop and not grad_any):
            return 'heads'
        if drop:
            return 'dropout'
        if not self.resnet:
            return 'plain'
        if not mlp and wide and B * rows >= 4096 and not grad_own:
            return 'dense-cumsum'
        return 'cumsum'

    def _output(self, t, lin_last, res, head, hidden, head_f, drop, pgrad, rows=None):
        """One side of the output stage: asks `head_route` once, runs what it says and records it.  hidden, head_f: the flood
        chain and its head ([] and None on the link side); pgrad: a parameter of the model needs a gradient; rows: N or E for the MLP
        model, whose heads emit (B, T, 1, rows * c)."""
        key = self.head_route(t.shape[0], t.shape[2], (res.precision, res.units, t.shape[-1]), head.units,
                              [(m.units, m.kernel.shape[0]) for m in hidden], drop, pgrad or _ag.grad_on(t, lin_last),
                              _ag.grad_on(t, lin_last, res.kernel, res.bias), rows is not None)
        self.last_head_route.append(key)
        run = getattr(self, self.HEAD_ROUTES[key])
        if key == 'heads':
            return run(res, t, lin_last, head, hidden, head_f)
        t = run(res, t, lin_last)
        view = (lambda o: o) if rows is None else (lambda o: o.reshape(o.shape[0], o.shape[1], rows, -1))      # :322-325
        out = view(head(t))
        if head_f is not None:
            f = t
            for ly in hidden:
                f = ly(f)
            out = torch.cat([out, view(head_f(f))], dim=-1)           # :330-333
        return out

    def _head_fused(self, res, t, lin_last, head, hidden, head_f):
        """Dense + cumsum + residual + activation with the output heads as the epilogue of the same streaming kernel (the 64-wide
        resnet output never reaches memory)."""
        pk = lambda m: _packed_kernel(m, m.kernel)
        return _lib.dense_cumsum_heads(
            t.contiguous(), pk(res), res.bias, lin_last.contiguous(), self.activation, (pk(head), head.bias, head.units, head.activation),
            [(pk(m), m.bias) for m in hidden], (pk(head_f), head_f.bias, head_f.activation, hidden[0].activation) if hidden else None)

    def _head_dropout(self, res, t, lin_last):
        y = self._drop(res(t), True)
        return _ag.CumsumActFn.apply(y, lin_last, self.activation) if self.resnet else y

    def _head_plain(self, res, t, lin_last):
        return res(t)

    def _head_dense_cumsum(self, res, t, lin_last):
        """Dense + cumsum over time + residual + activation in one streaming kernel."""
        return _lib.dense_cumsum(t.contiguous(), _packed_kernel(res, res.kernel), res.bias, lin_last.contiguous(), self.activation)

    def _head_cumsum(self, res, t, lin_last):
        y = res(t)
        if _ag.grad_on(y, lin_last):
            return _ag.CumsumActFn.apply(y, lin_last, self.activation)
        return _lib.cumsum_act(y.contiguous(), lin_last.contiguous(), self.activation)

    # ------------------------------------------------------------------ normalisation (:794-810)
    def set_norm(self, norm_x, norm_b, norm_y, norm_r, norm_e):
        for k, v in (('x', norm_x), ('b', norm_b), ('y', norm_y), ('r', norm_r), ('e', norm_e)):
            if v is not None:
                self._norms[k] = torch.as_tensor(np.asarray(v), dtype=torch.float32)

    def _norm(self, item, device):
        t = self._norms[item]
        if t.device != device:
            t = self._norms[item] = t.to(device)
        return t

    def _norm_parts(self, item, dim, device):
        """(maxi - mini, mini) of the first `dim` channels, computed once per norm tensor (the rollout calls normalize a dozen
        times per step on constants)."""
        normal = self._norm(item, device)
        key = (item, dim, str(device))
        hit = self._norm_derived.get(key)
        if hit is None or hit[0] is not normal:
            maxi, mini = normal[0, ..., :dim], normal[1, ..., :dim]
            hit = self._norm_derived[key] = (normal, (maxi - mini).contiguous(), mini.contiguous())
        return hit[1], hit[2]

    def normalize(self, dat, item, inverse=False):
        span, mini = self._norm_parts(item, dat.shape[-1], dat.device)
        return dat * span + mini if inverse else (dat - mini) / span

    # ------------------------------------------------------------------ actions (:364-398)
    def _act_edge_index(self):
        hits = [np.where((self.edges == ae).all(1))[0] for ae in self.act_edges]
        flat = [int(i) for e in hits for i in e]
        return sorted(set(flat), key=flat.index)

    def _dev_index(self, name, arr, device):
        """An int64 index list on the device, uploaded once."""
        key = (name, str(device))
        if key not in self._idx_cache:
            self._idx_cache[key] = torch.as_tensor(arr, dtype=torch.int64, device=device)
        return self._idx_cache[key]

    def get_edge_action(self, a, g=True):
        out = np.zeros(self.n_edge, dtype=np.int64)
        out[self._act_edge_index()] = np.arange(1, a.shape[-1] + 1)
        table = torch.cat([torch.ones_like(a[..., :1]), a], dim=-1)
        return table[..., self._dev_index('edge_action', out, a.device)].unsqueeze(-1)

    def _adj_pattern(self):
        """(CSR of the adjacency the node-side conv of block 2 runs on, raw values at its entries, entry position of every
        actuated (from, to) pair or -1).  Two-graph form: the node adjacency; graph_base: the combined node + link graph."""
        if getattr(self, '_adj_pat', None) is None:
            csr = self._base_filter if self.graph_base else self.graph.adj
            raw = np.ones(csr.nnz) if getattr(self, '_adj_raw', None) is None else self._adj_raw
            rp, col = np.asarray(csr.rowptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)
            pos = np.full(len(self.act_edges), -1, dtype=np.int64)
            for k, (u, v) in enumerate(np.asarray(self.act_edges, dtype=np.int64)):
                hit = np.nonzero(col[rp[u]:rp[u + 1]] == v)[0]
                if len(hit):
                    pos[k] = rp[u] + hit[0]
            self._adj_pat = (csr, raw, pos)
        return self._adj_pat

    def get_adj_action(self, a, g=True):
        """`get_adj_action` (emulator.py:343-362) for conv=GAT, in CSR form: a (B, T, n_act) settings -> edge mask
        (B, T, nnz) over the entries of the node adjacency.  The reference writes `adj[from_k, to_k] = a_k` (g=False) or
        multiplies that entry by a_k (g=True) -- the (from, to) entry only, not its transpose -- and casts the matrix to int:
        an entry survives iff trunc(value) != 0, so with a 0/1 adjacency any setting below 1 removes it."""
        csr, raw, pos = self._adj_pattern()
        dev = a.device
        ok = pos >= 0
        key = ('adj_action', str(dev), a.dtype)
        hit = self._idx_cache.get(key)               # constants of the model, uploaded once (a captured step cannot upload)
        if hit is None:
            hit = self._idx_cache[key] = (torch.as_tensor(np.trunc(raw) != 0, dtype=torch.float32, device=dev),
                                          torch.as_tensor(raw[pos[ok]], dtype=a.dtype, device=dev),
                                          torch.as_tensor(np.nonzero(ok)[0], device=dev), torch.as_tensor(pos[ok], device=dev))
        base, raw_w, src, dst = hit
        mask = base.expand(tuple(a.shape[:-1]) + (csr.nnz,)).clone()
        if ok.any():
            w = raw_w if g else torch.ones(int(ok.sum()), dtype=a.dtype, device=dev)
            val = a[..., src] * w
            mask[..., dst] = (torch.trunc(val) != 0).to(torch.float32)
        return mask

    def _adj_mask_from(self, adj, device):
        """Edge mask from what `forward` is given: the mask itself (..., nnz) or the reference's dense (..., n, n) adjacency."""
        csr, _, _ = self._adj_pattern()
        adj = torch.as_tensor(adj) if not isinstance(adj, torch.Tensor) else adj
        n = csr.n_rows
        if adj.dim() >= 2 and tuple(adj.shape[-2:]) == (n, n) and adj.shape[-1] != csr.nnz:
            rows = torch.as_tensor(np.repeat(np.arange(n), np.diff(csr.rowptr)), device=adj.device)
            cols = torch.as_tensor(np.asarray(csr.col, dtype=np.int64), device=adj.device)
            adj = (torch.trunc(adj[..., rows, cols].to(torch.float32)) != 0)
        elif adj.shape[-1] != csr.nnz:
            raise ValueError('ADJ %r is neither an edge mask (..., %d) nor a dense (..., %d, %d) adjacency' % (tuple(adj.shape), csr.nnz, n, n))
        return adj.to(device=device, dtype=torch.float32)

    def get_action(self, a, g=True):
        out_o, out_i = np.zeros(self.n_node, dtype=np.int64), np.zeros(self.n_node, dtype=np.int64)
        out_o[self.act_edges[:, 0]] = np.arange(1, a.shape[-1] + 1)
        out_i[self.act_edges[:, 1]] = np.arange(1, a.shape[-1] + 1)
        table = torch.cat([torch.ones_like(a[..., :1]), a], dim=-1)
        return table[..., self._dev_index('act_out', out_o, a.device)], table[..., self._dev_index('act_in', out_i, a.device)]

    # ------------------------------------------------------------------ post-processing (:680-770)
    def _from_node_index(self, device):
        """(idx (E,) int64, ok (E,) float): the node whose incidence entry of link e is positive -- its from-node -- read off the
        signed incidence CSR (`get_node_edge`, base.py:432-439: +1 at the from-node, then -1 at the to-node; a link from a node to
        itself therefore has no positive entry: ok = 0, as in the dense `clip(node_edge, 0, 1)`)."""
        key = ('from_node', str(device))
        if key not in self._idx_cache:
            ie = self.graph.inc_e
            rows, cols, vals = ie.rows(), np.asarray(ie.col, dtype=np.int64), np.asarray(ie.val)
            idx, ok = np.zeros(self.n_edge, dtype=np.int64), np.zeros(self.n_edge, dtype=np.float32)
            pos = vals > 0
            idx[rows[pos]], ok[rows[pos]] = cols[pos], 1.0
            self._idx_cache[key] = (torch.as_tensor(idx, device=device), torch.as_tensor(ok, device=device))
        return self._idx_cache[key]

    def _at_from_node(self, v):
        """v (..., N) -> (..., E): v @ clip(node_edge, 0, 1) without the dense matrix."""
        idx, ok = self._from_node_index(v.device)
        return v[..., idx] * ok

    def _flow_balance(self, flow):
        """q_in, q_out (B,T,N,1) from de-normalised link flows (B,T,E,1): HIP kernel on the incidence CSR."""
        if self._inc_handle is None:
            self._inc_handle = _lib.CsrHandle(self.graph.inc_n)
        ny = self._norm('y', flow.device)
        hit = self._norm_derived.get(('flow_scale', str(flow.device)))
        if hit is None or hit[0] is not ny:
            hit = self._norm_derived[('flow_scale', str(flow.device))] = (
                ny, ((ny[0, :, 1] > 1e-3).float() / ny[0, :, 1]).contiguous(), ((ny[0, :, 2] > 1e-3).float() / ny[0, :, 2]).contiguous())
        s_in, s_out = hit[1], hit[2]
        lead = flow.shape[:-2]
        if _ag.grad_on(flow):
            edges = self._dev_index('edges', self.edges, flow.device)
            q_in, q_out = _ag.FlowBalanceFn.apply(flow.reshape(-1, self.n_edge), self._inc_handle, self._inc_sign, s_in, s_out, edges)
        else:
            q_in, q_out = _lib.flow_balance(self._inc_handle, self._inc_sign, flow.reshape(-1, self.n_edge).contiguous(), s_in, s_out)
        return q_in.reshape(lead + (self.n_node, 1)), q_out.reshape(lead + (self.n_node, 1))

    def post_proc_tf(self, preds, a, b):
        """`post_proc_tf` (emulator.py:680-725): the graph-mode post-processing used by `predict_tf`, `_model`, MPC and MBRL."""
        return self._post_proc(preds, a, b, False)

    def post_proc(self, y, ey, a, b):
        """`post_proc` (emulator.py:643-678): the NumPy twin used by `predict` and `simulate`.  NOT equivalent to
        `post_proc_tf` where pumps are involved: the rated-pump override of the link flow is applied whenever the model has
        actions (the graph-mode form only when EVERY link is a pump, `self.pump.min() > 0`, :698), and the node pumps of the
        non-edge-fusion form open at depth > 0.01 instead of > 0 (:664-665 vs :710-711).  The offset gate is written without
        its `offset.max() > 0` guard (:649-653 vs :688), which changes nothing: with no offsets the expression is the flow."""
        return self._post_proc((y, ey), a, b, True)

    def _post_proc(self, preds, a, b, np_form):
        preds, edge_preds = preds
        pump_override = self._has_link_pump if np_form else self._has_pump      # :656-659 (always with actions) vs :698 (`pump.min() > 0`)
        depth_gate = 0.01 if np_form else 0.0                                      # :664-665 vs :710-711
        # `v @ clip(node_edge, 0, 1)` (:649,657,689,699): node_edge has one +1 per link, at its from-node (base.py:432-439), so the
        # dense (N, E) product is a gather of v at the from-nodes -- the same numbers from the incidence CSR, for any N
        if self.tide:
            h = preds[..., 0] * (1 - self.is_outfall) + b[..., -1]
            preds = torch.cat([h.unsqueeze(-1), preds[..., 1:]], dim=-1)
        if self._has_offset:
            inoff = self._at_from_node(self.normalize(preds, 'y', True)[..., 0] - self.hmin)
            flow, off = edge_preds[..., -1], self.offset
            flow = (flow * (flow > 0).float() * (off > 0).float() * (inoff > off).float() + flow * (flow <= 0).float() * (off > 0).float() +
                    flow * (off == 0).float()).unsqueeze(-1)
            edge_preds = torch.cat([edge_preds[..., :-1], flow], dim=-1)
        if self.act:
            ne_ = self._norm('e', preds.device)
            if pump_override:
                fl = self.pump * self._at_from_node((preds[..., 0] > 0.01).float())
                fl = fl * (ne_[0, :, 2] > 1e-3).float() / ne_[0, :, 2]
                flow = (edge_preds[..., -1] * (fl == 0).float() + fl).unsqueeze(-1)
            else:
                flow = edge_preds[..., -1:]
            edge_preds = torch.cat([edge_preds[..., :-1], flow * self.get_edge_action(a, True)], dim=-1)
            if not self.edge_fusion:
                ny = self._norm('y', preds.device)
                a_out, a_in = self.get_action(a[:, :self.seq_out], True)
                fli = self.pump_in * (preds[..., 0] > depth_gate).float() / ny[0, :, 1]
                flo = self.pump_out * (preds[..., 0] > depth_gate).float() / ny[0, :, 2]
                inflow = preds[..., 1] * (fli == 0).float() + fli
                outflow = preds[..., 2] * (flo == 0).float() + flo
                preds = torch.cat([torch.stack([preds[..., 0], inflow * a_in, outflow * a_out], dim=-1), preds[..., 3:]], dim=-1)
        if self.edge_fusion:
            span, mini = self._norm_parts('e', edge_preds.shape[-1], edge_preds.device)
            flow = edge_preds[..., -1:] * span[..., -1:] + mini[..., -1:]        # de-normalised flow channel only
            q_in, q_out = self._flow_balance(flow)
            preds = torch.cat([preds[..., :1], q_in, q_out, preds[..., 1:]], dim=-1)
        return preds, edge_preds

    def constrain_tf(self, y, r, h0=None):
        h, q_us, q_ds = y[..., 0], y[..., 1], y[..., 2]
        r = r.squeeze(-1)
        h = torch.minimum(torch.maximum(h, self.hmin), self.hmax)
        q_w = (q_us + r - q_ds).clamp(min=0) * (1 - self.is_outfall)
        if self.if_flood:
            f = (y[..., -1] > 0.5).float()
            h = self.hmax * f + h * (1 - f)
            y = torch.stack([h, q_us, q_ds, y[..., -1]], dim=-1)
        else:
            y = torch.stack([h, q_us, q_ds], dim=-1)
        if self.epsilon > 0:
            q_w = q_w * ((self.hmax - h) < self.epsilon).float()
        elif self.epsilon == 0:
            pass
        elif self.if_flood:
            q_w = q_w * f
        return q_w, y

    # ------------------------------------------------------------------ inference entry points
    def predict_tf(self, states, b, a=None, edge_state=None):
        """emulator.py:604-641 (graph mode: `post_proc_tf`)."""
        return self._predict(states, b, a, edge_state, False)

    def predict(self, states, b, a=None, edge_state=None):
        """emulator.py:566-602: the NumPy-mode entry point (`post_proc`, see there for how it differs from `predict_tf`);
        tensors stay on the device."""
        return self._predict(states, b, a, edge_state, True)

    def _predict(self, states, b, a, edge_state, np_form):
        x = states[:, -self.seq_in:]
        ex = edge_state[:, -self.seq_in:]
        assert b.shape[1] == self.seq_out
        # NumPy mode writes the setting INTO the adjacency entry (g=False, :572-574), graph mode multiplies the entry by it
        # (g=True, :611-613): the two differ on a weighted adjacency (length > 0), where entry * setting truncates to 0
        ae = self.get_edge_action(a, not np_form) if self.act else None
        adj = self.get_adj_action(a, not np_form) if self.act and self.use_adj else None
        nb_ = self.normalize(b, 'b')
        y, ey = self.forward(self.normalize(x, 'x'), nb_, self.normalize(ex, 'e'), ae, adj)
        return self._predict_tail(y, ey, a, b, nb_, x, np_form)

    def predict_tf_shared(self, state, b, a, edge_state):
        """`predict_tf` for a population that shares its history (the MPC candidates of `mpc.Problem`): state (T_in, N, C),
        b (seq_out, N, cb), edge_state (T_in, E, Ce) unbatched, a (pop, seq_out, n_act) -> what predict_tf returns on the inputs
        replicated pop times, to a tolerance (the history half runs at batch 1 and may take other kernels than at batch pop).
        One normalisation, `encode_history` at batch 1 without autograd (nothing of it depends on a), `decode(..., pop=pop)`,
        the same tail.  Autograd flows to a as in predict_tf; with use_adj the per-candidate mask enters block 2 only."""
        if not self.conv:
            raise NotImplementedError('predict_tf_shared needs a graph model (encode_history / decode); conv=False runs predict_tf')
        pop = a.shape[0]
        assert b.shape[0] == self.seq_out
        x, ex, b1 = state[-self.seq_in:].unsqueeze(0), edge_state[-self.seq_in:].unsqueeze(0), b.unsqueeze(0)
        ae = self.get_edge_action(a, True) if self.act else None
        adj = self.get_adj_action(a, True) if self.act and self.use_adj else None
        nb1 = self.normalize(b1, 'b')
        with torch.no_grad():
            history = self.encode_history(self.normalize(x, 'x'), self.normalize(ex, 'e'))
        y, ey = self.decode(history, nb1, ae, adj, pop=pop)
        rows = lambda t: t.expand((pop,) + tuple(t.shape[1:]))
        return self._predict_tail(y, ey, a, rows(b1), rows(nb1), rows(x), False)

    def _predict_tail(self, y, ey, a, b, nb_, x, np_form):
        """Everything of `_predict` after the forward: the HIP tail where it takes the model, else the tensor code."""
        fused = self._predict_tail_hip(y, ey, a, b, nb_, x, np_form)
        if fused is not None:
            return fused
        self.last_tail_path = 'torch'
        y, ey = self._post_proc((y, ey), a, nb_, np_form)
        ey = self.normalize(ey, 'e', True)
        ey = torch.cat([torch.minimum(ey[..., 0].clamp(min=0), self.ehmax).unsqueeze(-1), ey[..., 1:]], dim=-1)
        y = self.normalize(y, 'y', True)
        if self._has_any_pump:       # pumped-storage depth (:630-638)
            idx, ok = self._from_node_index(y.device)          # clip(node_edge, 0, 1) @ pump: the pumps leaving every node
            ps = ((self.area * torch.zeros_like(self.area).index_add_(0, idx, self.pump * ok)) > 0).float()
            h, qin, qout = y[..., 0], y[..., 1], y[..., 2]
            de = []
            for t in range(self.seq_out):
                prev = x[:, -1, :, 0] if t == 0 else de[-1] + (qin - qout)[:, t] / (self.area + 1e-6)
                de.append(torch.minimum(torch.maximum(prev, self.hmin), self.hmax))
            y = torch.cat([(h * (1 - ps) + torch.stack(de, dim=1) * ps).unsqueeze(-1), y[..., 1:]], dim=-1)
        q_w, y = self.constrain_tf(y, b[..., :1], x[:, -1:, :, 0])
        return torch.cat([y, q_w.unsqueeze(-1)], dim=-1), ey

    # ------------------------------------------------------------------ the predict tail as one HIP operator
    fused_tail = True         # False: `_predict` keeps its tensor code for everything after the forward
    last_tail_path = None      # 'hip', 'hip-train' (through autograd.PredictTailFn) or 'torch' after a predict_tf / predict call

    def _tail_spec(self, device, n_act, b_channels, ce):
        """The `_lib.TailSpec` of this model on `device`: the constants the tensor code of `_post_proc` / `_predict` precomputes,
        computed the same way, plus the index tables; built once and rebuilt when `set_norm` replaces a norm tensor."""
        ny, ne = self._norm('y', device), self._norm('e', device)
        key = ('tail', str(device))
        hit = self._norm_derived.get(key)
        if hit is not None and hit[0] is ny and hit[1] is ne and hit[2] == (n_act, b_channels, ce):
            return hit[3]
        N, E = self.n_node, self.n_edge
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        i32 = lambda arr: torch.as_tensor(np.concatenate([np.asarray(arr, dtype=np.int64).reshape(-1), [0]]), dtype=torch.int32, device=device)
        C = 3 + int(bool(self.if_flood))
        span_y, mini_y = self._norm_parts('y', C, device)
        span_e, mini_e = self._norm_parts('e', ce, device)
        idx, ok = self._from_node_index(device)
        area, pump = f32(self.area), f32(self.pump)
        ne2 = ne[0, :, 2] if ne.shape[-1] > 2 else torch.ones(E, device=device)
        tab = dict(is_outfall=f32(self.is_outfall), hmin=f32(self.hmin), hmax=f32(self.hmax), area_eps=area + 1e-6,
                   ps=((area * torch.zeros_like(area).index_add_(0, idx, pump * ok)) > 0).float(),
                   pump_in=f32(self.pump_in), pump_out=f32(self.pump_out), ny_in=f32(ny[0, :, 1]), ny_out=f32(ny[0, :, 2]),
                   scale_in=f32((ny[0, :, 1] > 1e-3).float() / ny[0, :, 1]), scale_out=f32((ny[0, :, 2] > 1e-3).float() / ny[0, :, 2]),
                   span_y=f32(span_y), mini_y=f32(mini_y), offset=f32(self.offset), pump=pump, pump_mask=f32((ne2 > 1e-3).float()),
                   pump_den=f32(ne2), ehmax=f32(self.ehmax), from_ok=f32(ok), span_e=f32(span_e), mini_e=f32(mini_e))
        # the (up to) two incidence entries of every link, for the backward gather
        inc = self.graph.inc_n
        rows, cols, vals = inc.rows(), np.asarray(inc.col, dtype=np.int64), np.asarray(inc.val, dtype=np.float64)
        link_node, link_sign = np.full((E, 2), -1, dtype=np.int64), np.zeros((E, 2), dtype=np.float32)
        count = np.bincount(cols, minlength=E)
        if len(cols) and count.max() > 2:
            return None                          # a link with more than two incidence entries: not a drainage link
        order = np.argsort(cols, kind='stable')
        slot = np.arange(len(cols)) - (np.cumsum(count) - count)[cols[order]]
        link_node[cols[order], slot], link_sign[cols[order], slot] = rows[order], vals[order]
        tab['link_sign'] = torch.as_tensor(np.concatenate([link_sign.reshape(-1), [0.0]]), dtype=torch.float32, device=device)
        act_link, act_in, act_out = np.zeros(E, dtype=np.int64), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
        if self.act:
            act_link[self._act_edge_index()] = np.arange(1, n_act + 1)
            if not self.edge_fusion:
                act_out[self.act_edges[:, 0]] = np.arange(1, n_act + 1)
                act_in[self.act_edges[:, 1]] = np.arange(1, n_act + 1)

        def lists(table):
            members = [np.nonzero(table == k + 1)[0] for k in range(n_act)]
            return np.concatenate([[0], np.cumsum([len(m) for m in members])]), np.concatenate(members + [np.zeros(0, dtype=np.int64)])
        ints = dict(from_node=i32(idx.cpu().numpy()), act_link=i32(act_link), act_in=i32(act_in), act_out=i32(act_out), link_node=i32(link_node))
        for name, table in (('al', act_link), ('ai', act_in), ('ao', act_out)):
            ptr, members = lists(table)
            ints[name + '_ptr'], ints[name + '_idx'] = i32(ptr), i32(members)
        tab.update(ints)
        spec = _lib.TailSpec(tab, N=N, E=E, cy=C - 2 if self.edge_fusion else C, ce=ce, n_act=n_act, b_channels=b_channels,
                             edge_fusion=self.edge_fusion, tide=self.tide, has_offset=self._has_offset, act=self.act, pump_override=0,
                             any_pump=self._has_any_pump, if_flood=bool(self.if_flood), epsilon=self.epsilon)
        self._norm_derived[key] = (ny, ne, (n_act, b_channels, ce), spec)
        return spec

    def _tail_takes(self, device, B, T, ce, a, n_act):
        """Do the tail kernels (uds_predict_tail, uds_fit_tail) take this model with `ce` link channels, settings `a` of
        (B, T, n_act) and its norms on `device`?  Not a local model of `shard_emulator` (its flows cross the cut between the link
        gates and the balance), 2 to 8 link channels, 'y' / 'e' norms of one row per node / link with the channels the kernels read,
        and for an actuated model fp32 settings on the device of which every one drives its links (and, without edge fusion, its
        two nodes): a fact of the model, looked up once per n_act (`_act_edge_index` walks the link list: 5 ms on 250 000 links)."""
        if hasattr(self, '_flow_exchange') or not 2 <= ce <= 8:
            return False
        ny, ne = self._norm('y', device), self._norm('e', device)
        if (tuple(ny.shape[1:]) != (self.n_node, ny.shape[-1]) or ny.shape[-1] < 3 + int(bool(self.if_flood)) or
                tuple(ne.shape[1:]) != (self.n_edge, ne.shape[-1]) or ne.shape[-1] < max(ce, 3 if self.act else 0)):
            return False
        if not self.act:
            return True
        if a is None or tuple(a.shape) != (B, T, n_act) or a.dtype != torch.float32 or not a.is_cuda:
            return False
        ok = self._idx_cache.get(('tail_act', n_act))
        if ok is None:
            ok = self._idx_cache[('tail_act', n_act)] = (len(self._act_edge_index()) == n_act and
                                                         (self.edge_fusion or len(self.act_edges) == n_act))
        return ok

    def _predict_tail_hip(self, y, ey, a, b, nb_, x, np_form):
        """Everything of `_predict` after the forward as `uds_predict_tail` (bit-identical to the tensor code below it), or None
        where the tensor route stays: `fused_tail` off, a local model of `shard_emulator` (its flows cross the cut between the
        link gates and the balance), shapes the kernels do not take (conv='False' models with other channel counts), NumPy mode
        under autograd, and `b` or a norm that needs a gradient."""
        if not self.fused_tail or not y.is_cuda:
            return None
        B, T, C = y.shape[0], self.seq_out, 3 + int(bool(self.if_flood))
        ce, bc = ey.shape[-1], b.shape[-1]
        cy = C - 2 if self.edge_fusion else C
        n_act = a.shape[-1] if self.act else 0
        if (tuple(y.shape) != (B, T, self.n_node, cy) or tuple(ey.shape) != (B, T, self.n_edge, ce) or
                tuple(b.shape) != (B, T, self.n_node, bc) or x.shape[-1] < 1 or any(t.dtype != torch.float32 for t in (y, ey, b, x)) or
                not self._tail_takes(y.device, B, T, ce, a, n_act)):
            return None
        if _ag.grad_on(b, nb_, *self._norms.values()):
            return None
        train = _ag.grad_on(y, ey, a if self.act else None, x)
        if train and np_form:
            return None
        spec = self._tail_spec(y.device, n_act, bc, ce)
        if spec is None:
            return None
        if self._inc_handle is None:
            self._inc_handle = _lib.CsrHandle(self.graph.inc_n)
        pump_override = self.act and (self._has_link_pump if np_form else self._has_pump)
        depth_gate = 0.01 if np_form else 0.0
        c = lambda t: t.detach().contiguous()
        h0, runoff, a_ = x[:, -1, :, 0], c(b[..., 0]), a if self.act else None
        if train:
            self.last_tail_path = 'hip-train'
            return _ag.PredictTailFn.apply(y, ey, a_, h0, c(nb_), runoff, self._inc_handle, self._inc_sign, spec, depth_gate, pump_override)
        self.last_tail_path = 'hip'
        return _lib.predict_tail(self._inc_handle, self._inc_sign, spec, c(y), c(ey), None if a_ is None else c(a_), c(nb_), runoff, c(h0),
                                 depth_gate, pump_override)

    def _model(self, x, a, b, ex, ae=None, adj=None, fit=False):
        """emulator.py:400-438 on normalised tensors; `roll` > 0 = autoregressive chunks of seq_out steps."""
        if self.roll:
            ys, eys = [], []
            for i in range(self.roll):
                sl = slice(i * self.seq_out, (i + 1) * self.seq_out)
                y, ey, x, ex = self._roll_step(x, ex, a[:, sl] if a is not None else None, b[:, sl], fit)
                ys.append(y)
                eys.append(ey)
            preds, edge_preds = torch.cat(ys, dim=1), torch.cat(eys, dim=1)
        else:
            if ae is None and self.act:
                ae = self.get_edge_action(a, True)
            if adj is None and self.act and self.use_adj:
                adj = self.get_adj_action(a, True)
            preds, edge_preds = self.post_proc_tf(self.forward(x, b, ex, ae, adj, training=fit), a, b)
        return preds.clamp(0, 1), edge_preds                          # :437

    def _roll_step(self, x, ex, a_i, b_i, fit=False):
        """One chunk of the autoregressive rollout (emulator.py:403-423): forward on the last seq_in steps, post-processing,
        then the window shifts by seq_out steps fed with the prediction (flood bit thresholded at 0.5)."""
        ae_i, adj_i = self._chunk_actions(a_i)                                              # :407
        y, ey = self.forward(x[:, -self.seq_in:], b_i, ex[:, -self.seq_in:], ae_i, adj_i, training=fit)
        y, ey = self.post_proc_tf((y, ey), a_i, b_i)
        return (y, ey) + self._shift_window(x, ex, y, ey, b_i, ae_i)

    def _chunk_actions(self, a_i):
        """(ae_i, adj_i): the link settings and the adjacency mask the forward of one chunk takes, from its settings a_i."""
        return (self.get_edge_action(a_i, True) if self.act else None,
                self.get_adj_action(a_i, True) if self.act and self.use_adj else None)

    def _shift_window(self, x, ex, y, ey, b_i, ae_i):
        """The next (x, ex) of the rollout (:413-423): the windows keep their last seq_in - seq_out steps and take the chunk's
        post-processed prediction y, ey with its boundary b_i (flood bit fed back as a hard 0/1, :417) and its link settings ae_i
        (ones for a model without actions)."""
        keep = self.seq_in - self.seq_out
        x_new = torch.cat([y[..., :-1], (y[..., -1:] > 0.5).float(), b_i] if self.if_flood else [y, b_i], dim=-1)
        x = torch.cat([x[:, -keep:], x_new], dim=1) if keep > 0 else x_new
        ex_new = torch.cat([ey, ae_i if self.act else torch.ones(ey.shape[:-1] + (1,), device=ey.device)], dim=-1)
        ex = torch.cat([ex[:, -keep:], ex_new], dim=1) if keep > 0 else ex_new
        return x, ex

    def _fused_roll_ok(self, x, b, ex):
        """The plain configuration whose post-forward part `uds_roll_update` covers: edge fusion, no control actions, no tide,
        no offset / pump gating, one runoff channel, state = [h, q_in, q_out, (flood)] + runoff, link state = 3 + setting."""
        cy = 1 + int(bool(self.if_flood))
        return (self.edge_fusion and not self.act and not self.tide and not self._has_offset and b.shape[-1] == 1 and
                x.shape[-1] == cy + 3 and ex.shape[-1] == 4 and self.seq_out <= self.seq_in)

    def _roll_step_fused(self, x_win, ex_win, b_i):
        """`_roll_step` on persistent windows: forward, then ONE kernel pair for post-processing + feedback (in place)."""
        if self._inc_handle is None:
            self._inc_handle = _lib.CsrHandle(self.graph.inc_n)
        y, ey = self.forward(x_win, b_i, ex_win, None)
        span, mini = self._norm_parts('e', ey.shape[-1], ey.device)
        dev = str(ey.device)
        hit = self._norm_derived.get(('roll_e', dev))
        if hit is None or hit[0] is not span:
            hit = self._norm_derived[('roll_e', dev)] = (span, span[..., -1].contiguous(), mini[..., -1].contiguous())
        ny = self._norm('y', ey.device)
        fs = self._norm_derived.get(('flow_scale', dev))
        if fs is None or fs[0] is not ny:
            fs = self._norm_derived[('flow_scale', dev)] = (
                ny, ((ny[0, :, 1] > 1e-3).float() / ny[0, :, 1]).contiguous(), ((ny[0, :, 2] > 1e-3).float() / ny[0, :, 2]).contiguous())
        preds = _lib.roll_update(self._inc_handle, self._inc_sign, hit[1], hit[2], fs[1], fs[2], y, ey, b_i, x_win, ex_win, self.if_flood)
        return preds, ey

    def rollout_graphed(self, x, a, b, ex):
        """`_model` with roll > 0 where every chunk replays ONE captured HIP graph (the step has ~60 small launches: with few
        snapshots per step the eager loop is bound by launch latency).  Same arguments and result as `_model(x, a, b, ex)`;
        the graph is re-captured when shapes change.  Parameters must not change between capture and replay (the packed
        weight buffers are baked in): call `drop_graph()` after loading or training."""
        if not self.roll:
            raise ValueError('rollout_graphed needs roll > 0')
        so = self.seq_out
        key = (tuple(x[:, -self.seq_in:].shape), tuple(b.shape[2:]), tuple(ex[:, -self.seq_in:].shape), None if a is None else tuple(a.shape[2:]),
               str(x.device))
        if self._graph is None or self._graph['key'] != key:
            G = dict(key=key, x=x[:, -self.seq_in:].clone(), ex=ex[:, -self.seq_in:].clone(), b=b[:, :so].clone(),
                     a=None if a is None else a[:, :so].clone())
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            fused = self._fused_roll_ok(G['x'], G['b'], G['ex'])     # post-processing + feedback as one kernel pair, in place
            with torch.cuda.stream(side), torch.no_grad():          # warm-up: caches, packed weights, tile plans
                for _ in range(2):
                    if fused:
                        self._roll_step_fused(G['x'].clone(), G['ex'].clone(), G['b'])
                    else:
                        self._roll_step(G['x'], G['ex'], G['a'], G['b'])
            torch.cuda.current_stream(x.device).wait_stream(side)
            G['graph'] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(G['graph']), torch.no_grad():
                if fused:
                    y, ey = self._roll_step_fused(G['x'], G['ex'], G['b'])
                else:
                    y, ey, xn, exn = self._roll_step(G['x'], G['ex'], G['a'], G['b'])
                    G['x'].copy_(xn)
                    G['ex'].copy_(exn)
            G['y'], G['ey'] = y, ey
            self._graph = G
        G = self._graph
        with torch.no_grad():
            G['x'].copy_(x[:, -self.seq_in:])
            G['ex'].copy_(ex[:, -self.seq_in:])
            ys = torch.empty((x.shape[0], self.roll * so) + tuple(G['y'].shape[2:]), device=x.device)
            eys = torch.empty((x.shape[0], self.roll * so) + tuple(G['ey'].shape[2:]), device=x.device)
            for i in range(self.roll):
                sl = slice(i * so, (i + 1) * so)
                G['b'].copy_(b[:, sl])
                if a is not None:
                    G['a'].copy_(a[:, sl])
                G['graph'].replay()
                ys[:, sl].copy_(G['y'])
                eys[:, sl].copy_(G['ey'])
        return ys.clamp(0, 1), eys

    def drop_graph(self):
        self._graph = None

    def simulate(self, states, runoff, a=None, edge_states=None):
        """emulator.py:521-564, with every sliding window of the event batched into ONE forward (the reference loops
        over time steps with a host round trip each).  states (n,T_in,N,C), runoff (n,T_out,N,b_in) -> (n,T_out,N,5), (n,T_out,E,3)."""
        runoff = runoff[:, :self.seq_out]
        return self.predict(states, runoff, a, edge_states)      # (the reference's loop body is `predict` on one window: NumPy-mode `post_proc`)

    # ------------------------------------------------------------------ training step (:440-484)
    def _loss_setup(self, device):
        """nwei / ewei / poswei exactly as the constructor of the reference builds them (emulator.py:82,99-106,116)."""
        if getattr(self, '_lw', None) is not None and self._lw[0] == device:
            return self._lw[1]
        g = lambda k, d: np.asarray(getattr(self._args, k, d), dtype=np.float64)
        nwei = np.repeat(g('nwei', np.ones(self.n_node))[:, None], 3 + int(self.balance), axis=-1).astype(np.float32)
        hmax, hmin, outf = (self.hmax.cpu().numpy().astype(np.float64), self.hmin.cpu().numpy().astype(np.float64),
                            self.is_outfall.cpu().numpy().astype(np.float64))
        if hmin.max() > 0:
            wei = (hmax - hmin) * (1 - outf) + (hmax - hmin).mean() * outf
            wei = (hmax.max() - hmin.min()) / wei
            nwei = nwei * np.stack([wei] + (2 + int(self.balance)) * [np.ones_like(wei)], axis=-1)
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)
        lw = dict(nwei=t(nwei), ewei=t(g('ewei', np.ones(self.n_edge))), poswei=t(g('poswei', np.ones(self.n_node))))
        self._lw = (device, lw)
        return lw

    @staticmethod
    def _mse(y_true, y_pred, sample_weight=None):
        """keras MeanSquaredError(): mean over the last axis, optional per-sample weights, then the mean over all samples."""
        per = ((y_pred - y_true) ** 2).mean(dim=-1)
        if sample_weight is not None:
            per = per * sample_weight
        return per.mean()

    @staticmethod
    def _bce(y_true, y_pred, sample_weight):
        """keras BinaryCrossentropy() on probabilities (clipped to [1e-7, 1 - 1e-7]), weighted, mean over all samples."""
        p = y_pred.clamp(1e-7, 1 - 1e-7)
        per = -(y_true * torch.log(p) + (1 - y_true) * torch.log(1 - p)).mean(dim=-1)
        return (per * sample_weight).mean()

    def get_node_loss(self, y, b, preds):
        lw = self._loss_setup(preds.device)
        if self.balance:
            q_w, pr = self.constrain_tf(self.normalize(preds, 'y', True), self.normalize(b, 'b', True)[..., :1])
            q_w = (q_w / self._norm('y', preds.device)[0, :, -1]).unsqueeze(-1)
            pr = self.normalize(pr, 'y').clamp(0, 1)
            return self._mse(torch.cat([y[..., :3], y[..., -1:]], dim=-1) * lw['nwei'], torch.cat([pr[..., :3], q_w], dim=-1) * lw['nwei'])
        return self._mse(y[..., :3] * lw['nwei'], preds[..., :3] * lw['nwei'])

    def get_flood_loss(self, y, preds):
        lw = self._loss_setup(preds.device)
        weight = lw['poswei'] * y[..., -2] + lw['nwei'][:, -1] * (1 - y[..., -2])
        return self._bce(y[..., -2:-1], preds[..., -1:], weight)

    # ------------------------------------------------------------------ the training tail as one HIP operator
    fused_fit_tail = True      # False: `fit_eval` / `fit_grad_norm` keep their tensor code for everything after the forward
    last_fit_tail_path = None  # 'hip' (through autograd.FitTailFn) or 'torch' after a fit_eval / fit_grad_norm call

    def _fit_tail_spec(self, x, a, b, y, ey):
        """(`_lib.TailSpec`, loss operands) when the tail of this step runs as `uds_fit_tail`, or None where the tensor route stays:
        `fused_fit_tail` off, a local model of `shard_emulator` (its flows cross the cut between the link gates and the balance),
        channel counts the kernels do not take (conv='False' models with a wider state; the rule of `_predict_tail_hip`), and a
        setting, boundary, target or norm that needs a gradient (the operator is differentiable in the network outputs only)."""
        if not self.fused_fit_tail or not x.is_cuda:
            return None
        if 'y' not in self._norms or 'e' not in self._norms or (self.balance and 'b' not in self._norms):
            return None                          # the kernels read the norms a plain model's tensor code never asks for
        dev, N, E = x.device, self.n_node, self.n_edge
        B, T = x.shape[0], self.seq_out * max(self.roll, 1)
        ce = self.e_out
        n_act = a.shape[-1] if self.act and a is not None else 0
        ny, nb = self._norm('y', dev), self._norm('b', dev) if self.balance else None
        if (self.n_out != (1 if self.edge_fusion else 3) or b.dim() != 4 or tuple(b.shape[:3]) != (B, T, N) or
                y.dim() != 4 or tuple(y.shape[:3]) != (B, T, N) or y.shape[-1] < 3 or tuple(ey.shape) != (B, T, E, ce) or
                (nb is not None and tuple(nb.shape[1:]) != (N, nb.shape[-1])) or
                any(t.dtype != torch.float32 or not t.is_cuda for t in (x, b, y, ey)) or not self._tail_takes(dev, B, T, ce, a, n_act)):
            return None
        if _ag.grad_on(a if self.act else None, b, y, ey, *self._norms.values()):
            return None
        spec = self._tail_spec(dev, n_act, b.shape[-1], ce)
        if spec is None:
            return None
        lw = self._loss_setup(dev)
        hit = self._norm_derived.get(('fit_tail', str(dev)))
        if hit is None or hit[0] is not ny or hit[1] is not nb or hit[2] is not lw:
            ops = dict(nwei=lw['nwei'].contiguous(), poswei=lw['poswei'].contiguous(), ewei=lw['ewei'].contiguous(), balance=self.balance)
            if self.balance:
                ops.update(qw_den=ny[0, :, -1].contiguous(), span_b=(nb[0, :, 0] - nb[1, :, 0]).contiguous(), mini_b=nb[1, :, 0].contiguous())
            hit = self._norm_derived[('fit_tail', str(dev))] = (ny, nb, lw, ops)
        if self._inc_handle is None:
            self._inc_handle = _lib.CsrHandle(self.graph.inc_n)
        return spec, dict(hit[3], sign=self._inc_sign)

    def _fit_losses(self, x, a, b, y, ex, ey, ae, fit, flood=False):
        """(node_loss, flood_loss or None, edge_loss) of one step on NORMALISED tensors, for `fit_eval` and `fit_grad_norm`: the
        network forward, then everything after it either as ONE HIP operator per chunk (`autograd.FitTailFn`: `post_proc_tf`,
        clamp, the three losses and their reverse mode) or as the tensor code (`_model`, `get_node_loss`, `get_flood_loss`, `_mse`).
        With `roll` the operator's unclamped `out_y` / `out_ey` feed the next window, the loss sums add up over the chunks and
        the division by the sample count follows.  flood=True (`fit_grad_norm`) asks for the flood loss whatever `balance` says; with
        `balance` the operator does not compute it and the tensor route stays."""
        fused = None if flood and self.balance else self._fit_tail_spec(x, a, b, y, ey)
        if fused is None:
            self.last_fit_tail_path = 'torch'
            preds, edge_preds = self._model(x, a, b, ex, ae, None, fit)
            lw = self._loss_setup(preds.device)
            node_loss = self.get_node_loss(y, b, preds)
            fl_loss = self.get_flood_loss(y, preds) if flood or (self.if_flood and not self.balance) else None
            return node_loss, fl_loss, self._mse(ey, edge_preds, lw['ewei'])
        self.last_fit_tail_path = 'hip'
        spec, ops = fused
        c = lambda t: None if t is None else t.detach().contiguous()
        so = self.seq_out
        tail = lambda ny_, ney_, sl: _ag.FitTailFn.apply(ny_, ney_, c(a[:, sl]) if self.act else None, c(b[:, sl]), c(y[:, sl]), c(ey[:, sl]),
                                                         self._inc_handle, spec, ops, self.act and self._has_pump)
        if not self.roll:
            adj = self.get_adj_action(a, True) if self.act and self.use_adj else None
            _, _, sums = tail(*self.forward(x, b, ex, ae, adj, training=fit), slice(None))
        else:
            sums = None
            for i in range(self.roll):                     # `_model` with roll > 0, `_roll_step` with the tail fused
                sl = slice(i * so, (i + 1) * so)
                a_i, b_i = (a[:, sl] if a is not None else None), b[:, sl]
                ae_i, adj_i = self._chunk_actions(a_i)
                out_y, out_ey, s = tail(*self.forward(x[:, -self.seq_in:], b_i, ex[:, -self.seq_in:], ae_i, adj_i, training=fit), sl)
                sums = s if sums is None else sums + s
                x, ex = self._shift_window(x, ex, out_y, out_ey, b_i, ae_i)
        rows = float(y.shape[0] * y.shape[1])
        node_loss, edge_loss = sums[0] / (rows * self.n_node), sums[2] / (rows * self.n_edge)
        fl_loss = sums[1] / (rows * self.n_node) if self.if_flood and not self.balance else None
        return node_loss, fl_loss, edge_loss

    def _fit_total_loss(self, node_loss, fl_loss, edge_loss):
        """The scalar a training step differentiates (emulator.py:466-473)."""
        loss = node_loss + edge_loss
        if self.gradnorm:                    # GradNorm task weights (emulator.py:470-473): constants for this step
            alpha = self._alphas(node_loss.device)
            loss = alpha[0].detach() * loss
        if self.if_flood:
            if fl_loss is None:
                raise NotImplementedError('if_flood with balance: the reference leaves fl_loss undefined here (emulator.py:466,473)')
            loss = loss + (alpha[1].detach() * fl_loss if self.gradnorm else fl_loss)
        return loss

    def fit_eval(self, x, a, b, y, ex, ey, fit=True):
        """One training (fit=True) or evaluation step on NORMALISED tensors (emulator.py:457-484): forward through
        `_model`, node MSE (+ weighted flood BCE) + link MSE, reverse mode through the HIP operators (autograd.py), Adam with
        per-variable clipnorm=1.  Returns [node_loss, (flood_loss,) edge_loss] as 0-d tensors.  With `graphed_fit` the step is one
        replay of a captured graph (`_fit_eval_graph`) unless `fit_graph_refusal` names a reason."""
        if self._graphed_fit:
            self.last_fit_refusal = self.fit_graph_refusal(x, a, b, y, ex, ey)
            if self.last_fit_refusal is None:
                return self._fit_eval_graph(x, a, b, y, ex, ey, fit)
        self.last_fit_path = 'eager'
        params = [p for p in self.parameters()]
        if fit:
            for p in params:
                p.requires_grad_(True)
        return self._fit_step((x, a, b, y, ex, ey), fit, params, captured=False)

    def _fit_step(self, inputs, fit, params, captured):
        """The step itself, once for both modes of `fit_eval`: losses, total loss, gradients zeroed, backward, optimizer step, the
        detached losses.  captured=False (the eager step): the loss is tested on the host, agreed over the data-parallel ranks,
        before backward; the gradients are all-reduced after it; the optimizer is created on first use and a `HipKerasAdam` reports
        after its step.  captured=True (inside a graph, one rank): nothing touches the host -- `HipKerasAdam.step(loss)` tests the
        loss and the gradient norms on the device, and `_fit_eval_graph` reads its status after the replay."""
        x, a, b, y, ex, ey = inputs
        with torch.set_grad_enabled(bool(fit)):
            ae = self.get_edge_action(a, True) if self.act else None
            node_loss, fl_loss, edge_loss = self._fit_losses(x, a, b, y, ex, ey, ae, fit)
            if fit:
                loss = self._fit_total_loss(node_loss, fl_loss, edge_loss)
                if not captured:
                    from .dist import all_ranks_finite, allreduce_gradients
                    if not all_ranks_finite(loss):       # agreed over the data-parallel ranks: all raise or none does
                        raise FloatingPointError('Loss contains NaN or Inf values.')
                for p in params:
                    p.grad = None
                loss.backward()
                if captured:
                    self._optimizer.step(loss)
                else:
                    allreduce_gradients(params)          # data-parallel ranks: one bucketed all-reduce (no-op on one rank)
                    if self._optimizer is None:
                        self._optimizer = (HipKerasAdam if self._graphed_fit else KerasAdam)(params, self.learning_rate, clipnorm=1.0)
                    self._optimizer.step()
                    if isinstance(self._optimizer, HipKerasAdam):
                        self._optimizer.raise_if_not_finite()
        return [node_loss.detach()] + ([fl_loss.detach()] if self.if_flood and fl_loss is not None else []) + [edge_loss.detach()]

    # ------------------------------------------------------------------ fit_eval as one captured graph per step
    def fit_graph_refusal(self, *tensors):
        """Why a `fit_eval` step of this model (on these tensors, if given) cannot be captured -- it then runs eager -- or None:
        every reason is a piece of HOST state the step reads, and the decision is made before anything is captured."""
        if self.dropout:
            return 'dropout > 0: the mask offsets of the dropout stream are host counters that advance per call'
        from torch import distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return 'a process group with %d ranks: the gradient all-reduce and the agreed finite flag run between host steps' % dist.get_world_size()
        where = [p for p in self.parameters()] + [t for t in tensors if isinstance(t, torch.Tensor)]
        if any(not t.is_cuda for t in where):
            return 'CPU tensors: a graph is captured on the device stream'
        return None

    def _fit_graph_key(self, x, a, b, y, ex, ey, fit):
        """What a captured step depends on beyond the values in device memory: shapes and device of the inputs, `fit`, the parameters
        (their storage and which of them train), the objects whose storage the graph reads (optimizer state, norms, GradNorm
        weights), the hyper-parameters and route flags read on the host, and for an evaluation step which dense NodeEdge layers
        have a bias off their support (a host decision of `NodeEdge.support_values`)."""
        shapes = tuple(None if t is None else (tuple(t.shape), str(t.dtype)) for t in (x, a, b, y, ex, ey))
        params = tuple((p.data_ptr(), bool(p.requires_grad or fit)) for p in self.parameters())
        opt = self._optimizer
        held = (None if opt is None or not fit else (id(opt), opt.m[0].data_ptr() if opt.m else 0),
                tuple((k, id(v)) for k, v in sorted(self._norms.items())),
                None if not (self.gradnorm and fit) or getattr(self, '_alpha', None) is None else self._alpha.data_ptr())
        rest = None if fit else tuple(m.support_values()[1] is None for m in self.modules() if isinstance(m, NodeEdge) and not m.sparse)
        return (shapes, str(x.device), bool(fit), params, held, self.roll, self.gradnorm, self.learning_rate, self.fused_fit_tail,
                self.dense_node_edge_train, self.fused_gat_backward, self.fused_temporal, self.snapshot_remainder, rest)

    def _invalidate_weight_packs(self):
        # Empty every module's PackCache, under whatever name it is held, so that the next forward rebuilds each packed or derived
        # copy of a weight: inside a capture that makes every pack a node of the graph (a replay bumps no version).
        for m in self.modules():
            for held in vars(m).values():
                if isinstance(held, PackCache):
                    held.clear()

    def _capture_fit_graph(self, inputs, fit, params):
        """Static input buffers, two warm-up steps on a side stream that leave the model as it was, then the capture on ONE stream
        (nothing forks inside it: the graph is a chain).  An error during warm-up or capture propagates."""
        dev = inputs[0].device
        G = dict(inputs=[None if t is None else t.detach().clone() for t in inputs], params=params)
        opt = self._optimizer
        if fit and not isinstance(opt, HipKerasAdam):
            raise TypeError('graphed_fit needs a HipKerasAdam optimizer, the model holds a %s' % type(opt).__name__)
        ne_dense = [m for m in self.modules() if isinstance(m, NodeEdge) and not m.sparse]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            if fit:
                with torch.no_grad():
                    saved = [t.detach().clone() for t in params + opt.m + opt.v + [opt.state]]
            for _ in range(2):                              # caches, handles, tile plans, kernel code objects, library workspaces
                self._fit_step(G['inputs'], fit, params, captured=True)
            if fit:
                with torch.no_grad():
                    for dst, src in zip(params + opt.m + opt.v + [opt.state], saved):
                        dst.copy_(src)
                for p in params:
                    p.grad = None
            else:
                for m in ne_dense:                          # asked of the device here: a capture cannot
                    m._capture_rest_none = m.support_values()[1] is None
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self._invalidate_weight_packs()
        G['graph'] = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(G['graph']):
                G['out'] = self._fit_step(G['inputs'], fit, params, captured=True)
        finally:
            self._invalidate_weight_packs()                 # a pack made while capturing holds nothing until a replay
            for m in ne_dense:
                m._capture_rest_none = None
        return G

    def _fit_eval_graph(self, x, a, b, y, ex, ey, fit):
        inputs = (x, a if self.act else None, b, y, ex, ey)
        params = [p for p in self.parameters()]
        if fit:
            for p in params:
                p.requires_grad_(True)
            if self.gradnorm:
                self._alphas(x.device)                      # created before the capture; fit_grad_norm updates it in place
            if self._optimizer is None:                     # before the key: the graph reads its moments and state
                self._optimizer = HipKerasAdam(params, self.learning_rate, clipnorm=1.0)
        if getattr(self, '_fit_graphs', None) is None:
            from collections import OrderedDict
            self._fit_graphs = OrderedDict()
        for item in list(self._norms):                      # on the device before the key names them (`_norm` moves them on first use)
            self._norm(item, x.device)
        key = self._fit_graph_key(*inputs, fit)
        G = self._fit_graphs.get(key)
        if G is None:
            G = self._capture_fit_graph(inputs, fit, params)
            self._fit_graphs[key] = G
            while len(self._fit_graphs) > self.FIT_GRAPHS:
                self._fit_graphs.popitem(last=False)
            self.last_fit_path = 'graph-capture'
        else:
            self._fit_graphs.move_to_end(key)
            self.last_fit_path = 'graph'
        with torch.no_grad():
            for dst, src in zip(G['inputs'], inputs):
                if dst is not None:
                    dst.copy_(src)
        G['graph'].replay()
        out = [t.clone() for t in G['out']]
        if fit:
            for p in params:                                # no kernel: the PackCache keys change, eager code re-packs from the new weights
                torch.autograd.graph.increment_version(p)
            self._optimizer.raise_if_not_finite()
        return out

    def drop_fit_graphs(self):
        """Free the captured `fit_eval` graphs (and the gradients that live in their memory pools)."""
        if getattr(self, '_fit_graphs', None):
            self._fit_graphs.clear()
            for p in self.parameters():
                p.grad = None

    # ------------------------------------------------------------------ GradNorm (:118-125,486-519)
    def _alphas(self, device):
        """[alpha_reg, alpha_cls]: the two trainable task weights (initially 1, kept at sum 2), with their own Adam(1e-4)."""
        if getattr(self, '_alpha', None) is None or self._alpha.device != device:
            self._alpha = torch.ones(2, device=device, dtype=torch.float32, requires_grad=True)
            self._alpha_optimizer = KerasAdam([self._alpha], 1e-4)
        return self._alpha

    def fit_grad_norm(self, x, a, b, y, ex, ey, ini_loss):
        """One GradNorm update of the task weights (`fit_grad_norm` / `_get_grad_norm`, emulator.py:486-519): the norms of
        alpha_task * d loss_task / d W at the shared layer W = `dense_resx` kernel are pulled (mean absolute error) towards
        mean(norms) * (relative inverse training rate) ** 0.5; one Adam(1e-4) step on the alphas, then they are rescaled to
        sum 2.  ini_loss = [node, flood, edge] losses of the first step.  Returns the alpha loss (0-d tensor)."""
        if not self.gradnorm:
            raise ValueError('fit_grad_norm needs args.gradnorm = True')
        if not self.if_flood:
            raise ValueError('GradNorm balances the regression and the flood-classification task: it needs if_flood')
        W = self.res_x.kernel
        flags = [(p, p.requires_grad) for p in self.parameters()]
        for p, _ in flags:
            p.requires_grad_(p is W)
        try:
            with torch.enable_grad():
                ae = self.get_edge_action(a, True) if self.act else None
                node_loss, fl_loss, edge_loss = self._fit_losses(x, a, b, y, ex, ey, ae, False, flood=True)
                reg_loss = node_loss + edge_loss
                g_reg, = torch.autograd.grad(reg_loss, W, retain_graph=True)
                g_cls, = torch.autograd.grad(fl_loss, W)
                alpha = self._alphas(reg_loss.device)
                norms = torch.stack([(alpha[0] * g_reg.detach()).norm(), (alpha[1] * g_cls.detach()).norm()])
                ini = [float(v) for v in ini_loss]
                r = torch.stack([reg_loss.detach() / (ini[0] + ini[-1]), fl_loss.detach() / ini[1]])
                target = norms.detach().mean() * (r / r.mean()) ** 0.5
                alpha_loss = (target - norms).abs().mean()
                alpha.grad = None
                alpha_loss.backward()
            self._alpha_optimizer.step()
            with torch.no_grad():
                alpha.mul_(2.0 / alpha.sum())
        finally:
            for p, f in flags:
                p.requires_grad_(f)
        return alpha_loss.detach()

    # ------------------------------------------------------------------ Keras checkpoints (:814-852)
    def keras_layer_map(self):
        """[(keras layer name, module, [(keras weight name, parameter name), ...])] in the creation order of
        `build_network` (emulator.py:166-341): the auto-numbered names `save_weights('model.h5')` stores the weights
        under (`dense`, `dense_1`, ..., `node_edge_k`, `mixed_gat_k` / `gcn_conv_k`, `conv1d_k`, `dense_resx`)."""
        count = {}

        def name(base):
            k = count.get(base, 0)
            count[base] = k + 1
            return base if k == 0 else '%s_%d' % (base, k)

        dense_w = [('kernel', 'kernel'), ('bias', 'bias')]
        ne_w = [('weight', 'weight'), ('bias', 'bias')]
        gat_w = [('kernel', 'kernel'), ('attn_kernel_self', 'attn_kernel_self'), ('attn_kernel_neigh', 'attn_kernel_neighs'), ('bias', 'bias')]
        out = [(name('dense'), self.embed_x, dense_w), (name('dense'), self.embed_b, dense_w), (name('dense'), self.embed_e, dense_w)]
        if self.act:
            out.append((name('dense'), self.embed_ae, dense_w))

        # DiffusionConv keeps its coefficients in `channels` DiffuseFeatures sub-layers (one (K + 1,) kernel each): the importer
        # takes them stacked in creation order as ONE (channels, K + 1) array under '<layer>/kernel:0'
        conv_name = {'GAT': 'mixed_gat', 'GCN': 'gcn_conv', 'Diffusion': 'diffusion_conv'}[self.conv_kind]
        conv_w = {'GAT': gat_w, 'GCN': dense_w, 'Diffusion': [('kernel', 'kernel')]}[self.conv_kind]

        def spatial(block):
            if not self.conv:
                for ly in block:
                    out.append((name('dense'), ly, dense_w))
                return
            if self.graph_base:
                for ly in block.layers:
                    out.append((name(conv_name), ly, conv_w))
                return
            for ly in block.layers:
                out.append((name('dense'), ly.dense_xe, dense_w))
                out.append((name('dense'), ly.dense_ex, dense_w))
                out.append((name('node_edge'), ly.node_edge_n, ne_w))
                out.append((name('node_edge'), ly.node_edge_e, ne_w))
                if ly.conv == 'GAT':
                    out.append((name('mixed_gat'), ly.gat_x, gat_w))
                    out.append((name('mixed_gat'), ly.gat_e, gat_w))
                else:
                    out.append((name(conv_name), ly.gcn_x, conv_w))
                    out.append((name(conv_name), ly.gcn_e, conv_w))

        def temporal(mods):
            for m in mods:
                if isinstance(m, _Recurrent):       # keras nests the weights in the layer's cell: gru/gru_cell/kernel:0, ...
                    # the cell objects are auto-numbered by a counter of their own: the k-th GRU layer saves
                    # 'gru_k/gru_k/gru_cell_k/kernel:0' (Keras 2.10 creates the cell without a name)
                    cell = name(m.KIND.lower() + '_cell')
                    out.append((name(m.KIND.lower()), m, [(cell + '/kernel', 'kernel'), (cell + '/recurrent_kernel', 'recurrent_kernel'),
                                                         (cell + '/bias', 'bias')]))
                else:
                    out.append((name('conv1d'), m, dense_w))

        spatial(self.block1)
        temporal(self.tem1_x)
        temporal(self.tem1_e)
        spatial(self.block2)
        temporal(self.tem2_x)
        temporal(self.tem2_e)
        out.append(('dense_resx', self.res_x, dense_w))
        out.append((name('dense'), self.res_e, dense_w))
        out.append((name('dense'), self.out, dense_w))
        for m in self.flood:
            out.append((name('dense'), m, dense_w))
        if self.if_flood:
            out.append((name('dense'), self.flood_out, dense_w))
        out.append((name('dense'), self.e_out_layer, dense_w))
        return out

    def load_keras_weights(self, weights):
        """Weights of a trained reference model, keyed the way Keras stores them in `model.h5`:
        `weights['<layer>/<weight>:0']` or `weights['<layer>/<layer>/<weight>:0']` (the HDF5 group path) or
        `weights['<layer>'] = [arrays in the layer's own order]`, values array-like.  `Emulator.load('model.h5')` reads the file
        with the minimal HDF5 reader of `gnn_uds_amd/h5.py` and calls this; arrays dumped elsewhere with h5py work the same.  Shapes are
        checked; NodeEdge parameters created with sparse=True take the dense (R, M) arrays on their support and refuse a bias
        that is non-zero off it (ValueError: nothing is dropped silently)."""
        weights = dict(weights)
        missing = []
        with torch.no_grad():
            for lname, mod, pairs in self.keras_layer_map():
                for idx, (kname, pname) in enumerate(pairs):
                    arr = _find_keras_weight(weights, lname, kname)
                    if arr is None and lname in weights and not hasattr(weights[lname], 'shape'):
                        arr = weights[lname][idx]
                    if arr is None:
                        missing.append('%s/%s' % (lname, kname))
                        continue
                    p = getattr(mod, pname)
                    t = torch.as_tensor(np.asarray(arr), dtype=torch.float32)
                    if getattr(mod, 'sparse', False) and t.dim() == 2:        # NodeEdge with one parameter per support entry
                        flat = mod._flat.cpu()
                        if pname == 'bias':
                            # the reference trains `b` as a full (R, M) matrix (emulator.py:36-45): entries off the incidence
                            # support act on the output (`+ b @ x`) and a sparse=True module has nowhere to keep them
                            off = t.clone()
                            off.reshape(-1)[flat] = 0.0
                            if bool((off != 0).any()):
                                raise ValueError('%s/%s: the checkpoint bias has %d non-zero entries off the incidence support (max |b| = %.3g); '
                                                 'a model built with args.sparse_params=True would drop them and change the outputs -- build it '
                                                 'with args.sparse_params=False (the fused kernel takes the dense remainder)'
                                                 % (lname, kname, int((off != 0).sum()), float(off.abs().max())))
                        t = t.reshape(-1)[flat]
                    if pname == 'kernel' and t.dim() == 2 and p.dim() == 3:   # GCNConv (F, C) vs GATConv (F, 1, C)
                        t = t.reshape(p.shape)
                    if tuple(t.shape) != tuple(p.shape):
                        raise ValueError('%s/%s: checkpoint shape %r, model expects %r' % (lname, kname, tuple(t.shape), tuple(p.shape)))
                    p.copy_(t.to(p.device))
        if missing:
            raise KeyError('weights not found in the checkpoint: %s' % ', '.join(missing))
        return self

    def export_keras_weights(self):
        """{'<layer>/<weight>:0': ndarray} under the Keras names (inverse of load_keras_weights; dense NodeEdge only)."""
        out = {}
        for lname, mod, pairs in self.keras_layer_map():
            if getattr(mod, 'sparse', False):
                raise NotImplementedError('NodeEdge(sparse=True) has no dense (R, M) parameters to export')
            for kname, pname in pairs:
                out['%s/%s:0' % (lname, kname)] = getattr(mod, pname).detach().cpu().numpy().copy()
        return out

    # ------------------------------------------------------------------ checkpoints (:814-852)
    def save(self, model_dir=None):
        """emulator.py:814-831: weights, the five normalisers, the optimizer state (`optim.npy` there, `optim.pt` here) and,
        with GradNorm, the task weights and THEIR optimizer (`gradnorm.ckpt` there, `gradnorm.pt` here).  A path ending in
        `.pt` names the weight file itself, as `.h5` does in the reference."""
        model_dir = model_dir if model_dir is not None else self.model_dir
        if model_dir.endswith('.pt'):
            weights, model_dir = model_dir, os.path.dirname(model_dir)
        else:
            weights = os.path.join(model_dir, 'model.pt')
        os.makedirs(model_dir or '.', exist_ok=True)
        torch.save(self.state_dict(), weights)
        for item, t in self._norms.items():
            np.save(os.path.join(model_dir, 'norm_%s.npy' % item), t.cpu().numpy())
        if self._optimizer is not None:
            torch.save(self._optimizer.state_dict(), os.path.join(model_dir, 'optim.pt'))
        if self.gradnorm and getattr(self, '_alpha', None) is not None:
            torch.save({'alpha': self._alpha.detach().cpu(), 'optimizer': self._alpha_optimizer.state_dict()}, os.path.join(model_dir, 'gradnorm.pt'))

    def load(self, model_dir=None, retrain=False):
        """emulator.py:833-852; `retrain=True` also restores the optimizer moments / step count and the GradNorm state, so
        that training resumes where it stopped (`--load_model`, main.py:199-205)."""
        model_dir = model_dir if model_dir is not None else self.model_dir
        self.drop_fit_graphs()
        keras = None
        if model_dir.endswith('.h5'):                     # the reference's own layout: a Keras weight file (:835-838)
            keras, model_dir = model_dir, os.path.dirname(model_dir)
        elif model_dir.endswith('.pt'):
            weights, model_dir = model_dir, os.path.dirname(model_dir)
        else:
            weights = os.path.join(model_dir, 'model.pt')
            if not os.path.exists(weights) and os.path.exists(os.path.join(model_dir, 'model.h5')):
                keras = os.path.join(model_dir, 'model.h5')   # a model directory written by the reference
        if keras is not None:
            from .h5 import read_keras_weights            # minimal HDF5 reader (no h5py in this image): see h5.py for what it covers
            self.load_keras_weights(read_keras_weights(keras))
        else:
            self.load_state_dict(torch.load(weights, weights_only=True))
        for item in 'xbyre':
            path = os.path.join(model_dir, 'norm_%s.npy' % item)
            if os.path.exists(path):
                self._norms[item] = torch.as_tensor(np.load(path), dtype=torch.float32)
        dev = next(self.parameters()).device
        path = os.path.join(model_dir, 'optim.pt')
        if retrain and os.path.exists(path):
            if self._optimizer is None:
                self._optimizer = (HipKerasAdam if self._graphed_fit else KerasAdam)([p for p in self.parameters()], self.learning_rate, clipnorm=1.0)
            self._optimizer.load_state_dict(torch.load(path, weights_only=True))
        path = os.path.join(model_dir, 'gradnorm.pt')
        if retrain and self.gradnorm and os.path.exists(path):
            sd = torch.load(path, weights_only=True)
            alpha = self._alphas(dev)
            with torch.no_grad():
                alpha.copy_(sd['alpha'])
            self._alpha_optimizer.load_state_dict(sd['optimizer'])
