"""torch.nn.Module mirrors of the reference's Keras / Spektral layers, running on the HIP engine.

The reference is TensorFlow/Keras + Spektral; "drop-in" therefore means: same layer
constructor arguments, same call convention `layer([x, a]) -> x'`, same weight names and shapes,
same tensor layouts -- re-expressed as `torch.nn.Module`s:

    Dense(units, activation)                      keras.layers.Dense        emulator.py:198,203,225-226,...
    NodeEdge(inci)                                emulator.py:27-45
    GATConv / MixedGAT(channels, activation=..)   spektral GATConv via emulator.py:18-25,229-230
    GCNConv(channels, activation=..) + preprocess spektral GCNConv via emulator.py:131-134
    SpatialLayer / SpatialBlock                   the loop bodies emulator.py:219-235, 272-288

Parameters are created with requires_grad=False (inference: no autograd graph is recorded).  After
`module.requires_grad_(True)` the same modules run through the autograd Functions of `autograd.py`
(HIP backward kernels; the training step of SURVEY.md a10).  All compute is HIP kernels behind the
C ABI (gnn_uds_amd/_lib.py); CPU tensors raise.
"""
import math
import os

import numpy as np
import torch
from torch import nn

from . import _lib
from . import autograd as _ag
from .graph import CSR, DrainageGraph, csr_from_dense


def _param(t):
    return nn.Parameter(t, requires_grad=False)


def _glorot_uniform(shape, device, generator=None):
    """Keras glorot_uniform incl. its fan rule for >2-D kernels (receptive field = prod(shape[:-2]))."""
    if len(shape) == 1:
        fan_in = fan_out = shape[0]
    elif len(shape) == 2:
        fan_in, fan_out = shape
    else:
        rf = int(np.prod(shape[:-2]))
        fan_in, fan_out = shape[-2] * rf, shape[-1] * rf
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    t = torch.rand(shape, generator=generator, dtype=torch.float32) * (2 * limit) - limit
    return t.to(device)


def _flatten_snapshots(x):
    """(..., M, F) -> (S, M, F) contiguous, plus the leading shape to restore."""
    if x.dim() < 2:
        raise _lib.UdsError('expected (..., elements, features), got %r' % (tuple(x.shape),))
    lead = tuple(x.shape[:-2])
    return x.reshape((-1,) + tuple(x.shape[-2:])).contiguous(), lead


class PackCache:
    """The packed or derived copies of a module's parameters (bf16 hi/lo fragments, column blocks, folded biases, support values,
    polynomial tables), rebuilt exactly when a parameter they were made from changes.  One entry per slot: a new key replaces the
    old value.  A plain object, no buffer: the contents are device memory tied to one parameter storage, so a copy or a pickle
    of the module starts empty.  `Emulator._invalidate_weight_packs` clears it around a graph capture ("Weight packs")."""

    def __init__(self):
        self._slots = {}

    def get(self, slot, tensors, build, extra=()):
        """The value of `slot`, from build() when the slot is empty or its key differs.  The key: (_version, data_ptr()) of every
        tensor the value depends on (None for an absent one), then `extra`."""
        key = tuple(None if t is None else (t._version, t.data_ptr()) for t in tensors) + tuple(extra)
        hit = self._slots.get(slot)
        if hit is None or hit[0] != key:
            hit = self._slots[slot] = (key, build())
        return hit[1]

    def peek(self, slot):
        """The value of `slot` or None; never builds."""
        hit = self._slots.get(slot)
        return None if hit is None else hit[1]

    def clear(self):
        self._slots.clear()

    def __deepcopy__(self, memo):
        return PackCache()

    def __reduce__(self):
        return PackCache, ()


def _packed_kernel(module, kernel2d):
    """bf16 hi/lo MFMA fragments of a (K, f_out) kernel, re-split only when the parameter changes."""
    packs = getattr(module, '_packs', None)
    if packs is None:
        packs = module._packs = PackCache()
    return packs.get('kernel', (module.kernel,), lambda: _lib.rowgemm_pack(kernel2d.contiguous()))


class Dense(nn.Module):
    """keras.layers.Dense(units, activation): act(x @ kernel + bias) on the last axis.

    precision='fp32': exact-fp32 FMA kernel (any shape).  precision='bf16x3': matrix-core kernel (operands split into
    bf16 hi + lo, 3 MFMA products, fp32 accumulate) when the input width is a multiple of 32 and units <= 64, the
    exact kernel otherwise."""

    def __init__(self, units, activation=None, use_bias=True, in_features=None, generator=None, precision='fp32'):
        super().__init__()
        self.units, self.activation, self.use_bias = int(units), activation or 'linear', use_bias
        self.precision = precision
        self._gen, self._packs = generator, PackCache()
        self.kernel = self.bias = None
        if self.activation not in _lib.ACT:
            raise ValueError('unknown activation %r' % (activation,))
        if in_features is not None:
            self.build(in_features, 'cpu')

    def build(self, in_features, device):
        self.kernel = _param(_glorot_uniform((int(in_features), self.units), device, self._gen))
        self.bias = _param(torch.zeros(self.units, device=device)) if self.use_bias else None

    def forward(self, x, activation=None):
        """activation: override of the layer's own (the reference applies the embedding's activation outside the layer,
        emulator.py:198-201)."""
        if self.kernel is None:
            self.build(x.shape[-1], x.device)
        act = activation or self.activation
        if _ag.grad_on(x, self.kernel, self.bias):
            return _ag.DenseFn.apply(x, self.kernel, self.bias, self, act)
        xc = x.contiguous()
        fi = xc.shape[-1]
        if self.precision == 'bf16x3' and _lib.rowgemm_supported(fi, fi, self.units):
            return _lib.rowgemm_forward(xc, _packed_kernel(self, self.kernel), self.bias, self.units, act)
        if self.precision == 'bf16x3' and self.units > 64 and self.units % 16 == 0 and _lib.rowgemm_supported(fi, fi, 64) and \
                xc.numel() // fi >= 4096:
            # wide outputs (d = 128): 64-column blocks of the kernel, each written into its columns of one output
            blocks = self._packs.get('blocks', (self.kernel, self.bias), lambda: [
                (c0, min(64, self.units - c0), _lib.rowgemm_pack(self.kernel[:, c0:c0 + 64].contiguous()),
                 None if self.bias is None else self.bias[c0:c0 + 64].contiguous()) for c0 in range(0, self.units, 64)])
            out = torch.empty(xc.shape[:-1] + (self.units,), device=xc.device, dtype=torch.float32)
            for c0, w, pk, bb in blocks:
                _lib.rowgemm_cat(xc, None, pk, bb, w, act, out=out, col0=c0)
            return out
        return _lib.dense_act(xc, self.kernel, self.bias, act)


class _GraphArg:
    """Turns the `a` of `layer([x, a])` into a device CSR handle, caching dense inputs by identity."""

    def __init__(self):
        self._cache = {}

    def handle(self, a, add_self_loops):
        if isinstance(a, _lib.CsrHandle):
            return a
        if isinstance(a, CSR):
            key = ('csr', id(a))
            if key not in self._cache:
                self._cache[key] = (a, _lib.CsrHandle(a))
            return self._cache[key][1]
        key = ('dense', id(a), add_self_loops)
        hit = self._cache.get(key)
        if hit is not None and hit[0] is a:
            return hit[1]
        dense = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        h = _lib.CsrHandle(csr_from_dense(dense, add_self_loops=add_self_loops))
        self._cache[key] = (a, h)
        return h


class GATConv(nn.Module):
    """spektral.layers.GATConv in batch/mixed mode.

    forward([x, a]): x (..., N, F); a = dense (N, N) 0/1 filter as in the reference
    (`emulator.py:143-145,229`), a `graph.CSR`, or a prebuilt `_lib.CsrHandle` (CSR inputs must
    already hold the self loops).  Weights keep Spektral's names and shapes:
    kernel (F,H,C), attn_kernel_self (C,H,1), attn_kernel_neighs (C,H,1), bias (H*C) or, with concat_heads=False, (C).

    attn_heads=1 without return_attn_coef is what the reference uses and runs on the single-head kernels.  attn_heads=H > 1,
    concat_heads=False and return_attn_coef=True run on uds_gat_aggregate_heads / uds_gat_backward_heads (C % 4 == 0,
    H*C <= 256): forward then returns `out` or `(out, attn)`, attn (..., H, nnz) in the entry order of the pattern
    (`dense_attn_coef` scatters it to Spektral's (..., N, H, N))."""

    def __init__(self, channels, attn_heads=1, concat_heads=True, dropout_rate=0.5, return_attn_coef=False,
                 add_self_loops=True, activation=None, use_bias=True, in_channels=None, generator=None):
        super().__init__()
        if int(attn_heads) < 1:
            raise ValueError('GATConv: attn_heads must be positive, got %r' % (attn_heads,))
        self.channels, self.attn_heads, self.concat_heads = int(channels), int(attn_heads), bool(concat_heads)
        self.return_attn_coef = bool(return_attn_coef)
        if (self.attn_heads > 1 or self.return_attn_coef) and self.channels % 4:
            raise ValueError('GATConv: channels must be a multiple of 4 for attn_heads > 1 or return_attn_coef, got %d' % self.channels)
        self.dropout_rate, self.add_self_loops = dropout_rate, add_self_loops
        self.activation, self.use_bias = activation or 'linear', use_bias
        self._gen, self._packs = generator, PackCache()
        self._graphs = _GraphArg()
        self.precision = 'fp32'      # numerics of the backward row GEMMs (the forward linear part is the exact kernel)
        # True: the single-head layer's backward is one uds_gat_backward_act call (activation, attention / aggregation, bias and
        # attention-kernel gradients); False: the chain of separate steps.  The forward pass is the same.
        self.fused_backward = False
        self.kernel = self.attn_kernel_self = self.attn_kernel_neighs = self.bias = None
        if in_channels is not None:
            self.build(in_channels, 'cpu')

    @property
    def output_dim(self):
        return self.channels * self.attn_heads if self.concat_heads else self.channels

    def build(self, in_channels, device):
        c, nh = self.channels, self.attn_heads
        self.kernel = _param(_glorot_uniform((int(in_channels), nh, c), device, self._gen))
        self.attn_kernel_self = _param(_glorot_uniform((c, nh, 1), device, self._gen))
        self.attn_kernel_neighs = _param(_glorot_uniform((c, nh, 1), device, self._gen))
        self.bias = _param(torch.zeros(self.output_dim, device=device)) if self.use_bias else None

    def dense_attn_coef(self, attn, a):
        """attn (..., H, nnz) as forward returns it -> Spektral's dense (..., N, H, N) coefficients (zero off the pattern of
        `a`); for small graphs."""
        h = self._graphs.handle(a, self.add_self_loops)
        rows = torch.as_tensor(np.repeat(np.arange(h.n_rows), np.diff(h._rowptr.astype(np.int64))), device=attn.device)
        cols = torch.as_tensor(h._col.astype(np.int64), device=attn.device)
        dense = attn.new_zeros(tuple(attn.shape[:-1]) + (h.n_rows, h.n_cols))
        dense[..., rows, cols] = attn
        return dense.transpose(-3, -2).contiguous()

    def _forward_heads(self, xs, xbs, h, lead, edge_mask, attn_dropout, want_attn):
        """attn_heads > 1, the mean over heads or return_attn_coef: uds_gat_aggregate_heads, under autograd GatHeadsFn."""
        nh = self.attn_heads
        coef = None
        if attn_dropout is not None and self.dropout_rate:      # one multiplier per (snapshot, head, pattern entry)
            ones = torch.ones((xs.shape[0], nh, h.nnz), device=xs.device, dtype=torch.float32)
            coef = _lib.dropout(ones, self.dropout_rate, attn_dropout.seed, attn_dropout.take(ones.numel()))
        mk = None if edge_mask is None else edge_mask.reshape(-1, edge_mask.shape[-1]).to(torch.float32).contiguous()
        if coef is not None or _ag.grad_on(xs, xbs, self.kernel, self.attn_kernel_self, self.attn_kernel_neighs, self.bias):
            out, alpha = _ag.GatHeadsFn.apply(xs, xbs, self.kernel, self.attn_kernel_self, self.attn_kernel_neighs, self.bias,
                                              self.activation, h, self.precision, self.concat_heads, coef, mk, want_attn)
        else:
            out, alpha, _ = _ag.gat_heads_forward(xs, xbs, self.kernel, self.attn_kernel_self, self.attn_kernel_neighs, self.bias,
                                                  self.activation, h, self.concat_heads, coef, mk, want_attn)
        out = out.reshape(lead + out.shape[-2:])
        return (out, alpha.reshape(lead + alpha.shape[-2:])) if want_attn else out

    def forward(self, inputs, xb=None, edge_mask=None, attn_dropout=None, return_attn_coef=None):
        """edge_mask (..., nnz): per-snapshot 0/1 over the entries of the pattern `a` (`use_adj`, emulator.py:268-271: the
        reference feeds a (S, N, N) adjacency here; the mask is that adjacency gathered at the static pattern's entries --
        `Emulator.get_adj_action`).  The diagonal always takes part (set_diag).  Under autograd or with attention dropout the
        layer runs on GatFn (uds_gat_aggregate_ex / uds_gat_backward_ex); otherwise on the inference kernel.
        attn_dropout: a DropoutStream = the layer runs in Keras' training mode and `dropout_rate` > 0: Spektral's dropout on the
        normalised attention coefficients (`attn_coef_drop = self.dropout(attn_coef)`), one mask entry per (snapshot, pattern entry)
        and, with attn_heads = H > 1, per head: S * H * nnz positions of the stream.
        With an edge mask the draw still covers every entry of the static pattern, masked or not (S * nnz values, the order
        and count of the unmasked layer), so the stream stays aligned with a model built without `use_adj`.
        return_attn_coef: overrides the constructor's setting for this call (True: return (out, attn))."""
        x, a = inputs
        if self.kernel is None:
            self.build(x.shape[-1] + (0 if xb is None else xb.shape[-1]), x.device)
        h = self._graphs.handle(a, self.add_self_loops)
        xs, lead = _flatten_snapshots(x)
        xbs = None if xb is None else _flatten_snapshots(xb)[0]
        want_attn = self.return_attn_coef if return_attn_coef is None else bool(return_attn_coef)
        if self.attn_heads > 1 or want_attn:
            return self._forward_heads(xs, xbs, h, lead, edge_mask, attn_dropout, want_attn)
        coef = None
        if attn_dropout is not None and self.dropout_rate:
            ones = torch.ones((xs.shape[0], h.nnz), device=xs.device, dtype=torch.float32)
            coef = _lib.dropout(ones, self.dropout_rate, attn_dropout.seed, attn_dropout.take(ones.numel()))
        mk = None if edge_mask is None else edge_mask.reshape(-1, edge_mask.shape[-1]).to(torch.float32).contiguous()
        fin = xs.shape[-1] + (0 if xbs is None else xbs.shape[-1])
        if coef is not None or _ag.grad_on(xs, xbs, self.kernel, self.attn_kernel_self, self.attn_kernel_neighs, self.bias):
            out = _ag.GatFn.apply(xs, xbs, self.kernel, self.attn_kernel_self, self.attn_kernel_neighs, self.bias,
                                  self.activation, h, self.precision, coef, mk, self.fused_backward)
        elif mk is not None:
            hx, s_self, s_nbr = _lib.dense_act(xs, self.kernel.reshape(fin, self.channels), None, 'linear', xbs,
                                               attn=(self.attn_kernel_self.reshape(-1), self.attn_kernel_neighs.reshape(-1)))
            out = _lib.gat_aggregate(h, hx, s_self, s_nbr, self.bias, self.activation, edge_mask=mk)
        elif self.precision == 'bf16x3' and fin % 32 == 0 and self.channels % 16 == 0 and xs.shape[0] * xs.shape[1] >= 4096:
            # wide layers (d = 128, the reference's default): the linear part on the matrix cores (split-bf16 row GEMM, 64
            # columns per launch), the attention projections as two matrix-vector products, then the CSR aggregation kernel
            w2 = self.kernel.reshape(fin, self.channels)

            def build():
                # per parameter version: the kernel's 64-column blocks and the two attention projections W a_self, W a_nbr
                # (s = hx a = z (W a): one more narrow row GEMM instead of a 600k-row matrix-vector product)
                cols = [_lib.rowgemm_pack(w2[:, c0:c0 + 64].contiguous()) for c0 in range(0, self.channels, 64)]
                wa = torch.stack([w2 @ self.attn_kernel_self.reshape(-1), w2 @ self.attn_kernel_neighs.reshape(-1)], dim=1)
                return cols, _lib.rowgemm_pack(wa.contiguous())
            cols, wa_packed = self._packs.get('wide', (self.kernel, self.attn_kernel_self, self.attn_kernel_neighs), build)
            if not all(_lib.rowgemm_supported(fin, 32, min(64, self.channels - 64 * i)) for i in range(len(cols))):
                raise _lib.UdsError('GATConv: %d -> %d does not fit the matrix-core row GEMM' % (fin, self.channels))
            hx = torch.empty(xs.shape[:-1] + (self.channels,), device=xs.device, dtype=torch.float32)
            for i, pk in enumerate(cols):
                _lib.rowgemm_cat(xs, xbs, pk, None, min(64, self.channels - 64 * i), 'linear', out=hx, col0=64 * i)
            s2 = _lib.rowgemm_cat(xs, xbs, wa_packed, None, 2, 'linear')
            s_self, s_nbr = s2[..., 0].contiguous(), s2[..., 1].contiguous()
            out = _lib.gat_aggregate(h, hx, s_self, s_nbr, self.bias, self.activation)
        else:
            out = _lib.gat_forward(h, xs, self.kernel, self.attn_kernel_self, self.attn_kernel_neighs, self.bias,
                                   self.activation, xbs)
        return out.reshape(lead + out.shape[-2:])


MixedGAT = GATConv   # emulator.py:18-25: only re-types the (inactive) attention dropout


class GCNConv(nn.Module):
    """spektral.layers.GCNConv: act(a_hat @ (x @ kernel) + bias); a_hat = GCNConv.preprocess(adj)."""

    def __init__(self, channels, activation=None, use_bias=True, in_channels=None, generator=None):
        super().__init__()
        self.channels, self.activation, self.use_bias = int(channels), activation or 'linear', use_bias
        self.units, self.precision = self.channels, 'fp32'      # what autograd.DenseFn reads from its module (exact-fp32 kernels)
        self._gen = generator
        self._cache = {}
        self.kernel = self.bias = None
        if in_channels is not None:
            self.build(in_channels, 'cpu')

    @staticmethod
    def preprocess(adj):
        """gcn_filter: D^-1/2 (A + I) D^-1/2, row-sum degrees, inf -> 0 (`emulator.py:133`).  A square `graph.CSR` (values, or
        ones when it has none) gives a `graph.CSR` with the normalised values on the pattern of A united with the diagonal."""
        if isinstance(adj, CSR):
            n = adj.n_rows
            val = np.ones(adj.nnz) if adj.val is None else np.asarray(adj.val, dtype=np.float64)
            rows, cols = adj.rows(), adj.col.astype(np.int64)
            diag = rows == cols
            miss = np.setdiff1d(np.arange(n, dtype=np.int64), rows[diag])            # rows whose diagonal A does not store
            from .graph import _csr_from_pairs
            ai = _csr_from_pairs(np.concatenate([rows, miss]), np.concatenate([cols, miss]), n, adj.n_cols,
                                 np.concatenate([val + diag, np.ones(miss.shape[0])]))
            rows, cols = ai.rows(), ai.col.astype(np.int64)
            deg = np.bincount(rows, weights=ai.val, minlength=n)
            with np.errstate(divide='ignore'):
                dinv = np.power(deg, -0.5)
            dinv[np.isinf(dinv)] = 0.0
            return CSR(ai.rowptr, ai.col, n, adj.n_cols, dinv[rows] * ai.val * dinv[cols])
        a = np.asarray(adj, dtype=np.float64) + np.eye(len(adj))
        deg = a.sum(axis=1)
        with np.errstate(divide='ignore'):
            dinv = np.power(deg, -0.5)
        dinv[np.isinf(dinv)] = 0.0
        return dinv[:, None] * a * dinv[None, :]

    def build(self, in_channels, device):
        self.kernel = _param(_glorot_uniform((int(in_channels), self.channels), device, self._gen))
        self.bias = _param(torch.zeros(self.channels, device=device)) if self.use_bias else None

    def _filter(self, a, device):
        hit = self._cache.get(id(a))
        if hit is not None and hit[0] is a:
            return hit[1], hit[2]
        if isinstance(a, CSR):
            if a.val is None:
                raise ValueError('GCNConv: a CSR filter must carry its values (GCNConv.preprocess(csr))')
            csr = a
        else:
            dense = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            csr = csr_from_dense(dense, keep_values=True)
        h = _lib.CsrHandle(csr)
        val = torch.as_tensor(csr.val, dtype=torch.float32, device=device)
        self._cache[id(a)] = (a, h, val)
        return h, val

    def forward(self, inputs):
        x, a = inputs
        if self.kernel is None:
            self.build(x.shape[-1], x.device)
        h, val = self._filter(a, x.device)
        xs, lead = _flatten_snapshots(x)
        if _ag.grad_on(x, self.kernel, self.bias):
            # training: x @ kernel and the propagation a_hat @ (.) through their autograd Functions (the filter values are
            # constants: no gradient), bias + activation as tensor ops
            hx = _ag.DenseFn.apply(xs, self.kernel, None, self, 'linear')
            out = _ag.SpmmFn.apply(val, hx, h)
            if self.bias is not None:
                out = out + self.bias
            out = _ag.apply_activation(out, self.activation)
            return out.reshape(lead + out.shape[-2:])
        hx = _lib.dense_act(xs, self.kernel, None, 'linear')
        out = _lib.csr_spmm(h, val, hx, self.bias, self.activation)
        return out.reshape(lead + out.shape[-2:])


class DiffusionConv(nn.Module):
    """spektral.layers.DiffusionConv(channels, K=6, activation='tanh') as the reference runs it (`emulator.py:135-138,229`:
    dense mixed mode, `net(embed_size, activation=...)([x, filter])`): `channels` DiffuseFeatures filters with K + 1
    coefficients each -- `kernel` (channels, K + 1), row q = theta_q, highest power first, glorot_uniform -- and
        out[..., q] = act( reduce_sum( polyval(theta_q, a_hat) @ x, -1 ) ),     no bias,
    where tf.math.polyval is Horner's rule on the ENTRIES of a_hat (element-wise powers).  A zero entry of a_hat therefore
    takes the constant coefficient theta_q[K]; with r = x.sum(-1) the dense (N, N) product collapses to the support of a_hat
    plus a rank-one term (uds_diffusion_forward).  a_hat = DiffusionConv.preprocess(adj): a dense array, or a `graph.CSR`
    carrying its values (no N x N array on the host).  Training: `autograd.DiffusionFn` (uds_diffusion_backward gives d r and
    d kernel; the feature sum r = x.sum(-1) stays a torch op in front, its backward broadcasts d r over the features).

    Two forms of the same layer (same parameters, names and shapes).  The table form (the default) prepares
    vals[p, q] = polyval(theta_q, a_p) - c0_q, (nnz, C), once per parameter version and the kernels read it per snapshot.
    `moments=True` never builds it: uds_diffusion_forward_m / uds_diffusion_backward_m expand the polynomial per row from the
    (nnz,) support values and `kernel` (`autograd.DiffusionMomentsFn`).  The caller that builds the layer picks the form from
    what it was given: SpatialLayer / GraphBaseBlock pass moments=True when their filter is a `graph.CSR` (a model built from
    `args.graph`, where nnz * C floats per layer is what does not fit).  `moments` is an argument of whoever constructs the layer:
    no `args` key or model option reaches it."""

    def __init__(self, channels, K=6, activation='tanh', in_channels=None, generator=None, moments=False):
        super().__init__()
        self.channels, self.K, self.activation = int(channels), int(K) + 1, activation or 'linear'      # spektral: self.K = K + 1
        if self.channels % 4:
            raise ValueError('DiffusionConv: channels must be a multiple of 4, got %d' % self.channels)
        lim = math.sqrt(6.0 / (2 * self.K))         # glorot_uniform on shape (K + 1,): fan_in = fan_out = K + 1
        self.kernel = _param((torch.rand((self.channels, self.K), generator=generator) * 2 - 1) * lim)
        self._cache, self._packs = {}, PackCache()
        self.moments = bool(moments)

    @staticmethod
    def preprocess(adj):
        """normalized_adjacency: D^-1/2 A D^-1/2 (no self loops added), row-sum degrees, inf -> 0 (`emulator.py:137-138`).
        A square `graph.CSR` (values, or ones when it has none) gives a `graph.CSR` with the normalised values."""
        if isinstance(adj, CSR):
            val = np.ones(adj.nnz) if adj.val is None else np.asarray(adj.val, dtype=np.float64)
            rows, cols = adj.rows(), adj.col.astype(np.int64)
            deg = np.bincount(rows, weights=val, minlength=adj.n_rows)
            with np.errstate(divide='ignore'):
                dinv = np.power(deg, -0.5)
            dinv[np.isinf(dinv)] = 0.0
            return CSR(adj.rowptr, adj.col, adj.n_rows, adj.n_cols, dinv[rows] * val * dinv[cols])
        a = np.asarray(adj, dtype=np.float64)
        deg = a.sum(axis=1)
        with np.errstate(divide='ignore'):
            dinv = np.power(deg, -0.5)
        dinv[np.isinf(dinv)] = 0.0
        return dinv[:, None] * a * dinv[None, :]

    def _filter(self, a, device):
        hit = self._cache.get(id(a))
        if hit is None or hit[0] is not a:
            if isinstance(a, CSR):
                if a.val is None:
                    raise ValueError('DiffusionConv: a CSR filter must carry its values (DiffusionConv.preprocess(csr))')
                csr = a
            else:
                dense = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
                csr = csr_from_dense(dense, keep_values=True)
            hit = self._cache[id(a)] = (a, _lib.CsrHandle(csr), torch.as_tensor(csr.val, dtype=torch.float32, device=device))
        if self.moments:
            return hit[1], None, None, hit[2]

        def build():
            av = hit[2].double()[:, None]
            th = self.kernel.detach().double()
            v = th[:, 0].expand(av.shape[0], -1)
            for k in range(1, self.K):                       # Horner, as tf.math.polyval
                v = v * av + th[:, k]
            return (v - th[:, -1]).float().contiguous(), th[:, -1].float().contiguous()
        vals, c0 = self._packs.get('table', (self.kernel,), build, extra=(id(a),))
        return hit[1], vals, c0, hit[2]

    def forward(self, inputs):
        x, a = inputs
        h, vals, c0, a_sup = self._filter(a, x.device)
        xs, lead = _flatten_snapshots(x)
        r = xs.sum(dim=-1)
        if self.moments:
            if _ag.grad_on(x, self.kernel):
                out = _ag.DiffusionMomentsFn.apply(r, self.kernel, h, a_sup, self.activation)
            else:
                out = _lib.diffusion_forward_m(h, a_sup, self.kernel.detach().contiguous(), r.contiguous(), r.sum(dim=-1).contiguous(),
                                               self.activation)
            return out.reshape(lead + out.shape[-2:])
        if _ag.grad_on(x, self.kernel):
            out = _ag.DiffusionFn.apply(r, self.kernel, h, a_sup, vals, c0, self.activation)
            return out.reshape(lead + out.shape[-2:])
        out = _lib.diffusion_forward(h, vals, c0, r.contiguous(), r.sum(dim=-1).contiguous(), self.activation)
        return out.reshape(lead + out.shape[-2:])


class NodeEdge(nn.Module):
    """`NodeEdge(inci)` (`emulator.py:27-45`): out = (weight * inci + bias) @ x, inci (R, M).

    `weight`, `bias` keep the reference's dense (R, M) shape by default.  The product is evaluated on
    the incidence support with the CSR kernel; a trained `bias` that is non-zero OFF the support makes
    the matrix genuinely dense, and that remainder is added by the hand-written split-bf16 MFMA GEMM
    (`remainder`: uds_remainder_forward; the check is re-done whenever the parameters change).  For networks where an (R, M) parameter cannot exist
    (N = 50k: 13 GB each) pass sparse=True: parameters then have one entry per support element
    (columns ascending inside a row)."""

    # True: a dense-parameter layer trains as ONE autograd Function (autograd.NodeEdgeDenseFn: the whole matrix on the split-bf16
    # GEMM, d bias and d weight from uds_node_edge_wgrad) where _dense_train_ok allows; Emulator.dense_node_edge_train
    dense_train = False

    def __init__(self, inci, sparse=False, device='cpu', generator=None):
        super().__init__()
        if isinstance(inci, CSR):
            csr = inci if inci.val is not None else CSR(inci.rowptr, inci.col, inci.n_rows, inci.n_cols,
                                                        np.ones(inci.nnz))
        else:
            dense = inci.detach().cpu().numpy() if isinstance(inci, torch.Tensor) else np.asarray(inci)
            csr = csr_from_dense(dense, keep_values=True)
        self.csr = csr
        self.sparse = bool(sparse)
        self.shape = (csr.n_rows, csr.n_cols)
        rows = torch.as_tensor(csr.rows(), dtype=torch.int64)
        cols = torch.as_tensor(csr.col.astype(np.int64))
        self.register_buffer('_flat', rows * csr.n_cols + cols, persistent=False)
        self.register_buffer('_ival', torch.as_tensor(csr.val, dtype=torch.float32), persistent=False)
        shape = (csr.nnz,) if self.sparse else self.shape
        w = torch.randn(shape, generator=generator, dtype=torch.float32) * 0.05      # 'random_normal'
        self.weight = _param(w.to(device))
        self.bias = _param(torch.zeros(shape, device=device))
        self._handle, self._packs = None, PackCache()
        self.precision = 'bf16x3'      # of the dense remainder GEMM; SpatialLayer sets it to its own
        self.last_train_path = None    # 'dense' or 'support+remainder': what the last forward under autograd ran

    def support_values(self):
        """weight*inci + bias on the support (nnz,), plus the off-support remainder of bias or None."""
        def build():
            flat, ival = self._flat.to(self.weight.device), self._ival.to(self.weight.device)
            if self.sparse:
                val, rest = self.weight * ival + self.bias, None
            else:
                val = self.weight.reshape(-1)[flat] * ival + self.bias.reshape(-1)[flat]
                rest = self.bias.clone()
                rest.reshape(-1).index_fill_(0, flat, 0.0)      # (an indexed store of a Python scalar uploads it: not capturable)
                if self.weight.is_cuda and torch.cuda.is_current_stream_capturing():
                    # a capture cannot ask the device: Emulator._capture_fit_graph asked before it began (None: keep the remainder)
                    if getattr(self, '_capture_rest_none', None):
                        rest = None
                elif not bool((rest != 0).any()):
                    rest = None
            return val.contiguous(), rest
        return self._packs.get('values', (self.weight, self.bias), build)

    def _rest_pack(self):
        """bf16 hi/lo planes of the off-support remainder (callers have checked that there is one), split once per update."""
        return self._packs.get('rest', (self.weight, self.bias), lambda: _lib.remainder_pack(self.support_values()[1]))

    def remainder(self, xs, precision='bf16x3'):
        """`rest @ xs`, rest = the trained bias off the incidence support (emulator.py:36-39,44): the dense GEMM on the
        matrix cores (uds_remainder_forward; `rest` is split into bf16 hi/lo once per parameter update), exact fp32 through
        rocBLAS when precision='fp32'.  None when the bias is zero off the support."""
        rest = self.support_values()[1]
        if rest is None:
            return None
        if precision != 'bf16x3' or xs.shape[-1] % 4 or xs.shape[-1] > 64:
            return torch.matmul(rest, xs)
        return _lib.remainder_forward(self._rest_pack(), tuple(rest.shape), xs)

    def remainder_of_dense(self, es, dense):
        """`rest @ dense(es)` with the Dense layer's output written straight into the GEMM's operand planes (uds_remainder_forward_dense);
        None when the shapes are not the ones that entry takes -- the caller then materialises dense(es) and calls remainder()."""
        rest = self.support_values()[1]
        if rest is None or dense.precision != 'bf16x3' or es.shape[-1] not in (64, 128) or dense.units not in (32, 64) or not es.is_cuda \
                or rest.shape[1] < 64:      # (a 30-row network fills half of that kernel's 64-row blocks: the flattened row GEMM is the better Dense there)
            return None
        return _lib.remainder_forward_dense(self._rest_pack(), tuple(rest.shape), es.contiguous(), _packed_kernel(dense, dense.kernel), dense.bias,
                                            dense.activation, dense.units)

    def handle(self):
        if self._handle is None:
            self._handle = _lib.CsrHandle(self.csr)
        return self._handle

    def dense_incidence(self):
        """The incidence values as a dense (R, M) tensor on the parameters' device: built once per module (a non-persistent buffer)."""
        if '_inci_dense' not in self._buffers:
            dense = torch.zeros(self.shape, device=self._flat.device, dtype=torch.float32)
            dense.reshape(-1)[self._flat] = self._ival
            self.register_buffer('_inci_dense', dense, persistent=False)
        if self._inci_dense.device != self.weight.device:
            self._inci_dense = self._inci_dense.to(self.weight.device)
        return self._inci_dense

    def _dense_train_ok(self, xs):
        """The one-Function route (dense_train) takes dense (R, M) parameters that both train, at 'bf16x3', on the GPU, at an h
        uds_node_edge_wgrad and the GEMM take."""
        h = xs.shape[-1]
        return self.dense_train and not self.sparse and self.precision == 'bf16x3' and h % 4 == 0 and 4 <= h <= 64 and xs.is_cuda \
            and self.weight.is_cuda and self.weight.requires_grad and self.bias.requires_grad

    def forward(self, x):
        if x.shape[-2] != self.shape[1]:
            raise _lib.UdsError('NodeEdge expects %d elements on axis -2, got %r' % (self.shape[1], tuple(x.shape)))
        xs, lead = _flatten_snapshots(x)
        grad = _ag.grad_on(xs, self.weight, self.bias)
        if grad and self._dense_train_ok(xs):
            self.last_train_path = 'dense'      # the whole layer as one Function
            out = _ag.NodeEdgeDenseFn.apply(self.weight, self.bias, xs, self)
            return out.reshape(lead + out.shape[-2:])
        if grad:
            self.last_train_path = 'support+remainder'
            # training: the support values are re-derived under autograd (gradients reach `weight` and `bias`); with the
            # reference's dense (R, M) parameters the bias also trains OFF the support (emulator.py:36-39,44), which is
            # a dense GEMM and only feasible for small networks -- sparse=True keeps one trainable entry per support element
            flat, ival = self._flat.to(self.weight.device), self._ival.to(self.weight.device)
            if self.sparse:
                val = self.weight * ival + self.bias
                out = _ag.SpmmFn.apply(val, xs, self.handle())
            else:
                val = self.weight.reshape(-1)[flat] * ival + self.bias.reshape(-1)[flat]
                out = _ag.SpmmFn.apply(val, xs, self.handle())
                if self.bias.requires_grad:
                    off = torch.ones_like(self.bias)
                    off.reshape(-1).index_fill_(0, flat, 0.0)
                    rest = self.bias * off
                    if self.precision == 'bf16x3' and xs.shape[-1] % 4 == 0 and xs.shape[-1] <= 64:
                        out = out + _ag.RemainderFn.apply(rest, xs)      # the N x E x (S h) products on the HIP MFMA GEMM
                    else:
                        out = out + torch.matmul(rest, xs)
            return out.reshape(lead + out.shape[-2:])
        val, rest = self.support_values()
        out = _lib.csr_spmm(self.handle(), val, xs)
        if rest is not None:
            out = out + self.remainder(xs, self.precision)
        return out.reshape(lead + out.shape[-2:])


class SpatialLayer(nn.Module):
    """One iteration of the spatial-block loop (`emulator.py:225-230`, `:278-283`), conv = GAT:

        x_e = Dense(d/2, act)(e);  e_x = Dense(d/2, act)(x)
        x = concat[x, NodeEdge(|node_edge|)(x_e)];  e = concat[e, NodeEdge(|node_edge|^T)(e_x)]
        x = GAT(d, act)([x, Adj]);  e = GAT(d, act)([e, Eadj])

    forward(x, e): x (..., N, Fx), e (..., E, Fe) -> (..., N, d), (..., E, d).  Uses the fused C-ABI
    entry uds_spatial_layer_forward (concats are never materialised)."""

    # True: on the remainder routes, rest @ Dense(.) of both sides runs as one launch of the snapshot kernel
    # (uds_remainder_snapshot_pair: x_e stays in LDS) where uds_remainder_snapshot_plan accepts the network; Emulator.snapshot_remainder
    snapshot_remainder = False

    def __init__(self, graph, embed_size, activation='relu', fx=None, fe=None, sparse_params=None, net=None,
                 generator=None, precision='bf16x3', conv='GAT', filters=None, attn_heads=1):
        super().__init__()
        if conv not in ('GAT', 'GCN', 'Diffusion'):
            raise NotImplementedError('conv=%r: GAT, GCN and Diffusion are built' % (conv,))
        self.attn_heads = int(attn_heads)
        if self.attn_heads < 1 or int(embed_size) % (4 * self.attn_heads):
            raise ValueError('embed_size must be a multiple of 4 * attn_heads (heads of d / H channels, float4 rows), got d=%d, H=%d'
                             % (int(embed_size), self.attn_heads))
        if self.attn_heads > 1 and conv != 'GAT':
            raise ValueError('attn_heads=%d needs conv=GAT, got %r' % (self.attn_heads, conv))
        if conv != 'GAT' and filters is None:
            raise ValueError("conv=%r needs filters=(preprocess(adj), preprocess(edge_adj)) of its layer class" % (conv,))
        self.conv, self.filters = conv, filters
        if precision not in _lib.PRECISION_FLAGS:
            raise ValueError("precision must be 'bf16x3' (fused kernel, split-bf16 MFMA, fp32 accumulate) or 'fp32' "
                             "(exact-fp32 unfused kernels), got %r" % (precision,))
        self.precision = precision
        if not isinstance(graph, DrainageGraph):
            raise TypeError('graph must be a gnn_uds_amd.graph.DrainageGraph')
        self.graph, self.d, self.h, self.activation = graph, int(embed_size), int(embed_size) // 2, activation
        if self.d % 8:
            raise ValueError('embed_size must be a multiple of 8 (float4 rows of width d/2), got %d' % self.d)
        if sparse_params is None:
            sparse_params = graph.n_node * graph.n_edge > (1 << 24)
        fx = self.d if fx is None else int(fx)
        fe = self.d if fe is None else int(fe)
        g = generator
        self.dense_xe = Dense(self.h, activation, in_features=fe, generator=g, precision=precision)          # emulator.py:225
        self.dense_ex = Dense(self.h, activation, in_features=fx, generator=g, precision=precision)          # emulator.py:226
        abs_n = CSR(graph.inc_n.rowptr, graph.inc_n.col, graph.n_node, graph.n_edge, np.abs(graph.inc_n.val))
        abs_e = CSR(graph.inc_e.rowptr, graph.inc_e.col, graph.n_edge, graph.n_node, np.abs(graph.inc_e.val))
        self.node_edge_n = NodeEdge(abs_n, sparse=sparse_params, generator=g)           # emulator.py:227
        self.node_edge_e = NodeEdge(abs_e, sparse=sparse_params, generator=g)           # emulator.py:228
        self.node_edge_n.precision = self.node_edge_e.precision = precision
        if conv == 'GAT':
            # attn_heads = H > 1 (not a reference key): H heads of d / H channels, concatenated -- the same width d
            nh = self.attn_heads
            self.gat_x = GATConv(self.d // nh, attn_heads=nh, activation=activation, in_channels=fx + self.h, generator=g)   # :229
            self.gat_e = GATConv(self.d // nh, attn_heads=nh, activation=activation, in_channels=fe + self.h, generator=g)   # :230
            self.gat_x.precision = self.gat_e.precision = precision
        elif conv == 'GCN':
            self.gcn_x = GCNConv(self.d, activation=activation, in_channels=fx + self.h, generator=g)
            self.gcn_e = GCNConv(self.d, activation=activation, in_channels=fe + self.h, generator=g)
        else:
            # emulator.py:229-230 with net = DiffusionConv; CSR filters (a model built from args.graph): the table-free form
            self.gcn_x = DiffusionConv(self.d, activation=activation, generator=g, moments=isinstance(filters[0], CSR))
            self.gcn_e = DiffusionConv(self.d, activation=activation, generator=g, moments=isinstance(filters[1], CSR))
        self._net, self._packs = net, PackCache()
        self.last_path = None     # which kernels the last forward ran: 'fused', 'fused+remainder', 'unfused' (tests, bench)
        self.last_route = None    # ... and the row of the route table (`route`) it took
        self.last_remainder = None   # per side what computed the dense remainder: 'snapshot', 'gemm' or None (no remainder); None before
                                     # a forward on a remainder route
        self._ws_rem_ok = None    # override for tests: False sends a d = 64 remainder to 'rem-split96' whatever the plan says

    def _packed_weights(self, p, fx, fe, remainder=False):
        """(packed bf16 hi/lo fragments of the four GEMM kernels, the augmented kernels of the remainder variant or {})."""
        def build():
            if not remainder:
                return _lib.spatial_pack_weights(p, fx, fe, self.h, self.d), {}
            # a trained dense NodeEdge bias through the fused kernel's 96-wide split-input variant: the dense remainder
            # `rest @ x_e` (S, R, 32) rides in as the 32 extra input columns, multiplied by the SAME rows of the GAT kernel
            # as the CSR aggregate ([x | rem | agg] @ [Wx; Wagg; Wagg] = [x | agg + rem] @ [Wx; Wagg]); the in-kernel
            # secondary MLP must not see those columns: zero rows under its kernel
            z = torch.zeros((self.h, self.h), device=p['xe_k'].device)
            aug = dict(xe_k=torch.cat([p['xe_k'], z]), ex_k=torch.cat([p['ex_k'], z]),
                       gx_k=torch.cat([p['gx_k'], p['gx_k'][-self.h:]]), ge_k=torch.cat([p['ge_k'], p['ge_k'][-self.h:]]))
            return _lib.spatial_pack_weights(dict(p, **aug), fx, fe, self.h, self.d), aug
        return self._packs.get('weights', (self.dense_xe.kernel, self.dense_ex.kernel, self.gat_x.kernel, self.gat_e.kernel), build,
                               extra=(fx, fe, remainder))

    def network(self):
        if self._net is None:
            self._net = _lib.NetworkHandle(self.graph)
        return self._net

    PACK_ROWS = 128       # rows of a full tile of the fused kernels (csrc/tile_plan.hpp: p_limit)

    def pack_factor(self):
        """Snapshots of this network that share one tile of the fused kernel: a network of 30 nodes fills a quarter of a
        128-row tile, and a tile costs its workgroup the same time a quarter full or full, so k = 128 // rows
        snapshots are laid side by side as k disjoint copies of the network (DrainageGraph.replicated)."""
        rows = max(self.graph.n_node, self.graph.n_edge)
        return max(1, self.PACK_ROWS // rows) if rows <= self.PACK_ROWS // 2 else 1

    def _replica(self, k):
        if getattr(self, '_rep', None) is None or self._rep[0] != k:
            self._rep = (k, _lib.NetworkHandle(self.graph.replicated(k)))
        return self._rep[1]

    def export_params(self):
        """Parameters as CPU tensors under the key names of uds_spatial_params_t (NodeEdge as
        'ne_*_w'/'ne_*_b' when dense, 'ne_*_v' support values when sparse)."""
        c = lambda t: None if t is None else t.detach().cpu().clone()
        if self.conv != 'GAT':
            raise NotImplementedError('export_params covers the GAT layer')
        if self.attn_heads > 1:
            raise NotImplementedError('export_params covers the single-head layer (uds_spatial_params_t has one head); attn_heads=%d'
                                      % self.attn_heads)
        p = dict(xe_k=c(self.dense_xe.kernel), xe_b=c(self.dense_xe.bias), ex_k=c(self.dense_ex.kernel),
                 ex_b=c(self.dense_ex.bias),
                 gx_k=c(self.gat_x.kernel), gx_as=c(self.gat_x.attn_kernel_self), gx_an=c(self.gat_x.attn_kernel_neighs),
                 gx_b=c(self.gat_x.bias),
                 ge_k=c(self.gat_e.kernel), ge_as=c(self.gat_e.attn_kernel_self), ge_an=c(self.gat_e.attn_kernel_neighs),
                 ge_b=c(self.gat_e.bias))
        for tag, ne in (('n', self.node_edge_n), ('e', self.node_edge_e)):
            if ne.sparse:
                p['ne_%s_v' % tag] = c(ne.support_values()[0])
            else:
                p['ne_%s_w' % tag], p['ne_%s_b' % tag] = c(ne.weight), c(ne.bias)
        return p

    # route -> (last_path, the method that runs it)
    ROUTES = {'chain': ('unfused', '_chain'), 'conv': ('unfused', '_conv'), 'entry': ('unfused', '_entry'),
              'fused': ('fused', '_fused'), 'fused-tiled': ('fused', '_fused_tiled'),
              'rem-ws': ('fused+remainder', '_fused_rem'), 'rem-d128': ('fused+remainder', '_fused_rem'),
              'rem-split96': ('fused+remainder', '_rem_split96')}

    def route(self, fx, fxb, fe, feb, S, plan_bits, adj_mask=False, attn_coef=False, attn_dropout=False, grad=False,
              remainder=False):
        """Which kernels a forward runs -> (route, split): a key of ROUTES, and whether xb / eb stay separate tensors (only
        'fused' reads split rows; every other route concatenates).  Plain values in, no tensor, no launch, no side effect:
        fx, fxb, fe, feb: widths of x, xb, e, eb (0 = absent); S: snapshots; plan_bits(fx, fe): info8[0] of
        uds_network_plan_info once the plans for those widths are built; adj_mask / attn_coef / attn_dropout: asked for;
        grad: autograd records for an operand or parameter; remainder: a NodeEdge bias is non-zero off the support.
        First match wins (widths are the concatenated ones, bf16x3 unless said):

          1   adj_mask, attn_heads > 1 or attn_coef (GAT only)                          chain
          2   conv is GCN / Diffusion                                                   conv
          3   attn_dropout or grad                                                      chain
          4a  remainder, d = 64, 64 / 64, plan bit 32 and _ws_rem_ok is not False       rem-ws
          4a' as 4a without the bit, or overridden                                      rem-split96
          4b  remainder, d = 128, fx = 128, fe = 128 with bit 8 / fe = 64 with bit 16   rem-d128
          4c  remainder, anything else                                                  chain
          5a  d = 64, fx and fe in {64, 96}; split iff every given piece is 64 + 32     fused
          5b  d = 128, fx = 128, fe = 128 with bit 8 / fe = 64 with bit 16              fused
          5c  fx, fe multiples of 32, h, d multiples of 16, S * N >= 4096               chain
          5d  everything left (fp32, d = 8, ...): the C entry without packed weights    entry

        5a / 5b with pack_factor() = k > 1 and S >= 16 k: fused-tiled (k snapshots per tile; a handful of snapshots -- the
        rollout's windows -- stay one launch).  4b: the launch refuses plans with p_cap > 64 with an error, not a fallback.
        5a does not look at plan bits 1 / 2 / 4: on a network whose d = 64 plan does not fit the LDS the C entry composes the
        layer unfused and last_path still says 'fused'."""
        if adj_mask or self.attn_heads > 1 or attn_coef:
            if self.conv != 'GAT':
                raise NotImplementedError('use_adj and return_attn_coef are built for conv=GAT (GCN / Diffusion would re-normalise '
                                          'the filter per snapshot and have no coefficients)')
            return 'chain', False
        if self.conv != 'GAT':
            return 'conv', False
        if attn_dropout or grad:
            return 'chain', False
        d64 = self.precision == 'bf16x3' and (self.h, self.d) == (32, 64)
        d128 = self.precision == 'bf16x3' and (self.h, self.d) == (64, 128)
        pieces = ((fx, fxb), (fe, feb))
        fx, fe = fx + fxb, fe + feb
        if remainder:
            if d64 and (fx, fe) == (64, 64):
                return ('rem-ws' if self._ws_rem_ok is not False and plan_bits(64, 64) & 32 else 'rem-split96'), False
            if d128 and fx == 128 and fe in (64, 128) and plan_bits(128, fe) & (8 if fe == 128 else 16):
                return 'rem-d128', False
            return 'chain', False
        if (d64 and fx in (64, 96) and fe in (64, 96)) or \
                (d128 and fx == 128 and fe in (64, 128) and plan_bits(128, fe) & (8 if fe == 128 else 16)):
            k = self.pack_factor()
            split = d64 and bool(fxb or feb) and all(b == 0 or (a, b) == (64, 32) for a, b in pieces)
            return ('fused-tiled' if k > 1 and S >= 16 * k else 'fused'), split
        if self.precision == 'bf16x3' and fx % 32 == 0 and fe % 32 == 0 and self.h % 16 == 0 and self.d % 16 == 0 \
                and S * self.graph.n_node >= 4096:
            return 'chain', False
        return 'entry', False

    def forward(self, x, e, xb=None, eb=None, adj_mask=None, attn_dropout=None, return_attn_coef=False):
        """xb / eb: extra columns appended to x / e (`concat([x, b])`, emulator.py:260-262) -- 32 on a 64-wide x / e are
        read in place by the fused kernel; every other route concatenates.  adj_mask (..., nnz of the node adjacency): the
        per-snapshot adjacency of `use_adj` (emulator.py:268-271,282) -- node side through the masked aggregation kernels.
        attn_dropout: a DropoutStream = Keras' training mode for the two GATConv layers (Spektral's attention dropout, rate 0.5).
        return_attn_coef: also return (alpha_x, alpha_e), (..., H, nnz) of the node and link adjacency (GAT only).
        `route` picks the kernels (its docstring is the table); last_route / last_path say what this call ran."""
        xs, lead_x = _flatten_snapshots(x)
        es, lead_e = _flatten_snapshots(e)
        xbs = None if xb is None else _flatten_snapshots(xb)[0]
        ebs = None if eb is None else _flatten_snapshots(eb)[0]
        grad = _ag.grad_on(x, e, xb, eb, *self.parameters())
        # per side (support values, off-support remainder or None), read once per call; support_values caches what it derives,
        # so it is not asked while autograd records
        ne = None if grad else (self.node_edge_n.support_values(), self.node_edge_e.support_values())
        remainder = ne is not None and (ne[0][1] is not None or ne[1][1] is not None)
        route, split = self.route(xs.shape[-1], 0 if xbs is None else xbs.shape[-1], es.shape[-1], 0 if ebs is None else ebs.shape[-1],
                                  xs.shape[0], lambda fx, fe: self.network().fused_bits(fx, fe), adj_mask is not None,
                                  bool(return_attn_coef), attn_dropout is not None, grad, remainder)
        if not split:
            xs = xs if xbs is None else torch.cat([xs, xbs], dim=-1)
            es = es if ebs is None else torch.cat([es, ebs], dim=-1)
            xbs = ebs = None
        self.last_route, (self.last_path, run) = route, self.ROUTES[route]
        self.last_remainder = (None, None)      # the remainder routes say what they ran (_remainders)
        if route == 'chain':
            ox, oe = self._chain(xs, es, adj_mask, attn_dropout, return_attn_coef)
        else:
            ox, oe = getattr(self, run)(ne, xs, es, xbs, ebs)
        back = lambda t, lead: t.reshape(lead + t.shape[-2:])
        if return_attn_coef:
            (ox, ax), (oe, ae) = ox, oe
            return back(ox, lead_x), back(oe, lead_e), (back(ax, lead_x), back(ae, lead_e))
        return back(ox, lead_x), back(oe, lead_e)

    def _chain(self, xs, es, adj_mask=None, attn_dropout=None, return_attn_coef=False):
        """The unfused composition Dense -> NodeEdge -> GAT: every operator its own launch, under autograd each with its own
        HIP backward (autograd.py); wide layers run their dense parts on the matrix cores (GATConv.forward).
        Attention-dropout draws: gat_x, then gat_e."""
        net = self.network()
        x_e, e_x = self.dense_xe(es), self.dense_ex(xs)
        ox = self.gat_x([xs, net.adj], xb=self.node_edge_n(x_e), edge_mask=adj_mask, attn_dropout=attn_dropout,
                        return_attn_coef=return_attn_coef)
        oe = self.gat_e([es, net.edge_adj], xb=self.node_edge_e(e_x), attn_dropout=attn_dropout, return_attn_coef=return_attn_coef)
        return ox, oe

    def _conv(self, ne, xs, es, xbs=None, ebs=None):
        """GCN a_hat @ ([x | agg] W) + b, or Diffusion: unfused composition of the Dense / NodeEdge / sparse kernels."""
        x_e, e_x = self.dense_xe(es), self.dense_ex(xs)
        ox = self.gcn_x([torch.cat([xs, self.node_edge_n(x_e)], dim=-1), self.filters[0]])
        oe = self.gcn_e([torch.cat([es, self.node_edge_e(e_x)], dim=-1), self.filters[1]])
        return ox, oe

    def _params(self, ne, fx=None, fe=None):
        """The tensors of uds_spatial_params_t; with widths, also the packed weights of the fused kernel for them (split once
        per parameter update, not per call) and the network's tile plans (those of the 96-wide variants are built on first use)."""
        xe, ex, gx, ge = self.dense_xe, self.dense_ex, self.gat_x, self.gat_e
        p = dict(xe_k=xe.kernel, xe_b=xe.bias, ex_k=ex.kernel, ex_b=ex.bias, ne_n_val=ne[0][0], ne_e_val=ne[1][0],
                 gx_k=gx.kernel, gx_as=gx.attn_kernel_self, gx_an=gx.attn_kernel_neighs, gx_b=gx.bias,
                 ge_k=ge.kernel, ge_as=ge.attn_kernel_self, ge_an=ge.attn_kernel_neighs, ge_b=ge.bias)
        if fx is not None:
            p['packed'] = self._packed_weights(p, fx, fe)[0]
            self.network().prepare(fx, fe)
        return p

    def _launch(self, net, p, xs, es, **pieces):
        return _lib.spatial_layer_forward(net, p, xs, es, self.h, self.d, self.activation, _lib.PRECISION_FLAGS[self.precision], **pieces)

    def _entry(self, ne, xs, es, xbs=None, ebs=None):
        return self._launch(self.network(), self._params(ne), xs, es)

    def _fused(self, ne, xs, es, xbs, ebs):
        p = self._params(ne, xs.shape[-1] + (0 if xbs is None else 32), es.shape[-1] + (0 if ebs is None else 32))
        return self._launch(self.network(), p, xs, es, xb=xbs, eb=ebs)

    def _fused_tiled(self, ne, xs, es, xbs, ebs):
        """Small network: k snapshots per tile.  (S, N, F) -> (S / k, k N, F) is a view; the NodeEdge values repeat per copy."""
        fx, fe = xs.shape[-1] + (0 if xbs is None else 32), es.shape[-1] + (0 if ebs is None else 32)
        p, k, S = self._params(ne, fx, fe), self.pack_factor(), xs.shape[0]
        N, E, Sm = self.graph.n_node, self.graph.n_edge, S // k * k
        rep = self._replica(k)
        rep.prepare(fx, fe)
        pk = dict(p, ne_n_val=p['ne_n_val'].repeat(k), ne_e_val=p['ne_e_val'].repeat(k))
        v = lambda t, R: None if t is None else t[:Sm].reshape(Sm // k, k * R, t.shape[-1])
        ox, oe = self._launch(rep, pk, v(xs, N), v(es, E), xb=v(xbs, N), eb=v(ebs, E))
        ox, oe = ox.reshape(Sm, N, self.d), oe.reshape(Sm, E, self.d)
        if Sm < S:     # the last S mod k snapshots one per tile
            t = lambda a: None if a is None else a[Sm:].contiguous()
            rx, re = self._launch(self.network(), p, t(xs), t(es), xb=t(xbs), eb=t(ebs))
            ox, oe = torch.cat([ox, rx]), torch.cat([oe, re])
        return ox, oe

    def _remainders(self, ne, xs, es):
        """rest_n @ Dense_xe(es), rest_e @ Dense_ex(xs) (zeros for a side without a remainder): the Dense outputs exist only
        for these products (the fused kernel has its own secondary MLP), so they go straight into the GEMM's operand planes
        (uds_remainder_forward_dense) when the shapes allow and UDS_REMAINDER_MATERIALISE is unset; else they are materialised first.
        With snapshot_remainder set (and UDS_REMAINDER_MATERIALISE unset) both products are ONE launch that keeps the Dense output in
        LDS (_snapshot_remainders) where uds_remainder_snapshot_plan accepts the network.  last_remainder says per side what ran."""
        direct = not os.environ.get('UDS_REMAINDER_MATERIALISE')
        sides = ((ne[0], self.node_edge_n, self.dense_xe, es, xs.shape[1]), (ne[1], self.node_edge_e, self.dense_ex, xs, es.shape[1]))
        snap = self._snapshot_remainders(sides) if self.snapshot_remainder and direct else None
        self.last_remainder = tuple(None if rest is None else ('gemm' if snap is None else 'snapshot') for (_, rest), *_ in sides)
        if snap is not None:
            return [torch.zeros((xs.shape[0], rows, self.h), device=xs.device, dtype=torch.float32) if rem is None else rem
                    for rem, (*_, rows) in zip(snap, sides)]
        rems = []
        for (_, rest), layer, dense, src, rows in sides:
            if rest is None:
                rem = torch.zeros((xs.shape[0], rows, self.h), device=xs.device, dtype=torch.float32)
            else:
                rem = layer.remainder_of_dense(src, dense) if direct else None
                if rem is None:
                    rem = layer.remainder(dense(src))
            rems.append(rem)
        return rems

    def _snapshot_remainders(self, sides):
        """The sides that have a remainder in ONE launch with x_e kept on chip (uds_remainder_snapshot_pair) -> per side the
        remainder or None; None when a side's shape is not one uds_remainder_snapshot_plan accepts (the caller keeps the GEMM path)."""
        args = []
        for (_, rest), layer, dense, src, _ in sides:
            if rest is None:
                args.append(None)
                continue
            F, h = src.shape[-1], dense.units
            if dense.precision != 'bf16x3' or F not in (64, 128) or h not in (32, 64) or not src.is_cuda \
                    or not _lib.remainder_snapshot_plan(rest.shape[0], rest.shape[1], F, h)['G']:
                return None
            args.append((layer._rest_pack(), tuple(rest.shape), src.contiguous(), _packed_kernel(dense, dense.kernel), dense.bias,
                         dense.activation, h))
        live = [a for a in args if a is not None]
        if len(live) == 2 and (live[0][2].shape[-1] != live[1][2].shape[-1] or live[0][5] != live[1][5]):
            return None
        return _lib.remainder_snapshot_pair(*args)

    def _fused_rem(self, ne, xs, es, xbs=None, ebs=None):
        """A trained dense NodeEdge bias (every checkpoint the reference trains, emulator.py:36-45): the dense remainder on the
        MFMA GEMM, added to the NodeEdge aggregate inside the fused kernel (uds_spatial_layer_forward_rem) -- the wave-specialised
        one at d = 64, the column-split one at d = 128."""
        rem_n, rem_e = self._remainders(ne, xs, es)
        return self._launch(self.network(), self._params(ne, xs.shape[-1], es.shape[-1]), xs, es, rem_x=rem_n, rem_e=rem_e)

    def _rem_split96(self, ne, xs, es, xbs=None, ebs=None):
        """d = 64 on a tile plan the wave-specialised kernel cannot hold: the remainder rides into the 96-wide split-input
        kernel as 32 extra input columns (_packed_weights)."""
        p = self._params(ne)
        rem_n, rem_e = self._remainders(ne, xs, es)
        packed, aug = self._packed_weights(p, 96, 96, remainder=True)
        self.network().prepare(96, 96)
        return self._launch(self.network(), dict(p, packed=packed, **aug), xs, es, xb=rem_n, eb=rem_e)


class GraphBaseBlock(nn.Module):
    """The spatial block of the `graph_base` variants (`emulator.py:220-223,273-276`): ONE graph over the N nodes and the
    E links (`get_node_based_adj` / `get_edge_based_adj`), one conv per layer over `concat([x, e], axis=-2)`, split back into
    node and link rows.  `filt`: the combined (N+E) x (N+E) pattern as a `graph.CSR` with self loops (GAT), or the normalised
    filter of GCN / Diffusion: dense, or a `graph.CSR` with values (then the Diffusion layers run their table-free form)."""

    def __init__(self, n_node, n_edge, filt, embed_size, n_sp_layer, activation='relu', f_in=None, generator=None, conv='GAT',
                 precision='bf16x3', attn_heads=1):
        super().__init__()
        if conv not in ('GAT', 'GCN', 'Diffusion'):
            raise NotImplementedError('conv=%r: GAT, GCN and Diffusion are built' % (conv,))
        self.n_node, self.n_edge, self.filt, self.conv = int(n_node), int(n_edge), filt, conv
        self.attn_heads = int(attn_heads)
        if self.attn_heads < 1 or (self.attn_heads > 1 and int(embed_size) % (4 * self.attn_heads)):
            raise ValueError('embed_size must be a multiple of 4 * attn_heads, got d=%d, H=%d' % (int(embed_size), self.attn_heads))
        if self.attn_heads > 1 and conv != 'GAT':
            raise ValueError('attn_heads=%d needs conv=GAT, got %r' % (self.attn_heads, conv))
        f_in = int(embed_size) if f_in is None else int(f_in)
        mk = {'GAT': GATConv, 'GCN': GCNConv, 'Diffusion': DiffusionConv}[conv]
        if conv == 'Diffusion' and isinstance(filt, CSR):
            mk = lambda d, **kw: DiffusionConv(d, moments=True, **kw)
        if self.attn_heads > 1:      # H heads of d / H channels, concatenated: the same width d (not a reference key)
            mk = lambda d, **kw: GATConv(int(d) // self.attn_heads, attn_heads=self.attn_heads, **kw)
        self.layers = nn.ModuleList([mk(embed_size, activation=activation, in_channels=(f_in if i == 0 else embed_size), generator=generator)
                                     for i in range(n_sp_layer)])
        for ly in self.layers:
            if conv == 'GAT':
                ly.precision = precision

    def forward(self, x, e, xb=None, eb=None, adj_mask=None, dropout=None, attn_dropout=None, attn_out=None):
        """attn_out: a list that receives every layer's attention coefficients (..., H, nnz of the combined pattern), GAT only."""
        if attn_out is not None and self.conv != 'GAT':
            raise NotImplementedError('attention coefficients exist for conv=GAT only')
        if xb is not None:
            x = torch.cat([x, xb], dim=-1)
        if eb is not None:
            e = torch.cat([e, eb], dim=-1)
        if x.shape[-1] != e.shape[-1]:
            raise _lib.UdsError('graph_base stacks node and link rows: widths %d and %d differ' % (x.shape[-1], e.shape[-1]))
        if adj_mask is not None and self.conv != 'GAT':
            raise NotImplementedError('use_adj is built for conv=GAT')
        z = torch.cat([x, e], dim=-2)
        for ly in self.layers:
            if attn_out is not None:
                z, alpha = ly([z, self.filt], edge_mask=adj_mask, attn_dropout=attn_dropout, return_attn_coef=True)
                attn_out.append(alpha)
            elif attn_dropout is not None and self.conv == 'GAT':
                z = ly([z, self.filt], edge_mask=adj_mask, attn_dropout=attn_dropout)
            else:
                z = ly([z, self.filt], edge_mask=adj_mask) if adj_mask is not None else ly([z, self.filt])
            if dropout is not None:      # Dropout on the node rows and on the link rows (emulator.py:234-235): one elementwise mask
                z = dropout(z)
        return z[..., :self.n_node, :].contiguous(), z[..., self.n_node:, :].contiguous()


class Dropout(nn.Module):
    """`keras.layers.Dropout(rate)` as the emulator uses it (`emulator.py:199-213,234-235,287-288,314-318`): identity unless
    called with training=True (`self.model(inp, training=fit)`, :411,434), then inverted dropout on the HIP kernel (uds_dropout,
    counter-based Philox4x32-10: the mask is a function of (seed, offset + element index), recomputed in the backward pass).
    `seed` comes from the generator given at construction (or torch's default one); every call consumes x.numel() positions of
    the stream, so successive calls and successive layers sharing one DropoutStream draw disjoint masks."""

    def __init__(self, rate, stream=None, generator=None):
        super().__init__()
        if not 0.0 <= rate < 1.0:
            raise ValueError('dropout rate %r outside [0, 1)' % (rate,))
        self.rate = float(rate)
        self.stream = stream if stream is not None else DropoutStream(generator=generator)

    def forward(self, x, training=False):
        if not training or self.rate == 0.0:
            return x
        x = x.contiguous()
        offset = self.stream.take(x.numel())
        return _ag.DropoutFn.apply(x, self.rate, self.stream.seed, offset)


class DropoutStream:
    """(seed, running offset) of one counter-based random stream shared by the Dropout layers of a model."""

    def __init__(self, seed=None, generator=None):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
        self.seed, self.offset = int(seed), 0

    def take(self, n):
        o = self.offset
        self.offset += (int(n) + 3) // 4 * 4      # whole counters: every call starts on the float4 path of the kernel
        return o

    def reseed(self, seed):
        self.seed, self.offset = int(seed), 0


class SpatialBlock(nn.Module):
    """`for _ in range(n_sp_layer)` (`emulator.py:219-235`): first layer takes (fx, fe) features."""

    def __init__(self, graph, embed_size, n_sp_layer, activation='relu', fx=None, fe=None, sparse_params=None,
                 generator=None, precision='bf16x3', conv='GAT', filters=None, attn_heads=1):
        super().__init__()
        layers = []
        for i in range(n_sp_layer):
            layers.append(SpatialLayer(graph, embed_size, activation, fx if i == 0 else None, fe if i == 0 else None,
                                       sparse_params, generator=generator, precision=precision, conv=conv, filters=filters,
                                       attn_heads=attn_heads))
        self.layers = nn.ModuleList(layers)
        self.graph = graph

    def graphed(self, x, e):
        """The block's inference forward on FIXED input buffers as one captured HIP graph: returns `replay()` -> (x', e'), which
        re-launches the L layer kernels back to back without the host work between them (argument packing, output allocation,
        launch latency: ~3 us per layer at the headline size, more than the layers themselves on small networks).  x, e are
        read in place at every replay -- write new snapshots into them; the outputs are overwritten by the next replay.
        Parameters must not change between capture and replay (packed weights are baked in): capture again after an update."""
        if not (x.is_cuda and e.is_cuda):
            raise _lib.UdsError('SpatialBlock.graphed needs device tensors')
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(torch.cuda.current_stream(x.device))
        with torch.cuda.stream(side), torch.no_grad():      # warm-up outside the capture: tile plans, packed weights, allocator
            for _ in range(2):
                self.forward(x, e)
        torch.cuda.current_stream(x.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            out = self.forward(x, e)

        def replay():
            graph.replay()
            return out
        replay.graph = graph
        return replay

    def forward(self, x, e, xb=None, eb=None, adj_mask=None, dropout=None, attn_dropout=None, attn_out=None):
        """attn_out: a list that receives one (alpha_x, alpha_e) pair per layer (the layers then run unfused), GAT only.
        xb / eb: extra input columns of the FIRST layer (`concat([x, b])` before block 2, emulator.py:260-262);
        adj_mask: the per-snapshot node adjacency of `use_adj`, seen by every layer of the block (emulator.py:268-282);
        dropout: callable applied to x and e after every layer (`Dropout(self.dropout)`, emulator.py:234-235,287-288), training only;
        attn_dropout: DropoutStream for Spektral's attention dropout inside the GATConv layers, training only."""
        net = self.layers[0].network() if self.layers[0].conv == 'GAT' else None
        for i, layer in enumerate(self.layers):
            layer._net = net
            kw = {'attn_dropout': attn_dropout} if attn_dropout is not None and layer.conv == 'GAT' else {}
            if attn_out is not None:
                x, e, alphas = layer(x, e, xb if i == 0 else None, eb if i == 0 else None, adj_mask=adj_mask, return_attn_coef=True, **kw)
                attn_out.append(alphas)
            else:
                x, e = layer(x, e, xb if i == 0 else None, eb if i == 0 else None, adj_mask=adj_mask, **kw)
            if dropout is not None:
                x, e = dropout(x), dropout(e)
        return x, e
