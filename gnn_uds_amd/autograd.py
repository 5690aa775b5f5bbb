"""Reverse mode for the HIP operators: `torch.autograd.Function` wrappers around the C ABI.

The reference trains through `tf.GradientTape` over the whole Keras model (`emulator.py:457-484`); here every HIP
operator of the forward carries its own backward, so `loss.backward()` on an `Emulator` output reaches all parameters:

    DenseFn        keras Dense                     dX = row GEMM with the transposed kernel (HIP), dW = X^T dZ (plain GEMM)
    Conv1DFn       causal dilated Conv1D           dX = the same kernels looking AHEAD (dilation < 0) with transposed taps
    SpmmFn         NodeEdge on its support / GCN   dX = spmm on the transposed pattern, dval = uds_csr_sddmm
    GatFn          MixedGAT(GATConv)               uds_gat_backward (softmax / leaky-relu / aggregation), then Dense rules
    GatHeadsFn     GATConv(attn_heads=H, ..)       uds_gat_aggregate_heads / uds_gat_backward_heads, then the same Dense rules
    DiffusionFn    DiffusionConv on its support    uds_diffusion_backward: d r (transposed pattern) and d kernel, 3 launches
    DiffusionMomentsFn  the same, no (nnz, C) table    uds_diffusion_backward_m: d kernel by the same launches, d r from row sums G_m
    AttnSumPoolFn  GlobalAttnSumPool(x | e)        uds_attn_sum_pool_backward: d x, d e and d attn_kernel in one pass, 2 launches
    CumsumActFn    relu(cumsum_T(x) + res)         reverse cumulative sum
    FlowBalanceFn  post_proc_tf incidence sums     gather along the link end nodes

    RecurrentFn    GRU / LSTM time recurrence     back-propagation through time in one launch (uds_recurrent_backward)
    RemainderFn    dense off-support NodeEdge bias  forward and d x on the split-bf16 MFMA GEMM (uds_remainder_forward)
    NodeEdgeDenseFn  a whole dense-parameter NodeEdge (NodeEdge.dense_train)  forward and d x the same GEMM on weight o inci + bias,
                   d bias and d weight in one call of uds_node_edge_wgrad

Weight gradients are GEMMs with a huge reduction dimension (rows) and tiny outputs: the split-K MFMA kernels uds_wgrad (up to
128 input rows with the bias row, 64 columns) and uds_wgrad_wide (up to 256 + the bias row, 256 columns), chosen by
`weight_grad_route`; exact-fp32 layers and anything wider take a library GEMM through `torch.mm`.  Activations are
differentiated from their outputs.
"""
import torch

from . import _lib


def act_grad(y, gy, act):
    """dL/dz from dL/dy for y = act(z), using only y (every activation here is invertible enough for that)."""
    act = act or 'linear'
    if act == 'linear':
        return gy
    if act == 'relu':
        return torch.ops.aten.threshold_backward(gy, y, 0.0)        # gy where y > 0 else 0, one kernel (no mask tensor)
    if act == 'tanh':
        return gy * (1.0 - y * y)
    if act == 'sigmoid':
        return gy * y * (1.0 - y)
    if act == 'hard_sigmoid':
        return gy * 0.2 * ((y > 0) & (y < 1)).to(gy.dtype)
    raise ValueError('unknown activation %r' % (act,))


def apply_activation(x, act):
    """The layer activations as differentiable tensor ops (used where no fused kernel applies them)."""
    act = act or 'linear'
    if act == 'linear':
        return x
    if act == 'relu':
        return torch.relu(x)
    if act == 'tanh':
        return torch.tanh(x)
    if act == 'sigmoid':
        return torch.sigmoid(x)
    if act == 'hard_sigmoid':
        return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)
    raise ValueError('unknown activation %r' % (act,))


def rows_matmul(x, w, precision='bf16x3'):
    """x (..., K) @ w (K, M) on the HIP row-GEMM kernels (matrix cores where the shape allows, in <= 64-column pieces)."""
    x = x.contiguous()
    K, M = w.shape
    lead = x.shape[:-1]
    x3 = x.reshape(1, -1, K)
    if precision == 'bf16x3' and K % 32 == 0:
        outs = []
        for c0 in range(0, M, 64):
            wc = w[:, c0:c0 + 64].contiguous()
            if not _lib.rowgemm_supported(K, K, wc.shape[1]):
                outs = None
                break
            outs.append(_lib.rowgemm_forward(x3, _lib.rowgemm_pack(wc), None, wc.shape[1], 'linear'))
        if outs is not None:
            out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=-1)
            return out.reshape(lead + (M,))
    return _lib.dense_act(x3, w.contiguous(), None, 'linear').reshape(lead + (M,))


# Shapes uds_wgrad refuses (more than 128 input rows with the bias row, more than 64 columns) go to uds_wgrad_wide (up to
# 256 + the bias row x 256) when True; False: to the library GEMM, as before the wide entry existed.
WIDE_WGRAD = True
# calls of weight_grad per route since the dict was last reset by hand (tests, tools/wgrad_wide_time.py)
ROUTE_COUNTS = {'wgrad': 0, 'wgrad_wide': 0, 'library': 0}
# GatFn.backward calls per path since the dict was last reset by hand: 'fused' = one uds_gat_backward_act call (fused_bwd),
# 'chain' = act_grad, uds_gat_backward[_ex], the bias sum and the attention-kernel weight_grad as separate steps
GAT_BWD_COUNTS = {'fused': 0, 'chain': 0}


def weight_grad_route(F, H, want_bias, precision):
    """'wgrad' (uds_wgrad), 'wgrad_wide' (uds_wgrad_wide) or 'library' (torch.mm) for the (F [+ bias row], H) weight gradient of
    a layer of this precision.  What uds_wgrad takes stays on it; 'fp32' models and anything wider than 256 stay on the library."""
    if precision != 'bf16x3':
        return 'library'
    if _lib.wgrad_supported(F, H, want_bias):
        return 'wgrad'
    if WIDE_WGRAD and _lib.wgrad_wide_supported(F, H, want_bias):
        return 'wgrad_wide'
    return 'library'


def weight_grad(x, gz, precision, want_bias, shift=0):
    """(dW, db) of y = x @ W + b summed over all leading axes: the HIP split-K MFMA kernels ('bf16x3'), else rocBLAS."""
    F, H = x.shape[-1], gz.shape[-1]
    route = weight_grad_route(F, H, want_bias, precision)
    ROUTE_COUNTS[route] += 1
    if route != 'library':
        x4 = x.contiguous().reshape((1, 1, -1, F)) if shift == 0 else x.contiguous()
        g4 = gz.contiguous().reshape((1, 1, -1, H)) if shift == 0 else gz.contiguous()
        return (_lib.wgrad if route == 'wgrad' else _lib.wgrad_wide)(x4, g4, shift, want_bias)
    if shift:
        T = x.shape[1]
        dw = x[:, :T - shift].reshape(-1, F).t().mm(gz[:, shift:].reshape(-1, H)) if shift < T else torch.zeros(F, H, device=x.device)
    else:
        dw = x.reshape(-1, F).t().mm(gz.reshape(-1, H))
    return dw, (gz.reshape(-1, H).sum(0) if want_bias else None)


class DenseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, module, act):
        xc = x.contiguous()
        fi = xc.shape[-1]
        # forward_precision: a module may ask for the exact forward and still take its gradients on the matrix cores (_Recurrent)
        if getattr(module, 'forward_precision', module.precision) == 'bf16x3' and _lib.rowgemm_supported(fi, fi, module.units):
            from .layers import _packed_kernel
            y = _lib.rowgemm_forward(xc, _packed_kernel(module, kernel), bias, module.units, act)
        else:
            y = _lib.dense_act(xc, kernel, bias, act)
        ctx.save_for_backward(xc, kernel, y)
        ctx.act, ctx.precision, ctx.has_bias = act, module.precision, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, kernel, y = ctx.saved_tensors
        gz = act_grad(y, gy.contiguous(), ctx.act)
        g2 = gz.reshape(-1, gz.shape[-1])
        dx = rows_matmul(gz, kernel.t(), ctx.precision) if ctx.needs_input_grad[0] else None
        dw, db = weight_grad(x, gz, ctx.precision, ctx.has_bias and ctx.needs_input_grad[2]) if ctx.needs_input_grad[1] else (None, None)
        if dw is None and ctx.has_bias and ctx.needs_input_grad[2]:
            db = g2.sum(0)
        return dx, dw, db, None, None


class RemainderFn(torch.autograd.Function):
    """`rest @ xs`, rest (R, M) = a dense NodeEdge bias off the incidence support (emulator.py:36-39,44), xs (S, M, h): the two
    N x E x (S h) products of a training step -- the forward and d xs = rest^T @ g -- run on the split-bf16 MFMA GEMM
    (uds_remainder_forward, the kernel of the inference path).  d rest = sum_s g_s xs_s^T has the parameter's own (R, M) shape:
    a plain library GEMM (it exists only for networks small enough to hold dense (R, M) parameters at all)."""

    @staticmethod
    def forward(ctx, rest, xs):
        xs = xs.contiguous()
        ctx.save_for_backward(rest, xs)
        return _lib.remainder_forward(_lib.remainder_pack(rest.contiguous()), tuple(rest.shape), xs)

    @staticmethod
    def backward(ctx, g):
        rest, xs = ctx.saved_tensors
        g = g.contiguous()
        dxs = drest = None
        if ctx.needs_input_grad[1]:
            rt = rest.t().contiguous()
            dxs = _lib.remainder_forward(_lib.remainder_pack(rt), tuple(rt.shape), g)
        if ctx.needs_input_grad[0]:
            R, M = rest.shape
            drest = torch.matmul(g.permute(1, 0, 2).reshape(R, -1), xs.permute(1, 0, 2).reshape(M, -1).t())
        return drest, dxs


class NodeEdgeDenseFn(torch.autograd.Function):
    """out = (weight o inci + bias) @ xs for the reference's dense (R, M) parameters (emulator.py:27-45), xs (S, M, h), as ONE
    operator: the full matrix Mx goes through the split-bf16 MFMA GEMM forward (uds_remainder_forward) and transposed for d xs,
    and (d bias, d weight) = (sum_s g_s xs_s^T, the same o inci) come from one call of uds_node_edge_wgrad on g and xs as they
    lie.  No spmm, sddmm, indexed read or mask product; the support entries are split-bf16 here, not exact fp32, which is why
    the route is a flag (NodeEdge.dense_train).  module: the NodeEdge (its dense incidence)."""

    @staticmethod
    def forward(ctx, weight, bias, xs, module):
        xs = xs.contiguous()
        inci = module.dense_incidence()
        mx = torch.addcmul(bias, weight, inci)
        ctx.save_for_backward(mx, xs, inci)
        return _lib.remainder_forward(_lib.remainder_pack(mx), tuple(mx.shape), xs)

    @staticmethod
    def backward(ctx, g):
        mx, xs, inci = ctx.saved_tensors
        g = g.contiguous()
        dxs = dw = db = None
        if ctx.needs_input_grad[2]:
            mt = mx.t().contiguous()
            dxs = _lib.remainder_forward(_lib.remainder_pack(mt), tuple(mt.shape), g)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            db, dw = _lib.node_edge_wgrad(g, xs, inci if ctx.needs_input_grad[0] else None)
        return dw, (db if ctx.needs_input_grad[1] else None), dxs, None


class RecurrentFn(torch.autograd.Function):
    """The time recurrence of a keras GRU / LSTM of H units (a multiple of 16 from 16 to 128) on the input projection xp
    (B, T, R, G*H): forward exact fp32 (uds_recurrent_forward_train), backward = back-propagation through time in one launch
    on the matrix cores (uds_recurrent_backward at 64 units, uds_recurrent_backward_h otherwise: gates recomputed from the
    saved xp and h), the recurrent kernel's gradient one split-K weight-gradient call per gate and 64-column block with a
    time shift of one, the recurrent bias its bias row (up to 64 units) or the column sum of darec (above: h and the bias
    row together exceed uds_wgrad's 128 input rows).  The Dense that made xp carries the rest (kernel, input bias, dx).
    Reference: emulator.py:158-161 inside the GradientTape of fit_eval (:457-484)."""

    @staticmethod
    def forward(ctx, xp, recurrent_kernel, recurrent_bias, kind, precision):
        xp = xp.contiguous()
        h, c = _lib.recurrent_forward_train(xp, recurrent_kernel, recurrent_bias, kind)
        ctx.save_for_backward(xp, recurrent_kernel, recurrent_bias, h, c)
        ctx.kind, ctx.precision = kind, precision
        return h

    @staticmethod
    def backward(ctx, gh):
        xp, U, rb, h, c = ctx.saved_tensors
        H = U.shape[0]
        G = U.shape[1] // H
        dxp, darec = _lib.recurrent_backward(xp, _lib.recurrent_pack_bwd(U), rb, h, c, gh.contiguous(), ctx.kind)
        dU = drb = None
        if ctx.needs_input_grad[1] or (rb is not None and ctx.needs_input_grad[2]):
            want_b = rb is not None and ctx.needs_input_grad[2]
            if H <= 64:
                parts = [weight_grad(h, darec[g], ctx.precision, want_b, shift=1) for g in range(G)]      # dU_g = sum_t h[t-1]^T darec_g[t]
                dU = torch.cat([p[0] for p in parts], dim=1)
                if want_b:
                    drb = torch.cat([p[1] if p[1] is not None else darec[g].reshape(-1, H).sum(0) for g, p in enumerate(parts)])
            else:
                # uds_wgrad takes 64 output columns and 128 input rows with the bias row: one call per gate and 64-column block,
                # the bias as the column sum of darec
                dU = torch.cat([weight_grad(h, darec[g][..., c0:c0 + 64].contiguous(), ctx.precision, False, shift=1)[0]
                                for g in range(G) for c0 in range(0, H, 64)], dim=1)
                if want_b:
                    drb = darec.reshape(G, -1, H).sum(1).reshape(-1)
        return (dxp if ctx.needs_input_grad[0] else None), dU, drb, None, None


class Conv1DFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, module):
        xc = x.contiguous()
        k, f, h = kernel.shape
        if module.precision == 'bf16x3' and _lib.rowgemm_supported(k * f, f, h):
            from .layers import _packed_kernel
            y = _lib.rowgemm_forward(xc, _packed_kernel(module, kernel.reshape(k * f, h)), bias, h, module.activation, taps=k,
                                     dilation=module.dilation_rate)
        else:
            y = _lib.conv1d_causal(xc, kernel, bias, module.dilation_rate, module.activation)
        ctx.save_for_backward(xc, kernel, y)
        ctx.act, ctx.precision, ctx.dil = module.activation, module.precision, module.dilation_rate
        return y

    @staticmethod
    def backward(ctx, gy):
        x, kernel, y = ctx.saved_tensors
        k, f, h = kernel.shape
        B, T, R, _ = x.shape
        gz = act_grad(y, gy.contiguous(), ctx.act).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            kt = kernel.transpose(1, 2).contiguous()                 # (k, h, f): tap j -> W_j^T
            if ctx.precision == 'bf16x3' and _lib.rowgemm_supported(k * h, h, f):
                dx = _lib.rowgemm_forward(gz, _lib.rowgemm_pack(kt.reshape(k * h, f)), None, f, 'linear', taps=k, dilation=-ctx.dil)
            else:
                dx = _lib.conv1d_causal(gz, kt, None, -ctx.dil, 'linear')
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(kernel)
            for j in range(k):
                dw[j], dbj = weight_grad(x, gz, ctx.precision, j == k - 1 and ctx.needs_input_grad[2], shift=(k - 1 - j) * ctx.dil)
                db = dbj if dbj is not None else db
        if db is None and ctx.needs_input_grad[2]:
            db = gz.reshape(-1, h).sum(0)
        return dx, dw, db, None


class SpmmFn(torch.autograd.Function):
    """out = A(val) @ x on a CSR pattern (no bias / activation: NodeEdge on its support)."""

    @staticmethod
    def forward(ctx, val, x, handle):
        xc = x.contiguous()
        ctx.save_for_backward(val, xc)
        ctx.handle = handle
        return _lib.csr_spmm(handle, val, xc)

    @staticmethod
    def backward(ctx, g):
        val, x = ctx.saved_tensors
        g = g.contiguous()
        dval = dx = None
        if ctx.needs_input_grad[1]:
            ht, perm = ctx.handle.transposed(g.device)
            dx = _lib.csr_spmm(ht, val[perm.long()].contiguous(), g)
        if ctx.needs_input_grad[0]:
            dval = _lib.csr_sddmm(ctx.handle, g, x)
        return dval, dx, None


class GatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xa, xb, kernel, a_self, a_nbr, bias, act, handle, precision, coef=None, edge_mask=None, fused_bwd=False):
        """coef (S, nnz) or None: multiplier of the normalised attention coefficients (Spektral's attention dropout).
        edge_mask (S, nnz) or None: per-snapshot edge mask of a `use_adj` layer (entry p of snapshot s takes part iff
        edge_mask[s, p] != 0 or p is the diagonal); forward and backward then run on uds_gat_aggregate_ex / _backward_ex.
        fused_bwd: backward takes activation, attention / aggregation, bias and attention-kernel gradients from ONE
        uds_gat_backward_act call instead of four steps (the forward pass is the same)."""
        xa = xa.contiguous()
        xb = None if xb is None else xb.contiguous()
        fin, d = xa.shape[-1] + (0 if xb is None else xb.shape[-1]), kernel.shape[-1]
        w2 = kernel.reshape(fin, d)
        fast = (precision == 'bf16x3' and xa.shape[-1] % 32 == 0 and (xb is None or xb.shape[-1] % 32 == 0) and d % 16 == 0 and
                all(_lib.rowgemm_supported(fin, 32, min(64, d - c0)) for c0 in range(0, d, 64)) and xa.shape[0] * xa.shape[1] >= 4096)
        if fast:
            # linear part on the matrix cores: 64-column blocks of the kernel written into one hx (rows read from their two
            # tensors), the attention projections as one narrow row GEMM with W a_self, W a_nbr, then the aggregation kernel
            hx = torch.empty(xa.shape[:-1] + (d,), device=xa.device, dtype=torch.float32)
            for c0 in range(0, d, 64):
                _lib.rowgemm_cat(xa, xb, _lib.rowgemm_pack(w2[:, c0:c0 + 64].contiguous()), None, min(64, d - c0), 'linear', out=hx, col0=c0)
            wa = torch.stack([w2 @ a_self.reshape(-1), w2 @ a_nbr.reshape(-1)], dim=1).contiguous()
            s2 = _lib.rowgemm_cat(xa, xb, _lib.rowgemm_pack(wa), None, 2, 'linear')
            s_self, s_nbr = s2[..., 0].contiguous(), s2[..., 1].contiguous()
            if edge_mask is not None:
                out = _lib.gat_aggregate_ex(handle, hx, s_self, s_nbr, bias, act, edge_mask=edge_mask, coef=coef)
            else:
                out = _lib.gat_aggregate(handle, hx, s_self, s_nbr, bias, act, coef=coef)
        else:
            out, (hx, s_self, s_nbr) = _lib.gat_forward(handle, xa, kernel, a_self, a_nbr, bias, act, xb, return_workspace=True)
            if edge_mask is not None:
                out = _lib.gat_aggregate_ex(handle, hx, s_self, s_nbr, bias, act, edge_mask=edge_mask, coef=coef)
            elif coef is not None:
                out = _lib.gat_aggregate(handle, hx, s_self, s_nbr, bias, act, coef=coef)
        ctx.save_for_backward(xa, xb, kernel, a_self, a_nbr, out, hx, s_self, s_nbr)
        ctx.act, ctx.handle, ctx.precision, ctx.has_bias, ctx.coef = act, handle, precision, bias is not None, coef
        ctx.edge_mask, ctx.fused_bwd = edge_mask, bool(fused_bwd)
        return out

    @staticmethod
    def _backward_fused(ctx, gout):
        """backward with fused_bwd: d_hx, the attention-kernel gradients and the bias gradient from uds_gat_backward_act; the
        input and kernel gradients from d_hx as in backward."""
        xa, xb, kernel, a_self, a_nbr, out, hx, s_self, s_nbr = ctx.saved_tensors
        d = out.shape[-1]
        GAT_BWD_COUNTS['fused'] += 1
        ht, perm = ctx.handle.transposed(gout.device)
        d_hx, _, _, db, da = _lib.gat_backward_act(
            ctx.handle, ht, perm, out, gout.contiguous(), ctx.act, hx, s_self, s_nbr, a_self.reshape(-1).contiguous(),
            a_nbr.reshape(-1).contiguous(), edge_mask=ctx.edge_mask, coef=ctx.coef, want_db=ctx.has_bias and ctx.needs_input_grad[5],
            want_da=ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        fa = xa.shape[-1]
        w2 = kernel.reshape(-1, d)
        dxa = dxb = dk = das = dan = None
        if ctx.needs_input_grad[0]:
            dxa = rows_matmul(d_hx, w2[:fa].t(), ctx.precision)
        if xb is not None and ctx.needs_input_grad[1]:
            dxb = rows_matmul(d_hx, w2[fa:].t(), ctx.precision)
        if ctx.needs_input_grad[2]:
            dk = weight_grad(xa, d_hx, ctx.precision, False)[0]
            if xb is not None:
                dk = torch.cat([dk, weight_grad(xb, d_hx, ctx.precision, False)[0]], dim=0)
            dk = dk.reshape(kernel.shape)
        if da is not None:
            das, dan = da[0].reshape(a_self.shape), da[1].reshape(a_nbr.shape)
        return dxa, dxb, dk, das, dan, db, None, None, None, None, None, None

    @staticmethod
    def backward(ctx, gout):
        if ctx.fused_bwd:
            return GatFn._backward_fused(ctx, gout)
        GAT_BWD_COUNTS['chain'] += 1
        xa, xb, kernel, a_self, a_nbr, out, hx, s_self, s_nbr = ctx.saved_tensors
        S, n, d = out.shape
        g = act_grad(out, gout.contiguous(), ctx.act).contiguous()
        ht, perm = ctx.handle.transposed(g.device)
        if ctx.edge_mask is not None:
            d_hx, ds_self, ds_nbr = _lib.gat_backward_ex(ctx.handle, ht, perm, g, hx, s_self, s_nbr, a_self.reshape(-1).contiguous(),
                                                         a_nbr.reshape(-1).contiguous(), edge_mask=ctx.edge_mask, coef=ctx.coef)
        else:
            d_hx, ds_self, ds_nbr = _lib.gat_backward(ctx.handle, ht, perm, g, hx, s_self, s_nbr, a_self.reshape(-1).contiguous(),
                                                      a_nbr.reshape(-1).contiguous(), coef=ctx.coef)
        fa = xa.shape[-1]
        w2 = kernel.reshape(-1, d)
        dxa = dxb = dk = das = dan = db = None
        # d[xa | xb] = d_hx W^T, each piece straight into its own tensor (no concatenated intermediate)
        if ctx.needs_input_grad[0]:
            dxa = rows_matmul(d_hx, w2[:fa].t(), ctx.precision)
        if xb is not None and ctx.needs_input_grad[1]:
            dxb = rows_matmul(d_hx, w2[fa:].t(), ctx.precision)
        if ctx.needs_input_grad[2]:
            dk = weight_grad(xa, d_hx, ctx.precision, False)[0]
            if xb is not None:
                dk = torch.cat([dk, weight_grad(xb, d_hx, ctx.precision, False)[0]], dim=0)
            dk = dk.reshape(kernel.shape)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            # d a_self = sum_r ds_self[r] hx[r, :], d a_nbr likewise: one (rows, 2)^T (rows, d) reduction
            da = weight_grad(torch.stack([ds_self, ds_nbr], dim=-1), hx, ctx.precision, False)[0]
            das, dan = da[0].reshape(a_self.shape), da[1].reshape(a_nbr.shape)
        if ctx.has_bias and ctx.needs_input_grad[5]:
            db = g.reshape(-1, d).sum(0)
        return dxa, dxb, dk, das, dan, db, None, None, None, None, None, None


def heads_score_matrix(a_self, a_nbr):
    """The block-diagonal (H*C, 2H) matrix that takes hx (.., H*C), head-major, to its 2H attention scores: column h holds
    attn_kernel_self[:, h, 0] in rows h*C .. (h+1)*C, column H + h attn_kernel_neighs[:, h, 0].  Also returns the two kernels
    head-major, (H*C,) each, as uds_gat_backward_heads takes them."""
    C, H = a_self.shape[0], a_self.shape[1]
    as_hm, an_hm = a_self.reshape(C, H).t().contiguous(), a_nbr.reshape(C, H).t().contiguous()        # (H, C)
    eye = torch.eye(H, device=a_self.device, dtype=a_self.dtype)
    m = torch.cat([as_hm.unsqueeze(-1) * eye.unsqueeze(1), an_hm.unsqueeze(-1) * eye.unsqueeze(1)], dim=-1)      # (H, C, 2H)
    return m.reshape(H * C, 2 * H).contiguous(), as_hm.reshape(-1), an_hm.reshape(-1)


def gat_heads_forward(xa, xb, kernel, a_self, a_nbr, bias, act, handle, concat, coef=None, edge_mask=None, want_attn=False):
    """The multi-head GATConv forward on the HIP kernels: hx = [xa | xb] @ kernel.reshape(F, H*C) and the 2H scores
    hx @ heads_score_matrix as exact-fp32 row products (uds_dense_act), then uds_gat_aggregate_heads.
    Returns out, alpha (S, H, nnz) or None, and (hx, s_self, s_nbr) for the backward."""
    fin, H, C = kernel.shape
    hx = _lib.dense_act(xa, kernel.reshape(fin, H * C), None, 'linear', xb)
    s2 = _lib.dense_act(hx, heads_score_matrix(a_self, a_nbr)[0], None, 'linear')
    s_self, s_nbr = s2[..., :H].contiguous(), s2[..., H:].contiguous()
    res = _lib.gat_aggregate_heads(handle, hx, s_self, s_nbr, bias, act, concat=concat, edge_mask=edge_mask, coef=coef,
                                   alpha_out=True if want_attn else None)
    out, alpha = res if want_attn else (res, None)
    return out, alpha, (hx, s_self, s_nbr)


class GatHeadsFn(torch.autograd.Function):
    """GATConv with attn_heads = H (kernel (F, H, C), attention kernels (C, H, 1)), concatenated or averaged heads:
    uds_gat_aggregate_heads / uds_gat_backward_heads, then the Dense rules of GatFn on the (F, H*C) view of the kernel.
    edge_mask (S, nnz) is shared by the heads, coef (S, H, nnz) is per head.  Returns (out, alpha); alpha (S, H, nnz) carries
    no gradient (an empty tensor when it was not asked for)."""

    @staticmethod
    def forward(ctx, xa, xb, kernel, a_self, a_nbr, bias, act, handle, precision, concat, coef=None, edge_mask=None, want_attn=False):
        xa = xa.contiguous()
        xb = None if xb is None else xb.contiguous()
        out, alpha, (hx, s_self, s_nbr) = gat_heads_forward(xa, xb, kernel, a_self, a_nbr, bias, act, handle, concat, coef, edge_mask, want_attn)
        ctx.save_for_backward(xa, xb, kernel, a_self, a_nbr, out, hx, s_self, s_nbr)
        ctx.act, ctx.handle, ctx.precision, ctx.has_bias, ctx.coef = act, handle, precision, bias is not None, coef
        ctx.edge_mask, ctx.concat = edge_mask, concat
        if alpha is None:
            alpha = out.new_empty(0)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, gout, _galpha):
        xa, xb, kernel, a_self, a_nbr, out, hx, s_self, s_nbr = ctx.saved_tensors
        fin, H, C = kernel.shape
        g = act_grad(out, gout.contiguous(), ctx.act).contiguous()
        ht, perm = ctx.handle.transposed(g.device)
        _, as_hm, an_hm = heads_score_matrix(a_self, a_nbr)
        d_hx, ds_self, ds_nbr = _lib.gat_backward_heads(ctx.handle, ht, perm, g, hx, s_self, s_nbr, as_hm, an_hm, concat=ctx.concat,
                                                        edge_mask=ctx.edge_mask, coef=ctx.coef)
        fa = xa.shape[-1]
        w2 = kernel.reshape(fin, H * C)
        dxa = dxb = dk = das = dan = db = None
        if ctx.needs_input_grad[0]:
            dxa = rows_matmul(d_hx, w2[:fa].t(), ctx.precision)
        if xb is not None and ctx.needs_input_grad[1]:
            dxb = rows_matmul(d_hx, w2[fa:].t(), ctx.precision)
        if ctx.needs_input_grad[2]:
            dk = weight_grad(xa, d_hx, ctx.precision, False)[0]
            if xb is not None:
                dk = torch.cat([dk, weight_grad(xb, d_hx, ctx.precision, False)[0]], dim=0)
            dk = dk.reshape(kernel.shape)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            # d a_self[:, h] = sum_r ds_self[r, h] hx[r, h*C:(h+1)*C]: the diagonal blocks of one (rows, 2H)^T (rows, H*C) reduction
            da = weight_grad(torch.cat([ds_self, ds_nbr], dim=-1), hx, ctx.precision, False)[0].reshape(2, H, H, C)
            da = da.diagonal(dim1=1, dim2=2)                                   # (2, C, H)
            das, dan = da[0].reshape(a_self.shape), da[1].reshape(a_nbr.shape)
        if ctx.has_bias and ctx.needs_input_grad[5]:
            db = g.reshape(-1, g.shape[-1]).sum(0)
        return dxa, dxb, dk, das, dan, db, None, None, None, None, None, None, None


class DiffusionFn(torch.autograd.Function):
    """DiffusionConv from the feature sums r = x.sum(-1) (S, n_cols): out = act(c0 tot + sum_p vals[p] r[col p]) on the CSR
    support (uds_diffusion_forward, the inference kernel).  `kernel` (C, K1) is an input only for its gradient: vals / c0 are
    its values prepared by the layer, `a` the filter's support values.  Backward: uds_diffusion_backward from the saved output
    -- d r (the tot term folded in) and d kernel, three launches, no host synchronisation."""

    @staticmethod
    def forward(ctx, r, kernel, handle, a, vals, c0, act):
        r = r.contiguous()
        tot = r.sum(dim=-1).contiguous()
        out = _lib.diffusion_forward(handle, vals, c0, r, tot, act)
        ctx.save_for_backward(r, tot, a, vals, c0, out)
        ctx.handle, ctx.act, ctx.K1 = handle, act, kernel.shape[1]
        return out

    @staticmethod
    def backward(ctx, gy):
        r, tot, a, vals, c0, out = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.data_ptr() % 16:                   # a view at an odd offset: the kernel reads 16-byte vectors
            gy = gy.clone()
        dr, dk = _lib.diffusion_backward(ctx.handle, a, vals, c0, r, tot, out, gy, ctx.K1, ctx.act)
        return (dr if ctx.needs_input_grad[0] else None), (dk if ctx.needs_input_grad[1] else None), None, None, None, None, None


class DiffusionMomentsFn(torch.autograd.Function):
    """DiffusionFn without the (nnz, C) table of polynomial values: the kernels expand the polynomial per row from `kernel`
    (C, K1) and the filter's support values `a` (uds_diffusion_forward_m / uds_diffusion_backward_m).  What a model built from
    a CSR graph runs (layers.DiffusionConv(moments=True))."""

    @staticmethod
    def forward(ctx, r, kernel, handle, a, act):
        r = r.contiguous()
        tot = r.sum(dim=-1).contiguous()
        theta = kernel.detach().contiguous()
        out = _lib.diffusion_forward_m(handle, a, theta, r, tot, act)
        ctx.save_for_backward(r, tot, a, theta, out)
        ctx.handle, ctx.act = handle, act
        return out

    @staticmethod
    def backward(ctx, gy):
        r, tot, a, theta, out = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.data_ptr() % 16:                   # a view at an odd offset: the kernel reads 16-byte vectors
            gy = gy.clone()
        dr, dk = _lib.diffusion_backward_m(ctx.handle, a, theta, r, tot, out, gy, ctx.act)
        return (dr if ctx.needs_input_grad[0] else None), (dk if ctx.needs_input_grad[1] else None), None, None, None


class AttnSumPoolFn(torch.autograd.Function):
    """GlobalAttnSumPool over the rows of x (B, Rx, F) followed by those of e (B, Re, F) or None (uds_attn_sum_pool_pair: the stack
    is never built).  Saves the output and the (max, sum of exponentials) pair of every sample; backward is one pass over the rows
    (uds_attn_sum_pool_backward), the kernel's gradient summed in a fixed order: two launches, no float atomics."""

    @staticmethod
    def forward(ctx, x, e, attn_kernel):
        x = x.contiguous()
        e = None if e is None else e.contiguous()
        out, stat = _lib.attn_sum_pool_pair(x, e, attn_kernel, want_stat=True)
        ctx.save_for_backward(x, e, attn_kernel, out, stat)
        return out

    @staticmethod
    def backward(ctx, g):
        x, e, k, out, stat = ctx.saved_tensors
        g = g.contiguous()
        if g.data_ptr() % 16:                    # a view at an odd offset: the kernel reads 16-byte vectors
            g = g.clone()
        dx, de, dk = _lib.attn_sum_pool_backward(x, e, k, out, stat, g, want_dx=ctx.needs_input_grad[0],
                                                 want_de=e is not None and ctx.needs_input_grad[1], want_dk=ctx.needs_input_grad[2])
        return dx, de, (None if dk is None else dk.reshape(k.shape))


class CumsumActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, act):
        y = _lib.cumsum_act(x.contiguous(), None if res is None else res.contiguous(), act)
        ctx.save_for_backward(y)
        ctx.act, ctx.has_res = act, res is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gz = act_grad(y, gy, ctx.act)
        dx = torch.flip(torch.cumsum(torch.flip(gz, dims=[1]), dim=1), dims=[1]) if ctx.needs_input_grad[0] else None
        dres = gz.sum(dim=1, keepdim=True) if ctx.has_res and ctx.needs_input_grad[1] else None
        return dx, dres, None


class DropoutFn(torch.autograd.Function):
    """keras Dropout in training mode (uds_dropout): the backward pass is the same kernel on the gradient with the same
    (seed, offset) -- the mask is recomputed, not stored."""

    @staticmethod
    def forward(ctx, x, rate, seed, offset):
        ctx.cfg = (rate, seed, offset)
        return _lib.dropout(x, rate, seed, offset)

    @staticmethod
    def backward(ctx, gy):
        rate, seed, offset = ctx.cfg
        return _lib.dropout(gy.contiguous(), rate, seed, offset), None, None, None


class FlowBalanceFn(torch.autograd.Function):
    """q_in, q_out (S,N) from signed link flows (S,E) (`emulator.py:717-724`); edges (E,2) int64 = [from, to] per link."""

    @staticmethod
    def forward(ctx, flow, handle, sign, scale_in, scale_out, edges):
        flow = flow.contiguous()
        ctx.save_for_backward(flow, scale_in, scale_out, edges)
        return _lib.flow_balance(handle, sign, flow, scale_in, scale_out)

    @staticmethod
    def backward(ctx, g_in, g_out):
        flow, scale_in, scale_out, edges = ctx.saved_tensors
        gi, go = g_in * scale_in, g_out * scale_out                     # (S,N)
        u, v = edges[:, 0], edges[:, 1]
        # from-node u: q_out += max(f,0), q_in += max(-f,0); to-node v: q_in += max(f,0), q_out += max(-f,0)
        pos = go[:, u] + gi[:, v]
        neg = gi[:, u] + go[:, v]
        dflow = torch.where(flow > 0, pos, torch.zeros_like(pos)) - torch.where(flow < 0, neg, torch.zeros_like(neg))
        return dflow, None, None, None, None, None


class PredictTailFn(torch.autograd.Function):
    """The tail of `Emulator.predict_tf` (everything after the network forward) as one HIP forward and one HIP backward
    (include/uds_hip.h: uds_predict_tail / uds_predict_tail_backward).  Differentiable in y, ey, a and h0; b_norm and runoff
    are constants here (the emulator keeps the tensor route when they need a gradient)."""

    @staticmethod
    def forward(ctx, y, ey, a, h0, b_norm, runoff, handle, sign, spec, depth_gate, pump_override):
        y, ey, h0 = y.contiguous(), ey.contiguous(), h0.contiguous()
        a = None if a is None else a.contiguous()
        ctx.save_for_backward(y, ey, h0, b_norm, runoff, sign, *([] if a is None else [a]))
        ctx.tail = (handle, spec, depth_gate, pump_override)
        out_y, out_ey = _lib.predict_tail(handle, sign, spec, y, ey, a, b_norm, runoff, h0, depth_gate, pump_override)
        return out_y, out_ey

    @staticmethod
    def backward(ctx, g_y, g_ey):
        y, ey, h0, b_norm, runoff, sign, *rest = ctx.saved_tensors
        a = rest[0] if rest else None
        handle, spec, depth_gate, pump_override = ctx.tail
        dy, dey, da, dh0 = _lib.predict_tail_backward(handle, sign, spec, y, ey, a, b_norm, runoff, h0, g_y.contiguous(), g_ey.contiguous(),
                                                      depth_gate, pump_override)
        return dy, dey, da, dh0, None, None, None, None, None, None, None


class FitTailFn(torch.autograd.Function):
    """The tail of a training step (`Emulator.fit_eval` / `fit_grad_norm` after the network forward) as one HIP forward and one HIP
    backward (include/uds_hip.h: uds_fit_tail / uds_fit_tail_backward): (out_y, out_ey, loss_sums).  Differentiable in y and ey
    only; the settings, the boundary, the targets and the weights are constants here (the emulator keeps the tensor route when one
    of them needs a gradient).  The backward keeps nothing of its own between calls: it may run more than once on one forward
    (`fit_grad_norm` takes two gradients with retain_graph)."""

    @staticmethod
    def forward(ctx, y, ey, a, b_norm, y_true, ey_true, handle, spec, lw, pump_override):
        y, ey = y.contiguous(), ey.contiguous()
        ctx.save_for_backward(y, ey, b_norm, y_true, ey_true, *([] if a is None else [a]))
        ctx.tail = (handle, spec, lw, pump_override)
        ctx.set_materialize_grads(False)          # an output nothing reads hands None to the backward: no zero tensor, a NULL pointer
        out_y, out_ey, sums = _lib.fit_tail(handle, spec, y, ey, a, b_norm, y_true, ey_true, lw, pump_override)
        return out_y, out_ey, sums

    @staticmethod
    def backward(ctx, g_y, g_ey, g_sums):
        y, ey, b_norm, y_true, ey_true, *rest = ctx.saved_tensors
        handle, spec, lw, pump_override = ctx.tail
        g_sums = torch.zeros(3, device=y.device, dtype=torch.float32) if g_sums is None else g_sums.contiguous()
        dy, dey = _lib.fit_tail_backward(handle, spec, y, ey, rest[0] if rest else None, b_norm, y_true, ey_true, lw, g_sums,
                                         None if g_y is None else g_y.contiguous(), None if g_ey is None else g_ey.contiguous(), pump_override)
        return dy, dey, None, None, None, None, None, None, None, None


class MpcObjectiveFn(torch.autograd.Function):
    """The MPC scenario objective of a population of predicted horizons as one HIP forward and one HIP backward (include/uds_hip.h:
    uds_mpc_objective / uds_mpc_objective_backward).  Differentiable in preds only: q_in0 is history, the weights and gamma are
    constants of the problem."""

    @staticmethod
    def forward(ctx, preds, q_in0, w_flood, w_out, w_smooth, gamma):
        preds = preds.contiguous()
        ctx.save_for_backward(preds, q_in0)
        ctx.weights = (w_flood, w_out, w_smooth, gamma)
        return _lib.mpc_objective(preds, q_in0, w_flood, w_out, w_smooth, gamma)

    @staticmethod
    def backward(ctx, g):
        preds, q_in0 = ctx.saved_tensors
        return _lib.mpc_objective_backward(preds, q_in0, g.contiguous(), *ctx.weights), None, None, None, None, None


def grad_on(*tensors):
    """True when autograd is recording and one of the tensors needs a gradient: the modules then take the Function path."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)
