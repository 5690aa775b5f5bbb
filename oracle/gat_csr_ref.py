"""TEST INFRASTRUCTURE ONLY: the GAT aggregation and its reverse mode on a CSR pattern, in fp64 NumPy, row by row as the
kernels walk them -- the reference of uds_gat_aggregate[_ex / _masked / _coef] and uds_gat_backward[_ex / _coef].  Pinned
against torch autograd of the dense restatement by tests/test_use_adj_grad_math.py and, on the degree ladder, against
oracle.sparse_csr.gat_conv_csr by tests/test_sparse_ref_math.py.  Per snapshot s and row i, with l_p = ss_i + sn_j (j = col p):

    survivors  P_i = {p in row i : mask[s, p] != 0 or j == i}          (spektral's set_diag after the rewrite)
    m_i        = max_{p in P_i} leaky(l_p)                             (over the survivors only)
    alpha_p    = exp(leaky(l_p) - m_i) / sum_{P_i} exp(..)  on P_i,  0 off it
    pre_i      = sum_p alpha_p coef_p hx_j,   out = act(pre + bias),   g = act'(out) gout
    q_p        = coef_p <g_i, hx_j>,   cbar_i = sum_p alpha_p q_p,   de_p = alpha_p (q_p - cbar_i) leaky'(l_p)  (0 off P_i)
    ds_self_i  = sum_{p in row i} de_p
    d_hx_j     = sum_{p : col p = j} alpha_p coef_p g_{row p} + a_nbr ds_nbr_j + a_self ds_self_j,   ds_nbr_j = sum_{col p = j} de_p

(coef: the attention-dropout multiplier, 1 without dropout.)  With mask = ones and coef = ones these are the unmasked entries.
A row without a survivor (no diagonal, every entry masked) has pre = 0 and contributes no gradient."""
import numpy as np


def leaky(v):
    return np.where(v > 0, v, 0.2 * v)


def act_fn(z, act):
    return {'relu': lambda t: np.maximum(t, 0.0), 'tanh': np.tanh, 'linear': lambda t: t}[act](z)


def act_grad(y, gy, act):
    return {'relu': gy * (y > 0), 'tanh': gy * (1.0 - y * y), 'linear': gy}[act]


def survivors(rowptr, col, mask):
    """(S, nnz) bool: entry p of snapshot s takes part."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return (mask != 0) | (col == rows)[None, :]


def masked_forward(rowptr, col, mask, coef, hx, ss, sn, bias, act):
    """out (S, n, d) and alpha (S, nnz) in fp64, row by row as the kernels walk them."""
    S, n, d = hx.shape
    on = survivors(rowptr, col, mask)
    alpha = np.zeros(mask.shape)
    out = np.empty((S, n, d))
    for s in range(S):
        for i in range(n):
            ps = np.arange(rowptr[i], rowptr[i + 1])
            ps = ps[on[s, ps]]
            pre = np.zeros(d)
            if len(ps):
                lg = leaky(ss[s, i] + sn[s, col[ps]])
                w = np.exp(lg - lg.max())
                alpha[s, ps] = w / w.sum()
                pre = (alpha[s, ps] * coef[s, ps]) @ hx[s, col[ps]]
            out[s, i] = act_fn(pre + bias, act)
    return out, alpha


def masked_backward(rowptr, col, mask, coef, hx, ss, sn, a_self, a_nbr, alpha, out, gout, act):
    """(d_hx (S, n, d), ds_self (S, n), ds_nbr (S, n)) in fp64: the row pass, then the transposed walk."""
    S, n, d = hx.shape
    on = survivors(rowptr, col, mask)
    g = act_grad(out, gout, act)
    de = np.zeros(mask.shape)
    ds_self = np.zeros((S, n))
    for s in range(S):
        for i in range(n):
            ps = np.arange(rowptr[i], rowptr[i + 1])
            q = coef[s, ps] * (hx[s, col[ps]] @ g[s, i])
            cbar = (alpha[s, ps] * q).sum()
            slope = np.where(ss[s, i] + sn[s, col[ps]] > 0, 1.0, 0.2)
            de[s, ps] = np.where(on[s, ps], alpha[s, ps] * (q - cbar) * slope, 0.0)
            ds_self[s, i] = de[s, ps].sum()
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    order = np.lexsort((rows, col))                  # the transposed pattern, column by column
    d_hx = np.zeros((S, n, d))
    ds_nbr = np.zeros((S, n))
    for s in range(S):
        for p in order:
            d_hx[s, col[p]] += alpha[s, p] * coef[s, p] * g[s, rows[p]]
            ds_nbr[s, col[p]] += de[s, p]
        d_hx[s] += np.outer(ds_nbr[s], a_nbr) + np.outer(ds_self[s], a_self)
    return d_hx, ds_self, ds_nbr, g


def masked_forward_backward_f32(rowptr, col, mask, coef, hx, ss, sn, a_self, a_nbr, gout):
    """The same forward (no bias, linear) and backward evaluated in NumPy float32, entries added in pattern order as the kernels
    add them (no fused multiply-add): (pre, d_hx, ds_self, ds_nbr) as float32.  What plain fp32 evaluation order costs against
    the fp64 functions above -- the yardstick for a GPU tolerance, not a reference."""
    f = np.float32
    S, n, d = hx.shape
    hx, g, ss, sn, coef = hx.astype(f), gout.astype(f), ss.astype(f), sn.astype(f), coef.astype(f)
    on = survivors(rowptr, col, mask)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    pre, alpha, de, ds_self = np.zeros((S, n, d), f), np.zeros(mask.shape, f), np.zeros(mask.shape, f), np.zeros((S, n), f)
    for s in range(S):
        for i in range(n):
            ps = np.arange(rowptr[i], rowptr[i + 1])
            j, o, cf = col[ps], on[s, ps], coef[s, ps]
            lg = ss[s, i] + sn[s, j]
            l = np.where(lg > 0, lg, f(0.2) * lg).astype(f)
            w = np.where(o, np.exp(l - l[o].max()), f(0)).astype(f) if o.any() else np.zeros(len(ps), f)
            q = ((hx[s, j] @ g[s, i]).astype(f) * cf).astype(f)
            den, cn, acc = f(0), f(0), np.zeros(d, f)
            for k in range(len(ps)):
                den, cn = f(den + w[k]), f(cn + w[k] * q[k])
                acc = (acc + f(w[k] * cf[k]) * hx[s, j[k]]).astype(f)
            inv = f(1) / den if den > 0 else f(0)
            pre[s, i] = acc * inv
            a = (w * inv).astype(f)
            dl = (a * (q - f(cn * inv))).astype(f)
            dv = np.where(o, np.where(lg > 0, dl, f(0.2) * dl), f(0)).astype(f)
            alpha[s, ps], de[s, ps] = a * cf, dv
            for v in dv:
                ds_self[s, i] = f(ds_self[s, i] + v)
    d_hx, ds_nbr = np.zeros((S, n, d), f), np.zeros((S, n), f)
    for s in range(S):
        for p in np.lexsort((rows, col)):
            d_hx[s, col[p]] = (d_hx[s, col[p]] + alpha[s, p] * g[s, rows[p]]).astype(f)
            ds_nbr[s, col[p]] = f(ds_nbr[s, col[p]] + de[s, p])
        d_hx[s] = (d_hx[s] + np.outer(ds_self[s], a_self.astype(f)) + np.outer(ds_nbr[s], a_nbr.astype(f))).astype(f)
    return pre, d_hx, ds_self, ds_nbr
