"""Training `use_adj` GAT models: the masked GAT layer under autograd (uds_gat_aggregate_ex / uds_gat_backward_ex, GatFn with an
edge mask) and everything that differentiates through it -- `Emulator._model`, `fit_eval`, `fit_grad_norm`, `roll > 0` and
`mpc.objective_and_gradient` / `hessp` on a model built with act + use_adj (emulator.py:178-180,268-271,343-362,457-484).

Tolerances are those of the unmasked counterpart of each check (tests/test_gpu_train.py, tests/test_gpu_dropout.py):
  kernels (exact fp32)           5e-6 of max(1, max|ref|)  (bitwise for an all-ones mask)
  layer, fp32                    1e-5                        layer, matrix-core linear part ('bf16x3')   4e-5
  layer with attention dropout   forward 2e-5, gradients 1e-4 * scale + 1e-7
  whole model                    losses 2e-5, gradients GRAD_TOL['GAT'] * scale + 1e-7 * gmax
  MPC                            objective 2e-5, gradient 2e-3 * gmax
The fp64 oracle (oracle/emulator_ref.py) takes the per-time-step adjacency as `ADJ` in `forward`; `OT.losses` and
`OE.model_rollout` pass none, so the losses here compose OE.forward(..., ADJ) with OE.post_proc themselves."""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd.layers import DropoutStream
from oracle import emulator_ref as OE
from oracle import sparse_csr as OS
from oracle import spektral_dense as OD
from oracle import train_ref as OT
from tests.test_gpu_dropout import _RefStream
from tests.test_gpu_train import GRAD_TOL, _problem
from tests.util import close, emulator_param_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------------------------------------------- patterns

def _headline():
    return U.DrainageGraph.from_edges(U.synthetic_drainage_network(10000, 12000, 0)).adj


def _hub():
    """The `hub` pattern of test_gat_backward: a junction with 30 conduits plus a chain (rows of more than 16 entries)."""
    edges = np.array([[0, i] for i in range(1, 31)] + [[i, i + 1] for i in range(30, 45)])
    return U.DrainageGraph.from_edges(edges, 46).adj


_PATTERNS = {'headline': _headline, 'hub': _hub}
_CACHE = {}


def _pattern(name):
    if name not in _CACHE:
        _CACHE[name] = _PATTERNS[name]()
    return _CACHE[name]


def _rows(csr):
    return np.repeat(np.arange(csr.n_rows), np.diff(np.asarray(csr.rowptr, dtype=np.int64)))


def _seeded_mask(csr, S, seed):
    """(S, nnz) 0/1: about 10 % of the entries off per snapshot, and in every snapshot three random rows lose every off-diagonal
    entry -- in snapshot 0 the widest row too (the other snapshots keep it partly masked: the multi-chunk path of a hub row).
    Diagonal entries are drawn like the others: the kernels must keep them anyway."""
    rng = np.random.default_rng(seed)
    rows, col = _rows(csr), np.asarray(csr.col, dtype=np.int64)
    mask = (rng.random((S, csr.nnz)) > 0.1).astype(np.float32)
    deg = np.diff(np.asarray(csr.rowptr, dtype=np.int64))
    for s in range(S):
        wipe = set(rng.choice(csr.n_rows, size=min(3, csr.n_rows), replace=False).tolist()) | ({int(np.argmax(deg))} if s == 0 else set())
        for r in wipe:
            mask[s, (rows == r) & (col != r)] = 0.0
    return mask


def _pruned(csr, keep):
    """CSR of the entries `keep` (nnz,) bool of a pattern (the diagonal kept as the kernels keep it)."""
    rows, col = _rows(csr), np.asarray(csr.col, dtype=np.int64)
    keep = keep | (rows == col)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=csr.n_rows))]).astype(np.int32)
    return U.graph.CSR(rowptr, col[keep].astype(np.int32), csr.n_rows, csr.n_cols), keep


def _operands(csr, S, d, dev, seed):
    g = torch.Generator().manual_seed(seed)
    n = csr.n_rows
    r = lambda *s: (torch.rand(*s, generator=g) - 0.5).to(dev)
    hx, ss, sn = r(S, n, d), r(S, n) * 4, r(S, n) * 4
    bias, grad, a_s, a_n = r(d) * 0.2, r(S, n, d), r(d), r(d)
    return hx, ss.contiguous(), sn.contiguous(), bias, grad, a_s, a_n


def _coef(S, nnz, dev, seed):
    return _lib.dropout(torch.ones((S, nnz), device=dev), 0.5, seed, 0)


WIDTHS = [8, 64, 128, 12]          # d / 4 = 2, 16, 32: grouped kernels; d = 12 (d / 4 = 3): the walking fallback


# ---------------------------------------------------------------------------------------------------------------- 1 / 2: kernels

@pytest.mark.parametrize('name,S', [('headline', 8), ('hub', 8)])
@pytest.mark.parametrize('d', WIDTHS)
def test_all_ones_mask_is_bitwise_the_unmasked_path(dev, name, S, d):
    csr = _pattern(name)
    h = _lib.CsrHandle(csr)
    ht, perm = h.transposed(dev)
    hx, ss, sn, bias, grad, a_s, a_n = _operands(csr, S, d, dev, seed=d)
    ones = torch.ones((S, csr.nnz), device=dev)
    for act in ('relu', 'tanh'):
        assert torch.equal(_lib.gat_aggregate_ex(h, hx, ss, sn, bias, act, edge_mask=ones), _lib.gat_aggregate(h, hx, ss, sn, bias, act))
    got = _lib.gat_backward_ex(h, ht, perm, grad, hx, ss, sn, a_s, a_n, edge_mask=ones)
    ref = _lib.gat_backward(h, ht, perm, grad, hx, ss, sn, a_s, a_n)
    for gt_, rf in zip(got, ref):
        assert torch.equal(gt_, rf)


def _per_snapshot_reference(csr, mask, coef, hx, ss, sn, bias, grad, a_s, a_n, act, dev):
    """The existing unmasked kernels, snapshot by snapshot, on the pattern with the masked entries removed."""
    outs, dh, dss, dsn = [], [], [], []
    for s in range(hx.shape[0]):
        sub, keep = _pruned(csr, mask[s] != 0)
        h = _lib.CsrHandle(sub)
        ht, perm = h.transposed(dev)
        cf = None if coef is None else coef[s:s + 1, torch.as_tensor(np.nonzero(keep)[0], device=dev)].contiguous()
        one = lambda t: t[s:s + 1].contiguous()
        outs.append(_lib.gat_aggregate(h, one(hx), one(ss), one(sn), bias, act, coef=cf))
        r = _lib.gat_backward(h, ht, perm, one(grad), one(hx), one(ss), one(sn), a_s, a_n, coef=cf)
        dh.append(r[0])
        dss.append(r[1])
        dsn.append(r[2])
    return torch.cat(outs), (torch.cat(dh), torch.cat(dss), torch.cat(dsn))


@pytest.mark.parametrize('name,S', [('headline', 8), ('hub', 8)])
@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('with_coef', [False, True])
def test_seeded_mask_matches_the_pruned_pattern(dev, name, S, d, with_coef):
    csr = _pattern(name)
    h = _lib.CsrHandle(csr)
    ht, perm = h.transposed(dev)
    hx, ss, sn, bias, grad, a_s, a_n = _operands(csr, S, d, dev, seed=100 + d)
    mask_np = _seeded_mask(csr, S, seed=d)
    rows, col = _rows(csr), np.asarray(csr.col)
    off = rows != col
    frac = float((mask_np[:, off] == 0).mean())
    assert frac > 0.05, frac
    deg_off = np.bincount(rows[off], minlength=csr.n_rows)
    for s in range(S):                    # some row with off-diagonal entries keeps none of them, in every snapshot
        kept = np.bincount(rows[off], weights=mask_np[s, off], minlength=csr.n_rows)
        assert ((deg_off > 0) & (kept == 0)).any()
    mask = torch.from_numpy(mask_np).to(dev)
    coef = _coef(S, csr.nnz, dev, seed=d) if with_coef else None
    out = _lib.gat_aggregate_ex(h, hx, ss, sn, bias, 'tanh', edge_mask=mask, coef=coef)
    got = _lib.gat_backward_ex(h, ht, perm, grad, hx, ss, sn, a_s, a_n, edge_mask=mask, coef=coef)
    ref_out, ref = _per_snapshot_reference(csr, mask_np, coef, hx, ss, sn, bias, grad, a_s, a_n, 'tanh', dev)
    close(out, ref_out.double().cpu(), 5e-6)
    for gt_, rf in zip(got, ref):
        close(gt_, rf.double().cpu(), 5e-6)
    # the mask does something
    assert float((out - _lib.gat_aggregate(h, hx, ss, sn, bias, 'tanh', coef=coef)).abs().max()) > 1e-3


@pytest.mark.parametrize('name', ['headline', 'hub'])
@pytest.mark.parametrize('d', WIDTHS)
def test_coef_only_matches_the_coef_entries(dev, name, d):
    csr = _pattern(name)
    S = 8
    h = _lib.CsrHandle(csr)
    ht, perm = h.transposed(dev)
    hx, ss, sn, bias, grad, a_s, a_n = _operands(csr, S, d, dev, seed=200 + d)
    coef = _coef(S, csr.nnz, dev, seed=7 + d)
    close(_lib.gat_aggregate_ex(h, hx, ss, sn, bias, 'relu', coef=coef), _lib.gat_aggregate(h, hx, ss, sn, bias, 'relu', coef=coef).double().cpu(), 5e-6)
    got = _lib.gat_backward_ex(h, ht, perm, grad, hx, ss, sn, a_s, a_n, coef=coef)
    ref = _lib.gat_backward(h, ht, perm, grad, hx, ss, sn, a_s, a_n, coef=coef)
    for gt_, rf in zip(got, ref):
        close(gt_, rf.double().cpu(), 5e-6)


def test_ex_entries_check_their_operands(dev):
    csr = _pattern('hub')
    h = _lib.CsrHandle(csr)
    hx, ss, sn, bias, grad, a_s, a_n = _operands(csr, 2, 8, dev, seed=1)
    with pytest.raises(_lib.UdsError):
        _lib.gat_aggregate_ex(h, hx, ss, sn, bias, 'relu', edge_mask=torch.ones((2, csr.nnz + 1), device=dev))
    with pytest.raises(_lib.UdsError):
        _lib.gat_aggregate_ex(h, hx, ss, sn, bias, 'relu', coef=torch.ones((3, csr.nnz), device=dev))


# ---------------------------------------------------------------------------------------------------------------- 3: layer

def _static_with_loops(gph):
    """(CSR with the self loops = the GAT pattern, dense 0/1 (N, N))."""
    return gph.adj, gph.adj.to_dense()


def _dense_adjacency(csr, mask):
    """(S, N, N) float64 adjacency of the reference: the static pattern with the masked entries removed."""
    S = mask.shape[0]
    adj = np.zeros((S, csr.n_rows, csr.n_cols))
    rows, col = _rows(csr), np.asarray(csr.col, dtype=np.int64)
    for s in range(S):
        adj[s, rows, col] = mask[s]
    return torch.from_numpy(adj)


class _StaticAttnStream(_RefStream):
    """_RefStream whose attention draw lays the (S, nnz) mask over the STATIC pattern (every entry, masked or not, in row-major
    order): what the engine draws under use_adj.  `_RefStream.attn` reads the pattern off its adjacency argument, which is
    the per-snapshot (S, N, N) one here."""

    def __init__(self, seed, static):
        super().__init__(seed)
        self.static = np.asarray(static, dtype=np.float64).copy()
        np.fill_diagonal(self.static, 1.0)

    def attn(self, coef, a_hat, rate=0.5):
        return _RefStream.attn(self, coef, torch.from_numpy(self.static), rate)


@pytest.mark.parametrize('act', ['tanh', 'relu'])
def test_masked_layer_gradients_match_the_dense_restatement(dev, networks, act):
    net = networks['shunqing']
    gph = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    csr, a_dense = _static_with_loops(gph)
    g = torch.Generator().manual_seed(5)
    S, F, C = 4, 24, 16
    mask = _seeded_mask(csr, S, seed=3)
    x = torch.randn(S, gph.n_node, F, generator=g, dtype=torch.float64)
    layer = U.GATConv(C, activation=act, in_channels=F, generator=g).to(dev)
    with torch.no_grad():
        layer.bias.normal_(0.0, 0.1)
    xd = x.float().to(dev).requires_grad_(True)
    layer.requires_grad_(True)
    out = layer([xd, csr], edge_mask=torch.from_numpy(mask).to(dev))
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gy.float().to(dev)).sum().backward()
    ref_p = [p.detach().double().cpu().requires_grad_(True) for p in (layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias)]
    xr = x.clone().requires_grad_(True)
    ref = OD.gat_conv_dense(xr, _dense_adjacency(csr, mask), *ref_p, act)
    (ref * gy).sum().backward()
    close(out.detach(), ref.detach(), 1e-5)
    for got, want in [(xd.grad, xr.grad)] + [(p.grad, r.grad) for p, r in zip((layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias), ref_p)]:
        close(got, want, 1e-5)
    static = OD.gat_conv_dense(x, torch.from_numpy(a_dense), *[p.detach() for p in ref_p], act)
    assert float((static - ref.detach()).abs().max()) > 1e-2          # the mask does something


def test_masked_layer_with_attention_dropout(dev, networks):
    net = networks['shunqing']
    gph = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    csr, a_dense = _static_with_loops(gph)
    g = torch.Generator().manual_seed(4)
    S, F, C = 3, 24, 16
    mask = _seeded_mask(csr, S, seed=9)
    x = torch.randn(S, gph.n_node, F, generator=g, dtype=torch.float64)
    layer = U.GATConv(C, activation='tanh', in_channels=F, generator=g).to(dev)
    with torch.no_grad():
        layer.bias.normal_(0.0, 0.1)
    st = DropoutStream(seed=99)
    xd = x.float().to(dev).requires_grad_(True)
    layer.requires_grad_(True)
    out = layer([xd, csr], edge_mask=torch.from_numpy(mask).to(dev), attn_dropout=st)
    assert st.offset == (S * csr.nnz + 3) // 4 * 4          # one draw over every entry of the static pattern, masked or not
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gy.float().to(dev)).sum().backward()
    ref_p = [p.detach().double().cpu().requires_grad_(True) for p in (layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias)]
    xr = x.clone().requires_grad_(True)
    rs = _StaticAttnStream(99, a_dense)
    OD.ATTN_DROPOUT = rs.attn
    try:
        ref = OD.gat_conv_dense(xr, _dense_adjacency(csr, mask), *ref_p, 'tanh')
    finally:
        OD.ATTN_DROPOUT = None
    (ref * gy).sum().backward()
    assert st.offset == rs.offset
    close(out.detach(), ref.detach(), 2e-5)
    for got, want in [(xd.grad, xr.grad)] + [(p.grad, r.grad) for p, r in zip((layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias), ref_p)]:
        err, scale = float((got.double().cpu() - want).abs().max()), float(want.abs().max())
        assert err <= 1e-4 * scale + 1e-7, (err, scale)
    # no gradients, training mode: still the dropout path (same stream position -> same output), not the inference kernel
    st.reseed(99)
    with torch.no_grad():
        again = layer([xd.detach(), csr], edge_mask=torch.from_numpy(mask).to(dev), attn_dropout=st)
        plain = layer([xd.detach(), csr], edge_mask=torch.from_numpy(mask).to(dev))
    assert torch.equal(again, out.detach())
    assert float((plain - again).abs().max()) > 1e-2


def test_masked_layer_on_the_matrix_core_path(dev):
    """Headline network, S * n >= 4096 and widths of the matrix-core row GEMM: GatFn's fast linear part, then the _ex kernels;
    against the fp64 sparse oracle per snapshot on the pruned pattern.  tanh, not relu: among 2.5 M pre-activations some lie
    within the forward's rounding of 0, and a relu' that flips there moves the input gradient by a whole upstream gradient
    entry (the unmasked path misses 4e-5 there by the same amount); the smooth activation leaves the operator's own error."""
    csr = _pattern('headline')
    g = torch.Generator().manual_seed(8)
    S, F, C = 2, 64, 128
    mask = _seeded_mask(csr, S, seed=21)
    x = torch.randn(S, csr.n_rows, F, generator=g, dtype=torch.float64) * 0.5
    layer = U.GATConv(C, activation='tanh', in_channels=F, generator=g).to(dev)
    layer.precision = 'bf16x3'
    with torch.no_grad():
        layer.bias.normal_(0.0, 0.1)
    xd = x.float().to(dev).requires_grad_(True)
    layer.requires_grad_(True)
    out = layer([xd, csr], edge_mask=torch.from_numpy(mask).to(dev))
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * gy.float().to(dev)).sum().backward()
    ref_p = [p.detach().double().cpu().requires_grad_(True) for p in (layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias)]
    xr = x.clone().requires_grad_(True)
    refs = []
    for s in range(S):
        sub, _ = _pruned(csr, mask[s] != 0)
        refs.append(OS.gat_conv_csr(xr[s:s + 1], sub.rowptr, sub.col, *ref_p, 'tanh'))
    ref = torch.cat(refs)
    (ref * gy).sum().backward()
    close(out.detach(), ref.detach(), 4e-5)
    for got, want in [(xd.grad, xr.grad)] + [(p.grad, r.grad) for p, r in zip((layer.kernel, layer.attn_kernel_self, layer.attn_kernel_neighs, layer.bias), ref_p)]:
        close(got, want, 4e-5)


# ---------------------------------------------------------------------------------------------------------------- 4 / 5: whole model

def _adj_problem(networks, name, dev, seed=3, B=2, **over):
    """_problem's model with act_edges = edges[::2] and use_adj, and its inputs drawn in _problem's order from the same seed
    except for the settings: a = (rand > 0.4) * (0.5 + rand) -- about 40 % closed, the rest in [0.5, 1.5), so truncation
    removes the entry of every setting below 1."""
    edges = np.array(networks[name]['edges'])
    args, norms, params, emul, _, _ = _problem(networks, name, dev, use_adj=True, act_edges=edges[::2], **over)
    assert emul.use_adj
    c = OE.config(args)
    n = c.n_node
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    T_out = c.seq_out * max(c.roll, 1)
    x, b, ex = rnd(B, c.seq_in, n, c.n_in), rnd(B, T_out, n, c.b_in) * 0.1, rnd(B, c.seq_in, len(edges), c.e_in)
    a = (rnd(B, T_out, len(args.act_edges)) > 0.4).double() * (0.5 + rnd(B, T_out, len(args.act_edges)))
    y = rnd(B, T_out, n, 5)
    y[..., -2] = (y[..., -2] > 0.7).double()
    ey = rnd(B, T_out, len(edges), 3)
    cpu_in = (x, a, b, y, ex, ey)
    return args, norms, params, emul, cpu_in, tuple(t.float().to(dev) for t in cpu_in)


def _ref_losses(args, params, norms, x, a, b, y, ex, ey, use_adj=True):
    """OT.losses (no balance, no roll) with the per-time-step adjacency of the settings passed to OE.forward."""
    c = OE.config(args)
    assert not getattr(args, 'balance', False) and not c.roll
    lw = OT.loss_weights(args, x.dtype)
    ae = OE.get_edge_action(c, a)
    adj = OE.get_adj_action(c, a) if use_adj else None
    yp, eyp = OE.forward(args, params, x, b, ex, ae, adj)
    yp, eyp = OE.post_proc(args, norms, yp, eyp, a, b)
    preds = yp.clamp(0, 1)
    out = [OT.mse(y[..., :3] * lw['nwei'], preds[..., :3] * lw['nwei'])]
    if c.if_flood:
        weight = lw['poswei'] * y[..., -2] + lw['nwei'][:, -1] * (1 - y[..., -2])
        out.append(OT.bce(y[..., -2:-1], preds[..., -1:], weight))
    out.append(OT.mse(ey, eyp, lw['ewei']))
    return out


def _ref_grads(args, params, norms, x, a, b, y, ex, ey, use_adj=True):
    leaves = list(OT.tree_leaves(params))
    for _, t in leaves:
        t.requires_grad_(True)
        t.grad = None
    ls = _ref_losses(args, params, norms, x, a, b, y, ex, ey, use_adj)
    sum(ls).backward()
    out = {n: (t.grad.clone() if t.grad is not None else torch.zeros_like(t)) for n, t in leaves}
    for _, t in leaves:
        t.requires_grad_(False)
        t.grad = None
    return [l.detach() for l in ls], out


def _check_model_grads(emul, args, dev_in, ref_losses, ref_grads):
    emul.requires_grad_(True)
    xd, ad, bd, yd, exd, eyd = dev_in
    ae = emul.get_edge_action(ad, True)
    preds, edge_preds = emul._model(xd, ad, bd, exd, ae, None, True)
    lw = emul._loss_setup(xd.device)
    ls = [emul.get_node_loss(yd, bd, preds)] + ([emul.get_flood_loss(yd, preds)] if emul.if_flood else []) + [emul._mse(eyd, edge_preds, lw['ewei'])]
    for got, ref in zip(ls, ref_losses):
        close(got, ref, 2e-5)
    sum(ls).backward()
    gmax = max(float(t.abs().max()) for t in ref_grads.values())
    n_checked = 0
    for pname, p, ref in emulator_param_pairs(emul, ref_grads):
        got = p.grad.detach().double().cpu() if p.grad is not None else torch.zeros_like(ref)
        ref = ref.reshape(got.shape)
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        assert err <= GRAD_TOL['GAT'] * scale + 1e-7 * gmax, '%s: grad err %.3e vs max|grad| %.3e' % (pname, err, scale)
        n_checked += 1
    assert n_checked == len(list(emul.parameters()))


def _mask_moves_the_gradients(ref_grads, free_grads):
    """max over tensors of |grad with ADJ - grad without| / its GRAD_TOL bound: the check above could not pass ignoring the mask."""
    gmax = max(float(t.abs().max()) for t in ref_grads.values())
    return max(float((ref_grads[k] - free_grads[k]).abs().max()) / (GRAD_TOL['GAT'] * float(ref_grads[k].abs().max()) + 1e-7 * gmax)
               for k in ref_grads)


def _attn_hook(st):
    """Attention-dropout hook of the oracle for a use_adj model: block 2's node side (graph_base: the combined graph) receives
    the per-snapshot (S, N, N) adjacency, laid over the static pattern `st.static`; every other GATConv (block 1, the line
    graph) receives its static 2-D filter, as in tests/test_gpu_dropout.py."""
    def attn(coef, a_hat, rate=0.5):
        return st.attn(coef, a_hat, rate) if a_hat.dim() == 3 else _RefStream.attn(st, coef, a_hat, rate)
    return attn


CASES = [('astlingen', dict(n_sp_layer=1)), ('shunqing', dict()), ('astlingen', dict(graph_base=1, n_sp_layer=2))]


@pytest.mark.parametrize('name,over', CASES)
def test_use_adj_emulator_gradients(dev, networks, name, over):
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, name, dev, **over)
    x, a, b, y, ex, ey = cpu_in
    c = OE.config(args)
    # the engine's fp32 truncation of the settings gives the oracle's fp64 adjacency at every pattern entry
    csr, _, _ = emul._adj_pattern()
    rows, col = _rows(csr), np.asarray(csr.col, dtype=np.int64)
    adj = OE.get_adj_action(c, a).clone()
    idx = torch.arange(adj.shape[-1])
    adj[..., idx, idx] = 1.0
    want = (adj[..., rows, col] != 0).float()
    got = emul.get_adj_action(dev_in[1]).cpu()
    assert torch.equal(got.reshape(want.shape), want)
    assert float((want == 0).sum()) > 0
    ref_losses, ref_grads = _ref_grads(args, params, norms, x, a, b, y, ex, ey)
    _, free_grads = _ref_grads(args, params, norms, x, a, b, y, ex, ey, use_adj=False)
    assert _mask_moves_the_gradients(ref_grads, free_grads) > 10.0
    _check_model_grads(emul, args, dev_in, ref_losses, ref_grads)


@pytest.mark.parametrize('name,over', [('astlingen', dict(dropout=0.1, n_sp_layer=1)), ('astlingen', dict(dropout=0.1, graph_base=1, n_sp_layer=1))])
def test_use_adj_emulator_gradients_under_dropout(dev, networks, name, over):
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, name, dev, **over)
    assert emul.dropout and emul.dropout_stream is not None
    x, a, b, y, ex, ey = cpu_in
    c = OE.config(args)
    emul.dropout_stream.reseed(2024)
    OE.DROPOUT = st = _StaticAttnStream(2024, c.adj)
    OD.ATTN_DROPOUT = _attn_hook(st)
    try:
        ref_losses, ref_grads = _ref_grads(args, params, norms, x, a, b, y, ex, ey)
    finally:
        OE.DROPOUT = OD.ATTN_DROPOUT = None
    _check_model_grads(emul, args, dev_in, ref_losses, ref_grads)


def test_graph_base_use_adj_training_mode_without_gradients_applies_attention_dropout(dev, networks):
    """ADVICE finding: graph_base + use_adj with training=True and no input requiring grad used to return the inference output
    (the edge-mask branch returned before the attention-dropout draw).  Now: the oracle's attention-dropout output, same stream."""
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, dropout=0.1, graph_base=1, n_sp_layer=1)
    x, a, b, y, ex, ey = cpu_in
    c = OE.config(args)
    xd, ad, bd, yd, exd, eyd = dev_in
    emul.requires_grad_(False)
    emul.dropout_stream.reseed(7)
    with torch.no_grad():
        got, got_e = emul.forward(xd, bd, exd, emul.get_edge_action(ad, True), emul.get_adj_action(ad, True), training=True)
        inf, _ = emul.forward(xd, bd, exd, emul.get_edge_action(ad, True), emul.get_adj_action(ad, True), training=False)
    OE.DROPOUT = st = _StaticAttnStream(7, c.adj)
    OD.ATTN_DROPOUT = _attn_hook(st)
    try:
        ref, ref_e = OE.forward(args, params, x, b, ex, OE.get_edge_action(c, a), OE.get_adj_action(c, a))
    finally:
        OE.DROPOUT = OD.ATTN_DROPOUT = None
    assert emul.dropout_stream.offset == st.offset
    close(got, ref, 2e-5)
    close(got_e, ref_e, 2e-5)
    assert float((got - inf).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- 6: training loops

def test_use_adj_fit_eval_steps_match_oracle_adam(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, embed_size=64, n_sp_layer=1, learning_rate=1e-3)
    x, a, b, y, ex, ey = cpu_in
    opt = OT.Adam(lr=1e-3)
    leaves = list(OT.tree_leaves(params))
    ref_hist = []
    for _ in range(3):
        ls, gr = _ref_grads(args, params, norms, x, a, b, y, ex, ey)
        ref_hist.append([float(l) for l in ls])
        opt.step(leaves, gr)
    hist = [[float(l) for l in emul.fit_eval(*dev_in)] for _ in range(3)]
    for h, r in zip(hist, ref_hist):
        assert np.allclose(h, r, rtol=2e-3, atol=1e-5), (hist, ref_hist)
    after = dict(OT.tree_leaves(params))
    for pname, p, ref in emulator_param_pairs(emul, after):
        err = float((p.detach().double().cpu() - ref).abs().max())
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)


def test_use_adj_rollout_and_grad_norm_train(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, roll=2, seq_in=4, seq_out=2, n_sp_layer=1)
    for _ in range(2):
        ls = emul.fit_eval(*dev_in)
        assert all(np.isfinite(float(v)) for v in ls)
    # every parameter receives a (finite) gradient through the rolled-out, masked model
    emul.requires_grad_(True)
    emul.zero_grad(set_to_none=True)
    xd, ad, bd, yd, exd, eyd = dev_in
    preds, edge_preds = emul._model(xd, ad, bd, exd, None, None, True)
    lw = emul._loss_setup(dev)
    ls = [emul.get_node_loss(yd, bd, preds)] + ([emul.get_flood_loss(yd, preds)] if emul.if_flood else []) + [emul._mse(eyd, edge_preds, lw['ewei'])]
    sum(ls).backward()
    missing = [n for n, p in emul.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing

    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, embed_size=64, n_sp_layer=1, gradnorm=True)
    ini = [float(l) for l in emul.fit_eval(*dev_in, fit=False)]
    for _ in range(2):
        loss = emul.fit_grad_norm(*dev_in, ini)
        assert np.isfinite(float(loss))
        got = emul._alphas(dev).detach().double().cpu()
        assert abs(float(got.sum()) - 2.0) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 7: MPC

def test_use_adj_mpc_objective_and_gradient(dev, networks, monkeypatch):
    from gnn_uds_amd import mpc as M
    from tests.util import emulator_args, emulator_norms, load_emulator
    net = networks['astlingen']
    edges, n = np.array(net['edges']), net['n_node']
    args = emulator_args(edges, n, seq_in=4, seq_out=2, n_sp_layer=1, if_flood=1, epsilon=0.0, use_adj=True, act_edges=edges[::2])
    norms = emulator_norms(args)
    params = OE.init_params(args, seed=3)
    c = OE.config(args)
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    T = c.seq_out
    state, runoff, edge_state = rnd(c.seq_in, n, 5), rnd(T, n, 1) * 0.05, rnd(c.seq_in, len(edges), 4)
    state[..., 3] = (state[..., 3] > 0.8).double()
    pop, n_step, n_act, r_step = 3, 1, len(args.act_edges), 2
    # decision values on both sides of 1, none within 1e-3 of an integer
    y = 0.3 + 1.2 * rnd(pop, n_step * n_act)
    y = torch.where((y - y.round()).abs() < 1e-3, y + 3e-3, y)
    assert (y < 1).any() and (y > 1).any() and float((y - y.round()).abs().min()) >= 1e-3
    tg = dict(flood_idx=torch.tensor([3, 7, 11]), flood_w=torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64),
              outflow_idx=torch.tensor([0]), outflow_w=torch.tensor([0.3], dtype=torch.float64),
              smooth_idx=torch.tensor([5, 9]), smooth_w=torch.tensor([0.7, 0.2], dtype=torch.float64))
    gamma = torch.tensor([1.0, 0.9, 0.8, 0.7][:T], dtype=torch.float64)
    idx = torch.as_tensor(OE._act_edge_index(c))
    fwd = OE.forward

    def forward_with_adj(args_, params_, X, B, E, AE=None, ADJ=None):
        # the settings are the actuated links' column of the edge action; ADJ is piecewise constant in them (no gradient)
        a_ = AE[..., idx, 0].detach()
        return fwd(args_, params_, X, B, E, AE, OE.get_adj_action(c, a_) if ADJ is None else ADJ)
    monkeypatch.setattr(OE, 'forward', forward_with_adj)
    yr = y.clone().requires_grad_(True)
    ref = OE.mpc_objective(args, params, norms, yr, state, runoff, edge_state, n_step, n_act, r_step, tg, gamma)
    (gref,) = torch.autograd.grad(ref.sum(), yr)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    assert emul.use_adj
    f = lambda t: t.float().to(dev)
    tgd = {k: (v.to(dev) if v.dtype == torch.int64 else f(v)) for k, v in tg.items()}
    obj, grad = M.objective_and_gradient(emul, f(y), f(state), f(runoff), f(edge_state), n_step, n_act, r_step, tgd, f(gamma))
    close(obj, ref.detach(), 2e-5)
    gmax = float(gref.abs().max())
    assert gmax > 0
    err = float((grad.double().cpu() - gref).abs().max())
    assert err <= 2e-3 * gmax, 'gradient err %.3e vs max|grad| %.3e' % (err, gmax)
    pvec = rnd(pop, n_step * n_act) - 0.5
    hp = M.hessp(emul, f(y), f(pvec), f(state), f(runoff), f(edge_state), n_step, n_act, r_step, tgd, f(gamma))
    assert tuple(hp.shape) == (pop, n_step * n_act) and bool(torch.isfinite(hp).all())
