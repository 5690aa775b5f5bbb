"""uds_gat_backward_act (k_gat_bwd_rows_g<G,NC,EX,true> / k_gat_bwd_rows<true>, k_gat_bwd_cols_g<G,NC,true> / k_gat_bwd_cols<true>,
k_gat_bwd_act_reduce), autograd.GatFn(fused_bwd=True) and Emulator.fused_gat_backward.

Entry level, per (width, S) on a 37-row degree ladder, every activation x {plain, mask, coef, both}:
  d_hx, ds_self, ds_nbr   torch.equal to what GatFn.backward calls on autograd.act_grad(out, gout, act) -- _lib.gat_backward_ex with an
                          edge mask, _lib.gat_backward (with the coef, if any) without one: the fold moves no bit
  db, da                  against the fp64 restatement (tests/test_gat_backward_act_math.py: restate) fed the same fp32 out / gout,
                          within GRAD_TOL['GAT'] * max|that gradient| + 1e-7 * max|any of the two| -- the bound _check_model_grads
                          of tests/test_gpu_use_adj_train.py puts on these gradients.  The error of the chain (g.sum(0), weight_grad)
                          against the same values is printed beside it.
  two runs bitwise equal; outputs in NaN-filled guarded buffers, the workspace guarded; inputs unchanged; want_db / want_da.
Widths: 16, 64, 128 (grouped kernels, G = 4, 16, 16 x 2 chunks) and 12 (the walking kernels).  n = 37 leaves the last row block
partly filled at every width; at d = 64 a workgroup holds 16 rows, so three workgroups (nine at S = 3) write partials and
S * n is no multiple of 16 (asserted).  One large case (d = 16, 3 x 44805 rows) has more row blocks than GAT_ACT_WG_MAX, so a
workgroup owns two.

Model level (astlingen, B = 2): gradients with Emulator.fused_gat_backward off and on -- every parameter but the GAT biases and
attention kernels bit-identical, all of them within GRAD_TOL['GAT'] of the fp64 oracle (_check_model_grads) -- for a plain, a
use_adj (graph_base) and a dropout model, and three fit_eval steps within the bound of test_use_adj_fit_eval_steps_match_oracle_adam.

Worst observed / allowed on an MI355X over all entry-level cases: db 0.0002, da 0.0004 (fused errors 2e-8 .. 4e-8 where the chain's
split-bf16 da has 3e-7 .. 7e-7 on the same inputs).

The plain model case is one of tests/test_gpu_train.py::test_emulator_gradients: astlingen with n_sp_layer=2 and the defaults misses
GRAD_TOL on embed_x.kernel (3.6e-5 against 1.0e-5 allowed) with the flag off and on alike, so it says nothing about the flag."""
import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from gnn_uds_amd import autograd as AG
from gnn_uds_amd.layers import GATConv
from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from oracle import train_ref as OT
from tests.test_gat_backward_act_math import ACTS, WG_MAX, restate
from tests.test_gpu_train import GRAD_TOL, _problem
from tests.test_gpu_use_adj_train import _StaticAttnStream, _adj_problem, _attn_hook, _check_model_grads, _ref_grads
from tests.util import Guarded, _pairs_csr, emulator_param_pairs, ladder, nan_in, sparse_lanes

pytestmark = pytest.mark.gpu

N = 37
VARIANTS = {'plain': (False, False), 'mask': (True, False), 'coef': (False, True), 'both': (True, True)}
LADDER = (2, 3, 4, 5, 8, 9, 16, 17)       # entries of rows 1 .. 8: G, G + 1 for G = 2, 4, 8, 16 (and 2 G = 4, 8, 16)
HUB = 32                                  # entries of the last row: its diagonal and 31 neighbours


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def small_ladder(n=N):
    """Directed n-row pattern in the manner of tests.util.ladder: every row holds its diagonal; rows 1 .. 8 hold LADDER[r - 1]
    entries, the last row 32 (a hub with 31 neighbours), rows 9 .. 12 point at node 0 (a column of the transposed pattern with
    more entries than most rows), every other row is isolated (its diagonal only)."""
    rng = np.random.default_rng(n)
    pairs = {(r, r) for r in range(n)}
    for r, deg in list(zip(range(1, 9), LADDER)) + [(n - 1, HUB)]:
        pairs |= {(r, int(c)) for c in rng.choice([c for c in range(n) if c != r], deg - 1, replace=False)}
    pairs |= {(r, 0) for r in range(9, 13)}
    return _pairs_csr(pairs, n, n)


class Case:
    """A pattern with handles and, per (S, d), fp32 operands on the device: hx, scores, attention kernels, gout, mask, coef."""

    def __init__(self, csr, dev):
        self.csr, self.n, self.dev = csr, csr.n_rows, dev
        self.h = _lib.CsrHandle(csr)
        self.ht, self.perm = self.h.transposed(dev)
        self.rows = torch.from_numpy(np.repeat(np.arange(csr.n_rows), np.diff(csr.rowptr.astype(np.int64))))
        self.col = torch.from_numpy(csr.col.astype(np.int64))

    def operands(self, S, d, seed=0):
        g = torch.Generator().manual_seed(1000 * S + d + seed)
        u = lambda *s: (torch.rand(*s, generator=g) - 0.5)
        nnz = self.csr.nnz
        op = dict(hx=u(S, self.n, d), gout=u(S, self.n, d), pre=u(S, self.n, d) * 8, ss=u(S, self.n) * 4, sn=u(S, self.n) * 4, a_self=u(d), a_nbr=u(d))
        mask = (torch.rand(S, nnz, generator=g) > 1.0 / 3.0).float()
        mask[0, self.rows == self.n - 1] = 0.0           # the hub row of snapshot 0 and row 7 everywhere: down to the diagonal
        mask[:, self.rows == 7] = 0.0
        op['mask'] = mask
        op['coef'] = (torch.rand(S, nnz, generator=g) > 0.5).float() * 2.0
        return op, {k: nan_in(v, self.dev) for k, v in op.items()}


@pytest.fixture(scope='module')
def case37(dev):
    csr = small_ladder()
    deg = np.diff(csr.rowptr)
    assert list(deg[1:9]) == list(LADDER) and deg[N - 1] == HUB and (deg == 1).sum() >= 10
    return Case(csr, dev)


def _bound(ref, gmax):
    return GRAD_TOL['GAT'] * float(ref.abs().max()) + 1e-7 * gmax


def _fused(cs, dv, act, variant, S, d, want_db=True, want_da=True):
    """One guarded call of the operator: (d_hx, ds_self, ds_nbr, db, da)."""
    mk, cf = VARIANTS[variant]
    dev, n, nnz = cs.dev, cs.n, cs.csr.nnz
    outs = [Guarded((S, n, d), dev), Guarded((S, n), dev), Guarded((S, n), dev), Guarded((d,), dev), Guarded((2, d), dev)]
    for o in outs:
        o.view.fill_(float('nan'))
    need = _lib.gat_backward_act_workspace_floats(S, n, nnz, d)
    ws = Guarded((need,), dev, torch.full((need,), float('nan')))
    views = tuple(o.view for o in outs)
    got = _lib.gat_backward_act(cs.h, cs.ht, cs.perm, dv['out'], dv['gout'], act, dv['hx'], dv['ss'], dv['sn'], dv['a_self'], dv['a_nbr'],
                                edge_mask=dv['mask'] if mk else None, coef=dv['coef'] if cf else None, want_db=want_db, want_da=want_da,
                                outputs=views, workspace=ws.view)
    torch.cuda.synchronize()
    for o, g_, name, want in zip(outs, got, ('d_hx', 'ds_self', 'ds_nbr', 'db', 'da'), (True, True, True, want_db, want_da)):
        if want:
            assert g_ is o.view
            o.check(name)
        else:
            assert g_ is None and bool(torch.isnan(o.view).all())       # not wanted: not returned, not written
            o.view.zero_()
            o.check(name)
    bits = ws.buf.view(torch.int32)
    from tests.util import PAD, SENTINEL
    assert bool((bits[:PAD] == SENTINEL).all()) and bool((bits[PAD + need:] == SENTINEL).all()), 'workspace: written outside'
    return got


def _chain(cs, dv, act, variant):
    """Today's steps on the same operands: (d_hx, ds_self, ds_nbr, db, da)."""
    mk, cf = VARIANTS[variant]
    g = AG.act_grad(dv['out'], dv['gout'], act).contiguous()
    if mk:          # as GatFn.backward chooses: the _ex entry with an edge mask, gat_backward (with the coef, if any) without one
        r = _lib.gat_backward_ex(cs.h, cs.ht, cs.perm, g, dv['hx'], dv['ss'], dv['sn'], dv['a_self'], dv['a_nbr'],
                                 edge_mask=dv['mask'], coef=dv['coef'] if cf else None)
    else:
        r = _lib.gat_backward(cs.h, cs.ht, cs.perm, g, dv['hx'], dv['ss'], dv['sn'], dv['a_self'], dv['a_nbr'], coef=dv['coef'] if cf else None)
    db = g.reshape(-1, g.shape[-1]).sum(0)
    da = AG.weight_grad(torch.stack([r[1], r[2]], dim=-1), dv['hx'], 'bf16x3', False)[0]
    return r + (db, da)


def _check_call(cs, op, dv, act, variant, S, d, worst):
    mk, cf = VARIANTS[variant]
    dv = dict(dv, out=nan_in(AG.apply_activation(op['pre'].to(cs.dev), act).contiguous(), cs.dev))
    before = {k: v.clone() for k, v in dv.items()}
    got = _fused(cs, dv, act, variant, S, d)
    old = _chain(cs, dv, act, variant)
    for name, a, b in zip(('d_hx', 'ds_self', 'ds_nbr'), got, old):
        assert torch.equal(a, b), '%s d%d S%d %s: %s differs from the chain' % (act, d, S, variant, name)
    out64 = dv['out'].double().cpu()
    if act == 'relu':
        assert bool((out64 == 0).any()) and bool((out64 > 0).any())
    if act == 'hard_sigmoid':
        assert bool((out64 == 0).any()) and bool((out64 == 1).any()) and bool(((out64 > 0) & (out64 < 1)).any())
    ref = restate(cs.rows, cs.col, out64, op['gout'].double(), act, op['hx'].double(), op['ss'].double(), op['sn'].double(),
                  op['a_self'].double(), op['a_nbr'].double(), op['mask'].double() if mk else None, op['coef'].double() if cf else None)
    gmax = max(float(ref[3].abs().max()), float(ref[4].abs().max()))
    for name, k in (('db', 3), ('da', 4)):
        err, err_old = float((got[k].double().cpu() - ref[k]).abs().max()), float((old[k].double().cpu() - ref[k]).abs().max())
        allowed = _bound(ref[k], gmax)
        print('%-12s d%-3d S%d %-5s %s: fused err %.3e  chain err %.3e  allowed %.3e  ratio %.4f' % (act, d, S, variant, name, err, err_old, allowed, err / allowed))
        worst[name] = max(worst[name], err / allowed)
        assert float(ref[k].abs().max()) > 1e-3
        assert err <= allowed, '%s d%d S%d %s: %s err %.3e, allowed %.3e (chain: %.3e)' % (act, d, S, variant, name, err, allowed, err_old)
    again = _fused(cs, dv, act, variant, S, d)
    for name, a, b in zip(('d_hx', 'ds_self', 'ds_nbr', 'db', 'da'), got, again):
        assert torch.equal(a, b), '%s: two runs differ' % name
    for k, v in before.items():
        assert torch.equal(v, dv[k]), 'input %s changed' % k
    return got


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('d', [16, 64, 128, 12])
def test_operator_against_the_chain_and_the_fp64_restatement(dev, case37, d, S):
    cs = case37
    G = sparse_lanes(d)[0]
    if d == 64:
        rows_per_wg = 256 // G
        assert rows_per_wg == 16 and -(-N // rows_per_wg) * S >= 3 and (S * N) % rows_per_wg != 0
    assert (G == 0) == (d == 12)
    op, dv = cs.operands(S, d)
    worst = dict(db=0.0, da=0.0)
    for act in ACTS:
        for variant in VARIANTS:
            _check_call(cs, op, dv, act, variant, S, d, worst)
    print('d%d S%d worst observed / allowed: db %.4f  da %.4f' % (d, S, worst['db'], worst['da']))


@pytest.mark.parametrize('d', [64, 12])
def test_unwanted_gradients_are_not_computed(dev, case37, d):
    S, cs = 3, case37
    op, dv = cs.operands(S, d)
    dv = dict(dv, out=nan_in(torch.tanh(op['pre']).to(dev), dev))
    full = _fused(cs, dv, 'tanh', 'both', S, d)
    for want_db, want_da in ((False, True), (True, False), (False, False)):
        part = _fused(cs, dv, 'tanh', 'both', S, d, want_db=want_db, want_da=want_da)
        assert (part[3] is None) == (not want_db) and (part[4] is None) == (not want_da)
        for a, b in zip(full, part):
            assert b is None or torch.equal(a, b)


def test_linear_activation_reads_gout_in_place(dev, case37):
    """act = linear stores no g (the column pass gathers gout): its part of the NaN-filled workspace stays NaN."""
    S, d, cs = 3, 64, case37
    op, dv = cs.operands(S, d)
    dv = dict(dv, out=nan_in(op['pre'].to(dev), dev))
    need = _lib.gat_backward_act_workspace_floats(S, cs.n, cs.csr.nnz, d)
    ws = torch.full((need,), float('nan'), device=dev)
    got = _lib.gat_backward_act(cs.h, cs.ht, cs.perm, dv['out'], dv['gout'], 'linear', dv['hx'], dv['ss'], dv['sn'], dv['a_self'], dv['a_nbr'],
                                workspace=ws)
    a4 = (S * cs.csr.nnz + 3) // 4 * 4
    assert bool(torch.isnan(ws[2 * a4:2 * a4 + S * cs.n * d]).all())
    assert all(bool(torch.isfinite(t).all()) for t in got)


def test_a_workgroup_owns_several_row_blocks(dev):
    """d = 16: 64 rows per block; 3 snapshots of 701 blocks are more items than GAT_ACT_WG_MAX, so every workgroup owns two
    consecutive blocks -- the last one of a snapshot and the first of the next among them -- and the last workgroup one."""
    S, d, n = 3, 16, 64 * 700 + 5
    blocks = -(-n // 64)
    assert blocks * S > WG_MAX and -(-blocks * S // WG_MAX) == 2 and blocks % 2 == 1
    cs = Case(ladder(n), dev)
    op, dv = cs.operands(S, d)
    worst = dict(db=0.0, da=0.0)
    for act, variant in (('tanh', 'plain'), ('relu', 'both')):
        _check_call(cs, op, dv, act, variant, S, d, worst)


def test_entry_refusals(dev, case37):
    cs, S, d = case37, 1, 16
    op, dv = cs.operands(S, d)
    dv = dict(dv, out=dv['gout'].clone())
    z = lambda *s: torch.zeros(*s, device=dev)
    lib = _lib.load()
    need = _lib.gat_backward_act_workspace_floats(S, N, cs.csr.nnz, d)
    ws, d_hx, ds1, ds2, db, da = z(need), z(S, N, d), z(S, N), z(S, N), torch.full((d,), 7.0, device=dev), z(2, d)
    p = lambda t: None if t is None else t.data_ptr()

    def call(handle_t=cs.ht, act=1, dd=d, ws_n=need, out=dv['out']):
        return lib.uds_gat_backward_act(cs.h.ptr, handle_t.ptr, p(cs.perm), p(out), p(dv['gout']), act, p(dv['hx']), p(dv['ss']), p(dv['sn']),
                                        p(dv['a_self']), p(dv['a_nbr']), None, None, S, dd, p(d_hx), p(ds1), p(ds2), p(db), p(da), p(ws), ws_n,
                                        torch.cuda.current_stream().cuda_stream)
    other = Case(small_ladder(41), dev)
    for kw, text in ((dict(act=5), b'unknown activation'), (dict(act=-1), b'unknown activation'), (dict(ws_n=need - 1), b'workspace'),
                     (dict(handle_t=other.ht), b'transpose'), (dict(dd=18), b'multiple of 4'), (dict(out=None), b'NULL')):
        assert call(**kw) == -22 and text in lib.uds_last_error(), (kw, lib.uds_last_error())
    torch.cuda.synchronize()
    assert bool((db == 7.0).all())                       # a refused call wrote nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((db == 7.0).any())


# ------------------------------------------------------------------------------------------------------------ model level

def _gat_parameter_ids(emul):
    ids = set()
    for m in emul.modules():
        if isinstance(m, GATConv):
            ids |= {id(t) for t in (m.bias, m.attn_kernel_self, m.attn_kernel_neighs) if t is not None}
    return ids


def _grads_off_and_on(emul, check):
    """check() runs the model's gradients and asserts them against the oracle; returns the gradients with the flag off and on."""
    res = {}
    for on in (False, True):
        emul.fused_gat_backward = on
        assert all(m.fused_backward == on for m in emul.modules() if isinstance(m, GATConv))
        for p in emul.parameters():
            p.grad = None
        AG.GAT_BWD_COUNTS['fused'] = AG.GAT_BWD_COUNTS['chain'] = 0
        try:
            check()
        except AssertionError as err:
            raise AssertionError('fused_gat_backward = %r: %s' % (on, err)) from err
        ran, idle = ('fused', 'chain') if on else ('chain', 'fused')
        assert AG.GAT_BWD_COUNTS[ran] >= sum(isinstance(m, GATConv) for m in emul.modules()) and AG.GAT_BWD_COUNTS[idle] == 0, AG.GAT_BWD_COUNTS
        res[on] = {name: p.grad.clone() for name, p in emul.named_parameters()}
    gat = _gat_parameter_ids(emul)
    n_same = 0
    for name, p in emul.named_parameters():
        if id(p) not in gat:
            assert torch.equal(res[False][name], res[True][name]), '%s: the flag moved a gradient it does not compute' % name
            n_same += 1
    assert gat and n_same
    return res


def test_emulator_gradients_with_the_flag_off_and_on(dev, networks):
    # a case of tests/test_gpu_train.py::test_emulator_gradients (a non-relu activation through the fold)
    args, norms, params, emul, cpu_in, dev_in = _problem(networks, 'astlingen', dev, activation='tanh', n_sp_layer=1)
    assert not emul.fused_gat_backward                                      # off by default
    ref_losses, ref_grads = OT.grads(args, params, norms, *cpu_in)
    _grads_off_and_on(emul, lambda: _check_model_grads(emul, args, dev_in, ref_losses, ref_grads))


def test_use_adj_graph_base_emulator_gradients(dev, networks):
    """The edge-mask path, and the graph_base block's GAT layers are reached by the flag."""
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, graph_base=1, n_sp_layer=2)
    ref_losses, ref_grads = _ref_grads(args, params, norms, *cpu_in)
    _grads_off_and_on(emul, lambda: _check_model_grads(emul, args, dev_in, ref_losses, ref_grads))


def test_dropout_emulator_gradients(dev, networks):
    """The attention-dropout coef path (with the edge mask of use_adj on block 2's node side)."""
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, dropout=0.1, n_sp_layer=1)
    c = OE.config(args)
    OE.DROPOUT = st = _StaticAttnStream(2024, c.adj)
    OD.ATTN_DROPOUT = _attn_hook(st)
    try:
        ref_losses, ref_grads = _ref_grads(args, params, norms, *cpu_in)
    finally:
        OE.DROPOUT = OD.ATTN_DROPOUT = None

    def check():
        emul.dropout_stream.reseed(2024)
        _check_model_grads(emul, args, dev_in, ref_losses, ref_grads)
    _grads_off_and_on(emul, check)


def test_fit_eval_steps_with_the_flag_on(dev, networks):
    args, norms, params, emul, cpu_in, dev_in = _adj_problem(networks, 'astlingen', dev, embed_size=64, n_sp_layer=1, learning_rate=1e-3)
    emul.fused_gat_backward = True
    AG.GAT_BWD_COUNTS['fused'] = AG.GAT_BWD_COUNTS['chain'] = 0
    opt = OT.Adam(lr=1e-3)
    leaves = list(OT.tree_leaves(params))
    ref_hist = []
    for _ in range(3):
        ls, gr = _ref_grads(args, params, norms, *cpu_in)
        ref_hist.append([float(l) for l in ls])
        opt.step(leaves, gr)
    hist = [[float(l) for l in emul.fit_eval(*dev_in)] for _ in range(3)]
    assert AG.GAT_BWD_COUNTS['fused'] > 0 and AG.GAT_BWD_COUNTS['chain'] == 0
    for h, r in zip(hist, ref_hist):
        assert np.allclose(h, r, rtol=2e-3, atol=1e-5), (hist, ref_hist)
    after = dict(OT.tree_leaves(params))
    for pname, p, ref in emulator_param_pairs(emul, after):
        err = float((p.detach().double().cpu() - ref).abs().max())
        assert err <= 3e-4, '%s: parameter after 3 Adam steps differs by %.3e' % (pname, err)
