"""GPU tests of graph-sharded training (gnn_uds_amd/dist.py: `HaloExchangeAll.adjoint`, `ShardedEmulator.loss_and_grad` /
`fit_eval`) and of the adjoint exchange kernels (uds_halo_pack_clear_all / uds_halo_accumulate_all).

Every part runs in its own thread on cuda:0 and holds its own replica of the whole Emulator (same args, same parameters).
Messages go through an in-process transport (`_Mailbox`: only `transport` is replaced, so packing, message layout and stream
order are the product's) and every cross-rank sum through `_Reducer`, a fixed-rank-order sum that gives every rank the same
bits.  Losses and summed gradients are compared with `Emulator._model` + the losses + `backward` on the whole network."""
import queue
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import dist as D
from tests.util import emulator_norms

pytestmark = pytest.mark.gpu
# |summed - whole| <= GRAD_REL max|g of the tensor| + GRAD_FLOOR max|g of any tensor|.  Both sides are fp32 / split-bf16
# computations of one function (each within GRAD_TOL['GAT'] = 1e-3 of the fp64 oracle, tests/test_gpu_train.py); a part sums
# its neighbours in its local order, so a relu argument within rounding of 0 may switch.  Observed: 5e-7 relative at 2 and
# 4 parts; at 8 parts 1.007e-4 on block 2 layer 0's link GAT bias, 0.82e-4 on its kernel, <= 1e-5 elsewhere.
GRAD_REL, GRAD_FLOOR = 2e-4, 1e-7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda', 0)


def _report(what, worst):
    print('REPORT %s worst err / bound = %.3e' % (what, worst))


# ------------------------------------------------------------------------------------------------ the adjoint kernels
def _lists(rng, n, P, counts, distinct_across):
    """P row lists of `counts` rows each, distinct within a list; across lists distinct (one permutation cut) or
    overlapping (some rows in 3 or more lists)."""
    if distinct_across:
        perm = rng.permutation(n)
        cuts = np.concatenate([[0], np.cumsum(counts)])
        return [perm[cuts[k]:cuts[k + 1]] for k in range(P)]
    hot = rng.permutation(n)[:4]                           # rows every non-empty list contains
    out = []
    for k in range(P):
        if counts[k] == 0:
            out.append(np.zeros(0, np.int64))
            continue
        rest = np.setdiff1d(rng.permutation(n)[:counts[k] + 4], hot)[:max(0, counts[k] - len(hot))]
        out.append(rng.permutation(np.concatenate([hot[:counts[k]], rest])))
    return out


@pytest.mark.parametrize('F', [1, 3, 4, 64])
@pytest.mark.parametrize('S', [1, 7])
def test_pack_clear_all_and_accumulate_all_bitwise(dev, F, S):
    """pack_clear_all = index_select then zeroing; accumulate_all = the current value plus the messages added in ascending
    peer order; peers with no node rows, no link rows or no rows; rows targeted by 3 or more peers; the unaligned per-float
    path; two runs give the same bits."""
    P = 5
    rng = np.random.default_rng(F * 10 + S)
    n_x, n_e = 300, 400
    gen = torch.Generator().manual_seed(F + S)
    x, e = torch.rand(S, n_x, F, generator=gen).to(dev), torch.rand(S, n_e, F, generator=gen).to(dev)
    nxs = [0, 12, 0, 9, 15]                    # peer 0: links only, peer 2: nothing, peer 4: nodes only
    nes = [10, 7, 0, 11, 0]
    off = lambda ks: torch.as_tensor(np.concatenate([[0], np.cumsum(ks)]), dtype=torch.int32, device=dev)
    cat = lambda parts: torch.as_tensor(np.concatenate(parts).astype(np.int32), device=dev)
    off_x, off_e = off(nxs), off(nes)
    # pack_clear_all over distinct rows
    ix, ie = _lists(rng, n_x, P, nxs, True), _lists(rng, n_e, P, nes, True)
    x2, e2 = x.clone(), e.clone()
    buf = _lib.halo_pack_clear_all(x2, e2, cat(ix), cat(ie), off_x, off_e)
    ref = torch.cat([torch.cat([x.index_select(1, torch.as_tensor(a, device=dev)), e.index_select(1, torch.as_tensor(b, device=dev))],
                               dim=1).reshape(-1) for a, b in zip(ix, ie)])
    rx, re_ = x.clone(), e.clone()
    rx[:, torch.as_tensor(np.concatenate(ix), device=dev)] = 0
    re_[:, torch.as_tensor(np.concatenate(ie), device=dev)] = 0
    assert torch.equal(buf, ref) and torch.equal(x2, rx) and torch.equal(e2, re_)
    # accumulate_all over rows shared by several peers
    sx, se = _lists(rng, n_x, P, nxs, False), _lists(rng, n_e, P, nes, False)
    peers_of = np.bincount(np.concatenate(sx), minlength=n_x)
    assert peers_of.max() >= 3
    msg = torch.rand(S * (sum(nxs) + sum(nes)) * F, generator=gen).to(dev)
    tgts, ptr, src = [], [0], []
    r0 = np.concatenate([[0], np.cumsum(np.asarray(nxs) + np.asarray(nes))])
    for kind, lists in ((0, sx), (1, se)):
        entries = sorted((int(row), q, r0[q] + (j if kind == 0 else nxs[q] + j)) for q, rows in enumerate(lists) for j, row in enumerate(rows))
        for row in sorted(set(t[0] for t in entries)):
            tgts.append(row)
            rs = [t[2] for t in entries if t[0] == row]   # ascending peer
            src.extend(rs)
            ptr.append(ptr[-1] + len(rs))
    tx = len(set(np.concatenate(sx).tolist()))
    i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32), device=dev)
    args = (off_x, off_e, i32(tgts[:tx]), i32(tgts[tx:]), i32(ptr), i32(src))
    want_x, want_e = x.clone(), e.clone()
    for q in range(P):
        block = msg[S * F * r0[q]:S * F * r0[q + 1]].reshape(S, nxs[q] + nes[q], F)
        rq = torch.as_tensor(sx[q], device=dev)
        want_x[:, rq] = want_x[:, rq] + block[:, :nxs[q]]
        rq = torch.as_tensor(se[q], device=dev)
        want_e[:, rq] = want_e[:, rq] + block[:, nxs[q]:]
    outs = []
    for _ in range(2):
        ax, ae = x.clone(), e.clone()
        _lib.halo_accumulate_all(msg, ax, ae, *args)
        outs.append((ax, ae))
    assert torch.equal(outs[0][0], want_x) and torch.equal(outs[0][1], want_e)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    if F == 4:                                 # unaligned operands take the per-float path: same bits
        big = torch.zeros(S * n_x * F + 1, device=dev)
        xu = big[1:].view(S, n_x, F)
        xu.copy_(x)
        eu = e.clone()
        assert xu.data_ptr() % 16
        _lib.halo_accumulate_all(msg, xu, eu, *args)
        assert torch.equal(xu, want_x) and torch.equal(eu, want_e)
        xu.copy_(x)
        assert torch.equal(_lib.halo_pack_clear_all(xu, e.clone(), cat(ix), cat(ie), off_x, off_e), ref) and torch.equal(xu, rx)


# ------------------------------------------------------------------------------------------------ rank threads
class _Mailbox(D.HaloExchangeAll):
    """HaloExchangeAll between rank THREADS: only the transport is replaced -- the peers' slices go through queues with the
    event that marks them written."""

    def __init__(self, base, mail):
        self.__dict__.update(base.__dict__)
        self.mail = mail
        self.calls = 0

    def __call__(self, x, e):
        self.calls += 1
        return super().__call__(x, e)

    def transport(self, msgs):
        st = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(st)
        for q, out, _ in msgs:
            if out is not None:
                self.mail[(self.prob.rank, q)].put((out, ev))
        for q, _, inc in msgs:
            if inc is not None:
                msg, qev = self.mail[(q, self.prob.rank)].get(timeout=120)
                st.wait_event(qev)
                inc.copy_(msg)
                msg.record_stream(st)


class _Reducer:
    """The ranks' sum in fixed rank order, computed by every rank from all ranks' tensors: the same bits everywhere."""

    def __init__(self, n):
        self.slots, self.barrier = [None] * n, threading.Barrier(n, timeout=120)

    def __call__(self, k, t):
        self.slots[k] = t
        self.barrier.wait()
        out = self.slots[0].clone()
        for r in range(1, len(self.slots)):
            out += self.slots[r]
        self.barrier.wait()
        return out


def _shards(replicas, probs, dev):
    mail = {(p, q): queue.Queue() for p in range(len(probs)) for q in range(len(probs))}
    red = _Reducer(len(probs))
    shards = []
    for k, (rep, p) in enumerate(zip(replicas, probs)):
        sh = D.shard_emulator(rep, p, dev)
        sh.exchange, sh.flow_exchange = _Mailbox(sh.exchange, mail), _Mailbox(sh.flow_exchange, mail)
        sh.reduce = (lambda t, k=k: red(k, t))
        shards.append(sh)
    return shards


def _run_ranks(shards, fn):
    out, errs = [None] * len(shards), []

    def main(k):
        try:
            r = fn(shards[k])
            torch.cuda.synchronize()
            out[k] = r
        except Exception as exc:              # surfaced in the main thread
            errs.append((k, exc))
    ts = [threading.Thread(target=main, args=(k,)) for k in range(len(shards))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    assert not errs, errs
    return out


def test_adjoint_on_device_is_the_transpose(dev):
    """The dot-product test of the exchange and its adjoint on the GPU path (one pack_clear and one accumulate launch), 4
    parts, fp32, 1e-6 relative."""
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(2000, 2500, 0))
    probs = D.build_partition_plan(g, 4)
    mail = {(p, q): queue.Queue() for p in range(4) for q in range(4)}
    exs = [_Mailbox(D.HaloExchangeAll(p, dev), mail) for p in probs]
    gen = torch.Generator().manual_seed(3)
    S, F = 3, 8
    mk = lambda rows: torch.randn(S, rows, F, generator=gen).to(dev)
    xs, es = [mk(len(p.nodes)) for p in probs], [mk(len(p.links)) for p in probs]
    gx, ge = [mk(len(p.nodes)) for p in probs], [mk(len(p.links)) for p in probs]
    fwd = _run_ranks(exs, lambda ex: ex(xs[ex.prob.rank].clone(), es[ex.prob.rank].clone()))
    adj = _run_ranks(exs, lambda ex: ex.adjoint(gx[ex.prob.rank].clone(), ge[ex.prob.rank].clone()))
    dot = lambda a, b: sum(float((u.double() * v.double()).sum()) for u, v in zip(a, b))
    lhs = dot([f[0] for f in fwd], gx) + dot([f[1] for f in fwd], ge)
    rhs = dot(xs, [a[0] for a in adj]) + dot(es, [a[1] for a in adj])
    norm = dot(xs, xs) ** 0.5 * (dot(gx, gx) + dot(ge, ge)) ** 0.5 + dot(es, es) ** 0.5 * (dot(gx, gx) + dot(ge, ge)) ** 0.5
    _report('adjoint dot product (4 parts, fp32)', abs(lhs - rhs) / (1e-6 * max(abs(lhs), 1.0)))
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), 1.0), (lhs, rhs, norm)
    assert all(ex.adjoint_calls == 1 for ex in exs)


# ------------------------------------------------------------------------------------------------ the C2 configuration
def _c2_args(recurrent='Conv1D', **over):
    N, E = 2000, 2500
    edges = U.synthetic_drainage_network(N, E, 0)
    g = U.DrainageGraph.from_edges(edges)
    part = np.asarray(D.partition_nodes(g, 8), dtype=np.int64)
    cut = np.nonzero(part[edges[:, 0]] != part[edges[:, 1]])[0]
    act_links = [int(cut[0]), int(cut[len(cut) // 2]), 7, 1900]
    rng = np.random.default_rng(5)
    a = dict(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=64, kernel_size=3,
             n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, epsilon=-1.0, edge_fusion=True, edges=edges, graph=g,
             act=True, act_edges=edges[act_links], conv='GAT', resnet=True, recurrent=recurrent, roll=0, model_dir=None,
             sparse_params=True, learning_rate=1e-3, is_outfall=(np.arange(N) % 97 == 0).astype(float), hmax=1.0 + rng.random(N),
             hmin=0.01 * rng.random(N), ehmax=0.3 + rng.random(E), tide=False)
    a.update(over)
    return SimpleNamespace(**a)


def _replica(args, dev, params=None):
    """One rank's copy of the whole model: same args, same parameters (non-zero biases, NodeEdge biases included)."""
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        if params is None:
            for name, p in emul.named_parameters():
                if float(p.abs().sum()) == 0:
                    p.add_(torch.rand(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev) * 0.05)
        else:
            for p, q in zip(emul.parameters(), params):
                p.copy_(q)
    norms = emulator_norms(args)
    emul.set_norm(*(norms[k].float().numpy() for k in 'xbyre'))
    return emul


def _data(args, dev, seed=5, B=2):
    N, E = args.state_shape[0], args.edge_state_shape[0]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    x, b, ex = r(B, 5, N, 5), r(B, 5, N, 1) * 0.1, r(B, 5, E, 4)
    a = r(B, 5, len(args.act_edges))
    y = r(B, 5, N, 5)
    y[..., -2] = (y[..., -2] > 0.7).double()
    ey = r(B, 5, E, 3)
    return tuple(t.float().to(dev) for t in (x, a, b, y, ex, ey))


def _whole(emul, data):
    """Loss and gradient of the whole network: `_model` + get_node_loss / get_flood_loss / _mse + backward."""
    x, a, b, y, ex, ey = data
    emul.requires_grad_(True)
    for p in emul.parameters():
        p.grad = None
    ae = emul.get_edge_action(a, True)
    preds, edge_preds = emul._model(x, a, b, ex, ae, None, True)
    lw = emul._loss_setup(preds.device)
    ls = [emul.get_node_loss(y, b, preds), emul.get_flood_loss(y, preds), emul._mse(ey, edge_preds, lw['ewei'])]
    sum(ls).backward()
    grads = {n: p.grad.detach().clone() for n, p in emul.named_parameters()}
    for p in emul.parameters():
        p.grad = None
    return [float(v) for v in ls], grads


def _local(sh, data):
    x, a, b, y, ex, ey = data
    ni = torch.as_tensor(sh.prob.nodes, device=x.device)
    lx, lb, lex, _ = sh.scatter_inputs(x, b, ex)
    return lx, a, lb, y.index_select(2, ni).contiguous(), lex, ey.index_select(2, torch.as_tensor(sh.prob.links, device=x.device)).contiguous()


def _check_grads(grads, ref, what):
    gmax = max(float(t.abs().max()) for t in ref.values())
    ratios = {}
    for name, r in ref.items():
        bound = GRAD_REL * float(r.abs().max()) + GRAD_FLOOR * gmax
        ratios[name] = float((grads[name].to(r.device) - r).abs().max()) / bound
    top = sorted(ratios.items(), key=lambda kv: -kv[1])[:6]
    print('TOP %s %s' % (what, ' '.join('%s=%.3g' % kv for kv in top)))
    _report(what, top[0][1])
    assert top[0][1] <= 1.0, (what, top)


def _sharded_grads(args, params, probs, dev, data, runs=1):
    replicas = [_replica(args, dev, params) for _ in probs]
    shards = _shards(replicas, probs, dev)
    res = [_run_ranks(shards, lambda sh: sh.loss_and_grad(*_local(sh, data))) for _ in range(runs)]
    return shards, res


@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_c2_loss_and_gradients(dev, n_parts):
    """C2 (GAT, Conv1D, resnet, edge fusion, if_flood = 3, actions on cut links, L = 3, d = 64, B = 2, T = 5, sparse NodeEdge
    parameters, non-zero biases): the summed loss is the whole-network loss (rtol 1e-5), the summed gradients the whole-
    network gradients (GRAD_REL / GRAD_FLOOR), 2L - 1 + 1 exchanges each way, the same bits on every rank and in two runs."""
    args = _c2_args()
    ref_model = _replica(args, dev)
    params = [p.detach().clone() for p in ref_model.parameters()]
    data = _data(args, dev)
    ref_loss, ref_grads = _whole(ref_model, data)
    probs = D.build_partition_plan(ref_model.graph, n_parts)
    shards, res = _sharded_grads(args, params, probs, dev, data, runs=2)
    L = args.n_sp_layer
    for sh in shards:
        assert sh.exchange.calls == 2 * (2 * L - 1) and sh.flow_exchange.calls == 2          # two runs
        assert sh.exchange.adjoint_calls == 2 * (2 * L - 1) and sh.flow_exchange.adjoint_calls == 2
    losses, grads = res[0][0]
    worst = max(abs(float(l) - r) / (1e-5 * abs(r)) for l, r in zip(losses, ref_loss))
    _report('C2 %d parts loss' % n_parts, worst)
    assert worst <= 1.0, ([float(l) for l in losses], ref_loss)
    _check_grads(grads, ref_grads, 'C2 %d parts grads' % n_parts)
    for run in res:
        for l2, g2 in run:
            assert all(torch.equal(u, v) for u, v in zip(l2, losses))
            assert all(torch.equal(g2[n], grads[n]) for n in grads)


def test_one_part_matches_the_unsharded_gradients(dev):
    """One part: no exchanges; gradients within 1e-6 max|g| per tensor of the unsharded model."""
    args = _c2_args()
    ref_model = _replica(args, dev)
    params = [p.detach().clone() for p in ref_model.parameters()]
    data = _data(args, dev)
    ref_loss, ref_grads = _whole(ref_model, data)
    probs = D.build_partition_plan(ref_model.graph, 1)
    shards, res = _sharded_grads(args, params, probs, dev, data)
    assert not shards[0].exchange.peers
    losses, grads = res[0][0]
    worst = 0.0
    gmax = max(float(t.abs().max()) for t in ref_grads.values())
    for name, r in ref_grads.items():
        bound = 1e-6 * float(r.abs().max()) + 1e-9 * gmax     # (floor: tensors whose whole gradient is ~1e-11)
        err = float((grads[name] - r).abs().max())
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (name, err, bound)
    _report('one part grads', worst)
    assert np.allclose([float(l) for l in losses], ref_loss, rtol=1e-6)


def test_gru_variant_2_parts(dev):
    args = _c2_args(recurrent='GRU', hidden_dim=64)
    ref_model = _replica(args, dev)
    params = [p.detach().clone() for p in ref_model.parameters()]
    data = _data(args, dev)
    ref_loss, ref_grads = _whole(ref_model, data)
    probs = D.build_partition_plan(ref_model.graph, 2)
    _, res = _sharded_grads(args, params, probs, dev, data)
    losses, grads = res[0][0]
    assert np.allclose([float(l) for l in losses], ref_loss, rtol=1e-5)
    _check_grads(grads, ref_grads, 'GRU 2 parts grads')


def test_three_fit_eval_steps_4_parts(dev):
    """Three sharded fit_eval steps against three whole-model fit_eval steps: losses (rtol 1e-4), parameters (1e-4 absolute
    at learning rate 1e-3), and the rank replicas bitwise identical after every step; fit=False evaluates only."""
    args = _c2_args()
    ref_model = _replica(args, dev)
    params = [p.detach().clone() for p in ref_model.parameters()]
    data = _data(args, dev)
    probs = D.build_partition_plan(ref_model.graph, 4)
    replicas = [_replica(args, dev, params) for _ in probs]
    shards = _shards(replicas, probs, dev)
    worst_l, worst_p = 0.0, 0.0
    for step in range(3):
        want = [float(v) for v in ref_model.fit_eval(*data)]
        got = _run_ranks(shards, lambda sh: [float(v) for v in sh.fit_eval(*_local(sh, data))])
        assert all(g == got[0] for g in got)
        worst_l = max(worst_l, max(abs(g - w) / (1e-4 * abs(w)) for g, w in zip(got[0], want)))
        assert np.allclose(got[0], want, rtol=1e-4), (step, got[0], want)
        for rep in replicas[1:]:
            assert all(torch.equal(p, q) for p, q in zip(rep.parameters(), replicas[0].parameters()))
        for (name, p), q in zip(ref_model.named_parameters(), replicas[0].parameters()):
            err = float((p.detach() - q.detach()).abs().max())
            worst_p = max(worst_p, err / 1e-4)
            assert err <= 1e-4, (step, name, err)
    _report('fit_eval 3 steps loss', worst_l)
    _report('fit_eval 3 steps params', worst_p)
    before = [p.detach().clone() for p in replicas[0].parameters()]
    ev = _run_ranks(shards, lambda sh: [float(v) for v in sh.fit_eval(*_local(sh, data), fit=False)])
    assert all(e == ev[0] for e in ev) and len(ev[0]) == 3
    assert all(torch.equal(p, q) for p, q in zip(before, replicas[0].parameters()))


def test_refusals_and_inference_unchanged(dev):
    """Dense NodeEdge parameters (ValueError), GradNorm, roll > 0 and dropout (NotImplementedError); the inference entry
    points still refuse gradient-carrying inputs."""
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(400, 480, 0))
    prob = D.build_partition_plan(g, 2)[0]
    base = dict(state_shape=(400, 4), edge_state_shape=(480, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=64, kernel_size=3,
                n_sp_layer=2, n_tp_layer=1, activation='relu', if_flood=3, edge_fusion=True, edges=g.edges, graph=g, act=False,
                model_dir=None, sparse_params=True)
    mk = lambda **o: U.Emulator('GAT', True, 'Conv1D', SimpleNamespace(**dict(base, **o)), generator=torch.Generator().manual_seed(1)).to(dev)
    z = torch.zeros(1, device=dev)
    for over, exc in ((dict(sparse_params=False), ValueError), (dict(gradnorm=True), NotImplementedError), (dict(roll=2), NotImplementedError)):
        sh = D.shard_emulator(mk(**over), prob, dev)
        with pytest.raises(exc):
            sh.loss_and_grad(z, z, z, z, z, z)
        with pytest.raises(exc):
            sh.fit_eval(z, z, z, z, z, z)
    with pytest.raises(NotImplementedError, match='dropout'):
        D.shard_emulator(mk(dropout=0.2), prob, dev)
    sh = D.shard_emulator(mk(), prob, dev)
    X = torch.rand(1, 5, 400, 5, device=dev, requires_grad=True)
    Bd, Ex = torch.rand(1, 5, 400, 1, device=dev), torch.rand(1, 5, 480, 4, device=dev)
    lx, lb, le, _ = sh.scatter_inputs(X, Bd, Ex)
    with pytest.raises(NotImplementedError, match='inference only'):
        sh.forward(lx, lb, le)
    with pytest.raises(NotImplementedError, match='inference only'):
        sh.predict_tf(lx, lb, None, le)
