"""Host side of graph-sharded training (gnn_uds_amd/dist.py: `HaloExchangeAll.adjoint`, `ShardedEmulator.loss_parts`,
`own_loss_weights`, the training refusals).

CPU only: the adjoint exchange on its CPU-tensor path (the gloo path), checked as the transpose of the forward exchange by
the dot-product test with all ranks in one process and with two gloo processes; the bookkeeping the summed gradient rests
on; and the own-row loss parts, whose sum over ranks is the whole-network loss.  The training step itself runs on the GPU
(tests/test_gpu_sharded_train.py)."""
import os
import queue
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd import dist as D

N, E = 2000, 2500


@pytest.fixture(scope='module')
def c2_graph():
    return U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0))


class _Mail(D.HaloExchangeAll):
    """HaloExchangeAll between rank THREADS of one process: only the transport is replaced (CPU tensors)."""

    def __init__(self, base, mail):
        self.__dict__.update(base.__dict__)
        self.mail = mail

    def transport(self, msgs):
        for q, out, _ in msgs:
            if out is not None:
                self.mail[(self.prob.rank, q)].put(out.clone())
        for q, _, inc in msgs:
            if inc is not None:
                inc.copy_(self.mail[(q, self.prob.rank)].get(timeout=120))


def _exchanges(probs, rows_of=None):
    mail = {(p, q): queue.Queue() for p in range(len(probs)) for q in range(len(probs))}
    return [_Mail(D.HaloExchangeAll(p, 'cpu', rows=None if rows_of is None else rows_of(p)), mail) for p in probs]


def _run(exs, fn):
    out, errs = [None] * len(exs), []

    def main(k):
        try:
            out[k] = fn(k, exs[k])
        except Exception as exc:              # surfaced in the main thread
            errs.append((k, exc))
    ts = [threading.Thread(target=main, args=(k,)) for k in range(len(exs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not errs, errs
    return out


def _local_tensors(probs, S, F, seed, link_only=False):
    g = torch.Generator().manual_seed(seed)
    xs = [None if link_only else torch.randn(S, len(p.nodes), F, generator=g, dtype=torch.float64) for p in probs]
    es = [torch.randn(S, len(p.links), F, generator=g, dtype=torch.float64) for p in probs]
    return xs, es


def _dot(a, b):
    return sum(float((u * v).sum()) for u, v in zip(a, b) if u is not None and v is not None)


@pytest.mark.parametrize('subset', ['plan', 'flow_rows'])
@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_adjoint_is_the_transpose_of_the_exchange(c2_graph, n_parts, subset):
    """<E(x), g> = <x, E^T(g)> summed over the ranks, fp64, to 1e-12 relative; E^T zeroes the received rows and adds the
    returned messages into the sent ones."""
    probs = D.build_partition_plan(c2_graph, n_parts)
    link_only = subset == 'flow_rows'
    exs = _exchanges(probs, D.flow_rows if link_only else None)
    S, F = 3, 5
    xs, es = _local_tensors(probs, S, F, 1, link_only)
    gx, ge = _local_tensors(probs, S, F, 2, link_only)
    fwd = _run(exs, lambda k, ex: ex(None if xs[k] is None else xs[k].clone(), es[k].clone()))
    adj = _run(exs, lambda k, ex: ex.adjoint(None if gx[k] is None else gx[k].clone(), ge[k].clone()))
    lhs = _dot([f[0] for f in fwd], gx) + _dot([f[1] for f in fwd], ge)
    rhs = _dot(xs, [a[0] for a in adj]) + _dot(es, [a[1] for a in adj])
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
    assert all(ex.adjoint_calls == 1 for ex in exs)
    for k, (ex, (ax, ae)) in enumerate(zip(exs, adj)):
        rx, re_ = ex.rows('recv')
        if not link_only and len(rx):
            assert not ax.index_select(1, rx).any()                        # a received row keeps no gradient
        if len(re_):
            assert not ae.index_select(1, re_).any()


def test_adjoint_accumulates_in_ascending_peer_order(c2_graph):
    """The CPU path adds the current value first, then the peers' messages in ascending peer order (the kernel's order)."""
    probs = D.build_partition_plan(c2_graph, 8)
    exs = _exchanges(probs)
    S, F = 2, 3
    gx, ge = _local_tensors(probs, S, F, 5)
    adj = _run(exs, lambda k, ex: ex.adjoint(gx[k].clone(), ge[k].clone()))
    many = 0
    for k, (ex, p) in enumerate(zip(exs, probs)):
        want_x, want_e = gx[k].clone(), ge[k].clone()
        for q in ex.peers:                                   # the returned message of q: q's gradient on its halo copies
            peer = probs[q]
            hn, he = peer.recv_nodes.get(k, np.zeros(0, np.int64)), peer.recv_links.get(k, np.zeros(0, np.int64))
            sn, se = p.send_nodes.get(q, np.zeros(0, np.int64)), p.send_links.get(q, np.zeros(0, np.int64))
            for dst, src, rows_d, rows_s in ((want_x, gx[q], sn, hn), (want_e, ge[q], se, he)):
                for i, j in zip(rows_d, rows_s):
                    dst[:, i] = dst[:, i] + src[:, j]
        no, lo = len(p.own_nodes), len(p.own_links)
        assert torch.equal(adj[k][0][:, :no], want_x[:, :no]) and torch.equal(adj[k][1][:, :lo], want_e[:, :lo])
        cnt = np.bincount(np.concatenate([p.send_nodes.get(q, np.zeros(0, np.int64)) for q in ex.peers]).astype(np.int64),
                          minlength=1)
        many = max(many, int(cnt.max()))
    assert many >= 2                                          # some own row is a halo row on several peers


def _gloo_worker(rank, world, port, result):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0))
        probs = D.build_partition_plan(g, world)
        S, F = 2, 4
        gx, ge = _local_tensors(probs, S, F, 3)
        ref = _run(_exchanges(probs), lambda k, ex: ex.adjoint(gx[k].clone(), ge[k].clone()))     # all ranks in one process
        ex = D.HaloExchangeAll(probs[rank], 'cpu')
        ox, oe = ex.adjoint(gx[rank].clone(), ge[rank].clone())
        same = torch.equal(ox, ref[rank][0]) and torch.equal(oe, ref[rank][1])
        changed = not torch.equal(ox, gx[rank])
        result.put((rank, same, changed, ex.adjoint_calls))
    finally:
        dist.destroy_process_group()


def test_adjoint_two_processes_gloo():
    ctx = mp.get_context('spawn')
    result = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, result)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    got = sorted(result.get(timeout=10) for _ in range(2))
    assert [r[1:] for r in got] == [(True, True, 1), (True, True, 1)], got


# ------------------------------------------------------------------------------------------------ bookkeeping
@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_every_support_entry_has_an_owner_and_maps_once(c2_graph, n_parts):
    """The summed gradient of a sparse NodeEdge parameter: the local support entries of a rank map to distinct global
    entries, and together the ranks cover every global entry."""
    probs = D.build_partition_plan(c2_graph, n_parts)
    for key, nnz in (('inc_n_pos', c2_graph.inc_n.nnz), ('inc_e_pos', c2_graph.inc_e.nnz)):
        seen = np.zeros(nnz, dtype=bool)
        for p in probs:
            pos = np.asarray(getattr(p, key), dtype=np.int64)
            assert len(np.unique(pos)) == len(pos)
            seen[pos] = True
        assert seen.all()


def test_accumulate_plan_lists_every_message_row_once(c2_graph):
    """The adjoint's CSR: every message row of the send buffer is added exactly once, into the row it was packed from, and
    each target's rows ascend (peer order)."""
    p = D.build_partition_plan(c2_graph, 8)[3]
    ex = D.HaloExchangeAll(p, 'cpu')
    a, d = ex.dev['acc'], ex.dev['send']
    n_rows = int(d['off_x'][-1] + d['off_e'][-1])
    assert sorted(a['src'].tolist()) == list(range(n_rows))
    tx = len(a['tgt_x'])
    tgt = np.concatenate([a['tgt_x'].numpy(), a['tgt_e'].numpy()])
    assert len(a['ptr']) == len(tgt) + 1
    for t in range(len(tgt)):
        rs = a['src'][a['ptr'][t]:a['ptr'][t + 1]]
        assert len(rs) >= 1 and np.all(np.diff(rs) > 0)
        for r in rs:
            k = int(np.searchsorted(d['off_x'] + d['off_e'], r, side='right') - 1)
            j = int(r - (d['off_x'][k] + d['off_e'][k]))
            nx_ = int(d['off_x'][k + 1] - d['off_x'][k])
            if t < tx:
                assert j < nx_ and int(d['idx_x'][d['off_x'][k] + j]) == tgt[t]
            else:
                assert j >= nx_ and int(d['idx_e'][d['off_e'][k] + j - nx_]) == tgt[t]


def _emulator(g, **over):
    rng = np.random.default_rng(1)
    ed = np.asarray(g.edges)
    a = dict(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=5, seq_out=5, embed_size=16, hidden_dim=16, kernel_size=3,
             n_sp_layer=2, n_tp_layer=1, activation='relu', if_flood=3, edge_fusion=True, edges=ed, graph=g, act=False,
             conv='GAT', resnet=True, recurrent='Conv1D', model_dir=None, sparse_params=True,
             is_outfall=(np.arange(N) % 211 == 0).astype(float), hmax=1 + rng.random(N), hmin=0.01 + rng.random(N) * 0.1,
             ehmax=0.3 + rng.random(E), nwei=0.5 + rng.random(N), ewei=0.5 + rng.random(E), poswei=1 + rng.random(N))
    a.update(over)
    args = SimpleNamespace(**a)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(0))
    gen = torch.Generator().manual_seed(4)
    mk = lambda rows, c: np.stack([0.5 + torch.rand(rows, c, generator=gen, dtype=torch.float64).numpy(), np.zeros((rows, c))])
    emul.set_norm(mk(N, 5), mk(N, 1), mk(N, 5), mk(N, 1), mk(E, 4))
    return emul


def args_h(emul, rows):
    r = torch.as_tensor(rows)
    return emul.hmax[r], emul.hmin[r]


@pytest.mark.parametrize('n_parts', [2, 4])
def test_sliced_loss_weights_and_loss_parts_sum_to_the_whole_loss(c2_graph, n_parts):
    """own_loss_weights are the global `_loss_setup` rows (its head-range reweighting uses all nodes' hmax / hmin); the
    per-rank own-row loss parts, normalised by the global counts, sum to the whole-network loss (fp64, 1e-12)."""
    emul = _emulator(c2_graph)
    lw = emul._loss_setup(torch.device('cpu'))
    probs = D.build_partition_plan(c2_graph, n_parts)
    shards = [D.shard_emulator(emul, p, 'cpu') for p in probs]
    for sh, p in zip(shards, probs):
        w = sh.own_loss_weights(torch.device('cpu'))
        assert torch.equal(w['nwei'], lw['nwei'][torch.as_tensor(p.own_nodes)])
        assert torch.equal(w['ewei'], lw['ewei'][torch.as_tensor(p.own_links)])
        assert torch.equal(w['poswei'], lw['poswei'][torch.as_tensor(p.own_nodes)])
        hmax, hmin = args_h(emul, p.own_nodes)
        assert float((hmax - hmin).mean()) != float((emul.hmax - emul.hmin).mean())      # a part alone would weigh differently
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    B, T = 2, 5
    y, preds = r(B, T, N, 5), r(B, T, N, 4)
    y[..., -2] = (y[..., -2] > 0.6).double()
    ey, eps = r(B, T, E, 3), r(B, T, E, 3)
    whole = [emul.get_node_loss(y, None, preds), emul.get_flood_loss(y, preds), emul._mse(ey, eps, lw['ewei'])]
    tot = [0.0, 0.0, 0.0]
    for sh, p in zip(shards, probs):
        ni, li = torch.as_tensor(p.nodes), torch.as_tensor(p.links)
        parts = sh.loss_parts(y[:, :, ni], None, preds[:, :, ni], ey[:, :, li], eps[:, :, li])
        assert len(parts) == 3
        tot = [a + float(b) for a, b in zip(tot, parts)]
    for a, b in zip(tot, whole):
        assert abs(a - float(b)) <= 1e-12 * abs(float(b)), (a, float(b))


def test_training_refusals(c2_graph):
    """Dense NodeEdge parameters (ValueError: no bounded halo once the bias trains off the support), GradNorm and roll > 0
    (NotImplementedError) are refused by the training entry points, before any exchange; dropout by shard_emulator."""
    p = D.build_partition_plan(c2_graph, 2)[0]
    z = torch.zeros(1)
    for over, exc, what in ((dict(sparse_params=False), ValueError, 'sparse NodeEdge'), (dict(gradnorm=True), NotImplementedError, 'GradNorm'),
                            (dict(roll=2), NotImplementedError, 'roll=2')):
        sh = D.shard_emulator(_emulator(c2_graph, **over), p, 'cpu')
        for call in (sh.loss_and_grad, lambda *a: sh.fit_eval(*a, fit=True), lambda *a: sh.fit_eval(*a, fit=False)):
            with pytest.raises(exc, match=what):
                call(z, z, z, z, z, z)
    with pytest.raises(NotImplementedError, match='dropout'):
        D.shard_emulator(_emulator(c2_graph, dropout=0.1), p, 'cpu')


def test_adjoint_entries_report_argument_errors():
    lib = _lib.load()
    assert lib.uds_halo_pack_clear_all(None, 4, None, 4, 1, 0, None, 0, None, 0, None, None, 1, None, None) == -22      # F = 0
    assert lib.uds_halo_pack_clear_all(None, 4, None, 4, 1, 4, None, 3, None, 0, None, None, 1, None, None) == -22      # NULL
    assert lib.uds_halo_accumulate_all(None, 1, 4, None, None, 0, None, 0, None, 0, None, None, 0, None, 4, None, 4, None) == -22
    assert lib.uds_halo_accumulate_all(None, 1, 4, None, None, 1, None, 2, None, 0, None, None, 2, None, 4, None, 4, None) == -22
    assert b'uds_halo_accumulate_all' in lib.uds_last_error()
    assert lib.uds_halo_accumulate_all(None, 0, 4, None, None, 1, None, 2, None, 0, None, None, 2, None, 4, None, 4, None) == 0


def test_refresh_copies_the_global_parameters_onto_the_local_support(c2_graph):
    """After an optimizer step on the global replica, `refresh` writes every local parameter in place: row-local ones as they
    are, sparse NodeEdge ones gathered at the rank's support positions (the local blocks carry wrapped names)."""
    emul = _emulator(c2_graph)
    p = D.build_partition_plan(c2_graph, 4)[2]
    sh = D.shard_emulator(emul, p, 'cpu')
    with torch.no_grad():
        for q in emul.parameters():
            q.add_(torch.rand(q.shape, generator=torch.Generator().manual_seed(q.numel())))
    before = {n: q._version for n, q in sh.local.named_parameters()}
    sh.refresh()
    gp = dict(emul.named_parameters())
    n_ne = 0
    for name, q in sh.local.named_parameters():
        gname = D.ShardedEmulator._global_name(name)
        src = gp[gname].detach()
        if '.node_edge_n.' in name or '.node_edge_e.' in name:
            src = src[torch.as_tensor(p.inc_n_pos if '.node_edge_n.' in name else p.inc_e_pos)]
            n_ne += 1
        assert torch.equal(q, src) and q._version > before[name], name
    assert n_ne == 2 * 2 * 2 * 2
