"""GPU tests of the graph-sharded whole `Emulator` (gnn_uds_amd/dist.py: `shard_emulator`, `ShardedEmulator`,
`HaloExchangeAll`) and of its one-launch exchange kernels (uds_halo_pack_all / uds_halo_unpack_all).

Every part of a node-cut plan runs in its own thread on cuda:0; the exchanges hand the packed buffers over in-process
(`_MailboxAll`, the pattern of tests/test_gpu_dist.py), with the same packing, message layout and stream discipline as the
RCCL path.  Own rows are compared with the unsharded HIP `Emulator` and with the fp64 oracle of the whole network."""
import queue
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib, mpc
from gnn_uds_amd import dist as D
from oracle import emulator_ref as OE
from tests.util import close, emulator_args, emulator_norms, load_emulator

pytestmark = pytest.mark.gpu
TOL_FWD_BF16X3 = 2e-5          # whole forward vs the fp64 oracle (tests/test_gpu_emulator.py TOL_FWD['bf16x3'])
TOL_UNSHARDED = 4e-6           # own rows vs the unsharded HIP model (tests/test_gpu_dist.py)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------ the exchange kernels
@pytest.mark.parametrize('F', [1, 3, 4, 5, 64])
@pytest.mark.parametrize('S', [1, 7])
@pytest.mark.parametrize('P', [1, 3, 8])
def test_pack_all_unpack_all_bitwise(dev, F, S, P):
    """halo_pack_all / halo_unpack_all against index_select / index_copy_, peers with no node rows, no link rows or none."""
    rng = np.random.default_rng(F * 100 + S * 10 + P)
    n_x, n_e = 300, 400
    gen = torch.Generator().manual_seed(P)
    x, e = torch.rand(S, n_x, F, generator=gen).to(dev), torch.rand(S, n_e, F, generator=gen).to(dev)
    nxs = [int(v) for v in rng.integers(0, 20, P)]
    nes = [int(v) for v in rng.integers(0, 20, P)]
    if P > 1:
        nxs[0] = 0                  # a peer with link rows only
        nes[-1] = 0                 # a peer with node rows only
    if P > 2:
        nxs[1] = nes[1] = 0         # a peer with nothing
    ix = [rng.permutation(n_x)[:k] for k in nxs]          # distinct rows per peer (unpack writes each once)
    ie = [rng.permutation(n_e)[:k] for k in nes]
    off = lambda ks: torch.as_tensor(np.concatenate([[0], np.cumsum(ks)]), dtype=torch.int32, device=dev)
    cat = lambda parts: torch.as_tensor(np.concatenate(parts).astype(np.int32), device=dev)
    idx_x, idx_e, off_x, off_e = cat(ix), cat(ie), off(nxs), off(nes)
    buf = _lib.halo_pack_all(x, e, idx_x, idx_e, off_x, off_e)
    ref = torch.cat([torch.cat([x.index_select(1, torch.as_tensor(a, device=dev)), e.index_select(1, torch.as_tensor(b, device=dev))],
                               dim=1).reshape(-1) for a, b in zip(ix, ie)])
    assert torch.equal(buf, ref)
    # unpack into other rows (each peer's rows distinct across peers here: one permutation cut into pieces)
    px, pe = rng.permutation(n_x)[:sum(nxs)], rng.permutation(n_e)[:sum(nes)]
    ux, ue = torch.as_tensor(px.astype(np.int32), device=dev), torch.as_tensor(pe.astype(np.int32), device=dev)
    x2, e2 = torch.zeros_like(x), torch.zeros_like(e)
    _lib.halo_unpack_all(buf, x2, e2, ux, ue, off_x, off_e)
    rx, re = torch.zeros_like(x), torch.zeros_like(e)
    pos, ox, oe = 0, 0, 0
    for k in range(P):
        msg = buf[S * F * pos:S * F * (pos + nxs[k] + nes[k])].reshape(S, nxs[k] + nes[k], F)
        rx.index_copy_(1, ux[ox:ox + nxs[k]].long(), msg[:, :nxs[k]])
        re.index_copy_(1, ue[oe:oe + nes[k]].long(), msg[:, nxs[k]:])
        pos, ox, oe = pos + nxs[k] + nes[k], ox + nxs[k], oe + nes[k]
    assert torch.equal(x2, rx) and torch.equal(e2, re)
    if F == 4:                       # unaligned operands take the per-float path: same result
        big = torch.zeros(S * n_x * F + 1, device=dev)
        xu = big[1:].view(S, n_x, F)
        xu.copy_(x)
        assert xu.data_ptr() % 16 and torch.equal(_lib.halo_pack_all(xu, e, idx_x, idx_e, off_x, off_e), buf)


# ------------------------------------------------------------------------------------------------ rank threads
class _MailboxAll(D.HaloExchangeAll):
    """HaloExchangeAll between rank THREADS: one pack launch, the peers' slices through queues with the event that marks them
    written, one unpack launch."""

    def __init__(self, base, mail):
        self.__dict__.update(base.__dict__)
        self.mail = mail
        self.calls = 0

    def __call__(self, x, e):
        if x is None:
            x = e.new_empty((e.shape[0], 0, e.shape[-1]))
        self.calls += 1
        if not self.peers:
            return x, e
        S, F = e.shape[0], e.shape[-1]
        st = torch.cuda.current_stream()
        sbuf = self.pack(x, e)
        ev = torch.cuda.Event()
        ev.record(st)
        for q in self.peers:
            if self.n_send[q][1] > self.n_send[q][0]:
                self.mail[(self.prob.rank, q)].put((self.message(sbuf, q, 'send', S, F), ev))
        rbuf = torch.empty(S * self.n_recv[self.peers[-1]][1] * F, device=e.device)
        for q in self.peers:
            if self.n_recv[q][1] > self.n_recv[q][0]:
                msg, qev = self.mail[(q, self.prob.rank)].get(timeout=300)
                st.wait_event(qev)
                self.message(rbuf, q, 'recv', S, F).copy_(msg)
                msg.record_stream(st)
        self.unpack(rbuf, x, e)
        return x, e


def _shards(emul, probs, dev):
    mail = {(p, q): queue.Queue() for p in range(len(probs)) for q in range(len(probs))}
    shards = []
    for p in probs:
        sh = D.shard_emulator(emul, p, dev)
        sh.exchange, sh.flow_exchange = _MailboxAll(sh.exchange, mail), _MailboxAll(sh.flow_exchange, mail)
        shards.append(sh)
    return shards


def _run_ranks(shards, fn):
    """fn(shard) in one thread per rank; returns the per-rank results."""
    out, errs = [None] * len(shards), []

    def main(k):
        try:
            with torch.no_grad():
                r = fn(shards[k])
            torch.cuda.synchronize()
            out[k] = r
        except Exception as exc:          # surfaced in the main thread
            errs.append((k, exc))
    ts = [threading.Thread(target=main, args=(k,)) for k in range(len(shards))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=600)
    assert not errs, errs
    return out


def _rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def _bulk_equal(out, ref, tol=2e-5):
    """As tests/test_gpu_emulator.py::test_predict_tf: no entry beyond the tolerance (hard thresholds may flip only within it)."""
    d = (out.double().cpu() - ref.double().cpu()).abs()
    bad = int((d > tol * max(1.0, float(ref.abs().max()))).sum())
    assert bad == 0, (bad, ref.numel(), float(d.max()))


@pytest.fixture(scope='module')
def c2(dev):
    """The shipped configuration on the C2-size network: GAT, Conv1D, resnet, edge fusion, if_flood = 3, actions on links that
    include cut links, 3 + 3 spatial layers, d = 64, B = 2, seq_in = seq_out = 5."""
    N, E = 2000, 2500
    edges = U.synthetic_drainage_network(N, E, 0)
    g = U.DrainageGraph.from_edges(edges)
    part = np.asarray(D.partition_nodes(g, 8), dtype=np.int64)
    cut = np.nonzero(part[edges[:, 0]] != part[edges[:, 1]])[0]
    act_links = [int(cut[0]), int(cut[len(cut) // 2]), 7, 1900]
    args = emulator_args(edges, N, n_sp_layer=3, n_tp_layer=2, if_flood=3, act=True, act_edges=edges[act_links], edge_fusion=True,
                         embed_size=64, hidden_dim=64, seq_in=5, seq_out=5)
    params = OE.init_params(args, seed=3)
    norms = emulator_norms(args)
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), params, dev)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    c = OE.config(args)
    gen = torch.Generator().manual_seed(5)
    X, Bd, Ex = _rnd(gen, 2, 5, N, c.n_in), _rnd(gen, 2, 5, N, 1) * 0.1, _rnd(gen, 2, 5, E, 4)
    a = _rnd(gen, 2, 5, len(act_links))
    return SimpleNamespace(args=args, params=params, norms=norms, emul=emul, X=X, Bd=Bd, Ex=Ex, a=a, N=N, E=E)


def test_one_part_is_the_unsharded_emulator(dev):
    """One part: the local numbering is the identity and there are no peers, so the sharded forward and predict_tf run the
    same kernels on the same rows as an Emulator built on the same DrainageGraph -- bit for bit."""
    N, E, T = 2000, 2500, 5
    edges = U.synthetic_drainage_network(N, E, 0)
    g = U.DrainageGraph.from_edges(edges)
    rng = np.random.default_rng(2)
    a = SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3,
                        n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=edges, act=True,
                        act_edges=edges[[3, 50]], graph=g, model_dir=None, hmax=1 + rng.random(N), ehmax=0.3 + rng.random(E))
    emul = U.Emulator('GAT', True, 'Conv1D', a, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        for name, p in emul.named_parameters():
            if float(p.abs().sum()) != 0 or 'node_edge' in name:  # biases (not all zero), as test_gpu_emulator.py's large forward
                continue
            p.add_(torch.rand(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev) * 0.05)
    norms = emulator_norms(SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), if_flood=3, tide=False))
    emul.set_norm(*(norms[k].float().numpy() for k in 'xbyre'))
    prob = D.build_partition_plan(g, 1)[0]
    assert np.array_equal(prob.nodes, np.arange(N)) and np.array_equal(prob.links, np.arange(E))
    sh = D.shard_emulator(emul, prob, dev)
    gen = torch.Generator().manual_seed(3)
    f = lambda t: t.float().to(dev)
    X, Bd, Ex, act = f(_rnd(gen, 2, T, N, 5)), f(_rnd(gen, 2, T, N, 1) * 0.1), f(_rnd(gen, 2, T, E, 4)), f(_rnd(gen, 2, T, 2))
    with torch.no_grad():
        AE = emul.get_edge_action(act)
        y, ey = emul(X, Bd, Ex, AE)
        sx, sb, se, sae = sh.scatter_inputs(X, Bd, Ex, AE)
        sy, sey = sh.forward(sx, sb, se, sae)
        assert torch.equal(sy, y) and torch.equal(sey, ey)
        py, pey = emul.predict_tf(X, Bd, act, Ex)
        qy, qey = sh.predict_tf(X, Bd, act, Ex)
    assert torch.equal(qy, py) and torch.equal(qey, pey)


@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_c2_sharded_forward_and_predict_tf(dev, c2, n_parts):
    """Own rows of the sharded forward against the unsharded HIP model (4e-6 relative) and the fp64 oracle of the whole
    network (2e-5); predict_tf against the oracle's predict_tf, as tests/test_gpu_emulator.py::test_predict_tf; every forward
    makes 2L - 1 exchanges, predict_tf two more (the flow column and the outputs)."""
    emul, f = c2.emul, (lambda t: t.float().to(dev))
    probs = D.build_partition_plan(emul.graph, n_parts)
    X, Bd, Ex, a = f(c2.X), f(c2.Bd), f(c2.Ex), f(c2.a)
    with torch.no_grad():
        AE = emul.get_edge_action(a)
        uy, uey = emul(X, Bd, Ex, AE)
    OE.SPARSE_SPATIAL = True
    try:
        ry, rey = OE.forward(c2.args, c2.params, c2.X, c2.Bd, c2.Ex, OE.get_edge_action(OE.config(c2.args), c2.a))
        py, pey = OE.predict(c2.args, c2.params, c2.norms, c2.X, c2.Bd, c2.a, c2.Ex)
    finally:
        OE.SPARSE_SPATIAL = False
    shards = _shards(emul, probs, dev)
    outs = _run_ranks(shards, lambda sh: sh.own(*sh.forward(*sh.scatter_inputs(X, Bd, Ex, AE))))
    L = emul.n_sp_layer
    for sh in shards:
        assert sh.exchange.calls == 2 * L - 1 and sh.flow_exchange.calls == 0
    for p, (oy, oey) in zip(probs, outs):
        ni, li = torch.as_tensor(p.own_nodes, device=dev), torch.as_tensor(p.own_links, device=dev)
        for o, u in ((oy, uy[:, :, ni]), (oey, uey[:, :, li])):
            assert float((o - u).abs().max()) <= TOL_UNSHARDED * max(1.0, float(u.abs().max()))
        close(oy, ry[:, :, p.own_nodes], TOL_FWD_BF16X3)
        close(oey, rey[:, :, p.own_links], TOL_FWD_BF16X3)
    def rank(sh):
        lx, lb, le, _ = sh.scatter_inputs(X, Bd, Ex)
        return sh.predict_tf(lx, lb, a, le)
    res = _run_ranks(shards, rank)
    for sh in shards:
        assert sh.exchange.calls == 2 * (2 * L - 1) + 1 and sh.flow_exchange.calls == 1
    for p, (ly, ley) in zip(probs, res):
        # exact on ALL local rows after the final exchange
        _bulk_equal(ly, py[:, :, p.nodes])
        _bulk_equal(ley, pey[:, :, p.links])


def _gates_model(dev, probs_parts=4, tide=True):
    """edge_fusion False, tide (optional), offsets, node pumps, and `pump > 0` on every link but one, that one owned by part 0."""
    N, E = 2000, 2500
    edges = U.synthetic_drainage_network(N, E, 0)
    g = U.DrainageGraph.from_edges(edges)
    probs = D.build_partition_plan(g, probs_parts)
    rng = np.random.default_rng(7)
    pump = 0.1 + rng.random(E)
    pump[int(probs[0].own_links[0])] = 0.0
    a = SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=64, kernel_size=3,
                        n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=False, edges=edges, act=True, tide=tide,
                        act_edges=edges[[int(probs[1].own_links[2]), int(probs[-1].own_links[4]), 11]], graph=g, model_dir=None,
                        hmax=1 + rng.random(N), hmin=rng.random(N) * 0.05, area=rng.random(N), pump=pump,
                        pump_in=rng.random(N) * (rng.random(N) > 0.7), pump_out=rng.random(N) * (rng.random(N) > 0.7),
                        offset=rng.random(E) * (rng.random(E) > 0.5), ehmax=0.3 + rng.random(E), epsilon=0.1,
                        is_outfall=(np.arange(N) % 97 == 0).astype(float))
    emul = U.Emulator('GAT', True, 'Conv1D', a, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        for name, p in emul.named_parameters():
            if float(p.abs().sum()) != 0 or 'node_edge' in name:  # biases (not all zero), as test_gpu_emulator.py's large forward
                continue
            p.add_(torch.rand(p.shape, generator=torch.Generator().manual_seed(p.numel() + 1)).to(dev) * 0.05)
    norms = emulator_norms(SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), if_flood=3, tide=tide))
    emul.set_norm(*(norms[k].float().numpy() for k in 'xbyre'))
    assert not emul._has_pump and emul._has_offset
    return emul, probs, N, E


def test_gates_variant_predict_tf(dev):
    """Link gates (offset, actions; NO rated-pump override: not every link is a pump) on own links, node gates, tide and the
    pumped-storage depth: predict_tf of every part equals the unsharded model on all local rows.  A part that decided
    `pump.min() > 0` on its own links would override its flows with the rated pumps."""
    emul, probs, N, E = _gates_model(dev)
    gen = torch.Generator().manual_seed(9)
    f = lambda t: t.float().to(dev)
    X, Bd, Ex, a = f(_rnd(gen, 2, 5, N, 5)), f(_rnd(gen, 2, 5, N, 2) * 0.1), f(_rnd(gen, 2, 5, E, 4)), f(_rnd(gen, 2, 5, 3))
    with torch.no_grad():
        uy, uey = emul.predict_tf(X, Bd, a, Ex)
    shards = _shards(emul, probs, dev)
    assert any(bool(float(sh.local.pump.min()) > 0) for sh in shards)        # a part that would decide alone differently
    def rank(sh):
        lx, lb, le, _ = sh.scatter_inputs(X, Bd, Ex)
        return sh.predict_tf(lx, lb, a, le)
    res = _run_ranks(shards, rank)
    assert float(uy[..., :3].std()) > 1e-3 and float(uey[..., -1].std()) > 1e-3      # not saturated
    for p, (ly, ley) in zip(probs, res):
        _bulk_equal(ly, uy[:, :, torch.as_tensor(p.nodes, device=dev)])
        _bulk_equal(ley, uey[:, :, torch.as_tensor(p.links, device=dev)])


def test_fed_back_chunks_predict_horizon(dev):
    """mpc.predict_horizon over 2 chunks on the sharded model, each rank feeding back its own local state (exact on all
    local rows after predict_tf's final exchange, no second scatter): own rows equal the unsharded horizon."""
    emul, probs, N, E = _gates_model(dev, tide=False)          # (the fed-back state carries one runoff channel)
    gen = torch.Generator().manual_seed(12)
    f = lambda t: t.float().to(dev)
    X, R, Ex, sett = f(_rnd(gen, 2, 5, N, 5)), f(_rnd(gen, 2, 10, N, 1) * 0.1), f(_rnd(gen, 2, 5, E, 4)), f(_rnd(gen, 2, 10, 3))
    with torch.no_grad():
        uy, uey = mpc.predict_horizon(emul, sett, X, R, Ex)
    shards = _shards(emul, probs, dev)

    def rank(sh):
        lx, lr, le, _ = sh.scatter_inputs(X, R, Ex)
        return sh.own(*mpc.predict_horizon(sh, sett, lx, lr, le))
    res = _run_ranks(shards, rank)
    for p, (oy, oey) in zip(probs, res):
        assert oy.shape[1] == 10
        _bulk_equal(oy, uy[:, :, torch.as_tensor(p.own_nodes, device=dev)])
        _bulk_equal(oey, uey[:, :, torch.as_tensor(p.own_links, device=dev)])


def test_c4_size_forward_8_parts(dev):
    """The 200k-node / 240k-link network (CSR `args.graph`, sparse NodeEdge parameters) at 8 parts, B = 1, seq_in = seq_out = 4:
    own rows of the sharded forward match the unsharded Emulator."""
    N, E, T = 200000, 240000, 4
    edges = U.synthetic_drainage_network(N, E, 0)
    g = U.DrainageGraph.from_edges(edges)
    a = SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3,
                        n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=edges, act=False, graph=g,
                        model_dir=None, sparse_params=True)
    emul = U.Emulator('GAT', True, 'Conv1D', a, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        for name, p in emul.named_parameters():
            if float(p.abs().sum()) != 0 or 'node_edge' in name:  # biases (not all zero), as test_gpu_emulator.py's large forward
                continue
            p.add_(torch.rand(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev) * 0.05)
    assert emul.block1.layers[0].node_edge_n.sparse
    gen = torch.Generator().manual_seed(2)
    X, Bd, Ex = torch.rand(1, T, N, 5, generator=gen).to(dev), torch.rand(1, T, N, 1, generator=gen).to(dev) * 0.1, torch.rand(1, T, E, 4, generator=gen).to(dev)
    with torch.no_grad():
        uy, uey = emul(X, Bd, Ex)
    probs = D.build_partition_plan(g, 8)
    shards = _shards(emul, probs, dev)
    outs = _run_ranks(shards, lambda sh: sh.own(*sh.forward(*sh.scatter_inputs(X, Bd, Ex)[:3])))
    for p, (oy, oey) in zip(probs, outs):
        ni, li = torch.as_tensor(p.own_nodes, device=dev), torch.as_tensor(p.own_links, device=dev)
        for o, u in ((oy, uy[:, :, ni]), (oey, uey[:, :, li])):
            assert float((o - u).abs().max()) <= TOL_UNSHARDED * max(1.0, float(u.abs().max()))
    assert float(uy.std()) > 1e-3 and float(uey.std()) > 1e-3          # the heads are not saturated
