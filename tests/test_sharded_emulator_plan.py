"""Host side of the graph-sharded whole `Emulator` (gnn_uds_amd/dist.py: `shard_emulator`, `flow_rows`, `HaloExchangeAll`).

CPU only: what is checked is the bookkeeping the sharded forward rests on -- which rows are local, who sends what, the
flow-exchange subset, the action columns, the sliced constants / norms, the flags inherited from the whole network and the
refusals.  The forward itself runs on the GPU (tests/test_gpu_sharded_emulator.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import dist as D
from tests.util import emulator_args

N, E = 2000, 2500


@pytest.fixture(scope='module')
def c2_graph():
    return U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0))


def _plan(g, n_parts):
    part = np.asarray(D.partition_nodes(g, n_parts), dtype=np.int64)
    return part, D.build_partition_plan(g, n_parts, part)


def _act_links(g, part):
    """Actuated links: a cut link, and a pair of links whose two links lie in different parts (a link's part is its
    from-node's)."""
    ed = np.asarray(g.edges, dtype=np.int64)
    lp = part[ed[:, 0]]
    cut = int(np.nonzero(part[ed[:, 0]] != part[ed[:, 1]])[0][0])
    a = int(np.nonzero(lp == lp.min())[0][3])
    b = int(np.nonzero(lp == lp.max())[0][5])
    return [cut, a, b]


def _args(g, part, **over):
    rng = np.random.default_rng(1)
    ed = np.asarray(g.edges)
    a = dict(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=5, seq_out=5, embed_size=64, hidden_dim=64, kernel_size=3,
             n_sp_layer=3, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=ed, graph=g, act=True,
             act_edges=ed[_act_links(g, part)], conv='GAT', resnet=True, recurrent='Conv1D', model_dir=None,
             is_outfall=(np.arange(N) == 0).astype(float), hmax=1 + rng.random(N), hmin=rng.random(N) * 0.1, area=rng.random(N),
             pump=np.zeros(E), pump_in=rng.random(N) * (rng.random(N) > 0.7), pump_out=np.zeros(N),
             offset=rng.random(E) * (rng.random(E) > 0.5), ehmax=0.3 + rng.random(E), tide=False)
    a.update(over)
    return SimpleNamespace(**a)


def _emulator(args):
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(4)
    mk = lambda rows, c: np.stack([0.5 + torch.rand(rows, c, generator=g, dtype=torch.float64).numpy(), np.zeros((rows, c))])
    emul.set_norm(mk(N, 5), mk(N, 1), mk(N, 5), mk(N, 1), mk(E, 4))
    return emul


@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_local_rows_halo_owners_and_flow_rows(c2_graph, n_parts):
    g = c2_graph
    part, probs = _plan(g, n_parts)
    ed = np.asarray(g.edges, dtype=np.int64)
    link_part = part[ed[:, 0]]
    for p in probs:
        # every link incident to an own node is local (the flow balance of an own node reads all of them)
        inc = np.nonzero(np.isin(ed[:, 0], p.own_nodes) | np.isin(ed[:, 1], p.own_nodes))[0]
        assert np.isin(inc, p.links).all()
        # every halo row is owned by exactly one peer and is listed in that peer's send list
        halo_n, halo_e = np.arange(len(p.own_nodes), len(p.nodes)), np.arange(len(p.own_links), len(p.links))
        rn = np.concatenate([p.recv_nodes[q] for q in p.recv_nodes]) if p.recv_nodes else np.zeros(0, np.int64)
        re = np.concatenate([p.recv_links[q] for q in p.recv_links]) if p.recv_links else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(rn), halo_n) and np.array_equal(np.sort(re), halo_e)
        for q in p.recv_nodes:
            assert (part[p.nodes[p.recv_nodes[q]]] == q).all() and (link_part[p.links[p.recv_links[q]]] == q).all()
            peer = probs[q]
            assert np.array_equal(peer.own_nodes[peer.send_nodes[p.rank]], p.nodes[p.recv_nodes[q]])
            assert np.array_equal(peer.own_links[peer.send_links[p.rank]], p.links[p.recv_links[q]])
    # the flow rows: exactly the halo links incident to own nodes, and what each sender sends is what its receiver expects
    rows = [D.flow_rows(p) for p in probs]
    for p, r in zip(probs, rows):
        halo_links = p.links[len(p.own_links):]
        want = halo_links[np.isin(ed[halo_links, 0], p.own_nodes) | np.isin(ed[halo_links, 1], p.own_nodes)]
        got = np.concatenate([p.links[v] for v in r['recv_links'].values()]) if r['recv_links'] else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(got), np.sort(want))
        assert 'recv_nodes' not in r and 'send_nodes' not in r
        for q, idx in r['recv_links'].items():
            assert np.array_equal(probs[q].own_links[rows[q]['send_links'][p.rank]], p.links[idx])
    assert sum(len(v) for r in rows for v in r['recv_links'].values()) > 0


@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_exchange_all_message_layout_on_cpu(c2_graph, n_parts):
    """HaloExchangeAll's buffers on CPU tensors (the gloo path): peer q's message is the (S, nx_q + ne_q, F) block at
    S F (off_x[q] + off_e[q]), and the unpacked halo rows equal the owners' rows."""
    g = c2_graph
    _, probs = _plan(g, n_parts)
    S, F = 3, 5
    gen = torch.Generator().manual_seed(2)
    X, Ex = torch.rand(S, N, F, generator=gen), torch.rand(S, E, F, generator=gen)
    exs = [D.HaloExchangeAll(p, 'cpu') for p in probs]
    loc = [(X[:, p.nodes].clone(), Ex[:, p.links].clone()) for p in probs]
    for (lx, le), p in zip(loc, probs):                   # spoil the halo rows
        lx[:, len(p.own_nodes):] = -1
        le[:, len(p.own_links):] = -1
    sent = [ex.pack(lx, le) for ex, (lx, le) in zip(exs, loc)]
    for k, (p, ex) in enumerate(zip(probs, exs)):
        rbuf = torch.empty(S * ex.n_recv[ex.peers[-1]][1] * F)
        for q in ex.peers:
            msg = exs[q].message(sent[q], p.rank, 'send', S, F)
            assert msg.numel() == S * F * (len(probs[q].send_nodes.get(p.rank, [])) + len(probs[q].send_links.get(p.rank, [])))
            ex.message(rbuf, q, 'recv', S, F).copy_(msg)
        ex.unpack(rbuf, *loc[k])
    for p, (lx, le) in zip(probs, loc):
        assert torch.equal(lx, X[:, p.nodes]) and torch.equal(le, Ex[:, p.links])


@pytest.mark.parametrize('n_parts', [2, 4, 8])
def test_actions_constants_and_norms_follow_the_global_model(c2_graph, n_parts):
    g = c2_graph
    part, probs = _plan(g, n_parts)
    emul = _emulator(_args(g, part))
    link_col, out_o, out_i = D.global_action_columns(emul)
    act_links = _act_links(g, part)
    assert sorted(link_col[act_links]) == [1, 2, 3] and len(set(part[np.asarray(g.edges)[act_links[1:], 0]])) == 2
    a = torch.rand(2, 5, 3, generator=torch.Generator().manual_seed(3))
    ref_e = emul.get_edge_action(a)
    ref_o, ref_i = emul.get_action(a)
    for p in probs[:2] + probs[-1:]:
        sh = D.shard_emulator(emul, p, 'cpu')
        loc = sh.local
        li, ni = torch.as_tensor(p.links), torch.as_tensor(p.nodes)
        assert np.array_equal(loc._edge_act_cols, link_col[p.links])
        assert torch.equal(sh.get_edge_action(a), ref_e[:, :, li])
        lo, lin = loc.get_action(a)
        assert torch.equal(lo, ref_o[..., ni]) and torch.equal(lin, ref_i[..., ni])
        for name in ('is_outfall', 'area', 'pump_in', 'pump_out', 'hmax', 'hmin'):
            assert torch.equal(getattr(loc, name), getattr(emul, name)[ni]), name
        for name in ('ehmax', 'pump', 'offset'):
            assert torch.equal(getattr(loc, name), getattr(emul, name)[li]), name
        for k in 'xbyr':
            assert torch.equal(loc._norms[k], emul._norms[k][:, ni]), k
        assert torch.equal(loc._norms['e'], emul._norms['e'][:, li])
        # parameters: the row-local ones unchanged, NodeEdge on the local support
        gl = emul.block2.layers[1].node_edge_n
        ll = loc.block2.block.layers[1].node_edge_n
        assert torch.equal(ll.weight, gl.weight[ni][:, li]) and torch.equal(loc.out.kernel, emul.out.kernel)
        assert not any(t.requires_grad for t in loc.parameters())


def test_flags_are_the_whole_networks(c2_graph):
    """`pump > 0` on every link but one, that one owned by part 0: the whole network has `_has_pump` False (not every link is
    a pump), parts 1.. on their own would say True -- each part must carry the global flags."""
    g = c2_graph
    part, probs = _plan(g, 4)
    pump = np.full(E, 0.5)
    lone = int(probs[0].own_links[0])
    pump[lone] = 0.0
    emul = _emulator(_args(g, part, pump=pump, pump_out=np.zeros(N), offset=np.zeros(E)))
    assert emul._has_pump is False and emul._has_link_pump and emul._has_any_pump and not emul._has_offset
    for p in probs:
        sh = D.shard_emulator(emul, p, 'cpu')
        for flag in ('_has_offset', '_has_pump', '_has_link_pump', '_has_any_pump'):
            assert getattr(sh.local, flag) == getattr(emul, flag), (p.rank, flag)
    assert bool(float(torch.as_tensor(pump[probs[1].links]).min()) > 0)      # what part 1 would have decided alone


def test_refusals(networks):
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(60, 72, 0))
    part = np.asarray(D.partition_nodes(g, 2), dtype=np.int64)
    prob = D.build_partition_plan(g, 2, part)[0]
    small = lambda **over: SimpleNamespace(**{**vars(_args(g, part)), 'state_shape': (60, 4), 'edge_state_shape': (72, 4),
                                              'is_outfall': np.zeros(60), 'hmax': np.ones(60), 'hmin': np.zeros(60), 'area': np.zeros(60),
                                              'pump_in': np.zeros(60), 'pump_out': np.zeros(60), 'pump': np.zeros(72), 'offset': np.zeros(72),
                                              'ehmax': np.ones(72), **over})
    build = lambda a: U.Emulator(a.conv, a.resnet, a.recurrent, a, generator=torch.Generator().manual_seed(0))
    cases = [(small(graph_base=1), NotImplementedError, 'graph_base'),
             (small(use_adj=True), NotImplementedError, 'use_adj'),
             (small(conv='False', seq_in=5, seq_out=5), NotImplementedError, 'conv=False'),
             (small(dropout=0.2), NotImplementedError, 'dropout')]
    for a, exc, word in cases:
        with pytest.raises(exc, match=word):
            D.shard_emulator(build(a), prob, 'cpu')
    # GCN (dense-matrix arguments: the CSR path is GAT only)
    net = networks['astlingen']
    ga = emulator_args(net['edges'], net['n_node'], conv='GCN')
    gcn = U.Emulator(ga.conv, ga.resnet, ga.recurrent, ga)
    with pytest.raises(NotImplementedError, match='GAT'):
        D.shard_emulator(gcn, D.build_partition_plan(gcn.graph, 2)[0], 'cpu')
    # a NodeEdge bias trained off the incidence support: no halo of bounded radius
    emul = build(small(sparse_params=False))
    ne = emul.block1.layers[1].node_edge_e
    sup = torch.zeros(ne.shape, dtype=torch.bool)
    sup.reshape(-1)[ne._flat] = True
    r, c = [int(v) for v in torch.nonzero(~sup)[0]]
    with torch.no_grad():
        ne.bias[r, c] = 0.1
    with pytest.raises(ValueError, match='off the incidence support'):
        D.shard_emulator(emul, prob, 'cpu')
    with torch.no_grad():
        ne.bias[r, c] = 0.0
        ne.bias.reshape(-1)[ne._flat[0]] = 0.1               # on the support: fine
    sh = D.shard_emulator(emul, prob, 'cpu')
    # inference only: no gradients across the cut
    X = torch.rand(1, 5, len(prob.nodes), 5, requires_grad=True)
    with pytest.raises(NotImplementedError, match='inference only'):
        sh.forward(X, torch.rand(1, 5, len(prob.nodes), 1), torch.rand(1, 5, len(prob.links), 4))
