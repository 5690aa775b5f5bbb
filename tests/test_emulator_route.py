"""Emulator.temporal_route / head_route: the tables that pick the kernels of the temporal and the output stage, row by row, on
models built on the CPU (no library: `rowgemm_supported` is a lambda); the window shift of the rollout against its formulas; and
the eligibility rule of the tail kernels (`_tail_takes`) as each of its two callers sees it."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd.emulator import TemporalLayer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YES, NO = (lambda k, f, h: True), (lambda k, f, h: False)
WIDE = ('bf16x3', 64, 64)


def build(**over):
    """astlingen (30 nodes, 29 links), embed 64, two temporal layers, actuated, flood head; norms of ones / zeros."""
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))['astlingen']
    edges, n = np.asarray(net['edges']), net['n_node']
    e = len(edges)
    args = SimpleNamespace(state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=4, seq_out=2, embed_size=64, hidden_dim=64, n_sp_layer=1,
                           n_tp_layer=2, if_flood=1, edges=edges, graph=U.DrainageGraph.from_edges(edges, n), act=True, act_edges=edges[[1, 4]],
                           conv='GAT', resnet=True, recurrent='Conv1D')
    for k, v in over.items():
        setattr(args, k, v)
    m = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1))
    mk = lambda rows, c: np.stack([np.ones((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    ne_ch = args.edge_state_shape[1]
    m.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, ne_ch))
    return m, n, e


@pytest.fixture(scope='module')
def model():
    return build()[0]


def conv(i, **change):
    return TemporalLayer(True, (3, 64, 64), 2 ** i, 'relu', 'bf16x3', 64)._replace(**change)


def stackable(n):
    return [conv(i) for i in range(n)]


def troute(m, lx, le=None, B=1, T=4, N=30, E=29, fx=64, fe=64, ok=YES, gx=(), ge=(), mlp=False):
    return m.temporal_route(B, T, N, E, fx, fe, lx, lx if le is None else le, ok, gx, ge, mlp)


# ---- temporal_route ----------------------------------------------------------------------------------------------------------
def test_the_model_describes_its_own_layers(model):
    assert [model.temporal_layer(ly) for ly in model.tem1_x] == stackable(2)
    gru = build(recurrent='GRU')[0]
    assert [gru.temporal_layer(ly) for ly in gru.tem2_e] == 2 * [TemporalLayer(False, None, None, None, 'bf16x3', 64)]


def test_temporal_row_0_the_mlp_model_runs_layers(model, monkeypatch):
    monkeypatch.setattr(model, 'fused_temporal', True)
    assert troute(model, stackable(2), B=256, mlp=True) == ('sides', ('layers', 'layers'))
    assert troute(model, stackable(2), mlp=True) == ('sides', ('layers', 'layers'))      # (where the graph model would pair)


@pytest.mark.parametrize('n,key', [(1, 'layers'), (2, 'stack'), (3, 'stack'), (4, 'layers')])
def test_temporal_row_1_stack_takes_two_or_three_layers(model, monkeypatch, n, key):
    monkeypatch.setattr(model, 'fused_temporal', True)
    form, keys = troute(model, stackable(n), B=256, ok=NO)
    assert (form, keys) == (('sides', ('stack', 'stack')) if key == 'stack' else ('pairs', n * ('layers',)))


def test_temporal_row_1_stream_threshold(model, monkeypatch):
    monkeypatch.setattr(model, 'fused_temporal', True)
    S = model.STACK_MIN_STREAMS
    assert S == 256
    assert troute(model, stackable(2), B=S, N=16, E=1) == ('sides', ('stack', 'stack'))
    assert troute(model, stackable(2), B=S - 1, N=16, E=16, ok=NO) == ('pairs', ('layers', 'layers'))
    assert troute(model, stackable(2), B=1, N=16 * (S - 1) + 1, E=16 * S) == ('sides', ('stack', 'stack'))        # ceil(rows / 16)
    assert troute(model, stackable(2), B=1, N=16 * (S - 1), E=16 * (S - 1), ok=NO) == ('pairs', ('layers', 'layers'))


@pytest.mark.parametrize('layers', [
    [conv(0), conv(1), conv(2, dilation=3)],                       # dilation (1, 2, 3)
    [conv(0), conv(1, activation='tanh')],                         # mixed activations
    [conv(0, precision='fp32'), conv(1)],                          # an fp32 layer
    [conv(0), conv(1, precision='fp32')],
    [conv(0, kernel=(3, 64, 32), out=32), conv(1, kernel=(3, 32, 64))],
    [conv(0, kernel=(2, 64, 64)), conv(1, kernel=(2, 64, 64))],
    [conv(0), TemporalLayer(False, None, None, None, 'bf16x3', 64)],
], ids=['dilation', 'activation', 'fp32-first', 'fp32-second', 'width', 'taps', 'recurrent'])
def test_temporal_row_1_refusals(model, monkeypatch, layers):
    monkeypatch.setattr(model, 'fused_temporal', True)
    assert troute(model, stackable(len(layers)), B=256)[1] == ('stack', 'stack')
    form, keys = troute(model, layers, B=256, ok=NO)
    assert form == 'pairs' and set(keys) == {'layers'}


def test_temporal_row_1_flag_input_width_and_grad(model, monkeypatch):
    assert troute(model, stackable(2), B=256, ok=NO) == ('pairs', ('layers', 'layers'))         # fused_temporal is off by default
    monkeypatch.setattr(model, 'fused_temporal', True)
    assert troute(model, stackable(2), B=256, fx=32, ok=NO) == ('sides', ('layers', 'stack'))
    for g in ((True,), (False, True), (False, False, True)):           # the input, the first or the last layer's parameters
        assert troute(model, stackable(2), B=256, gx=g, ok=NO) == ('sides', ('layers', 'stack'))
        assert troute(model, stackable(2), B=256, gx=g, ge=g, ok=NO) == ('pairs', ('layers', 'layers'))
    assert troute(model, stackable(2), B=256, gx=(False, False, False)) == ('sides', ('stack', 'stack'))


def test_temporal_row_2_a_stack_on_one_side_forces_layers_on_the_other(model, monkeypatch):
    shape = dict(B=1, T=4, N=4081, E=29)                               # 256 node streams, 2 link streams; 16324 rows: pair's shape
    assert troute(model, stackable(2), **shape) == ('pairs', ('pair', 'pair'))
    monkeypatch.setattr(model, 'fused_temporal', True)
    assert troute(model, stackable(2), **shape) == ('sides', ('stack', 'layers'))
    assert troute(model, stackable(2), B=1, T=4, N=29, E=4081) == ('sides', ('layers', 'stack'))


def test_temporal_row_3_different_lengths(model):
    assert troute(model, stackable(2), stackable(3)) == ('sides', ('layers', 'layers'))
    assert troute(model, stackable(2), []) == ('sides', ('layers', 'layers'))
    assert troute(model, [], []) == ('pairs', ())


def test_temporal_row_4_pair_row_threshold(model):
    assert troute(model, stackable(2), B=1, T=1, N=16384, E=5) == ('pairs', ('pair', 'pair'))
    assert troute(model, stackable(2), B=1, T=1, N=16385, E=5) == ('pairs', ('layers', 'layers'))
    assert troute(model, stackable(2), B=1, T=1, N=5, E=16385) == ('pairs', ('layers', 'layers'))         # max(N, E)
    assert troute(model, stackable(2), B=4, T=4, N=1024, E=1024) == ('pairs', ('pair', 'pair'))
    assert troute(model, stackable(2), B=4, T=4, N=1025, E=1024) == ('pairs', ('layers', 'layers'))


@pytest.mark.parametrize('kernel,key', [((3, 64, 64), 'pair'), ((1, 64, 64), 'pair'), ((3, 64, 32), 'pair'), ((2, 64, 64), 'layers'),
                                        ((3, 32, 32), 'layers'), ((1, 32, 32), 'layers'), ((3, 128, 64), 'layers')])
def test_temporal_row_4_k_steps(model, kernel, key):
    """k0 * k1 // 32 must be 2 or 6."""
    ly = [conv(0, kernel=kernel, out=kernel[2])]
    assert (kernel[0] * kernel[1] // 32 in (2, 6)) == (key == 'pair')
    assert troute(model, ly, fx=kernel[1], fe=kernel[1]) == ('pairs', (key,))


def test_temporal_row_4_asks_rowgemm_supported_with_the_gemm_shape(model):
    asked = []
    assert troute(model, stackable(2), ok=lambda *a: asked.append(a) or False) == ('pairs', ('layers', 'layers'))
    assert asked == [(192, 64, 64), (192, 64, 64)]


def test_temporal_row_4_the_two_sides_must_agree(model):
    lx = stackable(2)
    for other in (conv(1, dilation=1), conv(1, activation='tanh'), conv(1, precision='fp32'), conv(1, kernel=(3, 64, 32)),
                  TemporalLayer(False, None, None, None, 'bf16x3', 64)):
        assert troute(model, lx, [conv(0), other]) == ('pairs', ('pair', 'layers'))
    assert troute(model, 2 * [conv(0, precision='fp32')]) == ('pairs', ('layers', 'layers'))
    assert troute(model, lx, fx=32) == ('pairs', ('layers', 'pair'))                           # the first inputs differ in width
    assert troute(model, lx, fe=96) == ('pairs', ('layers', 'pair'))
    narrow = [conv(0, kernel=(3, 64, 32), out=32), conv(1)]                                       # the second layer's input is 32 wide
    assert troute(model, narrow) == ('pairs', ('pair', 'layers'))
    gru = 2 * [TemporalLayer(False, None, None, None, 'bf16x3', 64)]
    assert troute(model, gru) == ('pairs', ('layers', 'layers'))


def test_temporal_row_4_grad_is_the_input_or_a_layer_up_to_this_one(model):
    lx = stackable(3)
    assert troute(model, lx, gx=(False, False, False, False)) == ('pairs', ('pair', 'pair', 'pair'))
    assert troute(model, lx, gx=(True, False, False, False)) == ('pairs', ('layers', 'layers', 'layers'))
    assert troute(model, lx, ge=(False, True, False, False)) == ('pairs', ('layers', 'layers', 'layers'))
    assert troute(model, lx, gx=(False, False, True, False)) == ('pairs', ('pair', 'layers', 'layers'))
    assert troute(model, lx, ge=(False, False, False, True)) == ('pairs', ('pair', 'pair', 'layers'))


def test_temporal_stage_asks_once_runs_and_records(model, monkeypatch):
    """`_temporal` around the route, with the methods that launch replaced by recorders."""
    ran = []
    monkeypatch.setattr(model, '_tem_pair', lambda lx, le, x, e: ran.append('pair') or (x, e))
    monkeypatch.setattr(model, '_tem_stack', lambda mods, t: ran.append('stack') or t)
    monkeypatch.setattr(model, '_tem_layers', lambda mods, t: ran.append('layers%d' % len(mods)) or t)
    x, e = torch.zeros(1, 4, 4090, 64), torch.zeros(1, 4, 20, 64)
    model.last_temporal_route, model.last_temporal_path = [], None
    with torch.no_grad():
        model._temporal(model.tem1_x, model.tem1_e, x, e)
    assert ran == ['pair', 'pair'] and model.last_temporal_route == [('pairs', ('pair', 'pair'))] and model.last_temporal_path == 'layers'
    monkeypatch.setattr(model, 'fused_temporal', True)
    del ran[:]
    with torch.no_grad():
        model._temporal(model.tem2_x, model.tem2_e, x, e)
    assert ran == ['stack', 'layers2'] and model.last_temporal_route[1] == ('sides', ('stack', 'layers')) and model.last_temporal_path == 'stack'
    del ran[:]
    model.tem2_x[1].bias.requires_grad_(True)                      # autograd records for the second node layer
    try:
        model.last_temporal_route = []
        model._temporal(model.tem2_x, model.tem2_e, x, e)
        assert ran == ['pair', 'layers1', 'layers1'] and model.last_temporal_route == [('pairs', ('pair', 'layers'))]
        assert model.last_temporal_path == 'layers'
        with torch.no_grad():
            model._temporal(model.tem2_x, model.tem2_e, x, e)
        assert model.last_temporal_route[1] == ('sides', ('stack', 'layers'))
    finally:
        model.tem2_x[1].bias.requires_grad_(False)
    del ran[:]
    model._temporal(model.tem1_x, model.tem1_e, x, e, mlp=True)
    assert ran == ['layers2', 'layers2']


# ---- head_route --------------------------------------------------------------------------------------------------------------
FLOOD = [(32, 64)]


def hroute(m, B=1, rows=30, res=WIDE, head_units=3, hidden=(), **kw):
    return m.head_route(B, rows, res, head_units, list(hidden), **kw)


def test_head_row_1_heads(model):
    assert hroute(model) == 'heads'
    assert hroute(model, hidden=FLOOD) == 'heads'
    assert hroute(model, B=8, rows=4096, hidden=FLOOD) == 'heads'                          # before dense-cumsum
    assert hroute(model, head_units=4) == 'heads' and hroute(model, head_units=5) == 'cumsum'
    assert hroute(model, hidden=[(32, 64)] + 4 * [(32, 32)]) == 'heads'                    # 5 hidden layers
    assert hroute(model, hidden=[(32, 64)] + 5 * [(32, 32)]) == 'cumsum'                   # 6
    assert hroute(model, hidden=[(32, 64), (33, 32)]) == 'cumsum'                          # a 33-unit hidden layer
    assert hroute(model, hidden=[(32, 32)]) == 'cumsum'                                    # the first does not take 64
    for res in (('fp32', 64, 64), ('bf16x3', 32, 64), ('bf16x3', 64, 32), ('bf16x3', 64, 96)):
        assert hroute(model, res=res) == 'cumsum'
    assert hroute(model, mlp=True) == 'cumsum'


def test_head_row_2_dropout_comes_before_everything_but_refuses_heads(model):
    assert hroute(model, drop=True) == 'dropout'                                           # where heads would have run
    assert hroute(model, B=1, rows=4096, head_units=5, drop=True) == 'dropout'             # ... and dense-cumsum
    plain = build(resnet=False)[0]
    assert hroute(plain, drop=True) == 'dropout'
    assert hroute(model, drop=True, mlp=True) == 'dropout'


def test_head_row_3_plain_without_resnet():
    plain = build(resnet=False)[0]
    assert hroute(plain) == 'plain' and hroute(plain, B=1, rows=5000) == 'plain' and hroute(plain, grad_any=True, grad_own=True) == 'plain'
    assert hroute(plain, mlp=True) == 'plain'


def test_head_row_4_dense_cumsum_row_threshold(model):
    assert hroute(model, B=1, rows=4096, head_units=5) == 'dense-cumsum'
    assert hroute(model, B=1, rows=4095, head_units=5) == 'cumsum'
    assert hroute(model, B=64, rows=64, head_units=5) == 'dense-cumsum'
    assert hroute(model, B=63, rows=65, head_units=5) == 'cumsum'                          # 4095
    for res in (('fp32', 64, 64), ('bf16x3', 32, 64), ('bf16x3', 64, 32)):
        assert hroute(model, B=1, rows=4096, res=res) == 'cumsum'
    assert hroute(model, B=1, rows=4096, head_units=5, mlp=True) == 'cumsum'


def test_head_grad_on_an_unrelated_parameter_refuses_heads_only(model):
    assert hroute(model, B=1, rows=4096, grad_any=True) == 'dense-cumsum'
    assert hroute(model, B=1, rows=4095, grad_any=True) == 'cumsum'
    assert hroute(model, B=1, rows=4096, grad_any=True, grad_own=True) == 'cumsum'


class Head:
    """What `_output` reads of a head or hidden layer, recording its calls."""

    def __init__(self, units, ran, tag, in_features=64):
        self.units, self.ran, self.tag, self.kernel = units, ran, tag, torch.empty(in_features, units)

    def __call__(self, t):
        self.ran.append(self.tag)
        return t.new_zeros(t.shape[:-1] + (self.units,))


def test_output_stage_asks_once_runs_and_records(model, monkeypatch):
    ran = []
    for key, name in U.Emulator.HEAD_ROUTES.items():
        monkeypatch.setattr(model, name, lambda res, t, lin_last, *heads, _k=key: ran.append(_k) or t)
    head, head_f = Head(3, ran, 'head'), Head(1, ran, 'flood')
    x, e, lin = torch.zeros(1, 2, 4100, 64), torch.zeros(1, 2, 4090, 64), torch.zeros(1, 1, 4100, 64)
    model.last_head_route = []
    with torch.no_grad():
        model._output(x, lin, model.res_x, head, list(model.flood), head_f, False, False)
    assert ran == ['heads'] and model.last_head_route == ['heads']
    flood_bias = model.flood[0].bias
    flood_bias.requires_grad_(True)                                 # unrelated to the res layer: heads refuses, dense-cumsum does not
    try:
        del ran[:]
        pgrad = any(p.requires_grad for p in model.parameters())
        out = model._output(x, lin, model.res_x, head, [Head(32, ran, 'hidden')], head_f, False, pgrad)
        assert ran == ['dense-cumsum', 'head', 'hidden', 'flood'] and tuple(out.shape) == (1, 2, 4100, 4)
        model._output(e, lin[:, :, :4090], model.res_e, head, [], None, False, pgrad)
        assert model.last_head_route == ['heads', 'dense-cumsum', 'cumsum']                       # 4100 rows, then 4090
        model._output(x, lin, model.res_x, head, [], None, True, pgrad)
        assert model.last_head_route[-1] == 'dropout'
        out = model._output(x[:, :, :1], lin[:, :, :1], model.res_x, Head(90, ran, 'head'), [], None, False, pgrad, rows=30)     # the MLP model's view
        assert model.last_head_route[-1] == 'cumsum' and tuple(out.shape) == (1, 2, 30, 3)
    finally:
        flood_bias.requires_grad_(False)


def test_every_input_has_exactly_one_route(model):
    import itertools
    plain = build(resnet=False)[0]
    seen = set()
    for m, res, hu, hidden, rows in itertools.product((model, plain), (WIDE, ('fp32', 64, 64)), (3, 5), ([], FLOOD), (30, 4096)):
        for drop, ga, go, mlp in itertools.product((False, True), repeat=4):
            key = m.head_route(1, rows, res, hu, hidden, drop, ga, go, mlp)
            assert key in U.Emulator.HEAD_ROUTES and hasattr(m, U.Emulator.HEAD_ROUTES[key])
            assert not (mlp and key in ('heads', 'dense-cumsum'))
            seen.add(key)
    assert seen == set(U.Emulator.HEAD_ROUTES) and len(seen) == 5
    assert set(U.Emulator.TEMPORAL_ROUTES) == {'stack', 'pair', 'layers'}
    assert all(hasattr(model, name) for name in U.Emulator.TEMPORAL_ROUTES.values())


# ---- the window shift --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seq_in,seq_out', [(4, 2), (3, 3)], ids=['keep2', 'keep0'])
@pytest.mark.parametrize('if_flood', [0, 1])
@pytest.mark.parametrize('act', [False, True])
def test_window_shift_is_the_rollout_arithmetic(seq_in, seq_out, if_flood, act):
    m, n, e = build(seq_in=seq_in, seq_out=seq_out, if_flood=if_flood, act=act, edge_fusion=True)
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.rand(*s, generator=gen)
    cy = 1 + if_flood                                               # edge fusion: post-processing returns h, q_in, q_out (, flood)
    x, ex = r(2, seq_in + 1, n, cy + 3), r(2, seq_in + 1, e, 4)     # (a window longer than seq_in: only its tail is kept)
    y, ey, b_i, a_i = r(2, seq_out, n, cy + 2), r(2, seq_out, e, 3), r(2, seq_out, n, 1), 0.2 + 0.8 * r(2, seq_out, 2)
    ae_i, adj_i = m._chunk_actions(a_i)
    assert adj_i is None
    if act:
        want_ae = torch.ones(2, seq_out, e, 1)
        hits = [np.where((m.edges == pair).all(1))[0] for pair in m.act_edges]
        for k, links in enumerate(hits):
            want_ae[:, :, links, 0] = a_i[:, :, k:k + 1]
        assert torch.equal(ae_i, want_ae)
    else:
        assert ae_i is None
        want_ae = torch.ones(2, seq_out, e, 1)
    fed = y.clone()
    if if_flood:
        fed[..., -1] = (y[..., -1] > 0.5).float()
        assert set(fed[..., -1].unique().tolist()) == {0.0, 1.0}
    keep = seq_in - seq_out
    want_x = torch.cat([x[:, x.shape[1] - keep:], torch.cat([fed, b_i], dim=-1)], dim=1)
    want_ex = torch.cat([ex[:, ex.shape[1] - keep:], torch.cat([ey, want_ae], dim=-1)], dim=1)
    got_x, got_ex = m._shift_window(x, ex, y, ey, b_i, ae_i)
    assert tuple(got_x.shape) == (2, seq_in, n, cy + 3) and tuple(got_ex.shape) == (2, seq_in, e, 4)
    assert torch.equal(got_x, want_x) and torch.equal(got_ex, want_ex)


def test_chunk_actions_build_the_adjacency_mask_with_use_adj():
    m, n, e = build(use_adj=True)
    a_i = torch.tensor([[[1.0, 0.4]]])
    ae_i, adj_i = m._chunk_actions(a_i)
    assert torch.equal(ae_i, m.get_edge_action(a_i, True)) and torch.equal(adj_i, m.get_adj_action(a_i, True))
    assert tuple(adj_i.shape) == (1, 1, m.graph.adj.nnz) and float(adj_i.min()) == 0.0


# ---- the tail rule -----------------------------------------------------------------------------------------------------------
def parent_rule(m, dev, B, T, ce, a, n_act):
    """The conditions both callers spelled out before they shared `_tail_takes`, with the link walk done every time."""
    N, E, C = m.n_node, m.n_edge, 3 + int(bool(m.if_flood))
    ny, ne = m._norm('y', dev), m._norm('e', dev)
    if hasattr(m, '_flow_exchange') or not 2 <= ce <= 8:
        return False
    if tuple(ny.shape[1:]) != (N, ny.shape[-1]) or ny.shape[-1] < C or tuple(ne.shape[1:]) != (E, ne.shape[-1]) or ne.shape[-1] < max(ce, 3 if m.act else 0):
        return False
    if m.act and (a is None or tuple(a.shape) != (B, T, n_act) or a.dtype != torch.float32 or not a.is_cuda or
                  len(m._act_edge_index()) != n_act or (not m.edge_fusion and len(m.act_edges) != n_act)):
        return False
    return True


def norm(rows, c):
    return np.stack([np.ones((rows, c)), np.zeros((rows, c))]).astype(np.float32)


TAIL_CASES = {                                            # name: (model changes, norm changes, a, ce, `_flow_exchange`, taken)
    'plain': ({}, {}, (2, 2, 2), 3, False, True),
    'ce1': ({}, {}, (2, 2, 2), 1, False, False),
    'ce2': ({}, {}, (2, 2, 2), 2, False, True),
    'ce8': ({}, {'e': 8}, (2, 2, 2), 8, False, True),
    'ce9': ({}, {'e': 9}, (2, 2, 2), 9, False, False),
    'ny-short': ({}, {'y': 3}, (2, 2, 2), 3, False, False),          # if_flood: the kernels read 4 channels
    'ne-short': ({}, {'e': 2}, (2, 2, 2), 2, False, False),          # an actuated model reads the flow span: 3 channels
    'ne-short-no-act': (dict(act=False), {'e': 2}, None, 2, False, True),
    'ne-rows': ({}, {'e_rows': 5}, (2, 2, 2), 3, False, False),
    'a-wide': ({}, {}, (2, 2, 3), 3, False, False),                  # three settings for two actuated links
    'a-steps': ({}, {}, (2, 3, 2), 3, False, False),
    'a-none': ({}, {}, None, 3, False, False),
    'a-double': ({}, {}, 'double', 3, False, False),
    'flow-exchange': ({}, {}, (2, 2, 2), 3, True, False),
    'setting-without-link': ({}, {}, (2, 2, 2), 3, False, False),                  # (its act_edges are set in the test)
    'edge-fusion': (dict(edge_fusion=True), {}, (2, 2, 2), 3, False, True),
}


@pytest.mark.parametrize('case', list(TAIL_CASES))
def test_tail_rule_answers_as_the_separate_rules_did(case, monkeypatch):
    over, norms, a_shape, ce, exchange, taken = TAIL_CASES[case]
    if case == 'setting-without-link':
        over = dict(over, act_edges=np.array([build()[0].edges[1], [9999, 9998]]))
    m, n, e = build(**over)
    m._norms['y'] = torch.as_tensor(norm(n, norms.get('y', 5)))
    m._norms['e'] = torch.as_tensor(norm(norms.get('e_rows', e), norms.get('e', 4)))
    if exchange:
        m._flow_exchange = lambda x, e: (x, e)
    a = None if a_shape is None else torch.ones(2, 2, 2, dtype=torch.float64) if a_shape == 'double' else torch.ones(*a_shape)
    n_act = a.shape[-1] if m.act and a is not None else 0
    dev = torch.device('cpu')
    assert not m._tail_takes(dev, 2, 2, ce, a, n_act) or not m.act          # host tensors: an actuated model's settings are refused
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    want = parent_rule(m, dev, 2, 2, ce, a, n_act)
    assert want == taken
    assert m._tail_takes(dev, 2, 2, ce, a, n_act) == want
    assert m._tail_takes(dev, 2, 2, ce, a, n_act) == want                   # ... and from the cache


def test_tail_rule_walks_the_link_list_once_per_n_act(monkeypatch):
    m, n, e = build()
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    walks = []
    real = m._act_edge_index
    monkeypatch.setattr(m, '_act_edge_index', lambda: walks.append(1) or real())
    dev = torch.device('cpu')
    for _ in range(3):
        assert m._tail_takes(dev, 2, 2, 3, torch.ones(2, 2, 2), 2)
    assert len(walks) == 1
    assert not m._tail_takes(dev, 2, 2, 3, torch.ones(2, 2, 3), 3) and len(walks) == 2


def test_each_caller_keeps_its_own_conditions(monkeypatch):
    """`_predict_tail_hip` checks y's exact channel count, `_fit_tail_spec` the model's n_out; both stop at the shared rule, and
    both go on to `_tail_spec` where everything holds (recorded here: no library on this machine)."""
    m, n, e = build()
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    reached = []
    monkeypatch.setattr(m, '_tail_spec', lambda *args: reached.append(args[1:]))     # returns None: the caller does too
    z = lambda *s: torch.zeros(*s)
    B, T = 2, m.seq_out
    a, b, x = torch.ones(B, T, 2), z(B, T, n, 1), z(B, m.seq_in, n, 5)
    predict = lambda y, ey, a_=a: m._predict_tail_hip(y, ey, a_, b, b, x, False)
    assert predict(z(B, T, n, 4), z(B, T, e, 3)) is None and reached == [(2, 1, 3)]
    assert predict(z(B, T, n, 5), z(B, T, e, 3)) is None and len(reached) == 1          # y's exact channel count
    assert predict(z(B, T, n, 4), z(B, T, e, 1)) is None and len(reached) == 1          # ce = 1: the shared rule
    assert predict(z(B, T, n, 4), z(B, T, e, 3), torch.ones(B, T, 3)) is None and len(reached) == 1
    m.fused_tail = False
    assert predict(z(B, T, n, 4), z(B, T, e, 3)) is None and len(reached) == 1
    fit = lambda y, ey, a_=a: m._fit_tail_spec(x, a_, b, y, ey)
    assert fit(z(B, T, n, 5), z(B, T, e, 3)) is None and reached[1:] == [(2, 1, 3)]
    assert fit(z(B, T, n, 6), z(B, T, e, 3)) is None and len(reached) == 3              # the targets may be wider ...
    assert fit(z(B, T, n, 2), z(B, T, e, 3)) is None and len(reached) == 3              # ... but hold at least 3 channels
    assert fit(z(B, T, n, 5), z(B, T, e, 3), torch.ones(B, T, 3)) is None and len(reached) == 3     # the shared rule
    m.n_out = 2
    assert fit(z(B, T, n, 5), z(B, T, e, 3)) is None and len(reached) == 3              # the model's n_out
    m.n_out = 3
    m._flow_exchange = lambda x, e: (x, e)
    assert fit(z(B, T, n, 5), z(B, T, e, 3)) is None and len(reached) == 3
