"""SpatialLayer.route: the table that picks the kernels of one forward, row by row, on layers built on the CPU (no library:
the plan bits are a lambda, and NodeEdge.support_values() is tensor arithmetic)."""
import itertools

import numpy as np
import pytest
import torch

import gnn_uds_amd as U

NO_BITS = lambda fx, fe: 0
ALL_BITS = lambda fx, fe: 63


def only(bit):
    return lambda fx, fe: bit


@pytest.fixture(scope='module')
def graphs(networks):
    return {name: U.DrainageGraph.from_edges(np.array(networks[name]['edges']), networks[name]['n_node'])
            for name in ('astlingen', 'RedChicoSur')}


def make(gph, d, remainder=False, **kw):
    layer = U.SpatialLayer(gph, d, 'relu', sparse_params=False, generator=torch.Generator().manual_seed(3), **kw)
    if remainder:       # a trained dense bias: non-zero off the incidence support
        with torch.no_grad():
            layer.node_edge_n.bias.add_(0.01)
    return layer


def has_remainder(layer):
    return any(ne.support_values()[1] is not None for ne in (layer.node_edge_n, layer.node_edge_e))


def route(layer, fx, fe, S=2, fxb=0, feb=0, bits=ALL_BITS, **asked):
    return layer.route(fx, fxb, fe, feb, S, bits, remainder=has_remainder(layer), **asked)


def test_remainder_is_what_the_bias_makes_it(graphs):
    assert not has_remainder(make(graphs['astlingen'], 64))
    assert has_remainder(make(graphs['astlingen'], 64, remainder=True))


@pytest.mark.parametrize('asked,kw', [(dict(adj_mask=True), {}), (dict(), dict(attn_heads=2)), (dict(attn_coef=True), {})])
def test_row_1_mask_heads_and_coefficients_run_the_chain(graphs, asked, kw):
    assert route(make(graphs['RedChicoSur'], 64, **kw), 64, 64, **asked) == ('chain', False)
    assert route(make(graphs['RedChicoSur'], 64, **kw), 64, 64, fxb=32, feb=32, **asked) == ('chain', False)


def test_row_1_needs_gat(graphs):
    gph = graphs['astlingen']
    layer = make(gph, 64, conv='GCN', filters=(U.GCNConv.preprocess(gph.adj), U.GCNConv.preprocess(gph.edge_adj)))
    for asked in (dict(adj_mask=True), dict(attn_coef=True)):
        with pytest.raises(NotImplementedError, match='use_adj and return_attn_coef are built for conv=GAT'):
            route(layer, 64, 64, **asked)


def test_row_2_gcn_and_diffusion(graphs):
    gph = graphs['astlingen']
    gcn = make(gph, 64, conv='GCN', filters=(U.GCNConv.preprocess(gph.adj), U.GCNConv.preprocess(gph.edge_adj)))
    dif = make(gph, 64, conv='Diffusion', filters=(U.DiffusionConv.preprocess(gph.adj), U.DiffusionConv.preprocess(gph.edge_adj)))
    for layer in (gcn, dif):
        assert route(layer, 64, 64) == ('conv', False)
        assert route(layer, 64, 64, grad=True) == ('conv', False)


@pytest.mark.parametrize('asked', [dict(grad=True), dict(attn_dropout=True)])
def test_row_3_training_concatenates_a_splittable_input(graphs, asked):
    layer = make(graphs['RedChicoSur'], 64)
    assert route(layer, 64, 64, fxb=32, feb=32) == ('fused', True)                # the same call as inference stays split
    assert route(layer, 64, 64, fxb=32, feb=32, **asked) == ('chain', False)
    assert route(layer, 64, 64, fxb=32, **asked) == ('chain', False)


def test_row_4a_remainder_at_d64(graphs):
    layer = make(graphs['RedChicoSur'], 64, remainder=True)
    assert route(layer, 64, 64, bits=only(32)) == ('rem-ws', False)
    assert route(layer, 64, 64, bits=only(63 - 32)) == ('rem-split96', False)      # 4a': the plan does not fit the kernel
    layer._ws_rem_ok = False
    assert route(layer, 64, 64, bits=only(32)) == ('rem-split96', False)           # 4a': the override
    layer._ws_rem_ok = None
    assert route(layer, 64, 64, bits=only(32)) == ('rem-ws', False)


def test_row_4c_remainder_at_other_widths(graphs):
    layer = make(graphs['RedChicoSur'], 64, remainder=True)
    assert route(layer, 64, 64, fxb=32) == ('chain', False)                        # 96 wide once concatenated: no row-4 shape
    assert route(layer, 64, 64, fxb=32, feb=32) == ('chain', False)
    assert route(make(graphs['RedChicoSur'], 64, remainder=True, precision='fp32'), 64, 64) == ('chain', False)
    assert route(make(graphs['RedChicoSur'], 8, remainder=True), 8, 8) == ('chain', False)


@pytest.mark.parametrize('fe,bit', [(128, 8), (64, 16)])
def test_row_4b_remainder_at_d128(graphs, fe, bit):
    layer = make(graphs['RedChicoSur'], 128, remainder=True, fe=fe)
    assert route(layer, 128, fe, bits=only(bit)) == ('rem-d128', False)
    assert route(layer, 128, fe, bits=only(24 - bit)) == ('chain', False)          # only the other width's plan: 4c
    asked = []
    route(layer, 128, fe, bits=lambda fx, fe: asked.append((fx, fe)) or 0)
    assert asked == [(128, fe)]


def test_row_5a_fused_d64(graphs):
    layer = make(graphs['RedChicoSur'], 64)
    assert route(layer, 64, 64, bits=NO_BITS) == ('fused', False)                  # (5a never asks the plan)
    assert route(layer, 96, 64, bits=NO_BITS) == ('fused', False)
    assert route(layer, 64, 64, fxb=32, bits=NO_BITS) == ('fused', True)           # 64 + 32 stays split
    assert route(layer, 64, 64, fxb=32, feb=32, bits=NO_BITS) == ('fused', True)
    assert route(layer, 32, 64, fxb=32) == ('fused', False)                        # 32 + 32: concatenated, runs as 64
    assert route(layer, 64, 48, fxb=32, feb=48) == ('fused', False)                # one side not 64 + 32: both concatenated
    assert route(layer, 64, 64, S=1000, fxb=32) == ('fused', True)                 # pack factor 1: never tiled


@pytest.mark.parametrize('fe,bit', [(128, 8), (64, 16)])
def test_rows_5b_5c_5d_at_d128(graphs, fe, bit):
    layer = make(graphs['RedChicoSur'], 128, fe=fe)
    assert route(layer, 128, fe, bits=only(bit)) == ('fused', False)
    assert 10 * 443 >= 4096 > 9 * 443
    assert route(layer, 128, fe, S=10, bits=only(24 - bit)) == ('chain', False)    # 5c: no plan, enough rows for the matrix cores
    assert route(layer, 128, fe, S=9, bits=only(24 - bit)) == ('entry', False)     # 5d


def test_row_5d_fp32_and_narrow_layers(graphs):
    assert route(make(graphs['RedChicoSur'], 64, precision='fp32'), 64, 64, S=100) == ('entry', False)
    assert route(make(graphs['RedChicoSur'], 8), 8, 8, S=100) == ('entry', False)
    assert route(make(graphs['RedChicoSur'], 64), 32, 32, S=9) == ('entry', False)
    assert route(make(graphs['RedChicoSur'], 64), 32, 32, S=10) == ('chain', False)    # 5c at d = 64: a width the fused kernel has not


def test_fused_tiled_on_a_small_network(graphs):
    layer = make(graphs['astlingen'], 64)
    assert layer.pack_factor() == 4
    assert route(layer, 64, 64, S=64) == ('fused-tiled', False)
    assert route(layer, 64, 64, S=63) == ('fused', False)
    assert route(layer, 64, 64, S=64, fxb=32, feb=32) == ('fused-tiled', True)
    wide = make(graphs['astlingen'], 128)
    assert route(wide, 128, 128, S=64) == ('fused-tiled', False)
    assert route(wide, 128, 128, S=64, bits=NO_BITS) == ('entry', False)
    assert route(make(graphs['astlingen'], 64, remainder=True), 64, 64, S=64) == ('rem-ws', False)     # remainders are never tiled


def test_forward_asks_once_then_concatenates_runs_and_reports(graphs, monkeypatch):
    """forward around `route`, with the methods that launch replaced by recorders: one question per call, pieces kept apart
    only on a split route, last_route / last_path set by every call, leading dimensions restored."""
    layer = make(graphs['astlingen'], 64, fx=96, fe=96)
    asked, ran = [], []
    real = layer.route
    monkeypatch.setattr(layer, 'route', lambda *a: asked.append(a) or real(*a))
    for method in {m for _, m in U.SpatialLayer.ROUTES.values()}:
        def record(*args, _m=method):
            xs, es, *rest = args if _m == '_chain' else args[1:]      # (every other method takes the NodeEdge values first)
            ran.append((_m, xs.shape[-1], es.shape[-1]) + tuple(getattr(t, 'shape', [None])[-1] for t in rest[:2]))
            return xs.new_zeros(xs.shape[:2] + (64,)), es.new_zeros(es.shape[:2] + (64,))
        monkeypatch.setattr(layer, method, record)
    x, xb, e, eb = torch.ones(3, 2, 30, 64), torch.ones(3, 2, 30, 32), torch.ones(3, 2, 29, 64), torch.ones(3, 2, 29, 32)
    with torch.no_grad():
        ox, oe = layer(x, e, xb=xb, eb=eb)
    assert ran == [('_fused', 64, 64, 32, 32)] and (layer.last_route, layer.last_path) == ('fused', 'fused')
    assert tuple(ox.shape) == (3, 2, 30, 64) and tuple(oe.shape) == (3, 2, 29, 64)
    with torch.no_grad():
        layer(x, e, xb=xb, eb=eb, attn_dropout=object())
    assert ran[1] == ('_chain', 96, 96, None, None) and (layer.last_route, layer.last_path) == ('chain', 'unfused')
    layer.requires_grad_(True)
    layer(x, e, xb=xb)
    assert ran[2] == ('_chain', 96, 64, None, None) and (layer.last_route, layer.last_path) == ('chain', 'unfused')
    assert len(asked) == 3 and asked[0][:5] == (64, 32, 64, 32, 6)


def test_every_input_has_exactly_one_route(graphs):
    gph = graphs['astlingen']
    gcn = (U.GCNConv.preprocess(gph.adj), U.GCNConv.preprocess(gph.edge_adj))
    layers = [make(gph, 64), make(gph, 64, remainder=True), make(gph, 128), make(gph, 128, remainder=True), make(gph, 8),
              make(gph, 64, precision='fp32'), make(gph, 64, attn_heads=2), make(gph, 64, conv='GCN', filters=gcn),
              make(graphs['RedChicoSur'], 64), make(graphs['RedChicoSur'], 128, remainder=True)]
    overridden = make(gph, 64, remainder=True)
    overridden._ws_rem_ok = False
    seen = set()
    for layer in layers + [overridden]:
        rem = has_remainder(layer)
        for fx, fxb, fe, feb, S, bits in itertools.product((8, 32, 64, 96, 128), (0, 32), (8, 32, 64, 96, 128), (0, 32), (1, 10, 64),
                                                           (0, 8, 16, 32, 63)):
            for mask, coef, drop, grad in itertools.product((False, True), repeat=4):
                try:
                    name, split = layer.route(fx, fxb, fe, feb, S, only(bits), mask, coef, drop, grad, rem)
                except NotImplementedError:
                    assert layer.conv != 'GAT' and (mask or coef)
                    continue
                assert name in U.SpatialLayer.ROUTES and isinstance(split, bool)
                assert not split or (name in ('fused', 'fused-tiled') and (fxb or feb))
                assert U.SpatialLayer.ROUTES[name][0] == {'rem': 'fused+remainder', 'fus': 'fused'}.get(name[:3], 'unfused')
                seen.add(name)
    assert seen == set(U.SpatialLayer.ROUTES) and len(seen) == 8
