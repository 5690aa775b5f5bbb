"""CPU checks behind tests/test_gpu_snapshot_remainder.py: the Python restatement of the snapshot remainder's plan
(tests/snapshot_remainder_util.py) agrees with uds_remainder_snapshot_plan -- which answers without a device -- the shipped
networks are accepted within the LDS, the limit in M is where the restatement puts it, every case of the table reaches the plan
it claims and the table covers every plan, the fp64 references carry signal, and the layer switch leaves SpatialLayer.route
alone."""
import itertools
import random

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from tests import snapshot_remainder_util as SU
from tests.snapshot_remainder_util import CASES, PAIR_CASES, SHIPPED, case_id, plan

ALL_CASES = CASES + [c for pair in PAIR_CASES for c in pair]


def test_restatement_equals_the_library_over_a_grid():
    rng = random.Random(5)
    edges = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 447, 448, 449, 511, 512, 513, 520]
    sizes = sorted(set(edges + [rng.randint(1, 520) for _ in range(40)]))
    n = 0
    for R, M, F, h in itertools.product(sizes, sizes, (64, 128), (32, 64)):
        assert _lib.remainder_snapshot_plan(R, M, F, h) == plan(R, M, F, h), (R, M, F, h)
        n += 1
    assert n > 10000
    for R, M in ((0, 5), (5, 0), (-1, 5), (SU.MAX_ROWS + 1, 5), (5, SU.MAX_ROWS + 1), (SU.MAX_ROWS, 5)):
        assert _lib.remainder_snapshot_plan(R, M, 64, 32) == plan(R, M, 64, 32), (R, M)


@pytest.mark.parametrize('name', sorted(SHIPPED))
def test_shipped_networks_are_accepted(name, networks):
    n, m = SHIPPED[name]
    assert (networks[name]['n_node'], len(networks[name]['edges'])) == (n, m)
    for (R, M), (F, h) in itertools.product(((n, m), (m, n)), ((64, 32), (128, 64))):
        got = _lib.remainder_snapshot_plan(R, M, F, h)
        assert got == plan(R, M, F, h) and got['G'] >= 1 and 0 < got['lds'] <= 160 * 1024 and got['row_blocks'] in (1, 2), (R, M, F, h, got)
    # on the 30-row network a workgroup's matrix work is 256 columns, not one 32 x 32 tile
    if name == 'astlingen':
        assert plan(n, m, 64, 32)['G'] * 32 == 256 and plan(n, m, 128, 64)['G'] * 64 == 256


@pytest.mark.parametrize('F,h', [(64, 32), (64, 64), (128, 32), (128, 64)])
def test_the_limit_in_m(F, h):
    top = SU.largest_m(F, h)
    assert top == 576
    for R in (1, 20, 444):
        ok, over = _lib.remainder_snapshot_plan(R, top, F, h), _lib.remainder_snapshot_plan(R, top + 1, F, h)
        assert ok['G'] >= 1 and ok['lds'] <= 160 * 1024 and over == SU.REFUSED
    assert all(_lib.remainder_snapshot_plan(20, M, F, h)['G'] >= 1 for M in range(1, top + 1))
    assert not any(_lib.remainder_snapshot_plan(20, M, F, h)['G'] for M in range(top + 1, top + 200))


@pytest.mark.parametrize('F,h', [(96, 32), (64, 48), (96, 48), (32, 32), (64, 16), (256, 64), (128, 128), (0, 0)])
def test_other_widths_are_refused(F, h):
    assert _lib.remainder_snapshot_plan(30, 29, F, h) == SU.REFUSED == plan(30, 29, F, h)


@pytest.mark.parametrize('case', ALL_CASES, ids=case_id)
def test_case_reaches_the_plan_it_claims(case):
    q = _lib.remainder_snapshot_plan(case['R'], case['M'], case['F'], case['h'])
    assert (q['G'], q['row_blocks']) == case['claims'] and q == plan(case['R'], case['M'], case['F'], case['h'])


def test_table_covers_every_plan():
    ids = [case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    # every G the plan can give (NG = 4, 2, 1 column groups at h = 32 and 64: see snapshot_remainder_util) ...
    possible = {plan(1, M, F, h)['G'] for M in range(1, 700) for F in (64, 128) for h in (32, 64)} - {0}
    assert possible == {1, 2, 4, 8} == {c['claims'][0] for c in CASES}
    # ... at both widths, both row-block counts, every activation, one case without a bias, one with leading dimensions
    assert {(c['claims'][0], c['h']) for c in CASES} == {(8, 32), (4, 32), (2, 32), (4, 64), (2, 64), (1, 64)}
    assert {c['claims'][1] for c in CASES} == {1, 2}
    assert {c['act'] for c in CASES} == {'linear', 'relu', 'tanh', 'sigmoid', 'hard_sigmoid'}
    assert any(not c['bias'] for c in CASES) and any(c['lead'] for c in CASES)
    assert {(c['F'], c['h']) for c in CASES} == {(64, 32), (64, 64), (128, 32), (128, 64)}
    # S below G, S = 2 G + 1, more workgroups than the 256 CUs
    assert any(c['S'] < c['claims'][0] for c in CASES) and any(c['S'] == 2 * c['claims'][0] + 1 and c['claims'][0] > 1 for c in CASES)
    assert any(-(-c['S'] // c['claims'][0]) > 256 for c in CASES)
    for a, b in PAIR_CASES:
        assert (a['R'], a['M']) != (b['R'], b['M']) and all(a[k] == b[k] for k in ('S', 'F', 'h', 'act', 'bias'))


@pytest.mark.parametrize('case', ALL_CASES, ids=case_id)
def test_reference_carries_signal(case):
    p, ref = SU.data(case)
    assert tuple(ref.shape) == (case['S'], case['R'], case['h']) and ref.dtype == torch.float64
    assert float(ref.abs().max()) > 0.05


def test_the_switch_leaves_route_alone(networks):
    """SpatialLayer.route with snapshot_remainder set answers as without it, over the argument grid of tests/test_spatial_route.py."""
    graphs = {name: U.DrainageGraph.from_edges(np.array(networks[name]['edges']), networks[name]['n_node'])
              for name in ('astlingen', 'RedChicoSur')}

    def make(gph, d, remainder=False, **kw):
        layer = U.SpatialLayer(gph, d, 'relu', sparse_params=False, generator=torch.Generator().manual_seed(3), **kw)
        if remainder:
            with torch.no_grad():
                layer.node_edge_n.bias.add_(0.01)
        return layer

    assert U.SpatialLayer.snapshot_remainder is False
    gph = graphs['astlingen']
    gcn = (U.GCNConv.preprocess(gph.adj), U.GCNConv.preprocess(gph.edge_adj))
    specs = [(gph, 64, {}), (gph, 64, dict(remainder=True)), (gph, 128, {}), (gph, 128, dict(remainder=True)), (gph, 8, {}),
             (gph, 64, dict(precision='fp32')), (gph, 64, dict(attn_heads=2)), (gph, 64, dict(conv='GCN', filters=gcn)),
             (graphs['RedChicoSur'], 64, {}), (graphs['RedChicoSur'], 128, dict(remainder=True))]
    n = 0
    for g, d, kw in specs:
        off, on = make(g, d, **kw), make(g, d, **kw)
        on.snapshot_remainder = True
        assert 'snapshot_remainder' not in vars(off)
        rem = any(ne.support_values()[1] is not None for ne in (off.node_edge_n, off.node_edge_e))
        for fx, fxb, fe, feb, S, bits in itertools.product((8, 32, 64, 96, 128), (0, 32), (8, 32, 64, 96, 128), (0, 32), (1, 10, 64),
                                                           (0, 8, 16, 32, 63)):
            for mask, coef, drop, grad in itertools.product((False, True), repeat=4):
                got = []
                for layer in (off, on):
                    try:
                        got.append(layer.route(fx, fxb, fe, feb, S, lambda a, b: bits, mask, coef, drop, grad, rem))
                    except NotImplementedError as ex:
                        got.append(str(ex))
                assert got[0] == got[1]
                n += 1
    assert n == len(specs) * 5 * 2 * 5 * 2 * 3 * 5 * 16 and len(U.SpatialLayer.ROUTES) == 8


def test_emulator_switch_reaches_every_spatial_layer(networks):
    from tests.util import emulator_args
    net = networks['astlingen']
    args = emulator_args(net['edges'], net['n_node'])
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args)
    layers = list(emul.block1.layers) + list(emul.block2.layers)
    assert emul.snapshot_remainder is False and not any(ly.snapshot_remainder for ly in layers)
    emul.snapshot_remainder = True
    assert emul.snapshot_remainder is True and all(ly.snapshot_remainder for ly in layers) and len(layers) == 4
    emul.snapshot_remainder = False
    assert not any(ly.snapshot_remainder for ly in layers)
