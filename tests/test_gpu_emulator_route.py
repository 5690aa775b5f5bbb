"""Emulator.temporal_route / head_route on the GPU: every key of both tables is reached by a real forward, and what the forward
records (last_temporal_route / last_head_route) is what the route function returns for the plain values of that call.  astlingen
(30 nodes, tests/golden/networks.json, built as tests/test_gpu_fit_graph.py builds it) reaches pair, heads, cumsum, plain and
dropout; the synthetic 4090-node / 4100-link network of tests/test_gpu_conv_stack.py reaches stack, layers and -- with B = 1 on both
sides of the 4096-row threshold in one forward -- dense-cumsum next to cumsum.  The pair launch against its two single launches is
torch.equal (stack against layers: tests/test_gpu_conv_stack.py).  One eager and one graphed `fit_eval` step from the same weights
go through the one step body and are compared as tests/test_gpu_fit_graph.py compares them: torch.equal on every tensor."""
import pytest
import torch

from gnn_uds_amd import _lib
from tests.test_gpu_conv_stack import _emulator
from tests.test_gpu_fit_graph import batch, build, pair, same_losses, same_model

pytestmark = pytest.mark.gpu

WIDE = ('bf16x3', 64, 64)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def want_routes(m, B, n, e, drop=False, grad_any=False, grad_tem=False):
    """What the two route functions return for a forward of `m` on B windows: [stage 1, stage 2], [node side, link side].
    grad_tem: autograd records for the input of the temporal stages."""
    stages = []
    for mods_x, mods_e, T in ((m.tem1_x, m.tem1_e, m.seq_in), (m.tem2_x, m.tem2_e, m.seq_out)):
        lx, le = [m.temporal_layer(ly) for ly in mods_x], [m.temporal_layer(ly) for ly in mods_e]
        g = (grad_tem,) + len(lx) * (False,)
        stages.append(m.temporal_route(B, T, n, e, 64, 64, lx, le, _lib.rowgemm_supported, g, g))
    hidden = [(ly.units, ly.kernel.shape[0]) for ly in m.flood]
    heads = [m.head_route(B, n, WIDE, m.out.units, hidden, drop, grad_any, grad_tem),
             m.head_route(B, e, WIDE, m.e_out_layer.units, [], drop, grad_any, grad_tem)]
    return stages, heads


def small_forward(m, n, e, dev, training=False):
    x, a, b, _, ex, _ = batch(m, n, e, dev, 3)
    out = m.forward(x, b, ex, m.get_edge_action(a, True), training=training)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in out)
    return m.last_temporal_route, m.last_head_route


def test_small_network_pair_and_heads(dev):
    m, n, e = build(dev)
    with torch.no_grad():
        tem, heads = small_forward(m, n, e, dev)
    assert tem == 2 * [('pairs', ('pair', 'pair'))] and heads == ['heads', 'heads'] and m.last_temporal_path == 'layers'
    assert (tem, heads) == want_routes(m, 2, n, e)


def test_small_network_cumsum_under_an_unrelated_gradient(dev):
    m, n, e = build(dev)
    m.flood_out.bias.requires_grad_(True)              # heads refuses; 60 rows are no dense-cumsum shape
    tem, heads = small_forward(m, n, e, dev)
    assert tem == 2 * [('pairs', ('pair', 'pair'))] and heads == ['cumsum', 'cumsum']
    assert (tem, heads) == want_routes(m, 2, n, e, grad_any=True)


def test_small_network_plain_without_resnet(dev):
    m, n, e = build(dev, resnet=False)
    with torch.no_grad():
        tem, heads = small_forward(m, n, e, dev)
    assert heads == ['plain', 'plain'] and (tem, heads) == want_routes(m, 2, n, e)


def test_small_network_dropout(dev):
    m, n, e = build(dev, dropout=0.1)
    with torch.no_grad():
        tem, heads = small_forward(m, n, e, dev, training=True)
        assert heads == ['dropout', 'dropout'] and (tem, heads) == want_routes(m, 2, n, e, drop=True)
        tem, heads = small_forward(m, n, e, dev)                 # the same model in inference
    assert heads == ['heads', 'heads']


def test_pair_launch_equals_its_two_single_launches(dev):
    m, n, e = build(dev)
    gen = torch.Generator().manual_seed(11)
    x, ed = torch.rand(2, 5, n, 64, generator=gen).to(dev) - 0.5, torch.rand(2, 5, e, 64, generator=gen).to(dev) - 0.5
    with torch.no_grad():
        for lx, le in zip(m.tem2_x, m.tem2_e):                   # dilation 1, then 2
            px, pe = m._tem_pair(lx, le, x, ed)
            assert torch.equal(px, lx(x)) and torch.equal(pe, le(ed))
            assert bool(px.abs().sum() > 0) and bool(pe.abs().sum() > 0)
            x, ed = px, pe


def test_large_network_dense_cumsum_on_one_side_of_the_threshold(dev):
    m, (X, B, E) = _emulator(dev, 2)
    n, e = m.n_node, m.n_edge
    assert (n, e) == (4090, 4100) and X.shape[0] == 1
    m.flood_out.bias.requires_grad_(True)              # heads refuses; the res layers record nothing
    out = m(X, B, E)
    torch.cuda.synchronize()
    assert m.last_head_route == ['cumsum', 'dense-cumsum']       # 4090 node rows, 4100 link rows
    assert m.last_temporal_route == 2 * [('pairs', ('layers', 'layers'))]        # 6 * 4100 rows: past the pair launch
    assert (m.last_temporal_route, m.last_head_route) == want_routes(m, 1, n, e, grad_any=True)
    assert all(bool(torch.isfinite(o).all()) for o in out)


def test_large_network_stack(dev):
    m, (X, B, E) = _emulator(dev, 2)
    m.fused_temporal = True                            # 256 node streams, 257 link streams
    with torch.no_grad():
        m(X, B, E)
    torch.cuda.synchronize()
    assert m.last_temporal_route == 2 * [('sides', ('stack', 'stack'))] and m.last_temporal_path == 'stack'
    assert m.last_head_route == ['heads', 'heads']
    assert (m.last_temporal_route, m.last_head_route) == want_routes(m, 1, m.n_node, m.n_edge)


def test_one_eager_and_one_graphed_step_are_the_same_step(dev):
    g, r, n, e = pair(dev)
    bt = batch(g, n, e, dev, 10)
    start = [p.detach().clone() for p in g.parameters()]
    same_losses(g.fit_eval(*bt), r.fit_eval(*bt))
    assert (g.last_fit_path, r.last_fit_path, g.last_fit_refusal) == ('graph-capture', 'eager', None)
    same_model(g, r)
    assert g._optimizer.t == 1 and max(float((p.detach() - q).abs().max()) for p, q in zip(g.parameters(), start)) > 1e-4
