"""uds_conv_stack_forward on the GPU: k_conv3_stack<L, ACT> against the layer chain it replaces (bit for bit), against the fp64
reference, under forced time segmentations, in guarded and poisoned memory, under graph capture, and wired into Emulator.forward.
tests/conv_stack_util.py holds the cases, the plan mirror and the reference; tests/test_conv_stack_math.py checks on the CPU that the
cases reach every layout and that the reference carries signal.

Plain allocations, valid shapes: nothing here is meant to fault; refusals are asserted as return codes on the CPU.

Tolerance of the parity test, relative to max(1, max|ref|): TOL[L].  It is set from the LAYER CHAIN, not from the kernel under test:
with UDS_TOL_REPORT=1 the parity test also runs L successive uds_rowgemm_forward calls (kernels this file's subject does not touch)
on the case and prints their error against the same reference next to the stack's.

MEASURED on an MI355X (UDS_TOL_REPORT=1), worst max|out - ref| / max(1, max|ref|) over all 28 cases, the small ones included:
                                    L = 2                                    L = 3
  layer chain (sets the bound)      7.858e-6  [B86R33T29-L2-tanh]            9.854e-6  [B16R250T57-L3-tanh]
  test_parity_with_the_fp64_reference (k_conv3_stack)
                                    7.858e-6  [B86R33T29-L2-tanh]            9.854e-6  [B16R250T57-L3-tanh]
  allowed TOL[L] = 3 x the chain's  2.357e-5  (observed / allowed 0.333)     2.956e-5  (0.333)
  the project's per-layer bound     L * 1e-4 = 2e-4                          3e-4
The two rows agree because the worst cases have >= 256 streams, where the stack equals the chain bit for bit; on the four small
cases (the chain runs k_rowgemm_small there) the two errors also agreed to the printed digits, at most 7.8e-6 before scaling.
Every other test of this file is torch.equal.
"""
import os

import pytest
import torch

from gnn_uds_amd import _lib
from tests import conv_stack_util as CU
from tests import rowgemm_util as RU
from tests.conv_stack_util import BIG_CASES, CASES, REPEAT_CASE, case_id
from tests.util import PAD, SENTINEL, Guarded, nan_in

pytestmark = pytest.mark.gpu

# TOL[L] = 3 x the layer chain's worst (MEASURED above), and never above the project's per-layer row-GEMM bound L * 1e-4.
TOL = {2: 3 * 7.858e-6, 3: 3 * 9.854e-6}
assert all(TOL[L] <= L * 1e-4 for L in TOL)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _report(tag, c, err, lim):
    if os.environ.get('UDS_TOL_REPORT'):
        print('%-6s %-40s err %.3e allowed %.3e ratio %.3f' % (tag, case_id(c), err, lim, err / lim))


def operands(dev, c, p=None):
    """x, [(packed, bias)] on the device, every one a view inside a NaN-filled allocation."""
    p = p or CU.stack_inputs(c)
    x = nan_in(p['x'], dev)
    layers = [(nan_in(_lib.rowgemm_pack(k.reshape(192, 64).float().to(dev).contiguous()), dev), nan_in(b, dev)) for k, b in zip(p['k'], p['b'])]
    return x, layers


def nan_out(dev, c):
    """A guarded output pre-filled with NaN: an element the kernel does not write shows."""
    out = Guarded((c['B'], c['T'], c['R'], 64), dev)
    out.view.fill_(float('nan'))
    return out


def run_stack(dev, c, x, layers, n_seg=None):
    """The case through the entry into a guarded, NaN-pre-filled output; the (B, T, R, 64) result."""
    out = nan_out(dev, c)
    got = _lib.conv_stack_forward(x, layers, c['act'], n_seg=c['n_seg'] if n_seg is None else n_seg, out=out.view)
    assert got is out.view
    torch.cuda.synchronize()
    out.check(case_id(c))           # guards intact, every element written (finite)
    return out.view


def run_chain(c, x, layers):
    y = x
    for i, (pk, b) in enumerate(layers):
        y = _lib.rowgemm_forward(y, pk, b, 64, c['act'], taps=3, dilation=2 ** i)
    torch.cuda.synchronize()
    return y


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max()), max(1.0, float(ref.abs().max()))


# ---- 1. bitwise against the layer chain ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', BIG_CASES, ids=case_id)
def test_bitwise_equal_to_the_layer_chain(dev, case):
    c = case
    for i in range(c['L']):
        assert RU.conv_stream_taken(c['B'], c['R'], 3, 64, 64, 2 ** i, 64), 'the chain must run k_conv3_stream'
    x, layers = operands(dev, c)
    want = run_chain(c, x, layers)
    assert torch.equal(run_stack(dev, c, x, layers), want)                       # the case's own segmentation (planner or forced)
    other = 2 if c['T'] >= 2 and len(CU.segments(c)) != 2 else 1
    assert torch.equal(run_stack(dev, c, x, layers, n_seg=other), want)          # ... and another one


# ---- 2. segmentation changes no bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in CASES if c['T'] >= 5 and not c['n_seg']][::3] + CU.SMALL_CASES[-2:], ids=case_id)
def test_segmentation_changes_no_bit(dev, case):
    x, layers = operands(dev, case)
    one = run_stack(dev, case, x, layers, n_seg=1).clone()
    for n in (2, 3, case['T']):
        assert torch.equal(run_stack(dev, case, x, layers, n_seg=n), one), n


# ---- 3. fp64 parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_parity_with_the_fp64_reference(dev, case):
    p, ref = CU.data(case)
    x, layers = operands(dev, case, p)
    got = run_stack(dev, case, x, layers)
    err, scale = _err(got, ref)
    _report('stack', case, err / scale, TOL[case['L']])
    if os.environ.get('UDS_TOL_REPORT'):      # the figure the bound is set from: the layer chain on the same case
        cerr, _ = _err(run_chain(case, x, layers), ref)
        _report('chain', case, cerr / scale, TOL[case['L']])
    assert err <= TOL[case['L']] * scale, (err, TOL[case['L']] * scale)


# ---- 4. memory discipline --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in CASES if c['B'] >= 2 and c['T'] in (2, 9, 15, 7)], ids=case_id)
def test_a_poisoned_batch_element_stays_where_it_is(dev, case):
    """Batch element 1 of x is NaN: element 0 is finite and bit-equal to its result on the clean input (a ragged block re-reads its
    last valid row, never the next element's)."""
    x, layers = operands(dev, case)
    clean = run_stack(dev, case, x, layers)[0].clone()
    xp = x.clone()
    xp[1] = float('nan')
    out = nan_out(dev, case)
    _lib.conv_stack_forward(xp, layers, case['act'], n_seg=case['n_seg'], out=out.view)
    torch.cuda.synchronize()
    bits = out.buf.view(torch.int32)
    assert bool((bits[:PAD] == SENTINEL).all()) and bool((bits[PAD + out.n:] == SENTINEL).all())
    assert bool(torch.isfinite(out.view[0]).all()) and torch.equal(out.view[0], clean)


# ---- 5. repeatability ------------------------------------------------------------------------------------------------------
def test_more_units_than_resident_waves_repeat(dev):
    c = REPEAT_CASE
    assert len(CU.segments(c)) * CU.streams(c['B'], c['R']) > CU.SLOTS
    x, layers = operands(dev, c)
    first = run_stack(dev, c, x, layers).clone()
    assert torch.equal(run_stack(dev, c, x, layers), first)


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result(dev):
    c = BIG_CASES[5]
    x, layers = operands(dev, c)
    eager = run_stack(dev, c, x, layers).clone()                     # the warm-up call
    out = torch.full_like(eager, float('nan'))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            _lib.conv_stack_forward(x, layers, c['act'], out=out)
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- 7. model wiring -------------------------------------------------------------------------------------------------------
def _emulator(dev, n_tp_layer, n_node=4090, n_edge=4100, hidden_dim=64, edges=None):
    from types import SimpleNamespace
    import gnn_uds_amd as U
    if edges is None:
        edges = U.synthetic_drainage_network(n_node, n_edge, seed=0)
        g = U.DrainageGraph.from_edges(edges)
    else:
        g = U.DrainageGraph.from_edges(edges, n_node)
    a = SimpleNamespace(state_shape=(g.n_node, 4), edge_state_shape=(g.n_edge, 4), seq_in=6, seq_out=6, embed_size=64, hidden_dim=hidden_dim,
                        kernel_size=3, n_sp_layer=1, n_tp_layer=n_tp_layer, activation='relu', if_flood=3, edge_fusion=True, edges=g.edges,
                        act=False, graph=g, model_dir=None)
    emul = U.Emulator('GAT', True, 'Conv1D', a, precision='bf16x3', generator=torch.Generator().manual_seed(1)).to(dev)
    gen = torch.Generator().manual_seed(3)
    X, B, E = (torch.rand(1, 6, g.n_node, 5, generator=gen).to(dev), torch.rand(1, 6, g.n_node, 1, generator=gen).to(dev),
               torch.rand(1, 6, g.n_edge, 4, generator=gen).to(dev))
    for m in emul.modules():                    # trained-like: no zero bias
        if getattr(m, 'bias', None) is not None and m.bias.dim() == 1:
            m.bias.data.copy_(torch.rand(m.bias.shape, generator=gen) * 0.2 - 0.1)
    return emul, (X, B, E)


def _forward(emul, inputs, fused):
    emul.fused_temporal = fused
    emul.last_temporal_path = None
    with torch.no_grad():
        out = emul(*inputs)
    torch.cuda.synchronize()
    return [o.clone() for o in out], emul.last_temporal_path


@pytest.mark.parametrize('n_tp_layer', [2, 3])
def test_model_takes_the_stack_and_moves_no_bit(dev, n_tp_layer):
    emul, inputs = _emulator(dev, n_tp_layer)
    on, path_on = _forward(emul, inputs, True)
    off, path_off = _forward(emul, inputs, False)
    assert (path_on, path_off) == ('stack', 'layers')
    assert len(on) == len(off) and all(torch.equal(a, b) for a, b in zip(on, off))
    assert all(bool(torch.isfinite(a).all()) for a in on)


def test_model_keeps_the_layers_where_the_stack_does_not_apply(dev):
    import json
    import numpy as np
    emul, inputs = _emulator(dev, 4)
    assert _forward(emul, inputs, True)[1] == 'layers'                               # n_tp_layer = 4
    emul, inputs = _emulator(dev, 2, hidden_dim=32)
    assert _forward(emul, inputs, True)[1] == 'layers'                               # hidden_dim = 32
    net = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'networks.json')))['astlingen']
    emul, inputs = _emulator(dev, 2, n_node=net['n_node'], edges=np.asarray(net['edges']))
    assert _forward(emul, inputs, True)[1] == 'layers'                               # 30 nodes: the small-network pair launch
    emul, inputs = _emulator(dev, 2)
    emul.fused_temporal = True
    for q in emul.parameters():
        q.requires_grad_(True)
    out = emul(*inputs)                                                              # parameters require grad: the training path
    torch.cuda.synchronize()
    assert emul.last_temporal_path == 'layers' and any(o.requires_grad for o in out)
