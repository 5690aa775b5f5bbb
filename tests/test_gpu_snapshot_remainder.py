"""fp64 parity of the one-launch remainder of a trained NodeEdge (gnn_uds_amd/csrc/kernels_remainder_snapshot.hpp:
uds_remainder_snapshot, uds_remainder_snapshot_pair), its refusals, its capture into a HIP graph, and the layer / model switch
that selects it (SpatialLayer.snapshot_remainder, Emulator.snapshot_remainder).  tests/snapshot_remainder_util.py holds the case
table, the restated plan and the cached inputs and fp64 references; tests/test_snapshot_remainder_math.py checks on the CPU that
every case reaches the plan it claims and that the references carry signal.

Memory set-up as in tests/test_gpu_remainder_routes.py: the C entries are called with pointers; every input is an exactly sized view
inside a NaN-filled allocation (a read of a row past M, or of a snapshot past S, turns the result NaN), the packed planes and the
output are views inside sentinel-filled allocations checked on both sides, and the output is pre-filled with NaN, so an element
nobody writes shows.  Plain allocations, valid shapes: nothing here is meant to fault.

Bounds, relative to max(1, max|ref|) through tests.util.close, against fp64 references:
  entries   TOL_DENSE = 1e-5 (tests/remainder_util.py), the project's bound for rest @ act(e W + b); the tiled path measures 0.69 of it
  layer     1e-5, the project's per-layer bound (tests/test_gpu_parity.py: TOL_BF16X3), against oracle.spektral_dense.spatial_layer_dense
  model     2e-5, the project's whole-forward bound (tests/test_gpu_emulator.py: TOL_FWD), against oracle.emulator_ref.forward
The pair entry, the wrapper with leading dimensions, a second call and the replays of a captured graph are compared bit for bit.

MEASURED on an MI355X (worst observed / allowed; `report` prints every figure with -s):
  entries   0.814  [G8 rb1 R30M29S17h32-F64-relu]   err 8.136e-6 of 1.000e-5; 0.799 at M = 576 (h = 32, F = 64), 0.774 at 443 x 444,
            0.757 / 0.765 / 0.670 on 30 x 29 with S = 5 / 600 / 2060; the rest 0.17 - 0.62
  pair      0.934  [single R30M29S9h32-F64-relu]    err 9.344e-6 of 1.000e-5; the other three sides 0.69 - 0.75; the pair entry, either
            side alone through it and the wrappers: the bits of the single-side calls
  layer     0.064 - 0.088 of 1e-5, astlingen and shunqing, d = 64 and 128; flag off: the bits of a layer without the attribute
  model     0.048 / 0.127 of 2e-5 (nodes / links) at d = 64, 0.029 / 0.161 at d = 128
These ratios are those of the arithmetic, not of this kernel: uds_remainder_forward_dense, the tiled path, gives the SAME BITS on
every case of the table and of the pairs (max |tiled - snapshot| = 0 at all 24, so 0.934 there too) -- both split the operands
alike and add the k-steps in ascending order into fp32 -- and tests/test_gpu_remainder_routes.py explains why signed inputs take
0.6 - 0.7 of the 1e-5 whatever the kernel (its own worst case, 0.693, is one of five shapes; here there are 24).
No bound was raised after a failure: every test passed at its first run.
"""
import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from oracle import spektral_dense as OD
from tests import snapshot_remainder_util as SU
from tests.remainder_util import TOL_DENSE
from tests.snapshot_remainder_util import CASES, PAIR_CASES, case_id
from tests.util import Guarded, close, emulator_args, emulator_norms, load_emulator, load_spatial_layer, nan_in, spatial_params

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC07FC0
TOL_LAYER = 1e-5
TOL_FWD = 2e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def nan_guarded(shape, dev):
    g = Guarded(shape, dev)
    g.view.view(torch.int32).fill_(NAN16)
    return g


def report(fam, what, got, ref, tol):
    err = float((got.detach().double().cpu() - ref).abs().max())
    lim = tol * max(1.0, float(ref.abs().max()))
    print('%-8s %-44s err %.3e allowed %.3e ratio %.3f' % (fam, what, err, lim, err / lim))


class Operands:
    """One side's device operands: rest packed by uds_remainder_pack into guarded memory, e / W image / bias in NaN-filled memory."""

    def __init__(self, dev, c):
        self.c = c
        self.p, self.ref = SU.data(c)
        lib = _lib.load()
        R, M = c['R'], c['M']
        n = lib.uds_remainder_packed_bytes(R, M)
        self.rest = nan_in(self.p['rest'], dev)
        self.pk = nan_guarded((n // 4,), dev)
        rc = lib.uds_remainder_pack(self.rest.data_ptr(), R, M, self.pk.view.data_ptr(), _stream())
        assert rc == 0, lib.uds_last_error()
        self.e, self.b = nan_in(self.p['e'], dev), nan_in(self.p['b'], dev)
        self.pw = nan_in(_lib.rowgemm_pack(self.p['W'].to(dev).contiguous()), dev)
        torch.cuda.synchronize()
        self.pk.check(case_id(c) + ': packed planes')
        self.before = self.pk.view.clone()

    def out(self, dev):
        return nan_guarded((self.c['S'], self.c['R'], self.c['h']), dev)

    def group(self, out):
        """The per-side arguments of uds_remainder_snapshot_pair."""
        return [self.pk.view.data_ptr(), self.c['R'], self.c['M'], self.e.data_ptr(), self.pw.data_ptr(), _ptr(self.b), out.view.data_ptr()]

    def single(self, out, **over):
        c = dict(self.c, **over)
        return _lib.load().uds_remainder_snapshot(self.pk.view.data_ptr(), c['R'], c['M'], self.e.data_ptr(), c['F'], self.pw.data_ptr(), _ptr(self.b),
                                                  _lib.ACT[c['act']], c['S'], c['h'], out.view.data_ptr(), _stream())

    def check(self, out, what):
        torch.cuda.synchronize()
        out.check(what + ': out')
        self.pk.check(what + ': packed planes')
        assert torch.equal(self.pk.view.view(torch.int32), self.before.view(torch.int32)), 'the packed planes changed'


_OPS = {}


def operands(dev, c):
    if case_id(c) not in _OPS:
        _OPS[case_id(c)] = Operands(dev, c)
    return _OPS[case_id(c)]


# ---- uds_remainder_snapshot ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_entry(dev, case):
    c = case
    what = 'G%d rb%d %s' % (c['claims'] + (case_id(c),))
    op = Operands(dev, c)
    out = op.out(dev)
    rc = op.single(out)
    assert rc == 0, _lib.load().uds_last_error()
    op.check(out, what)
    report('entry', what, out.view, op.ref, TOL_DENSE)
    close(out.view, op.ref, TOL_DENSE)
    again = op.out(dev)
    assert op.single(again) == 0
    op.check(again, what)
    assert torch.equal(again.view, out.view)
    if c['lead']:                                                    # the wrapper keeps leading dimensions
        got = _lib.remainder_snapshot(op.pk.view, (c['R'], c['M']), op.e.reshape(c['lead'] + (c['M'], c['F'])), op.pw, op.b, c['act'], c['h'])
        assert tuple(got.shape) == c['lead'] + (c['R'], c['h']) and torch.equal(got.reshape(out.view.shape), out.view)


def test_wrapper_with_no_snapshots(dev):
    c = CASES[0]
    op = operands(dev, c)
    got = _lib.remainder_snapshot(op.pk.view, (c['R'], c['M']), op.e[:0], op.pw, op.b, c['act'], c['h'])
    assert tuple(got.shape) == (0, c['R'], c['h'])
    with pytest.raises(_lib.UdsError):
        _lib.remainder_snapshot(op.pk.view, (c['R'], c['M']), op.e[:0].cpu(), op.pw, op.b, c['act'], c['h'])
    a, b = _lib.remainder_snapshot_pair((op.pk.view, (c['R'], c['M']), op.e[:0], op.pw, op.b, c['act'], c['h']), None)
    assert tuple(a.shape) == (0, c['R'], c['h']) and b is None


# ---- uds_remainder_snapshot_pair -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIR_CASES, ids=lambda p: case_id(p[0]) + '+' + case_id(p[1]))
def test_pair(dev, pair):
    """Both sides in one launch, then each side alone through the pair entry (the other NULL): the bits of the single-side calls."""
    lib = _lib.load()
    ops = [operands(dev, c) for c in pair]
    c = pair[0]
    alone = []
    for op in ops:
        out = op.out(dev)
        assert op.single(out) == 0, lib.uds_last_error()
        op.check(out, case_id(op.c))
        report('pair', 'single ' + case_id(op.c), out.view, op.ref, TOL_DENSE)
        close(out.view, op.ref, TOL_DENSE)
        alone.append(out)
    tail = [c['F'], _lib.ACT[c['act']], c['S'], c['h'], _stream()]
    none = [None, 0, 0, None, None, None, None]
    both = [op.out(dev) for op in ops]
    rc = lib.uds_remainder_snapshot_pair(*ops[0].group(both[0]), *ops[1].group(both[1]), *tail)
    assert rc == 0, lib.uds_last_error()
    for op, out, ref in zip(ops, both, alone):
        op.check(out, 'pair ' + case_id(op.c))
        assert torch.equal(out.view, ref.view)
    for i, op in enumerate(ops):                                     # one side NULL, in either position
        out = op.out(dev)
        groups = [none, none]
        groups[i] = op.group(out)
        rc = lib.uds_remainder_snapshot_pair(*groups[0], *groups[1], *tail)
        assert rc == 0, lib.uds_last_error()
        op.check(out, 'pair, side %d only' % i)
        assert torch.equal(out.view, alone[i].view)
    rc = lib.uds_remainder_snapshot_pair(*none, *none, *tail)
    assert rc == -22 and b'both sides are NULL' in lib.uds_last_error()
    # the wrapper: tuples of tensors, None for a side
    side = lambda op: (op.pk.view, (op.c['R'], op.c['M']), op.e, op.pw, op.b, op.c['act'], op.c['h'])
    w0, w1 = _lib.remainder_snapshot_pair(side(ops[0]), side(ops[1]))
    assert torch.equal(w0, alone[0].view) and torch.equal(w1, alone[1].view)
    w0, w1 = _lib.remainder_snapshot_pair(None, side(ops[1]))
    assert w0 is None and torch.equal(w1, alone[1].view)
    with pytest.raises(_lib.UdsError):
        _lib.remainder_snapshot_pair(None, None)
    with pytest.raises(_lib.UdsError):                               # the sides must share S
        _lib.remainder_snapshot_pair(side(ops[0]), side(ops[1])[:2] + (ops[1].e[:1],) + side(ops[1])[3:])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """UDS_EINVAL (-22) with a text, nothing launched: the output keeps its NaN fill."""
    lib = _lib.load()
    c = CASES[0]
    op = operands(dev, c)
    out = op.out(dev)
    top = SU.largest_m(c['F'], c['h'])
    for over, text in ((dict(M=top + 1), b'refused'), (dict(F=96), b'F = 96'), (dict(h=48), b'h = 48'), (dict(act=None, S=-1), b'S = -1'),
                       (dict(R=0), b'bad shape'), (dict(S=(1 << 24) + 1), b'S = ')):
        assert op.single(out, **over) == -22, over
        assert text in lib.uds_last_error(), (over, lib.uds_last_error())
    rc = lib.uds_remainder_snapshot(op.pk.view.data_ptr(), c['R'], c['M'], op.e.data_ptr(), c['F'], op.pw.data_ptr(), _ptr(op.b), 9, c['S'], c['h'],
                                    out.view.data_ptr(), _stream())
    assert rc == -22 and b'activation' in lib.uds_last_error()
    for args in ((None, op.e.data_ptr(), op.pw.data_ptr(), out.view.data_ptr()), (op.pk.view.data_ptr(), None, op.pw.data_ptr(), out.view.data_ptr()),
                 (op.pk.view.data_ptr(), op.e.data_ptr(), None, out.view.data_ptr()), (op.pk.view.data_ptr(), op.e.data_ptr(), op.pw.data_ptr(), None),
                 (op.pk.view.data_ptr(), op.e.data_ptr() + 4, op.pw.data_ptr(), out.view.data_ptr())):
        rc = lib.uds_remainder_snapshot(args[0], c['R'], c['M'], args[1], c['F'], args[2], _ptr(op.b), _lib.ACT[c['act']], c['S'], c['h'], args[3], _stream())
        assert rc == -22 and lib.uds_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.view).all())
    # the wrappers: e of the wrong row count; a shape the plan refuses
    with pytest.raises(_lib.UdsError, match='against rest'):
        _lib.remainder_snapshot(op.pk.view, (c['R'], c['M']), op.e[:, :-1].contiguous(), op.pw, op.b, c['act'], c['h'])
    with pytest.raises(_lib.UdsError, match='against rest'):
        _lib.remainder_snapshot_pair((op.pk.view, (c['R'], c['M'] + 1), op.e, op.pw, op.b, c['act'], c['h']), None)
    e_wide = torch.zeros(1, top + 1, c['F'], device=dev)
    with pytest.raises(_lib.UdsError, match='refused'):
        _lib.remainder_snapshot(op.pk.view, (c['R'], top + 1), e_wide, op.pw, op.b, c['act'], c['h'])
    e96 = torch.zeros(1, c['M'], 96, device=dev)
    with pytest.raises(_lib.UdsError, match='F = 96'):
        _lib.remainder_snapshot(op.pk.view, (c['R'], c['M']), e96, op.pw, op.b, c['act'], c['h'])
    with pytest.raises(_lib.UdsError, match='h = 48'):
        _lib.remainder_snapshot(op.pk.view, (c['R'], c['M']), op.e, op.pw, op.b, c['act'], 48)


# ---- capture -------------------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_the_same_bits(dev):
    """One call captured into a HIP graph (a linear graph: one kernel node) and replayed twice, the output re-poisoned in between."""
    c = PAIR_CASES[1][1]
    op = operands(dev, c)
    eager = op.out(dev)
    assert op.single(eager) == 0
    op.check(eager, 'eager')
    out = op.out(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert op.single(out) == 0                                   # warm-up on the capture's stream, outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = op.single(out)
    assert rc == 0, _lib.load().uds_last_error()
    for _ in range(2):
        out.view.view(torch.int32).fill_(NAN16)
        graph.replay()
        op.check(out, 'replay')
        assert torch.equal(out.view, eager.view)


# ---- SpatialLayer.snapshot_remainder -------------------------------------------------------------------------------------------------
def _layer_setup(networks, name, d, dev, S=3):
    net = networks[name]
    gph = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
    p = spatial_params(gph.n_node, gph.n_edge, d, d, d, seed=7)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(S, gph.n_node, d, generator=g, dtype=torch.float64)
    e = torch.rand(S, gph.n_edge, d, generator=g, dtype=torch.float64)
    p['ne_n_b'] = torch.randn(p['ne_n_b'].shape, generator=g, dtype=torch.float64) * 0.01      # trained off the support
    p['ne_e_b'] = torch.randn(p['ne_e_b'].shape, generator=g, dtype=torch.float64) * 0.01
    mats = (torch.from_numpy(gph.adj.to_dense()), torch.from_numpy(gph.edge_adj.to_dense()), torch.from_numpy(gph.inc_n.to_dense()))
    return gph, p, x, e, mats


@pytest.mark.parametrize('name,d', [('astlingen', 64), ('astlingen', 128), ('shunqing', 64), ('shunqing', 128)])
def test_layer(dev, networks, name, d):
    gph, p, x, e, mats = _layer_setup(networks, name, d, dev)
    xd, ed = x.float().to(dev), e.float().to(dev)
    rx, re = OD.spatial_layer_dense(x, e, p, *mats)
    plain = load_spatial_layer(U.SpatialLayer(gph, d, 'relu', sparse_params=False), p, dev)          # never has the attribute set
    off = load_spatial_layer(U.SpatialLayer(gph, d, 'relu', sparse_params=False), p, dev)
    on = load_spatial_layer(U.SpatialLayer(gph, d, 'relu', sparse_params=False), p, dev)
    off.snapshot_remainder, on.snapshot_remainder = False, True
    assert 'snapshot_remainder' not in vars(plain) and plain.last_remainder is None
    with torch.no_grad():
        px, pe = plain(xd, ed)
        fx, fe = off(xd, ed)
        ox, oe = on(xd, ed)
    what = '%s d=%d' % (name, d)
    report('layer', what + ' nodes', ox, rx, TOL_LAYER)
    report('layer', what + ' links', oe, re, TOL_LAYER)
    close(ox, rx, TOL_LAYER); close(oe, re, TOL_LAYER)
    close(px, rx, TOL_LAYER); close(pe, re, TOL_LAYER)
    assert on.last_path == 'fused+remainder' and on.last_remainder == ('snapshot', 'snapshot')
    assert on.last_route == plain.last_route == off.last_route == ('rem-ws' if d == 64 else 'rem-d128')
    assert off.last_path == plain.last_path == 'fused+remainder' and off.last_remainder == plain.last_remainder == ('gemm', 'gemm')
    assert torch.equal(fx, px) and torch.equal(fe, pe)               # flag off: the bits of a layer that never had the attribute
    if d == 64:                                                      # the third remainder route goes through _remainders as well
        on._ws_rem_ok = False
        with torch.no_grad():
            sx, se = on(xd, ed)
        assert on.last_route == 'rem-split96' and on.last_remainder == ('snapshot', 'snapshot')
        close(sx, rx, TOL_LAYER); close(se, re, TOL_LAYER)
        on._ws_rem_ok = None
    # trained on the node side only
    p1 = dict(p, ne_e_b=torch.zeros_like(p['ne_e_b']))
    rx, re = OD.spatial_layer_dense(x, e, p1, *mats)
    load_spatial_layer(on, p1, dev)
    with torch.no_grad():
        ox, oe = on(xd, ed)
    assert on.last_remainder == ('snapshot', None) and on.last_path == 'fused+remainder'
    close(ox, rx, TOL_LAYER); close(oe, re, TOL_LAYER)
    # a support-only layer has no remainder to report
    p0 = dict(p1, ne_n_b=torch.zeros_like(p['ne_n_b']))
    load_spatial_layer(on, p0, dev)
    with torch.no_grad():
        on(xd, ed)
    assert on.last_path == 'fused' and on.last_remainder == (None, None)


def test_layer_keeps_the_gemm_when_asked_to_materialise(dev, networks, monkeypatch):
    gph, p, x, e, mats = _layer_setup(networks, 'astlingen', 64, dev)
    on = load_spatial_layer(U.SpatialLayer(gph, 64, 'relu', sparse_params=False), p, dev)
    on.snapshot_remainder = True
    monkeypatch.setenv('UDS_REMAINDER_MATERIALISE', '1')
    with torch.no_grad():
        ox, oe = on(x.float().to(dev), e.float().to(dev))
    assert on.last_remainder == ('gemm', 'gemm')
    rx, re = OD.spatial_layer_dense(x, e, p, *mats)
    close(ox, rx, TOL_LAYER); close(oe, re, TOL_LAYER)


# ---- Emulator.snapshot_remainder -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('embed', [64, 128])
def test_model(dev, networks, embed):
    """The whole network on astlingen with trained dense NodeEdge biases in every spatial layer, the switch on: the forward against the
    fp64 oracle; every 64 / 64 and 128 / 128 layer reports the snapshot kernel (at d = 64 the 96-wide first layer of block 2 is the
    unfused chain, which needs x_e as a tensor)."""
    net = networks['astlingen']
    args = emulator_args(net['edges'], net['n_node'], n_sp_layer=2, n_tp_layer=1, seq_in=4, seq_out=3, embed_size=embed, hidden_dim=64)
    params = OE.init_params(args, seed=3)
    g = torch.Generator().manual_seed(17)
    for blk in ('block1', 'block2'):
        for q in params[blk]:
            for key in ('node_edge_n', 'node_edge_e'):
                q[key]['bias'] = torch.randn(q[key]['bias'].shape, generator=g, dtype=torch.float64) * 0.02
    emul = load_emulator(U.Emulator(args.conv, args.resnet, args.recurrent, args), params, dev)
    norms = emulator_norms(args)
    emul.set_norm(*(norms[k].numpy() for k in 'xbyre'))
    emul.snapshot_remainder = True
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    B, N, E = 2, args.state_shape[0], args.edge_state_shape[0]
    X, Bd = rnd(B, args.seq_in, N, args.state_shape[1] + 1), rnd(B, args.seq_out, N, 1) * 0.1
    Ex, a = rnd(B, args.seq_in, E, 4), rnd(B, args.seq_out, 2)
    ry, rey = OE.forward(args, params, X, Bd, Ex, OE.get_edge_action(OE.config(args), a))
    f = lambda t: t.float().to(dev)
    with torch.no_grad():
        y, ey = emul(f(X), f(Bd), f(Ex), emul.get_edge_action(f(a)))
    report('model', 'astlingen d=%d nodes' % embed, y, ry, TOL_FWD)
    report('model', 'astlingen d=%d links' % embed, ey, rey, TOL_FWD)
    close(y, ry, TOL_FWD); close(ey, rey, TOL_FWD)
    layers = list(emul.block1.layers) + list(emul.block2.layers)
    got = [(ly.last_route, ly.last_remainder) for ly in layers]
    snap = ('snapshot', 'snapshot')
    if embed == 64:
        assert got == [('rem-ws', snap), ('rem-ws', snap), ('chain', (None, None)), ('rem-ws', snap)], got
    else:
        assert got == [('rem-d128', snap)] * 4, got
