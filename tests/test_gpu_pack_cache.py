"""Every site that keeps packed or derived parameter copies in a layers.PackCache, on the GPU, at the smallest shape that takes
its route: a forward, one parameter changed (in place under no_grad, then in a second pass through `p.data = new`), a forward
again -- bit-equal (torch.equal) to a freshly built module that was loaded with the updated parameters and has never cached
anything, and different from the output before the update.  Counters on the four pack entries of _lib check that a second
forward packs nothing, that a cleared cache packs what a fresh module packs, and that an update re-packs what depends on the
changed parameter and nothing else (a second, untouched instance of the layer packs nothing).

The `p.data =` pass on the bias of a recurrent layer whose input projection runs on the row GEMM (LSTM at F = 128, GRU at
F = 32: the cached fold of the biases) is the one case the per-site keys this cache replaced got wrong: they held the bias by
version alone, and the forward after `bias.data = bias + 0.1` kept the old fold (on an MI355X: off by 9.1e-2 and 1.0e-1 from
the fresh module).  'spatial-remainder' takes the route the plan gives (astlingen: rem-ws); 'spatial-remainder-split96' sets the
layer's own override so that the 96-wide packing (the `remainder` variant of the 'weights' slot) is covered as well."""
import json
import os

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib
from gnn_uds_amd.emulator import GRU, LSTM, Conv1D
from gnn_uds_amd.graph import CSR
from gnn_uds_amd.layers import PackCache
from tests.util import ladder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_FNS = ('rowgemm_pack', 'recurrent_pack', 'remainder_pack', 'spatial_pack_weights')
FULL = 'what a fresh module packs'
NONE = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture
def counts(monkeypatch):
    seen = {}
    for name in PACK_FNS:
        def counted(*args, _fn=getattr(_lib, name), _name=name, **kw):
            seen[_name] = seen.get(_name, 0) + 1
            return _fn(*args, **kw)
        monkeypatch.setattr(_lib, name, counted)
    return seen


def rnd(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * 2 - 1


class Site:
    """make() -> a new module on the device, seeded; run(module) -> one output tensor; expect: parameter name -> the pack calls
    the forward after changing it makes (FULL: those of a fresh module's first forward); delta(module, name, seed): what to add."""

    def __init__(self, make, run, expect, delta=None, after=None):
        self.make, self.run, self.expect, self.after = make, run, expect, after
        self.delta = delta or (lambda m, name, seed: rnd(seed, *m.get_parameter(name).shape).to(m.get_parameter(name).device) * 0.1)


def dense_site(dev, fi, units, rows):
    x = rnd(1, rows, fi).to(dev)
    make = lambda: U.Dense(units, 'tanh', in_features=fi, generator=torch.Generator().manual_seed(2), precision='bf16x3').to(dev)
    return Site(make, lambda m: m(x), {'kernel': FULL, 'bias': FULL if units > 64 else NONE})


def conv1d_site(dev):
    x = rnd(1, 1, 4, 5, 64).to(dev)
    make = lambda: Conv1D(64, 3, 2, 'tanh', in_features=64, generator=torch.Generator().manual_seed(2), precision='bf16x3').to(dev)
    return Site(make, lambda m: m(x), {'kernel': FULL, 'bias': NONE})


def gat_site(dev):
    csr = ladder(128)
    h, x = _lib.CsrHandle(csr), rnd(1, 32, 128, 32).to(dev)

    def make():
        m = U.GATConv(16, activation='tanh', in_channels=32, generator=torch.Generator().manual_seed(2)).to(dev)
        m.precision = 'bf16x3'
        return m
    return Site(make, lambda m: m([x, h]), {'kernel': FULL, 'attn_kernel_self': FULL, 'attn_kernel_neighs': FULL, 'bias': NONE})


def diffusion_site(dev):
    csr = ladder(67)
    filt = U.DiffusionConv.preprocess(CSR(csr.rowptr, csr.col, csr.n_rows, csr.n_cols, 0.5 + np.random.default_rng(3).random(csr.nnz)))
    x = rnd(1, 2, 67, 8).to(dev)
    make = lambda: U.DiffusionConv(8, K=3, generator=torch.Generator().manual_seed(2)).to(dev)

    def after(m):
        assert not m.moments and m._packs.peek('table') is not None
    return Site(make, lambda m: m([x, filt]), {'kernel': NONE}, after=after)      # the table is torch arithmetic: no pack entry


def spatial_site(dev, remainder, split96=False):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))['astlingen']
    g = U.DrainageGraph.from_edges(np.asarray(net['edges']), net['n_node'])
    handle = _lib.NetworkHandle(g)
    x, e = rnd(1, 1, g.n_node, 64).to(dev), rnd(2, 1, g.n_edge, 64).to(dev)

    def make():
        m = U.SpatialLayer(g, 64, 'tanh', sparse_params=False, net=handle, generator=torch.Generator().manual_seed(3)).to(dev)
        for i, ne in enumerate((m.node_edge_n, m.node_edge_e)):
            if remainder:
                ne.bias.data = rnd(10 + i, *ne.shape).to(dev) * 0.05
        if split96:
            m._ws_rem_ok = False      # the layer's own override: the remainder rides into the 96-wide kernel whatever the plan says
        return m

    def delta(m, name, seed):
        p = m.get_parameter(name)
        d = rnd(seed, *p.shape).to(dev) * 0.1
        if name.endswith('.bias') and name.startswith('node_edge') and not remainder:      # stay on the support: the route stays 'fused'
            on = torch.zeros(p.numel(), device=dev)
            on[m.get_submodule(name.split('.')[0])._flat] = 1.0
            d = d * on.reshape(p.shape)
        return d

    def after(m):
        assert m.last_route in (('rem-split96',) if split96 else ('rem-ws', 'rem-split96') if remainder else ('fused',)), m.last_route
        print('SpatialLayer route:', m.last_route)
    expect = {n: NONE for n, _ in make().named_parameters()}
    for side in ('dense_xe', 'dense_ex'):      # with a remainder the Dense kernels are packed for rest @ Dense(.) as well
        expect[side + '.kernel'] = {'spatial_pack_weights': 1, 'rowgemm_pack': 1} if remainder else {'spatial_pack_weights': 1}
    for side in ('gat_x', 'gat_e'):
        expect[side + '.kernel'] = {'spatial_pack_weights': 1}
    if remainder:
        for name in ('node_edge_n.weight', 'node_edge_n.bias', 'node_edge_e.weight', 'node_edge_e.bias'):
            expect[name] = {'remainder_pack': 1}
    return Site(make, lambda m: torch.cat([t.reshape(-1) for t in m(x, e)]), expect, delta, after)


def recurrent_site(dev, cls, F):
    x = rnd(1, 1, 2, 5, F).to(dev)

    def make():
        m = cls(64, in_features=F, generator=torch.Generator().manual_seed(2), precision='bf16x3').to(dev)
        m.bias.data = m.bias.detach() + rnd(4, *m.bias.shape).to(dev) * 0.1
        return m
    return Site(make, lambda m: m(x), {'kernel': FULL, 'recurrent_kernel': FULL, 'bias': FULL})


SITES = {
    'dense-rowgemm': lambda dev: dense_site(dev, 32, 16, 5),
    'dense-blocks': lambda dev: dense_site(dev, 32, 80, 4096),
    'conv1d': conv1d_site,
    'gat-wide': gat_site,
    'diffusion-table': diffusion_site,
    'spatial-fused': lambda dev: spatial_site(dev, False),
    'spatial-remainder': lambda dev: spatial_site(dev, True),
    'spatial-remainder-split96': lambda dev: spatial_site(dev, True, split96=True),
    'gru-f64-direct': lambda dev: recurrent_site(dev, GRU, 64),
    'lstm-f128-projected': lambda dev: recurrent_site(dev, LSTM, 128),
    'gru-f32-projected': lambda dev: recurrent_site(dev, GRU, 32),
}
# the pack calls of a fresh module's first forward, from the code of each route (recurrent_pack packs its G or 2 G slices with rowgemm_pack)
FIRST = {
    'dense-rowgemm': {'rowgemm_pack': 1}, 'dense-blocks': {'rowgemm_pack': 2}, 'conv1d': {'rowgemm_pack': 1}, 'gat-wide': {'rowgemm_pack': 2},
    'diffusion-table': {}, 'spatial-fused': {'spatial_pack_weights': 1},
    'spatial-remainder': {'spatial_pack_weights': 1, 'remainder_pack': 2, 'rowgemm_pack': 2},
    'spatial-remainder-split96': {'spatial_pack_weights': 1, 'remainder_pack': 2, 'rowgemm_pack': 2},
    'gru-f64-direct': {'recurrent_pack': 1, 'rowgemm_pack': 6}, 'lstm-f128-projected': {'recurrent_pack': 1, 'rowgemm_pack': 8},
    'gru-f32-projected': {'recurrent_pack': 1, 'rowgemm_pack': 6},
}


def caches(m):
    return [c for mod in m.modules() for c in vars(mod).values() if isinstance(c, PackCache)]


def held(m):
    return [(slot, id(v[1])) for c in caches(m) for slot, v in sorted(c._slots.items())]


@pytest.mark.parametrize('site', sorted(SITES))
def test_cache_follows_every_parameter(dev, counts, site):
    s = SITES[site](dev)

    def forward(m):
        counts.clear()
        with torch.no_grad():
            y = s.run(m)
        return y, dict(counts)

    a = s.make()
    y0, first = forward(a)
    assert first == FIRST[site], first
    if s.after:
        s.after(a)
    before = held(a)
    assert before
    y0b, again = forward(a)
    assert again == {} and torch.equal(y0b, y0) and held(a) == before          # packed once per update
    for c in caches(a):
        c.clear()
    y0c, cleared = forward(a)
    assert cleared == first and torch.equal(y0c, y0)
    b = s.make()                                                               # a second instance: none of a's updates concern it
    yb = forward(b)[0]
    seed = 100
    for how in ('in place', '.data ='):
        for name in s.expect:
            what = '%s, %s %s' % (site, name, how)
            y_old = forward(a)[0]
            p, seed = a.get_parameter(name), seed + 1
            d = s.delta(a, name, seed)
            if how == 'in place':
                with torch.no_grad():
                    p.add_(d)
            else:
                version = p._version
                p.data = p.detach() + d
                assert p._version == version, what
            y_new, packed = forward(a)
            want = first if s.expect[name] is FULL else s.expect[name]
            assert packed == want, (what, packed, want)
            yb2, other = forward(b)
            assert other == {} and torch.equal(yb2, yb), what
            assert not torch.equal(y_new, y_old), what                         # the update reaches the output
            fresh = s.make()
            for n, q in fresh.named_parameters():
                q.data = a.get_parameter(n).detach().clone()
            assert not held(fresh)
            y_ref = forward(fresh)[0]
            assert torch.equal(y_new, y_ref), '%s: max abs difference %.3e' % (what, float((y_new - y_ref).abs().max()))
