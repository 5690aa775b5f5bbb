"""layers.PackCache, the one cache of packed or derived parameter copies: its key rule (version and storage pointer of every
tensor, then `extra`), one entry per slot, clear / copy / pickle leave it empty; and Emulator._invalidate_weight_packs empties the
cache of every module of a model.  CPU tensors, no library."""
import copy
import pickle

import torch

import gnn_uds_amd as U
from gnn_uds_amd import _lib, layers
from gnn_uds_amd.layers import PackCache
from tests.test_emulator_route import build

OLD_NAMES = ('_packed', '_blocks', '_wide', '_val_cache', '_rest_packed', '_vals')


class Builder:
    """build() that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_build_runs_once_per_key():
    c, b, t = PackCache(), Builder(), torch.zeros(3)
    first = c.get('s', (t,), b)
    assert c.get('s', (t,), b) is first and c.get('s', (t,), b) is first and b.calls == 1
    assert c.peek('s') is first and c.peek('other') is None and b.calls == 1


def test_every_way_a_parameter_changes_rebuilds():
    c, b = PackCache(), Builder()
    t = torch.nn.Parameter(torch.zeros(3), requires_grad=False)
    seen = [c.get('s', (t,), b)]
    with torch.no_grad():
        t.add_(1.0)                                         # an in-place op: the version moves
    seen.append(c.get('s', (t,), b))
    v = t._version
    t.data = torch.ones(3)                                  # new storage under the same version
    assert t._version == v
    seen.append(c.get('s', (t,), b))
    torch.autograd.graph.increment_version(t)               # what a graph replay and HipKerasAdam do
    seen.append(c.get('s', (t,), b))
    seen.append(c.get('s', (t,), b, extra=(96,)))
    seen.append(c.get('s', (t,), b, extra=(64,)))
    assert b.calls == 6 and len({id(o) for o in seen}) == 6
    assert c.get('s', (t,), b, extra=(64,)) is seen[-1] and b.calls == 6


def test_each_tensor_of_the_key_counts_and_none_is_accepted():
    c, b = PackCache(), Builder()
    k, bias = torch.zeros(2, 2), torch.zeros(2)
    a = c.get('s', (k, None), b)
    assert c.get('s', (k, None), b) is a and b.calls == 1
    assert c.get('s', (k, bias), b) is not a and b.calls == 2      # a bias appeared
    bias.add_(1.0)
    c.get('s', (k, bias), b)
    assert b.calls == 3                                            # the second tensor alone changed
    c.get('s', (k, None), b)
    assert b.calls == 4


def test_slots_are_independent():
    c, b1, b2, t = PackCache(), Builder(), Builder(), torch.zeros(3)
    x, y = c.get('x', (t,), b1), c.get('y', (t,), b2, extra=(1,))
    assert x is not y and (b1.calls, b2.calls) == (1, 1)
    c.get('y', (t,), b2, extra=(2,))
    assert c.peek('x') is x and c.get('x', (t,), b1) is x and (b1.calls, b2.calls) == (1, 2)


def test_a_slot_holds_one_entry():
    c, b, t = PackCache(), Builder(), torch.zeros(3)
    for extra in ((64, 64, False), (96, 96, True), (64, 64, False)):      # SpatialLayer between its two packings
        c.get('weights', (t,), b, extra=extra)
    assert b.calls == 3 and len(c._slots) == 1


def test_a_failed_build_leaves_the_slot_as_it_was():
    c, t = PackCache(), torch.zeros(3)

    def bad():
        raise _lib.UdsError('no')
    try:
        c.get('s', (t,), bad)
    except _lib.UdsError:
        pass
    assert c.peek('s') is None


def test_clear_copy_and_pickle_leave_it_empty():
    c, b, t = PackCache(), Builder(), torch.zeros(3)
    c.get('s', (t,), b)
    for other in (copy.deepcopy(c), pickle.loads(pickle.dumps(c)), copy.deepcopy({'m': c})['m']):
        assert isinstance(other, PackCache) and other is not c and other.peek('s') is None and not other._slots
    assert c.peek('s') is not None
    c.clear()
    assert c.peek('s') is None and not c._slots
    c.get('s', (t,), b)
    assert b.calls == 2
    layer = U.Dense(4, in_features=4)
    layer._packs.get('s', (layer.kernel,), b)
    twin = copy.deepcopy(layer)
    assert twin._packs is not layer._packs and twin._packs.peek('s') is None and layer._packs.peek('s') is not None


def test_the_model_clears_every_modules_cache(monkeypatch):
    monkeypatch.setattr(_lib, 'rowgemm_pack', lambda k: object())
    for recurrent in ('Conv1D', 'GRU'):
        m = build(recurrent=recurrent)[0]
        for mod in m.modules():                             # the caches that exist only once _packed_kernel was asked
            if isinstance(getattr(mod, 'kernel', None), torch.Tensor) and mod.kernel.dim() >= 2:
                layers._packed_kernel(mod, mod.kernel.reshape(-1, mod.kernel.shape[-1]))
        held = [mod._packs for mod in m.modules() if hasattr(mod, '_packs')]
        kinds = {type(mod).__name__ for mod in m.modules() if hasattr(mod, '_packs')}
        assert {'Dense', 'GATConv', 'NodeEdge', 'SpatialLayer', recurrent} <= kinds, kinds
        for packs in held:
            packs.get('planted', (), object)
            assert packs.peek('planted') is not None
        m._invalidate_weight_packs()
        assert all(not packs._slots for packs in held)
        for mod in m.modules():
            assert not [n for n in OLD_NAMES if n in mod.__dict__], type(mod).__name__


def test_invalidation_names_no_attribute():
    import ast
    import inspect
    import textwrap
    fn = ast.parse(textwrap.dedent(inspect.getsource(U.Emulator._invalidate_weight_packs)))
    assert not [n for n in ast.walk(fn) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
