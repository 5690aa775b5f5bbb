"""Host-side planning of `Emulator.graphed_fit` (no device): `fit_graph_refusal` names every piece of host state a captured step
would read, the graph key changes with each of its parts, and the flag converts an existing optimizer through its state_dict."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gnn_uds_amd as U
from gnn_uds_amd.emulator import HipKerasAdam, KerasAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 3


def build(**over):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))['astlingen']
    edges, n = np.asarray(net['edges']), net['n_node']
    e = len(edges)
    args = SimpleNamespace(state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=16, hidden_dim=16, n_sp_layer=1,
                           n_tp_layer=1, if_flood=1, edges=edges, graph=U.DrainageGraph.from_edges(edges, n), act=True, act_edges=edges[[1, 4]],
                           conv='GAT', resnet=True, recurrent='Conv1D', tide=True, is_outfall=np.asarray(net['is_outfall'], dtype=float))
    for k, v in over.items():
        setattr(args, k, v)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1))
    mk = lambda rows, c: np.stack([np.ones((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, 4))
    return emul, n, e


def tensors(n, e, B=2):
    return (torch.zeros(B, T, n, 5), torch.ones(B, T, 2), torch.zeros(B, T, n, 2), torch.zeros(B, T, n, 5), torch.zeros(B, T, e, 4),
            torch.zeros(B, T, e, 3))


def test_refusal_reasons(monkeypatch):
    m, n, e = build()
    assert type(m).graphed_fit.fget(m) is False and m.last_fit_path is None and m.last_fit_refusal is None
    assert 'CPU tensors' in m.fit_graph_refusal()                 # this model lives on the host
    assert 'CPU tensors' in m.fit_graph_refusal(*tensors(n, e))
    d, _, _ = build(dropout=0.1)
    assert 'dropout' in d.fit_graph_refusal() and 'host counters' in d.fit_graph_refusal()
    from torch import distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    assert 'process group with 2 ranks' in m.fit_graph_refusal()
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 1)
    assert 'CPU tensors' in m.fit_graph_refusal()                 # one rank: no all-reduce, the next reason decides
    # on the device none of these holds: what is left to refuse is decided by where the tensors live
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    assert m.fit_graph_refusal(*tensors(n, e)) is None


def test_key_changes_with_each_of_its_parts():
    m, n, e = build()
    x, a, b, y, ex, ey = tensors(n, e)
    key = lambda fit=True, t=(x, a, b, y, ex, ey): m._fit_graph_key(*t, fit)
    base = key()
    assert key() == base and hash(base) is not None
    assert key(False) != base
    assert key(t=tensors(n, e, 3)) != base                         # input shapes
    assert key(t=(x.double(), a, b, y, ex, ey)) != base
    for name, value in (('roll', 2), ('gradnorm', True), ('learning_rate', 5e-4), ('fused_fit_tail', False), ('dense_node_edge_train', True),
                        ('fused_gat_backward', True), ('fused_temporal', True), ('snapshot_remainder', True)):
        old = getattr(m, name)
        setattr(m, name, value)
        assert key() != base, name
        setattr(m, name, old)
        assert key() == base, name
    p = next(m.parameters())
    p.requires_grad_(False)
    frozen = key(False)
    p.requires_grad_(True)
    assert key(False) != frozen                                    # the set of parameters that train
    with torch.no_grad():
        p.data = p.data.clone()                                    # the same values in other storage
    assert key() != base
    base = key()
    m._optimizer = HipKerasAdam(list(m.parameters()), m.learning_rate, clipnorm=1.0)
    with_opt = key()
    assert with_opt != base and key(False) == m._fit_graph_key(x, a, b, y, ex, ey, False)
    m.set_norm(*[np.stack([np.ones(s), np.zeros(s)]).astype(np.float32) for s in ((n, 5), (n, 2), (n, 5), (n, 1), (e, 4))])
    assert key() != with_opt                                       # new norm tensors
    # an evaluation step also depends on which dense NodeEdge layers carry a bias off their support
    ev = key(False)
    ne = [mod for mod in m.modules() if type(mod).__name__ == 'NodeEdge'][0]
    with torch.no_grad():
        ne.bias.add_(0.5)
    assert key(False) != ev


def test_the_flag_converts_the_optimizer_and_back():
    m, n, e = build()
    params = list(m.parameters())
    m._optimizer = KerasAdam(params, m.learning_rate, clipnorm=1.0)
    m._optimizer.t = 7
    for k, t in enumerate(m._optimizer.m):
        t.fill_(0.25 + k)
    m.graphed_fit = True
    assert isinstance(m._optimizer, HipKerasAdam) and m._optimizer.t == 7 and float(m._optimizer.m[3].flatten()[0]) == 3.25
    sd = m._optimizer.state_dict()
    assert sd['t'] == 7 and isinstance(sd['t'], int)
    m.graphed_fit = False
    assert type(m._optimizer) is KerasAdam and m._optimizer.t == 7 and float(m._optimizer.m[3].flatten()[0]) == 3.25
    with pytest.raises(ValueError, match='does not match'):
        HipKerasAdam(params[:2]).load_state_dict(sd)
