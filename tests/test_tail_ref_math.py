"""CPU checks of oracle/tail_ref.py, the fp64 references of tests/test_gpu_tail_entries.py:

  - `roll_update_ref` is one post-forward step of `oracle.emulator_ref.model_rollout` (post_proc + window feedback);
  - `dense_cumsum_heads_ref` is the tail of `oracle.emulator_ref.forward` (res_x -> out / flood / flood_out, res_e -> e_out);
  - the heads cases of the GPU file can see a failure: every output column carries signal, the bounded activations are not
    saturated, and a 0.05 change of any single layer's bias moves the reference by at least 5x the case's allowed error.
"""
import pytest
import torch

from oracle import emulator_ref as OE
from oracle.tail_ref import dense_cumsum_heads_ref, roll_update_ref
from tests.util import HEADS_CASES, emulator_args, emulator_norms, heads_case_id, heads_inputs, heads_ref, heads_tol

SATURATION = {'hard_sigmoid': (0.0, 1.0), 'sigmoid': (0.0, 1.0), 'tanh': (-1.0, 1.0)}


@pytest.mark.parametrize('if_flood', [0, 3])
@pytest.mark.parametrize('seq_out', [1, 2, 5])
def test_roll_update_ref_is_one_step_of_model_rollout(networks, monkeypatch, if_flood, seq_out):
    net = networks['astlingen']
    seq_in = 5
    args = emulator_args(net['edges'], net['n_node'], act=False, if_flood=if_flood, seq_in=seq_in, seq_out=seq_out, roll=2)
    c = OE.config(args)
    norms = emulator_norms(args)
    norms['y'][0, 3, 1] = norms['y'][0, 7, 2] = norms['y'][0, 11, 1] = norms['y'][0, 11, 2] = 5e-4      # below 1e-3: the flow scale is 0
    norms['e'][1, :, 2] = torch.linspace(-0.2, 0.3, c.n_edge, dtype=torch.float64)                      # a non-zero minimum
    g = torch.Generator().manual_seed(10 * seq_out + if_flood)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    B, N, E, cy = 2, c.n_node, c.n_edge, 1 + int(bool(if_flood))
    x, ex, b = rnd(B, seq_in, N, cy + 3), rnd(B, seq_in, E, 4), rnd(B, 2 * seq_out, N, 1)
    y, ey = rnd(B, seq_out, N, cy), rnd(B, seq_out, E, 3) * 2 - 1
    if if_flood:
        y[0, 0, :3, -1] = torch.tensor([0.5, 0.5 + 2.0 ** -40, 0.5 - 2.0 ** -40], dtype=torch.float64)

    seen = []

    def fake_forward(args_, params_, X, Bd, Ex, AE=None, ADJ=None):
        seen.append((X.clone(), Bd.clone(), Ex.clone()))
        return y, ey

    monkeypatch.setattr(OE, 'forward', fake_forward)
    ys, eys = OE.model_rollout(args, None, norms, x, None, b, ex)
    assert len(seen) == 2 and torch.equal(seen[0][0], x) and torch.equal(seen[0][2], ex)

    span, mini = norms['e'][0, :, 2] - norms['e'][1, :, 2], norms['e'][1, :, 2]
    ny = norms['y']
    scale_in, scale_out = (ny[0, :, 1] > 1e-3).double() / ny[0, :, 1], (ny[0, :, 2] > 1e-3).double() / ny[0, :, 2]
    assert int((scale_in == 0).sum()) == 2 and int((scale_out == 0).sum()) == 2
    inc = torch.as_tensor(c.node_edge, dtype=torch.float64)
    preds, x_new, ex_new = roll_update_ref(inc, span, mini, scale_in, scale_out, y, ey, b[:, :seq_out], x, ex, if_flood)
    pp, ep = OE.post_proc(args, norms, y, ey, None, b[:, :seq_out])
    assert torch.equal(ep, ey)
    assert preds.shape == pp.shape and torch.allclose(preds, pp, rtol=1e-13, atol=1e-15)
    assert torch.allclose(ys[:, :seq_out], preds.clamp(0, 1), rtol=1e-13, atol=1e-15)
    # the windows the second chunk's forward was given
    assert x_new.shape == seen[1][0].shape and torch.allclose(x_new, seen[1][0], rtol=1e-13, atol=1e-15)
    assert torch.equal(ex_new, seen[1][2])
    q = [1, 2]                                                       # q_in, q_out: the only computed channels
    rest = [ch for ch in range(cy + 3) if ch not in q]
    assert torch.equal(x_new[..., rest], seen[1][0][..., rest])        # copies, thresholded bit included
    if if_flood:
        assert x_new[0, seq_in - seq_out, :3, cy + 1].tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize('if_flood', [0, 1, 3])
def test_dense_cumsum_heads_ref_is_the_tail_of_forward(networks, if_flood):
    net = networks['astlingen']
    args = emulator_args(net['edges'], net['n_node'], act=False, if_flood=if_flood, seq_in=4, seq_out=3)
    c = OE.config(args)
    p = OE.init_params(args, seed=2)
    g = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    X, Bd, E = rnd(2, 4, c.n_node, c.n_in), rnd(2, 3, c.n_node, 1), rnd(2, 4, c.n_edge, 4)
    tail = {}
    out, e_out = OE.forward(args, p, X, Bd, E, tail=tail)
    out_plain, e_plain = OE.forward(args, p, X, Bd, E)
    assert torch.equal(out, out_plain) and torch.equal(e_out, e_plain)        # the hook changes nothing
    kb = lambda q: (q['kernel'], q['bias'])
    hidden = [kb(q) for q in p['flood']]
    assert len(hidden) == if_flood
    fk, fb = kb(p['flood_out']) if if_flood else (None, None)
    node = dense_cumsum_heads_ref(tail['x'], *kb(p['res_x']), tail['res'], c.activation, *kb(p['out']), 'hard_sigmoid', hidden, c.activation,
                                  fk, fb, 'sigmoid')
    link = dense_cumsum_heads_ref(tail['e'], *kb(p['res_e']), tail['res_e'], c.activation, *kb(p['e_out']), 'tanh')
    assert node.shape == out.shape and torch.allclose(node, out, rtol=0, atol=1e-14)
    assert link.shape == e_out.shape and torch.allclose(link, e_out, rtol=0, atol=1e-14)


def test_heads_cases_cover_what_the_kernel_branches_on():
    col = lambda k: {c[k] for c in HEADS_CASES}
    acts = {'linear', 'relu', 'tanh', 'sigmoid', 'hard_sigmoid'}
    assert col('n_hidden') == set(range(6)) and col('n_a') == {1, 2, 3, 4} and col('T') == {1, 2, 3, 4, 7}
    assert {(c['B'], c['R']) for c in HEADS_CASES} == {(1, 1), (1, 15), (1, 16), (3, 17), (2, 33), (1, 70)}
    assert col('act') == acts and col('act_a') == acts and col('act_h') == acts | {None} and col('act_f') == acts | {None}
    for nh in (4, 5):
        assert any(c['n_hidden'] == nh and c['B'] > 1 and c['R'] % 16 for c in HEADS_CASES)
    assert not all(c['res'] for c in HEADS_CASES) and not all(c['bias'] for c in HEADS_CASES)
    assert {n for c in HEADS_CASES for n in c['no_bias']} >= {'a', 'h0', 'f'}
    assert all(c['act_h'] not in ('sigmoid', 'hard_sigmoid') or c['n_hidden'] == 1 for c in HEADS_CASES)


@pytest.mark.parametrize('case', HEADS_CASES, ids=heads_case_id)
def test_heads_case_can_see_a_failure(case):
    p = heads_inputs(case)
    ref = heads_ref(case, p)
    n_out = case['n_a'] + (1 if case['n_hidden'] else 0)
    assert ref.shape == (case['B'], case['T'], case['R'], n_out)
    # distinct non-zero biases, residuals that differ between batch elements
    biases = [t for t in [p['b'], p['a_bias'], p['f_bias']] + [hb for _, hb in p['hidden']] if t is not None]
    assert all(bool((t != 0).all()) for t in biases)
    assert len({float(t.flatten()[0]) for t in biases}) == len(biases)
    if case['res'] and case['B'] > 1:
        assert not torch.equal(p['res'][0], p['res'][1])
    # signal in every column
    if case['B'] * case['T'] * case['R'] >= 16:
        std = ref.reshape(-1, n_out).std(dim=0)
        assert float(std.min()) >= 0.02, std
    # bounded activations away from saturation
    for cols, act in ((slice(0, case['n_a']), case['act_a']), (slice(case['n_a'], n_out), case['act_f'])):
        if act in SATURATION and ref[..., cols].numel():
            v = ref[..., cols]
            near = sum(((v - s).abs() <= 1e-3).double().sum() for s in SATURATION[act])
            assert float(near) <= 0.2 * v.numel(), (act, float(near), v.numel())
    # a 0.05 change of one layer's bias (a missing bias counts as zeros) is at least 5x the allowed error
    allowed = heads_tol(case) * max(1.0, float(ref.abs().max()))
    bump = lambda t, n: (torch.zeros(n, dtype=torch.float64) if t is None else t) + 0.05
    variants = {'resnet': dict(b=bump(p['b'], 64)), 'head a': dict(a_bias=bump(p['a_bias'], case['n_a']))}
    for i, (H, hb) in enumerate(p['hidden']):
        variants['hidden %d' % (i + 1)] = dict(hidden=p['hidden'][:i] + [(H, bump(hb, 32))] + p['hidden'][i + 1:])
    if case['n_hidden']:
        variants['flood output'] = dict(f_bias=bump(p['f_bias'], 1))
    for name, change in variants.items():
        moved = float((heads_ref(case, {**p, **change}) - ref).abs().max())
        assert moved >= 5 * allowed, (name, moved, allowed)
