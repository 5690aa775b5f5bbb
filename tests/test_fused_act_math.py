"""CPU checks behind tests/test_gpu_fused_acts.py: the parameters of tests/fused_act_util.py drive the pre-activations of both
epilogues of the spatial layer through every region of every activation, and the fp64 references would see what a wrong
epilogue computes.

Every check runs on each of the seven distinct layers of rows a-h (600 / 720, S = 2).  Measured over all of them: the regions
below -2.5, inside and above 2.5 hold 17-20 %, 59-65 % and 17-22 % of the pre-activations; the smallest move of a planted mistake
is 62 x the GPU bound (leaky relu in the Dense epilogue, link output of 128 / 128 / 128), every hard_sigmoid mistake moves the
outputs by at least 99 x and a mistake in the GAT epilogue by at least 971 x."""
import pytest
import torch

from tests import fused_act_util as FA
from tests import fused_chunk_util as FC

S = 2
SHAPE_IDS = ['%d-%d-%d%s' % (fx, fe, d, '-trained' if t else '') for fx, fe, d, t in FA.SHAPES]
EPILOGUES = ('Dense xe', 'GAT nodes', 'Dense ex', 'GAT links')      # the order pre_activations gives them in


@pytest.fixture(scope='module', params=FA.SHAPES, ids=SHAPE_IDS)
def layer(request):
    """(g, p, x, e, {act: pre-activations}) of one layer shape with the spread biases."""
    fx, fe, d, trained = request.param
    g = FC.graph(FA.NET)
    p = FA.act_params(g, fx, fe, d, trained=trained)
    x, e = FC.inputs(g, fx, fe, S)
    return g, p, x, e, {act: FA.pre_activations(g, p, x, e, act) for act in FA.ACTS}


def test_rows_cover_their_shapes():
    assert set(FA.ROWS) == set('abcdefgh') and len(FA.SHAPES) == 7      # d and e share a layer
    assert FA.ACTS == ('relu', 'linear', 'tanh', 'sigmoid', 'hard_sigmoid') and set(FA.MUTANTS) == set(FA.ACTS)
    assert [len(FA.MUTANTS[a]) for a in FA.ACTS] == [2, 2, 3, 1, 4]


def test_biases_are_the_only_change():
    g = FC.graph(FA.NET)
    p, q = FA.act_params(g, 96, 64, 64), FC.params(g, 96, 64, 64)
    assert set(p) == set(q)
    for key in p:
        if key not in FA.BIASES:
            assert torch.equal(p[key], q[key]), key
            continue
        want = torch.linspace(-FA.LIM, FA.LIM, p[key].numel(), dtype=torch.float64).float().double()
        assert torch.equal(p[key].sort().values, want) and not torch.equal(p[key], want), key      # a permutation, fp32 values
        assert torch.equal(p[key], FA.act_params(g, 96, 64, 64)[key]), key                          # seeded
    p, q = FA.act_params(g, 64, 64, 64, trained=True), FC.params(g, 64, 64, 64, dense=True, trained=True)
    for key in p:             # dense NodeEdge weights: raised to the mean of the support-only values (fused_act_util.NE_MEAN)
        if key in ('ne_n_w', 'ne_e_w'):
            assert torch.equal(p[key], (q[key] + FA.NE_MEAN).float().double()), key
        elif key not in FA.BIASES:
            assert torch.equal(p[key], q[key]), key


def test_every_region_of_every_epilogue_is_reached(layer):
    """Below -2.5, inside, above 2.5: each holds at least 10 % of the pre-activations of each of the four epilogues, whatever the
    activation in front of the GAT."""
    *_, pres = layer
    for act in FA.ACTS:
        flat = [t for pair in pres[act] for t in pair]
        for name, pre in zip(EPILOGUES, flat):
            shares = [float((pre < -FA.CLAMP).double().mean()), float((pre.abs() <= FA.CLAMP).double().mean()),
                      float((pre > FA.CLAMP).double().mean())]
            print('fused-acts regions %s %s: %.3f %.3f %.3f' % (act, name, *shares))
            assert min(shares) >= 0.10, (act, name, shares)


def test_the_old_parameters_do_not_reach_the_clamps(layer):
    """Why act_params exists: with FC.params' own biases no pre-activation of either epilogue reaches +-2.5."""
    g, p, x, e, _ = layer
    old = FC.params(g, x.shape[-1], e.shape[-1], p['gx_b'].numel(), dense='ne_n_w' in p, trained='ne_n_w' in p)
    for act in FA.ACTS:
        for pair in FA.pre_activations(g, old, x, e, act):
            for pre in pair:
                assert float(pre.abs().max()) < FA.CLAMP, (act, float(pre.abs().max()))


def test_equal_activations_give_the_oracle(layer):
    g, p, x, e, _ = layer
    for act in FA.ACTS:
        for got, want in zip(FA.epilogue_ref(g, p, x, e, act, act), FC.reference(g, p, x, e, act)):
            assert torch.equal(got, want), act


def test_a_wrong_epilogue_shows(layer):
    """Each planted mistake, in the Dense epilogue only and in the GAT epilogue only, moves both outputs by at least 50 x the
    bound of the GPU tests."""
    g, p, x, e, pres = layer
    for act in FA.ACTS:
        ref = tuple(FA._fn(act)(pre_g) for _, pre_g in pres[act])
        need = [50 * FC.TOL_BF16X3 * max(1.0, float(r.abs().max())) for r in ref]
        for name, fn in FA.MUTANTS[act]:
            for where, bad in (('Dense', FA.epilogue_ref(g, p, x, e, fn, act)), ('GAT', tuple(fn(pre_g) for _, pre_g in pres[act]))):
                for side, b, r, lim in zip(('nodes', 'links'), bad, ref, need):
                    moved = float((b - r).abs().max())
                    print('fused-acts mutant %s <- %s in %s, %s: %.0f x the bound' % (act, name, where, side, 50 * moved / lim))
                    assert moved >= lim, (act, name, where, side, moved, lim)
