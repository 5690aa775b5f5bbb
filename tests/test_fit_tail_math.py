"""CPU side of the fit-tail tests.

1. For every case tests/test_gpu_fit_tail.py uses, the patched oracle's gradients evaluated in fp32 agree with its fp64 self within
   TENSOR_ROUTE_GATE x max|gradient|: no gate, clamp or clip sits within fp32 rounding of its threshold for the chosen seeds (the
   GPU file asserts the same of the tensor route before it compares the HIP route with it).  The fp32 losses are printed beside
   the bound of the GPU file: fp32 tensor arithmetic clips a saturated probability at fl(1 - 1e-7) = 1 - 2^-23, which puts
   log(1.19e-7) where the definition has log(1e-7), so the flood loss of the fp32 composition misses that bound wherever a
   prediction saturates; that is reported, not asserted (the HIP operator clips p and 1 - p apart and is held to the bound).
2. uds_fit_tail / uds_fit_tail_backward refuse bad arguments with UDS_EINVAL and their own message before they touch a device
   (the pattern of tests/test_predict_tail_math.py).
"""
import ctypes

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from oracle import emulator_ref as OE
from tests import fit_tail_util as FT


@pytest.fixture(scope='module')
def built(networks):
    cache = {}

    def get(name):
        if name not in cache:
            cfg = FT.case_configs(networks)[name]
            args, norms = FT.setup(cfg, networks)
            cache[name] = (cfg, args, norms, FT.case_inputs(args, cfg['seed']))
        return cache[name]
    return get


@pytest.mark.parametrize('name', FT.CASES)
def test_fp32_oracle_gradients_sit_on_no_kink(built, name):
    cfg, args, norms, inp = built(name)
    g_loss, gy, gey = FT.upstream(args, inp, cfg['seed'], name == FT.ROLL)
    ref = FT.reference_grads(args, norms, inp, g_loss, gy, gey)
    g32 = FT.reference_grads(args, norms, inp, g_loss, gy, gey, torch.float32)
    for k in ('y', 'ey'):
        gmax = float(ref[k].abs().max())
        err = float((g32[k] - ref[k]).abs().max())
        assert gmax > 0 and err <= FT.TENSOR_ROUTE_GATE * gmax, (name, k, err, gmax)
    l64, l32 = FT.reference_losses(args, norms, inp), FT.reference_losses(args, norms, inp, torch.float32)
    for what, a, b, n in zip(('node', 'flood', 'edge'), l64, l32, FT.counts(args, inp)):
        if float(a) != 0:
            print('fit-tail %-22s %-5s fp64 %.9e fp32 oracle rel err %.3e bound %.3e' % (name, what, float(a), abs(float(b) - float(a)) / float(a), FT.loss_bound(n)))
    assert float(l64[0]) > 0 and float(l64[2]) > 0
    c = OE.config(args)
    assert (float(l64[1]) > 0) == bool(c.if_flood and not getattr(args, 'balance', False))


def test_cases_cover_the_branches(networks):
    cfgs = FT.case_configs(networks)
    assert set(FT.CASES) == set(cfgs) and set(FT.PLAIN) == set(FT.configs(networks))
    args, _ = FT.setup(cfgs[FT.BIG], networks)
    rows = FT.B * args.seq_out * args.state_shape[0]
    assert rows >= 4 * 256 and rows % 256 != 0
    for name in FT.BALANCE:
        assert FT.setup(cfgs[name], networks)[0].balance
    args, _ = FT.setup(cfgs['node_gates_balance'], networks)
    assert args.epsilon == 0.1 and args.if_flood and not args.edge_fusion
    args, _ = FT.setup(cfgs['plain_balance'], networks)
    assert not args.if_flood
    args, _ = FT.setup(cfgs[FT.ROLL], networks)
    assert args.roll == 2 and FT.case_inputs(args, 1).y.shape[1] == 2 * args.seq_out
    assert FT.loss_bound(1 << 10) == 18 * 2.0 ** -24


# ---- argument checks ----------------------------------------------------------------------------------------------------------
_BUF = np.zeros(64, dtype=np.float32)
P = _BUF.ctypes.data - _BUF.ctypes.data % 16 + 16       # a 16-byte aligned address
Q = P + 4                                               # misaligned by one float
EINVAL = -22


def _params(**over):
    p = _lib.TailParams()
    vals = dict(N=5, E=4, cy=2, ce=3, n_act=2, b_channels=1, edge_fusion=1, tide=0, has_offset=0, act=1, pump_override=0, any_pump=0,
                if_flood=1)
    vals.update(over)
    for k, v in vals.items():
        setattr(p, k, v)
    for n in _lib.TailParams.FLOAT_TABLES + _lib.TailParams.INT_TABLES:
        if n not in over:
            setattr(p, n, P)
    return p


LEAD = 'inc_n sign p y ey a b_norm y_true ey_true nwei poswei ewei qw_den span_b mini_b B T cyt balance '
ENTRIES = {'uds_fit_tail': LEAD + 'out_y out_ey loss_sums workspace', 'uds_fit_tail_backward': LEAD + 'g_loss g_out_y g_out_ey dy dey workspace'}

# (arguments changed, uds_tail_t fields changed, text after '<entry>: ')
BAD = [
    (dict(y_true=None), {}, 'NULL y_true/ey_true/nwei/poswei/ewei/workspace'),
    (dict(ewei=None), {}, 'NULL y_true/ey_true/nwei/poswei/ewei/workspace'),
    (dict(workspace=None), {}, 'NULL y_true/ey_true/nwei/poswei/ewei/workspace'),
    (dict(balance=2), {}, 'balance=2 (0 or 1)'),
    (dict(balance=1, qw_den=None), {}, 'balance needs qw_den, span_b and mini_b'),
    (dict(balance=1, mini_b=None), {}, 'balance needs qw_den, span_b and mini_b'),
    (dict(cyt=2), {}, 'cyt=2 (3 <= cyt <= 16)'),
    (dict(cyt=17), {}, 'cyt=17 (3 <= cyt <= 16)'),
    (dict(y_true=Q), {}, 'tensors must be 16-byte aligned'),
    (dict(workspace=Q), {}, 'tensors must be 16-byte aligned'),
    (dict(y=None), {}, 'NULL y/ey/b_norm/runoff/h0'),
    (dict(b_norm=None), {}, 'NULL y/ey/b_norm/runoff/h0'),
    (dict(p=None), {}, 'NULL argument'),
    (dict(T=0), {}, 'bad sizes B=2 T=0 N=5 E=4 ce=3 n_act=2 b_channels=1'),
    (dict(B=-1), {}, 'bad sizes B=-1 T=3 N=5 E=4 ce=3'),
    ({}, dict(ce=9), 'bad sizes B=2 T=3 N=5 E=4 ce=9'),
    ({}, dict(cy=4), 'cy=4 does not go with edge_fusion=1 if_flood=1 (needs 2)'),
    (dict(a=None), {}, 'act needs the settings a and n_act >= 1'),
    (dict(ey=Q), {}, 'tensors must be 16-byte aligned'),
    ({}, dict(hmax=None), 'NULL table in uds_tail_t'),
    (dict(B=1 << 20, T=1 << 20), {}, 'batch x steps x rows exceeds the int32 index'),
]
ONLY = {
    'uds_fit_tail': [(dict(out_y=None), {}, 'NULL output'), (dict(loss_sums=None), {}, 'NULL output'), (dict(out_ey=Q), {}, 'tensors must be 16-byte aligned')],
    'uds_fit_tail_backward': [(dict(g_loss=None), {}, 'NULL g_loss / gradient output'), (dict(dey=None), {}, 'NULL g_loss / gradient output'),
                              (dict(dy=Q), {}, 'tensors must be 16-byte aligned'), (dict(g_out_ey=Q), {}, 'tensors must be 16-byte aligned')],
}
ALL_BAD = [(e, c) for e in ENTRIES for c in BAD + ONLY[e]]


def _call(entry, changes, fields):
    p = _params(**fields)
    good = {n: P for n in ENTRIES[entry].split()}
    good.update(p=ctypes.addressof(p), B=2, T=3, cyt=5, balance=0)
    good.update(changes)
    lib = _lib.load()
    rc = getattr(lib, entry)(*[good[n] for n in ENTRIES[entry].split()], None)
    return rc, lib.uds_last_error().decode()


@pytest.mark.parametrize('entry,case', ALL_BAD, ids=['%s-%s' % (e, c[2].split(' (')[0][:40].replace(' ', '_')) + '-%d' % i for i, (e, c) in enumerate(ALL_BAD)])
def test_bad_argument_is_refused_with_its_message(entry, case):
    changes, fields, text = case
    rc, msg = _call(entry, changes, fields)
    assert rc == EINVAL and msg.startswith(entry + ': ' + text), (rc, msg)


def test_optional_gradients_may_be_null_but_the_rest_is_still_checked():
    """g_out_y / g_out_ey are optional: with both NULL the call gets as far as the next check (here: the incidence handle, which is
    looked into last)."""
    rc, msg = _call('uds_fit_tail_backward', dict(g_out_y=None, g_out_ey=None, T=0), {})
    assert rc == EINVAL and msg.startswith('uds_fit_tail_backward: bad sizes'), (rc, msg)


def test_workspace_size():
    lib = _lib.load()
    assert lib.uds_fit_tail_workspace_floats(5, 4, 2, 3) == 3 * 1024                     # the partials of the three losses
    assert lib.uds_fit_tail_workspace_floats(300, 4, 64, 5) == 2 * 64 * 5 * 300          # the node gradients of q_in / q_out
    assert lib.uds_fit_tail_workspace_floats(-1, 4, 2, 3) == 0
