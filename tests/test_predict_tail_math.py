"""CPU side of the predict-tail tests.

1. For every case tests/test_gpu_predict_tail.py uses, the patched oracle evaluated in fp32 agrees with its fp64 self within the
   GPU file's tolerance at EVERY entry: no hard gate (offset, depth > 0.01, flood bit, epsilon band, clip) sits within fp32
   rounding of its threshold, so the GPU test can allow zero outliers.  A case that breaks this gets another seed here.
2. uds_predict_tail / uds_predict_tail_backward refuse bad arguments with UDS_EINVAL and their own message before they touch a
   device (the pattern of tests/test_entry_checks.py: one aligned host address, never read).
"""
import ctypes

import numpy as np
import pytest
import torch

from gnn_uds_amd import _lib
from tests import predict_tail_util as PT

CASES = ['ef_act', 'ef_pumps_offset_tide', 'ef_all_pumps', 'node_gates', 'eps0', 'plain', 'T1', 'synth300', 'synth300_noloop']


@pytest.mark.parametrize('np_form', [False, True], ids=['predict_tf', 'predict'])
@pytest.mark.parametrize('name', CASES)
def test_fp32_oracle_flips_no_gate(networks, name, np_form):
    cfg = PT.configs(networks)[name]
    args, norms = PT.setup(cfg, networks)
    inp = PT.inputs(args, cfg['seed'])
    ry, rey = PT.reference(args, norms, inp, np_form, torch.float64)
    y32, ey32 = PT.reference(args, norms, inp, np_form, torch.float32)
    for what, out, ref, tol in (('y', y32, ry, PT.tol_y(cfg['T'])), ('ey', ey32, rey, PT.TOL_FLOW)):
        lim = tol * max(1.0, float(ref.abs().max()))
        d = (out.double() - ref).abs()
        assert int((d > lim).sum()) == 0, (name, what, float(d.max()), lim)
    # the case carries signal: flooding volume, both flow directions, and (where the model has them) gated flows
    assert float(ry[..., -1].max()) > 0 and float(rey[..., -1].max()) > 0 > float(rey[..., -1].min())


def test_cases_cover_the_branches(networks):
    cfgs = PT.configs(networks)
    assert set(CASES) == set(cfgs)
    args, _ = PT.setup(cfgs['synth300'], networks)
    ne = np.asarray(args.node_edge)
    assert ne.shape[0] == 300 and 2 * ne.shape[0] % 256 != 0
    assert not ne[:, 5].any() and not ne[298].any() and (ne[:, 2] == ne[:, 3]).all()      # self loop, isolated node, parallel link
    args, _ = PT.setup(cfgs['ef_pumps_offset_tide'], networks)
    assert args.pump.min() == 0 < args.pump.max() and args.offset.max() > 0 and args.tide       # predict overrides, predict_tf does not
    args, _ = PT.setup(cfgs['node_gates'], networks)
    assert args.pump.min() > 0 and args.pump_in.max() > 0 and args.pump_out.max() > 0 and args.epsilon == 0.1


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


FWD = 'inc_n sign p y ey a b_norm runoff h0 B T out_y out_ey'
BWD = 'inc_n sign p y ey a b_norm runoff h0 B T g_out_y g_out_ey dy dey da dh0 workspace'
ENTRIES = {'uds_predict_tail': FWD, 'uds_predict_tail_backward': BWD}

# (arguments changed, uds_tail_t fields changed, text after '<entry>: ')
BAD = [
    (dict(y=None), {}, 'NULL y/ey/b_norm/runoff/h0'),
    (dict(h0=None), {}, 'NULL y/ey/b_norm/runoff/h0'),
    (dict(p=None), {}, 'NULL argument'),
    (dict(sign=None), {}, 'NULL argument'),
    (dict(T=0), {}, 'bad sizes B=2 T=0 N=5 E=4 ce=3 n_act=2 b_channels=1'),
    (dict(B=-1), {}, 'bad sizes B=-1 T=3 N=5 E=4 ce=3'),
    ({}, dict(ce=1), 'bad sizes B=2 T=3 N=5 E=4 ce=1'),
    ({}, dict(ce=9), 'bad sizes B=2 T=3 N=5 E=4 ce=9'),
    ({}, dict(cy=4), 'cy=4 does not go with edge_fusion=1 if_flood=1 (needs 2)'),
    ({}, dict(cy=2, edge_fusion=0), 'cy=2 does not go with edge_fusion=0 if_flood=1 (needs 4)'),
    ({}, dict(cy=2, if_flood=0), 'cy=2 does not go with edge_fusion=1 if_flood=0 (needs 1)'),
    (dict(a=None), {}, 'act needs the settings a and n_act >= 1'),
    ({}, dict(n_act=0), 'act needs the settings a and n_act >= 1'),
    (dict(y=Q), {}, 'tensors must be 16-byte aligned'),
    (dict(ey=Q), {}, 'tensors must be 16-byte aligned'),
    (dict(a=Q), {}, 'tensors must be 16-byte aligned'),
    (dict(runoff=Q), {}, 'tensors must be 16-byte aligned'),
    ({}, dict(hmax=None), 'NULL table in uds_tail_t'),
    ({}, dict(from_node=None), 'NULL table in uds_tail_t'),
    ({}, dict(al_idx=None), 'act needs the action tables of uds_tail_t'),
    (dict(B=1 << 20, T=1 << 20), {}, 'batch x steps x rows exceeds the int32 index'),
]
ONLY = {
    'uds_predict_tail': [(dict(out_y=None), {}, 'NULL output'), (dict(out_ey=Q), {}, 'tensors must be 16-byte aligned')],
    'uds_predict_tail_backward': [(dict(g_out_y=None), {}, 'NULL gradient / workspace'), (dict(workspace=None), {}, 'NULL gradient / workspace'),
                                  (dict(dey=Q), {}, 'tensors must be 16-byte aligned'), (dict(dh0=Q), {}, 'tensors must be 16-byte aligned'),
                                  (dict(da=None), {}, 'act needs da')],
}
ALL_BAD = [(e, c) for e in ENTRIES for c in BAD + ONLY[e]]


def _call(entry, changes, fields):
    p = _params(**fields)
    good = {n: P for n in ENTRIES[entry].split()}
    good.update(p=ctypes.addressof(p), B=2, T=3)
    good.update(changes)
    lib = _lib.load()
    rc = getattr(lib, entry)(*[good[n] for n in ENTRIES[entry].split()], None)
    return rc, lib.uds_last_error().decode()


@pytest.mark.parametrize('entry,case', ALL_BAD, ids=['%s-%s' % (e, c[2].split(' (')[0][:40].replace(' ', '_')) + '-%d' % i for i, (e, c) in enumerate(ALL_BAD)])
def test_bad_argument_is_refused_with_its_message(entry, case):
    changes, fields, text = case
    rc, msg = _call(entry, changes, fields)
    assert rc == EINVAL and msg.startswith(entry + ': ' + text), (rc, msg)


def test_workspace_size():
    lib = _lib.load()
    assert lib.uds_predict_tail_workspace_floats(5, 4, 2, 3) == 3 * 32 + 24      # 3 x (B T N rounded to 4 floats) + B T E
    assert lib.uds_predict_tail_workspace_floats(-1, 4, 2, 3) == 0


def test_struct_layout_matches_the_header():
    """uds_tail_t: 13 int32 + 2 floats, padded to 8, then 33 pointers."""
    assert ctypes.sizeof(_lib.TailParams) == 64 + 33 * 8
    assert _lib.TailParams.is_outfall.offset == 64 and _lib.TailParams.ao_idx.offset == 64 + 32 * 8
