"""The argument checks of the MPC entries (uds_mpc_objective / _backward, uds_ce_draw, uds_ce_update): every bad argument returns
UDS_EINVAL (-22) with its message before anything is launched -- no device is needed, the operands are aligned host addresses
that are never read.  Sibling by sibling with the same bad argument, as tests/test_entry_checks.py does."""
import numpy as np
import pytest

from gnn_uds_amd import _lib

_BUF = np.zeros(64, dtype=np.float32)
P = _BUF.ctypes.data - _BUF.ctypes.data % 16 + 16       # a 16-byte aligned host address (never read)
Q = P + 4                                               # misaligned by one float

OBJ_ORDER = {'uds_mpc_objective': ('preds', 'q_in0', 'q0_stride', 'pop', 'T', 'N', 'C', 'w_flood', 'w_out', 'w_smooth', 'gamma', 'out'),
             'uds_mpc_objective_backward': ('preds', 'q_in0', 'q0_stride', 'g', 'pop', 'T', 'N', 'C', 'w_flood', 'w_out', 'w_smooth', 'gamma', 'out')}
OBJ_GOOD = dict(preds=P, q_in0=P, q0_stride=0, g=P, pop=3, T=2, N=30, C=5, w_flood=P, w_out=P, w_smooth=P, gamma=P, out=P)


def _call(lib, entry, order, good, **over):
    args = dict(good, **over)
    return getattr(lib, entry)(*[args[k] for k in order], None), lib.uds_last_error().decode()


@pytest.mark.parametrize('entry', sorted(OBJ_ORDER))
def test_objective_entries_refuse_bad_arguments(entry):
    lib = _lib.load()
    call = lambda **over: _call(lib, entry, OBJ_ORDER[entry], OBJ_GOOD, **over)
    for name in ('preds', 'q_in0', 'out') + (('g',) if 'g' in OBJ_ORDER[entry] else ()):
        rc, msg = call(**{name: None})
        assert rc == -22 and msg == '%s: NULL argument' % entry, name
    for C in (1, 9, 0, -1):
        rc, msg = call(C=C)
        assert rc == -22 and '%s: C=%d outside [2, 8]' % (entry, C) in msg
    for T in (0, 4097, -1):
        rc, msg = call(T=T)
        assert rc == -22 and '%s: T=%d outside [1, 4096]' % (entry, T) in msg
    for over in (dict(pop=-1), dict(pop=(1 << 20) + 1), dict(N=0), dict(N=(1 << 24) + 1), dict(pop=1 << 62)):
        rc, msg = call(**over)
        assert rc == -22 and '%s: pop=%d' % (entry, over.get('pop', 3)) in msg and 'N=%d' % over.get('N', 30) in msg, over
    rc, msg = call(pop=1 << 20, T=4096, N=1 << 24)
    assert rc == -22 and 'too large for one launch' in msg
    for stride in (1, 29, 31, -30):
        rc, msg = call(q0_stride=stride)
        assert rc == -22 and '%s: q0_stride=%d' % (entry, stride) in msg
    rc, msg = call(w_flood=None, w_out=None, w_smooth=None)
    assert rc == -22 and msg == '%s: no weight vector given' % entry
    for name in ('preds', 'q_in0', 'w_flood', 'w_out', 'w_smooth', 'gamma', 'out') + (('g',) if 'g' in OBJ_ORDER[entry] else ()):
        rc, msg = call(**{name: Q})
        assert rc == -22 and msg == '%s: every pointer must be 16-byte aligned' % entry, name
    # the checks come before the empty-input return: a bad argument is refused at pop = 0 too, a good call launches nothing
    rc, msg = call(pop=0, C=9)
    assert rc == -22 and 'C=9' in msg
    rc, msg = call(pop=0, preds=None)
    assert rc == -22 and 'NULL argument' in msg
    for over in (dict(), dict(q0_stride=30), dict(gamma=None), dict(w_flood=None), dict(w_out=None, w_smooth=None)):
        rc, _ = call(pop=0, **over)
        assert rc == 0, over


DRAW_ORDER = ('mean', 'std', 'n_var', 'pop', 'seed', 'count', 'out')
DRAW_GOOD = dict(mean=P, std=P, n_var=6, pop=16, seed=1, count=P, out=P)
UPDATE_ORDER = ('y', 'obj', 'pop', 'n_var', 'n_elite', 'smooth', 'std_min', 'mean', 'std', 'best_y', 'best_obj', 'status')
UPDATE_GOOD = dict(y=P, obj=P, pop=16, n_var=6, n_elite=4, smooth=0.3, std_min=1e-3, mean=P, std=P, best_y=P, best_obj=P, status=P)
CE = {'uds_ce_draw': (DRAW_ORDER, DRAW_GOOD, ('mean', 'std', 'count', 'out')),
      'uds_ce_update': (UPDATE_ORDER, UPDATE_GOOD, ('y', 'obj', 'mean', 'std', 'best_y', 'best_obj', 'status'))}


@pytest.mark.parametrize('entry', sorted(CE))
def test_cross_entropy_entries_refuse_bad_arguments(entry):
    lib = _lib.load()
    order, good, pointers = CE[entry]
    call = lambda **over: _call(lib, entry, order, good, **over)
    for name in pointers:
        rc, msg = call(**{name: None})
        assert rc == -22 and msg == '%s: NULL argument' % entry, name
        rc, msg = call(**{name: Q})
        assert rc == -22 and msg == '%s: every pointer must be 16-byte aligned' % entry, name
    for pop in (1, 0, 1025, -1):
        rc, msg = call(pop=pop, n_elite=1)
        assert rc == -22 and msg == '%s: pop=%d outside [2, 1024]' % (entry, pop)
    for n_var in (0, 1025, -1):
        rc, msg = call(n_var=n_var)
        assert rc == -22 and msg == '%s: n_var=%d outside [1, 1024]' % (entry, n_var)


def test_ce_update_refuses_its_own_bad_arguments():
    lib = _lib.load()
    call = lambda **over: _call(lib, 'uds_ce_update', UPDATE_ORDER, UPDATE_GOOD, **over)
    for n_elite in (0, 17, -1):
        rc, msg = call(n_elite=n_elite)
        assert rc == -22 and msg == 'uds_ce_update: n_elite=%d outside [1, pop=16]' % n_elite
    for over in (dict(smooth=-0.1), dict(smooth=1.5), dict(smooth=float('nan')), dict(std_min=-1.0), dict(std_min=float('inf')),
                 dict(std_min=float('nan'))):
        rc, msg = call(**over)
        assert rc == -22 and 'uds_ce_update: smooth=' in msg and 'std_min=' in msg, over
