"""The one-launch remainder of a trained NodeEdge on the shipped networks (gnn_uds_amd/csrc/kernels_remainder_snapshot.hpp:
uds_remainder_snapshot_plan, uds_remainder_snapshot, uds_remainder_snapshot_pair): the Python restatement of the plan, the case
table and the cached inputs / fp64 references shared by tests/test_snapshot_remainder_math.py (CPU) and
tests/test_gpu_snapshot_remainder.py (GPU).  Inputs and references are those of tests/remainder_util.py (dense_inputs,
dense_act_ref, gemm_ref).

plan(R, M, F, h) restates uds::snapshot_plan.  A workgroup keeps the bf16 hi / lo image of x_e for NG groups of 64 columns
(a column = one feature of one snapshot, G = 64 NG / h snapshots) in LDS, rows of Kp + 8 bf16, Kp = M rounded up to 64:
  bytes per group   2 planes x 64 x (Kp + 8) x 2 B = 256 (Kp + 8)
  NG                min(4, 80 KiB // bytes per group), at least 1: two workgroups per CU while the image allows it
  refused (G = 0)   one group above 160 KiB, i.e. M > 576; F not 64 / 128; h not 32 / 64; R or M not in 1 .. 2^20
  row blocks        2 blocks of 16 rows of `rest` per wave pass when ceil(ceil(R / 16) / 2) NG >= 8 (a pass for each wave), else 1
With Kp a multiple of 64, NG is 4 (Kp = 64), 2 (Kp = 128) or 1 (Kp >= 192): G is 8, 4, 2 at h = 32 and 4, 2, 1 at h = 64.
"""
from tests import remainder_util as RU
from tests.remainder_util import pad_k

LDS_MAX = 160 * 1024
LDS_TWO = 80 * 1024
MAX_GROUPS = 4
WAVES = 8
PAD = 8
MAX_ROWS = 1 << 20
REFUSED = dict(G=0, lds=0, row_blocks=0)
SHIPPED = {'astlingen': (30, 29), 'shunqing': (113, 131), 'chaohu': (140, 141), 'hague': (210, 210), 'RedChicoSur': (443, 444)}


def group_bytes(M):
    return 2 * 64 * (pad_k(M) + PAD) * 2


def plan(R, M, F, h):
    if not (0 < R <= MAX_ROWS and 0 < M <= MAX_ROWS and F in (64, 128) and h in (32, 64)):
        return dict(REFUSED)
    per = group_bytes(M)
    if per > LDS_MAX:
        return dict(REFUSED)
    ng = max(1, min(MAX_GROUPS, LDS_TWO // per))
    nrb = (R + 15) // 16
    return dict(G=ng * 64 // h, lds=ng * per, row_blocks=2 if ((nrb + 1) // 2) * ng >= WAVES else 1)


def largest_m(F, h):
    """The largest M the restated plan accepts at R = 1 (the plan's answer does not depend on R beyond its range)."""
    lo, hi = 1, MAX_ROWS + 1          # accepted at lo, refused at hi; acceptance is monotone in M
    assert plan(1, lo, F, h)['G'] and not plan(1, hi, F, h)['G']
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(1, mid, F, h)['G'] else (lo, mid)
    return lo


# ---- cases: claims = (G, row blocks per wave pass) -------------------------------------------------------------------------------
def _case(R, M, S, F, h, act, bias, claims, lead=None):
    return dict(R=R, M=M, S=S, F=F, h=h, act=act, bias=bias, claims=claims, lead=lead)


CASES = [
    # the smallest shipped network, both sides: one partly filled workgroup (S < G)
    _case(30, 29, 5, 64, 32, 'relu', True, (8, 1)),
    _case(29, 30, 3, 128, 64, 'tanh', True, (4, 1)),
    _case(1, 1, 1, 64, 32, 'linear', False, (8, 1)),
    # M = 63, 64, 65 at R = 40: one k-step of 64, exactly, and one row into the second (3 row blocks: at Kp = 64 two per pass, the
    # last pass half empty)
    _case(40, 63, 3, 64, 32, 'sigmoid', True, (8, 2)),
    _case(40, 64, 3, 128, 64, 'relu', True, (4, 2)),
    _case(40, 65, 3, 64, 64, 'hard_sigmoid', True, (2, 1)),
    # R = 31, 32, 33 at M = 70: the last row block one short, full, and a third block of one row
    _case(31, 70, 2, 128, 32, 'linear', True, (4, 1)),
    _case(32, 70, 2, 64, 32, 'relu', True, (4, 1)),
    _case(33, 70, 2, 128, 64, 'tanh', True, (2, 1)),
    _case(113, 131, 7, 64, 64, 'sigmoid', True, (1, 1)),
    # two row blocks per pass with an odd block count: the second block of the last pass lies wholly past R; leading dims (2, 2)
    _case(131, 113, 4, 128, 32, 'hard_sigmoid', False, (4, 2), lead=(2, 2)),
    # the LDS limit of the shipped networks, 28 row blocks
    _case(443, 444, 3, 128, 64, 'relu', True, (1, 2)),
    _case(444, 443, 3, 64, 32, 'relu', True, (2, 2)),
    # a last, partly filled workgroup behind two full ones: S = 2 G + 1
    _case(30, 29, 17, 64, 32, 'relu', True, (8, 1)),
    # S = 600 on the smallest network (75 workgroups of 8 snapshots), and 258 workgroups: more than the 256 CUs
    _case(30, 29, 600, 64, 32, 'relu', True, (8, 1)),
    _case(30, 29, 2060, 64, 32, 'tanh', True, (8, 1)),
]
# the largest M the plan accepts, at every (F, h)
for _F, _h, _act in ((64, 32, 'relu'), (64, 64, 'tanh'), (128, 32, 'sigmoid'), (128, 64, 'linear')):
    CASES.append(_case(20, largest_m(_F, _h), 3, _F, _h, _act, True, (2 if _h == 32 else 1, 1)))

# the pair entry: (side 0, side 1) share F, h, act, S and the bias flag; R, M differ
PAIR_CASES = [(_case(30, 29, 9, 64, 32, 'relu', True, (8, 1)), _case(29, 30, 9, 64, 32, 'relu', True, (8, 1))),
              (_case(113, 131, 3, 128, 64, 'tanh', True, (1, 1)), _case(131, 113, 3, 128, 64, 'tanh', True, (2, 2)))]


def case_id(c):
    return RU.case_id(c)


# ---- inputs and references, computed once per case ---------------------------------------------------------------------------
_DATA = {}


def data(c):
    """(inputs of remainder_util.dense_inputs, fp64 rest @ act(e W + b) of shape (S, R, h)); cached, never modified."""
    key = case_id(c)
    if key not in _DATA:
        p = RU.dense_inputs(c)
        _DATA[key] = (p, RU.gemm_ref(p['rest'], RU.dense_act_ref(c, p)))
    return _DATA[key]
