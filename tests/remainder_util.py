"""The dense remainder GEMM of a trained NodeEdge (gnn_uds_amd/csrc/kernels_gemm.hpp: uds_remainder_pack, uds_remainder_forward,
uds_remainder_forward_dense): the Python restatement of the host routing, the case tables, the seeded inputs and the fp64
references shared by tests/test_remainder_route_math.py (CPU: the restatement agrees with the library, every case reaches the
route it claims, every route is reached, the references carry signal) and tests/test_gpu_remainder_routes.py (GPU parity in
guarded memory).

plan(R, M, S, h) restates remainder_plan (gnn_uds_amd/csrc/uds_hip.hip) for the product (R x Kp) x (Kp x Nc), Nc = S h, Kp = M
rounded up to 64:
  ('v1', tiles)                         k_remainder_gemm, 128 x 128 tiles: Nc < 256 or R < 128 (or an operand image of 4 GiB)
  ('v2', t_main, t_rest, ks, pieces)    k_remainder_gemm2<2>, 256 x 256 tiles: t_main tiles computed whole (ks = 1: all of them),
                                        t_rest tiles -- those past the last whole round of 256 -- cut along K into ks pieces of
                                        `pieces` k-steps of 32 each, added by k_remainder_gemm2_reduce.  ks is the k <= min(512 /
                                        t_rest, 8, Kp / 256) with the smallest ceil(t_rest k / 256) / k + 0.01 k.
A piece starts at the absolute k-step sum(pieces[:p]); the kernel picks its LDS buffer by the parity of that step.
"""
import torch

MAX_PIECES = 512          # REMAINDER_MAX_PIECES
PIECE_BYTES = 256 * 256 * 4
ACTS = ('linear', 'relu', 'tanh', 'sigmoid', 'hard_sigmoid')

# Bounds of tests/test_gpu_remainder_routes.py, relative to max(1, max|ref|) through tests.util.close, always against an fp64
# reference; its docstring (MEASURED) holds the figures they are set from.  The project's bound for the split-bf16 GEMM is
# TOL_BF16X3 = 1e-5 and none of these exceeds it; on signed inputs the arithmetic alone (emulate) takes 0.58 of it, so the three
# bounds against the fp64 product stay AT 1e-5 and the kernel's own share is bounded separately, against emulate.
TOL_GEMM = 1e-5           # uds_remainder_forward against the fp64 product: worst 5.79e-6 (0.579), the CPU model's 0.579
TOL_MODEL = 3e-6          # uds_remainder_forward against emulate(): the kernel's fp32 accumulation alone, 4.8 x the worst 6.2e-7
TOL_PLANES = 8e-5         # hi + lo of the planes k_dense_split_planes writes against act(e W + b): a split-bf16 Dense over F terms,
                          # 3.5 x the worst 2.27e-5 (the project's TOL_ROWGEMM for that Dense is 1e-4)
TOL_DENSE = 1e-5          # uds_remainder_forward_dense against rest @ act(e W + b): worst 6.9e-6 (0.693)
TOL_DXS = 1e-5            # RemainderFn, d xs: the same GEMM on rest^T: worst 5.3e-6 (0.525)
TOL_DREST = 3e-6          # RemainderFn, d rest: a library fp32 GEMM over S h terms, 4.4 x the worst 6.8e-7


def pad_k(k):
    return (k + 63) // 64 * 64


def plan(R, M, S, h):
    Nc, Kp = S * h, pad_k(M)
    if not (Nc * Kp * 2 < 1 << 32 and R * Kp * 2 < 1 << 32 and Nc >= 256 and R >= 128):
        return ('v1', ((Nc + 127) // 128) * ((R + 127) // 128))
    n_ctile = (Nc + 255) // 256
    tiles = n_ctile * ((R + 255) // 256)
    t_main = tiles // 256 * 256
    t_rest = tiles - t_main
    ks = 1
    if t_rest:
        best = 1e300
        for k in range(1, min(MAX_PIECES // t_rest, 8, Kp // 32 // 8) + 1):
            cost = ((t_rest * k + 255) // 256) / k + 0.01 * k
            if cost < best - 1e-9:
                best, ks = cost, k
    if ks == 1:
        t_main, t_rest = tiles, 0
    n_k_all = Kp // 32
    return ('v2', t_main, t_rest, ks, tuple(n_k_all * (p + 1) // ks - n_k_all * p // ks for p in range(ks)))


def packed_bytes(R, M):
    return 2 * R * pad_k(M) * 2


def workspace_bytes(R, M, S, h):
    q = plan(R, M, S, h)
    return 2 * S * h * pad_k(M) * 2 + (q[2] * q[3] * PIECE_BYTES if q[0] == 'v2' else 0)


def piece_starts(pieces):
    return tuple(sum(pieces[:p]) for p in range(len(pieces)))


def xcd_order(nblk):
    """Workgroup b -> tile, as k_remainder_gemm and both parts of k_remainder_gemm2 order them: workgroups b, b + 8, .. share an XCD
    and get a contiguous run of tiles (the first nblk % 8 XCDs one tile more)."""
    q8, r8 = nblk // 8, nblk % 8
    out = []
    for b in range(nblk):
        xcd = b % 8
        out.append((xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + b // 8)
    return out


def route(c):
    return plan(c['R'], c['M'], c['S'], c['h'])


def dense_route(c):
    """(k_dense_split_planes instantiation KT = F / 32, the GEMM's route)."""
    return (c['F'] // 32,) + route(c)


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _case(R, M, S, h, claims, lead=False):
    return dict(R=R, M=M, S=S, h=h, claims=claims, lead=lead)


def _whole(tiles):
    return ('v2', tiles, 0, 1)      # + the one piece: filled in below


GEMM_CASES = [
    # k_remainder_gemm: one row / one link / one 4-column group; one short of either v2 condition; the 128-tile edges on both
    # sides (Nc is a multiple of 4: 132 is the first width past 128); M = 63, 64, 65 round the k-step; S = 1
    _case(1, 1, 1, 4, ('v1', 1)),
    _case(1, 70, 3, 12, ('v1', 1)),
    _case(5, 1, 2, 20, ('v1', 1)),
    _case(127, 100, 8, 32, ('v1', 2)),
    _case(128, 65, 7, 36, ('v1', 2)),
    _case(128, 64, 4, 32, ('v1', 1)),
    _case(129, 63, 11, 12, ('v1', 4)),
    _case(130, 65, 1, 64, ('v1', 2)),
    _case(300, 129, 3, 64, ('v1', 6), lead=True),
    # more tiles than XCDs, and no multiple of 8: the XCD-aware tile order deals runs of unequal length (xcd_order)
    _case(1300, 70, 7, 36, ('v1', 22)),
    _case(100, 70, 40, 32, ('v1', 10)),
    # k_remainder_gemm2, whole tiles: both conditions met exactly; R = 255, 256, 257; one ragged 4-column group in the second
    # column tile (Nc = 260); two k-steps (Kp = 64); Kp = 448, the longest K that refuses a cut
    _case(128, 100, 8, 32, _whole(1)),
    _case(255, 64, 64, 4, _whole(1)),
    _case(256, 400, 13, 20, _whole(2)),
    _case(257, 200, 8, 36, _whole(4)),
    _case(300, 129, 22, 12, _whole(4), lead=True),
    # k_remainder_gemm2, every tile cut: ks = 2 .. 8
    _case(128, 449, 8, 32, ('v2', 0, 1, 2, (8, 8))),
    _case(129, 705, 64, 4, ('v2', 0, 1, 3, (8, 8, 8))),
    _case(255, 1025, 22, 12, ('v2', 0, 2, 4, (8, 9, 8, 9))),
    _case(257, 1300, 13, 20, ('v2', 0, 4, 5, (8, 8, 9, 8, 9))),
    _case(300, 1537, 15, 36, ('v2', 0, 6, 6, (8, 8, 9, 8, 8, 9))),      # 3 column tiles x 2 row tiles
    _case(130, 1800, 4, 64, ('v2', 0, 1, 7, (8, 8, 8, 9, 8, 8, 9))),
    _case(130, 2000, 8, 32, ('v2', 0, 1, 8, (8,) * 8)),
]
# 272 tiles: one whole round of 256 and 16 tiles cut in two, in the same launch (the only case of this size: 18 GFLOP in fp64)
MIXED_CASE = _case(4096, 512, 68, 64, ('v2', 256, 16, 2, (8, 8)))
GEMM_CASES.append(MIXED_CASE)
for _c in GEMM_CASES:
    if len(_c['claims']) == 4:
        _c['claims'] = _c['claims'] + ((pad_k(_c['M']) // 32,),)


def _dense_case(R, M, S, F, h, act, bias, claims):
    return dict(R=R, M=M, S=S, F=F, h=h, act=act, bias=bias, claims=claims)


DENSE_CASES = [
    # F x h = {64, 128} x {32, 64}; all five activations; one without a bias; M below 64, at 64, not a multiple of 64; each route
    _dense_case(130, 40, 3, 64, 32, 'relu', True, (2, 'v1', 2)),
    _dense_case(70, 64, 2, 64, 64, 'tanh', True, (2, 'v1', 1)),
    _dense_case(200, 130, 8, 128, 32, 'sigmoid', False, (4, 'v2', 1, 0, 1, (6,))),
    _dense_case(129, 449, 4, 128, 64, 'hard_sigmoid', True, (4, 'v2', 0, 1, 2, (8, 8))),
    _dense_case(257, 300, 5, 64, 64, 'linear', True, (2, 'v2', 4, 0, 1, (10,))),
]

# RemainderFn: the forward is plan(R, M, S, h), the backward's GEMM is plan(M, R, S, h) (rest^T packed, g in the place of xs).
# claims = (forward route, backward route) without the piece lengths
FN_CASES = [
    dict(R=70, M=50, S=3, h=12, claims=(('v1', 1), ('v1', 1))),
    dict(R=130, M=100, S=8, h=32, claims=(('v2', 1, 0, 1), ('v1', 2))),
    dict(R=100, M=129, S=13, h=20, claims=(('v1', 3), ('v2', 2, 0, 1))),
    dict(R=257, M=449, S=5, h=64, claims=(('v2', 0, 4, 2), ('v2', 4, 0, 1))),
]


def case_id(c):
    s = 'R%dM%dS%dh%d' % (c['R'], c['M'], c['S'], c['h'])
    if 'F' in c:
        s += '-F%d-%s%s' % (c['F'], c['act'], '' if c['bias'] else '-nobias')
    return s + ('-lead' if c.get('lead') else '')


# ---- inputs and references --------------------------------------------------------------------------------------------------
def _seed(c):
    return 7 * c['R'] + 13 * c['M'] + 1000 * c['S'] + c['h'] + c.get('F', 0)


def gemm_inputs(c):
    """rest (R, M) = 0.05 randn (the scale of the reference's 'random_normal' parameters), x (S, M, h) = randn: signed, fp32."""
    g = torch.Generator().manual_seed(_seed(c))
    return dict(rest=(torch.randn(c['R'], c['M'], generator=g, dtype=torch.float64) * 0.05).float(),
                x=torch.randn(c['S'], c['M'], c['h'], generator=g, dtype=torch.float64).float())


def dense_inputs(c):
    """gemm_inputs with e (S, M, F) = randn in the place of x, W (F, h) = randn / sqrt(F) (pre-activations of unit scale: every
    activation is used over its curved part), b (h,) = 0.1 randn or None."""
    g = torch.Generator().manual_seed(_seed(c))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(rest=(rn(c['R'], c['M']) * 0.05).float(), e=rn(c['S'], c['M'], c['F']).float(),
                W=(rn(c['F'], c['h']) / c['F'] ** 0.5).float(), b=(rn(c['h']) * 0.1).float() if c['bias'] else None)


def gemm_ref(rest, x):
    """(S, R, h) fp64 of the fp32 values the kernel sees."""
    return torch.matmul(rest.double(), x.double())


def dense_act_ref(c, p):
    """act(e W + b), (S, M, h) fp64."""
    from oracle import spektral_dense as OD
    z = p['e'].double() @ p['W'].double()
    return OD.activation(c['act'])(z + p['b'].double() if p['b'] is not None else z)


def split_bf16(v):
    """(hi, lo) as raw int16 bits: hi = bf16(v) rounded to nearest even, lo = bf16(v - hi) -- what k_split_rows_bf16 is to give."""
    v = v.float()
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return hi.view(torch.int16), lo.view(torch.int16)


def planes64(v):
    hi, lo = split_bf16(v)
    return hi.view(torch.bfloat16).double(), lo.view(torch.bfloat16).double()


def rest_planes(rest):
    """The (2, R, Kp) int16 image uds_remainder_pack is to write: hi plane, lo plane, K padded with zero bits."""
    R, M = rest.shape
    out = torch.zeros(2, R, pad_k(M), dtype=torch.int16)
    out[0, :, :M], out[1, :, :M] = split_bf16(rest)
    return out


def x_planes(x):
    """The (2, S h, Kp) int16 image at the front of the workspace: row (s, f) = x[s, :, f], split, K padded with zero bits."""
    S, M, h = x.shape
    out = torch.zeros(2, S * h, pad_k(M), dtype=torch.int16)
    hi, lo = split_bf16(x.permute(0, 2, 1).reshape(S * h, M))
    out[0, :, :M], out[1, :, :M] = hi, lo
    return out


def emulate(rest, x, k_range=None):
    """The split-bf16 product in fp64: hi hi + lo hi + hi lo of the rounded operands (the kernel's arithmetic without its fp32
    accumulation), over links k_range = (k0, k1) when given."""
    if k_range is not None:
        rest, x = rest[:, k_range[0]:k_range[1]], x[:, k_range[0]:k_range[1]]
    rh, rl = planes64(rest)
    xh, xl = planes64(x)
    return torch.matmul(rh + rl, xh + xl) - torch.matmul(rl, xl)


def fn_inputs(c):
    """gemm_inputs and an upstream gradient (S, R, h) = randn."""
    p = gemm_inputs(c)
    g = torch.Generator().manual_seed(_seed(c) + 1)
    p['g'] = torch.randn(c['S'], c['R'], c['h'], generator=g, dtype=torch.float64).float()
    return p


def fn_ref(p):
    """(out, d rest, d xs) by autograd over the fp64 product."""
    rest, xs = p['rest'].double().requires_grad_(), p['x'].double().requires_grad_()
    out = torch.matmul(rest, xs)
    d_rest, d_xs = torch.autograd.grad((out * p['g'].double()).sum(), (rest, xs))
    return out.detach(), d_rest, d_xs
