"""GRU / LSTM entries (uds_recurrent_forward[_train], uds_recurrent_fused, uds_recurrent_backward[_h]): the route mirror, the case
tables, the fp64 references and a CPU model of the split-bf16 arithmetic, shared by tests/test_recurrent_route_math.py (CPU: every
case reaches the route it claims, the references are what they stand for, the bounds hold for the reference alone, wrong variants
cannot pass) and tests/test_gpu_recurrent_routes.py (GPU parity at every route).  No device is touched here.

The route mirror restates the host-side `if`s in plain Python; each function cites what it restates.  route(case) names what a
case runs:
  ('lds', G, rows, threads)          k_recurrent<G>: U in LDS, `rows` series per workgroup, blockDim = rows * H
  ('stream', G, groups, threads)     k_recurrent_stream<G>: U streamed, `groups` row groups of 8 series, blockDim = groups * H
  ('mfma', G, KTX)                   k_recurrent_mfma<G, KTX>, KTX = F / 32 k-steps of input rows, 0 = given projection
  ('bwd64', G)                       k_recurrent_bwd<G> (uds_recurrent_backward)
  ('bwd_h', G, H, in_lds)            k_recurrent_bwd_h<G, H> (uds_recurrent_backward_h), the packed image staged in LDS or read in place
"""
import zlib

import numpy as np
import torch

from tests.util import f32_exact

GATES = {'GRU': 3, 'LSTM': 4}
LDS_BYTES = 160 * 1024
RC_STREAM_RPT = 8                            # kernels_dense.hpp: rows per thread of k_recurrent_stream
TRAIN_WIDTHS = (16, 32, 48, 64, 80, 96, 112, 128)      # _lib.RECURRENT_TRAIN_WIDTHS (held to it by the CPU tests)

TOL_FP32 = 5e-6                              # tests/test_gpu_parity.py: TOL
TOL_BF16X3 = 2e-5                            # tests/test_gpu_emulator.py: TOL_FWD['bf16x3']
TOL_GRAD = 1e-3                              # tests/test_gpu_recurrent_widths.py: of the largest reference gradient of the tensor
BWD_MARGIN = 3.0                             # backward: allowed = BWD_MARGIN x the split-bf16 model's own error against fp64


# ---------------------------------------------------------------------------------------------------------------------------
# route mirror
# ---------------------------------------------------------------------------------------------------------------------------
def recurrent_rows(H):
    """uds_recurrent_forward_train (uds_hip.hip): rows = max(1, 256 / H)."""
    return max(1, 256 // H)


def recurrent_lds_bytes(G, H):
    """uds_recurrent_forward_train: U (H x G H floats) plus the states of `rows` series."""
    return (H * G * H + recurrent_rows(H) * H) * 4


def recurrent_stream_groups(H):
    """kernels_dense.hpp: recurrent_stream_groups."""
    return 1 if H >= 256 else 256 // H


def forward_route(kind, H):
    """uds_recurrent_forward_train: k_recurrent where U and the states fit the LDS, k_recurrent_stream above."""
    G = GATES[kind]
    assert 0 < H <= 256, 'the entry refuses this width'
    if recurrent_lds_bytes(G, H) <= LDS_BYTES:
        return ('lds', G, recurrent_rows(H), recurrent_rows(H) * H)
    return ('stream', G, recurrent_stream_groups(H), recurrent_stream_groups(H) * H)


def recurrent_mfma_lds(G, ktx):
    """kernels_recurrent.hpp: recurrent_mfma_lds -- G slices of W (ktx k-steps) and of U (2 k-steps), 4 blocks x hi / lo x 64 lanes."""
    return G * (ktx + 2) * (4 * 2 * 64) * 16


def recurrent_mfma_supported(G, F):
    """kernels_recurrent.hpp: recurrent_mfma_supported."""
    return F in (0, 64, 128) and recurrent_mfma_lds(G, F // 32) <= LDS_BYTES


def fused_route(kind, F):
    """launch_recurrent_mfma (kernels_recurrent.hpp)."""
    G = GATES[kind]
    assert recurrent_mfma_supported(G, F), 'the entry refuses this form'
    return ('mfma', G, F // 32)


def fused_units(B, R):
    """(batch element, 16-row block) units of the three matrix-core kernels; four waves = four units per workgroup."""
    return B * ((R + 15) // 16)


def recurrent_bwd_packed_bytes(G, H):
    """kernels_recurrent_bwd.hpp: recurrent_bwd_packed_bytes, 0 for a width that is not built."""
    if H not in TRAIN_WIDTHS or G not in (3, 4):
        return 0
    return 2 * G * ((H + 31) // 32) * (H // 16) * 2 * 64 * 16


def bwd_route(kind, H):
    """_lib.recurrent_bwd_route and launch_recurrent_bwd_h_t: 64 is the old kernel, the others stage the image where it fits."""
    G = GATES[kind]
    assert H in TRAIN_WIDTHS, 'no backward kernel at this width'
    if H == 64:
        return ('bwd64', G)
    return ('bwd_h', G, H, recurrent_bwd_packed_bytes(G, H) <= LDS_BYTES)


def route(c):
    if c['fam'] == 'exact':
        return forward_route(c['kind'], c['H'])
    if c['fam'] == 'fused':
        return fused_route(c['kind'], c['F'])
    if c['fam'] == 'bwd':
        return bwd_route(c['kind'], c['H'])
    raise ValueError(c['fam'])


# ---------------------------------------------------------------------------------------------------------------------------
# case tables: every case carries the route it claims (tests/test_recurrent_route_math.py holds them to route())
# ---------------------------------------------------------------------------------------------------------------------------
# (route, rows or groups, threads) as read off the launch code, GRU / LSTM: the LDS route ends at 116 / 100 units; 240, 202, 200,
# 232 and 234 threads are no multiple of 64
EXACT_CLAIMS = {
    'GRU': {4: ('lds', 64, 256), 20: ('lds', 12, 240), 64: ('lds', 4, 256), 100: ('lds', 2, 200), 101: ('lds', 2, 202),
            116: ('lds', 2, 232), 117: ('stream', 2, 234), 128: ('stream', 2, 256), 200: ('stream', 1, 200), 256: ('stream', 1, 256)},
    'LSTM': {4: ('lds', 64, 256), 20: ('lds', 12, 240), 64: ('lds', 4, 256), 100: ('lds', 2, 200), 101: ('stream', 2, 202),
             116: ('stream', 2, 232), 117: ('stream', 2, 234), 128: ('stream', 2, 256), 200: ('stream', 1, 200), 256: ('stream', 1, 256)},
}
EXACT_WIDTHS = (4, 20, 64, 100, 101, 116, 117, 128, 200, 256)
FIRST_STREAMED = {'GRU': 117, 'LSTM': 101}


def _ex(kind, B, T, R, H, bias):
    r, n, threads = EXACT_CLAIMS[kind][H]
    return dict(fam='exact', kind=kind, B=B, T=T, R=R, H=H, bias=bias, claims=(r, GATES[kind], n, threads))


def _exact_cases():
    out = []
    for kind in ('GRU', 'LSTM'):
        shapes = [(2, 9, 37, H) for H in EXACT_WIDTHS]
        for H in (20, FIRST_STREAMED[kind]):            # one series, one step; fewer series than a workgroup holds, two steps
            shapes += [(1, 1, 1, H), (3, 2, 5, H)]
        shapes += [(2, 96, 37, 64), (2, 96, 37, 128)]
        out += [_ex(kind, B, T, R, H, bias) for (B, T, R, H) in shapes for bias in (True, False)]
    return out


EXACT_CASES = _exact_cases()

FUSED_FORMS = (('GRU', 0), ('GRU', 64), ('GRU', 128), ('LSTM', 0), ('LSTM', 64))      # <3,0> <3,2> <3,4> <4,0> <4,2>
FUSED_ROWS = ((1, 1), (1, 15), (2, 16), (3, 17), (2, 37), (1, 64))                    # 1, 1, 2, 6, 6, 4 units on 4-wave workgroups


def _fu(kind, F, B, T, R, bias):
    return dict(fam='fused', kind=kind, F=F, B=B, T=T, R=R, H=64, bias=bias, claims=('mfma', GATES[kind], F // 32))


def _fused_cases():
    out = []
    for kind, F in FUSED_FORMS:
        shapes = [(B, T, R) for (B, R) in FUSED_ROWS for T in (1, 2, 3, 9)] + [(3, 96, 17)]
        for bias in ((True, False) if kind == 'GRU' else (False,)):      # b_rec is the TF2 GRU's; NULL for the LSTM
            out += [_fu(kind, F, B, T, R, bias) for (B, T, R) in shapes]
    return out


FUSED_CASES = _fused_cases()

BWD_ROWS = ((1, 1), (3, 17), (2, 32))


def _bw(kind, B, T, R, H, bias):
    claims = ('bwd64', GATES[kind]) if H == 64 else ('bwd_h', GATES[kind], H, H < 64)      # 180 KiB and more from 80 units up
    return dict(fam='bwd', kind=kind, B=B, T=T, R=R, H=H, bias=bias, claims=claims)


def _bwd_cases():
    out = []
    for kind in ('GRU', 'LSTM'):
        for H in TRAIN_WIDTHS:
            for (B, R) in BWD_ROWS:
                for T in (1, 2, 9) + ((64,) if H in (64, 128) else ()):
                    # the GRU carries its recurrent bias as in the layer; the LSTM has none there, the entry takes one: at T = 9
                    out.append(_bw(kind, B, T, R, H, kind == 'GRU' or T == 9))
    return out


BWD_CASES = _bwd_cases()


# saturated gates: one case per forward kernel and kind, at widths that also have a backward kernel (staged image, the 64-unit
# kernel, image read in place).  T = 5, two batch elements, 19 series (a ragged second block)
def _sat(fam, kind, H, claims):
    return dict(fam=fam, kind=kind, F=0, B=2, T=5, R=19, H=H, bias=kind == 'GRU', sat=True, claims=claims)


SAT_CASES = [
    _sat('exact', 'GRU', 48, ('lds', 3, 5, 240)), _sat('exact', 'LSTM', 48, ('lds', 4, 5, 240)),
    _sat('exact', 'GRU', 128, ('stream', 3, 2, 256)), _sat('exact', 'LSTM', 128, ('stream', 4, 2, 256)),
    _sat('fused', 'GRU', 64, ('mfma', 3, 0)), _sat('fused', 'LSTM', 64, ('mfma', 4, 0)),
]
SAT_VALUES = (-100.0, -60.0, 0.0, 60.0, 100.0)
SAT_MODERATE_EVERY = 3                       # series r with r % 3 == 2 keep moderate (uniform +-1) pre-activations
SAT_HU = 4.0                                 # |h U| <= 4: |h| <= 1 and every column of U sums to at most 4 in absolute value

# a GRU of 96 units: 109 KiB of dynamic LDS, above the 64 KiB a kernel gets without raising its limit -- per device
TWO_DEVICE_CASE = dict(fam='exact', kind='GRU', B=2, T=3, R=5, H=96, bias=True, claims=('lds', 3, 2, 192))

ALL_CASES = EXACT_CASES + FUSED_CASES + BWD_CASES + SAT_CASES + [TWO_DEVICE_CASE]


def case_id(c):
    s = '%s-%s-B%dT%dR%d-H%d' % (c['fam'], c['kind'], c['B'], c['T'], c['R'], c['H'])
    if c['fam'] == 'fused':
        s += '-F%d' % c['F']
    return s + ('' if c['bias'] else '-norb') + ('-sat' if c.get('sat') else '')


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: fp64 tensors of fp32 values (the device sees the same numbers)
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(c):
    return np.random.default_rng(zlib.crc32((c.get('data_of') or case_id(c)).encode()))


def _uni(rng, lim, *shape):
    return torch.from_numpy(f32_exact(rng.uniform(-lim, lim, shape)))


def _glorot(rng, fan_in, fan_out):
    return _uni(rng, (6.0 / (fan_in + fan_out)) ** 0.5, fan_in, fan_out)


def _bias(rng, n):
    b = _uni(rng, 0.1, n)
    return torch.where(b == 0, torch.full_like(b, 0.05), b)


def inputs(c):
    """Uniform +-1 inputs, Glorot-uniform kernels, biases uniform in +-0.1 and never zero (as test_recurrent_layer_64 draws them).
      exact / bwd   xp (B,T,R,G H), U (H, G H), rb (G H) or None; bwd also gh (B,T,R,H) uniform in +-1
      fused         x (B,T,R,F) with W (F, G 64) and b_in (G 64), or F = 0: x (B,T,R,G 64) the given projection, W = b_in = None;
                    U (64, G 64), rb (G 64) or None
      saturated     xp / x drawn from SAT_VALUES per element, series r % 3 == 2 uniform in +-1; U uniform in +-SAT_HU / H."""
    rng = _rng(c)
    B, T, R, H, G = c['B'], c['T'], c['R'], c['H'], GATES[c['kind']]
    p = {}
    if c.get('sat'):
        xp = torch.from_numpy(rng.choice(np.array(SAT_VALUES), size=(B, T, R, G * H)))
        keep = torch.arange(R) % SAT_MODERATE_EVERY == SAT_MODERATE_EVERY - 1
        xp[:, :, keep] = _uni(rng, 1.0, B, T, int(keep.sum()), G * H)
        p.update(x=xp, W=None, b_in=None, U=_uni(rng, SAT_HU / H, H, G * H), gh=_uni(rng, 1.0, B, T, R, H))
    elif c['fam'] == 'fused':
        F = c['F']
        # F = 128: with +-1 inputs the split-bf16 model alone reaches 0.39 of TOL_BF16X3, past the third it is allowed (0.29 at F = 64, 0.17
        # at F = 128 with +-0.5); the inputs shrink, the bound stays
        p['x'] = _uni(rng, 0.5 if F == 128 else 1.0, B, T, R, F if F else G * H)
        p['W'] = _glorot(rng, F, G * H) if F else None
        p['b_in'] = _bias(rng, G * H) if F else None
        p['U'] = _glorot(rng, H, G * H)
    else:
        p['x'] = _uni(rng, 1.0, B, T, R, G * H)
        p['U'] = _glorot(rng, H, G * H)
        if c['fam'] == 'bwd':
            p['gh'] = _uni(rng, 1.0, B, T, R, H)
    p['rb'] = _bias(rng, G * H) if c['bias'] else None
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# the recurrence, any dtype: the fp64 reference, the plain fp32 evaluation, and the wrong variants the tests must catch
# ---------------------------------------------------------------------------------------------------------------------------
WRONG = ('swap_zr', 'reset_before', 'no_rb', 'state_t2', 'no_cell_carry')


def recurrence(kind, xp, U, rb=None, eps=None, wrong=None):
    """(h, c) over xp (B, T, R, G H), zero initial state; c is None for the GRU.  TF 2.10 / Keras conventions as
    oracle.emulator_ref.gru_sequence / lstm_sequence (GRU reset_after=True, gates z, r, h; LSTM gates i, f, c, o); the LSTM part is
    the cell-state loop of tests/test_gpu_recurrent_widths.py::test_inference_at_128_units.  rb is added to the recurrent product
    of every gate.  eps (B, T, R, G H): added to the recurrent pre-activation h[t-1] U + rb -- its gradient is `darec`.
    wrong: one of WRONG, the mistakes of tests/test_recurrent_route_math.py."""
    B, T, R, GH = xp.shape
    H = U.shape[0]
    assert wrong is None or wrong in WRONG
    b = torch.zeros(GH, dtype=xp.dtype) if rb is None or wrong == 'no_rb' else rb
    h = c = before = torch.zeros(B, R, H, dtype=xp.dtype)
    gate = lambda v, g: v[..., g * H:(g + 1) * H]
    hs, cs = [], []
    for t in range(T):
        src = before if wrong == 'state_t2' else h
        a = src @ U + b
        if eps is not None:
            a = a + eps[:, t]
        x = xp[:, t]
        if kind == 'GRU':
            gz, gr = (1, 0) if wrong == 'swap_zr' else (0, 1)
            z, r = torch.sigmoid(gate(x, gz) + gate(a, gz)), torch.sigmoid(gate(x, gr) + gate(a, gr))
            if wrong == 'reset_before':                # reset_after=False: the reset gate applied to the state, before the product
                cand = torch.tanh(gate(x, 2) + (r * src) @ gate(U, 2) + gate(b, 2))
            else:
                cand = torch.tanh(gate(x, 2) + r * gate(a, 2))
            new = z * h + (1 - z) * cand
        else:
            s = x + a
            kept = torch.zeros_like(c) if wrong == 'no_cell_carry' else c
            c = torch.sigmoid(gate(s, 1)) * kept + torch.sigmoid(gate(s, 0)) * torch.tanh(gate(s, 2))
            new = torch.sigmoid(gate(s, 3)) * torch.tanh(c)
            cs.append(c)
        before, h = h, new
        hs.append(h)
    return torch.stack(hs, dim=1), (torch.stack(cs, dim=1) if kind == 'LSTM' else None)


def last_row_of_block_repeats(out):
    """The wrong variant of a 16-row block: its last live row (r % 16 == 15, or the last series) stores its neighbour's values."""
    R = out.shape[2]
    bad = out.clone()
    for r in range(1, R):
        if r % 16 == 15 or r == R - 1:
            bad[:, :, r] = out[:, :, r - 1]
    return bad


def projection(c, p):
    """(xp, rb) the recurrence of a forward case runs on, in fp64.  uds_recurrent_fused at F = 0 takes the projection with the
    recurrent bias of the z and r gates folded in by the caller (include/uds_hip.h): there only the candidate gate's part of rb
    counts."""
    if c['fam'] == 'fused' and c['F']:
        return p['x'] @ p['W'] + p['b_in'], p['rb']
    rb = p['rb']
    if c['fam'] == 'fused' and rb is not None:
        rb = rb.clone()
        rb[:2 * c['H']] = 0
    return p['x'], rb


def forward_ref(c, p, wrong=None, dtype=torch.float64):
    """(h, c) of a forward case: fp64 reference, or its plain evaluation in `dtype`, or a wrong variant."""
    xp, rb = projection(c, p)
    return recurrence(c['kind'], xp.to(dtype), p['U'].to(dtype), None if rb is None else rb.to(dtype), wrong=wrong)


def backward_ref(c, p, wrong=None):
    """(dxp (B,T,R,G H), darec (G,B,T,R,H)) of sum(h * gh) in fp64: autograd over the recurrence on xp, darec on an explicit
    recurrent pre-activation leaf."""
    G, H = GATES[c['kind']], c['H']
    xp = p['x'].clone().requires_grad_(True)
    eps = torch.zeros_like(xp).requires_grad_(True)
    h, _ = recurrence(c['kind'], xp, p['U'], p['rb'], eps=eps, wrong=wrong)
    (h * p['gh']).sum().backward()
    B, T, R, _ = xp.shape
    return xp.grad, eps.grad.reshape(B, T, R, G, H).permute(3, 0, 1, 2, 4).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU model of the split-bf16 arithmetic (k_recurrent_mfma, k_recurrent_bwd[_h]): operands as bf16 hi + lo, three products, fp32
# accumulation, the state re-split every step, gates in exact fp32.  A model of the arithmetic, not of the kernels' indexing.
# ---------------------------------------------------------------------------------------------------------------------------
def split(v):
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def mm3(a, w):
    """a @ w as the kernels form it: hi * hi + lo * hi + hi * lo of the bf16 splits, summed in fp32."""
    ah, al = split(a)
    wh, wl = split(w)
    return ah @ wl + al @ wh + ah @ wh


def model_forward(c, p):
    """h (B,T,R,64) of a one-launch forward case in fp32."""
    kind, H, G = c['kind'], c['H'], GATES[c['kind']]
    f = lambda t: None if t is None else t.float()
    x, W, b_in, U, rb = f(p['x']), f(p['W']), f(p['b_in']), f(p['U']), f(p['rb'])
    B, T, R, _ = x.shape
    gate = lambda v, g: v[..., g * H:(g + 1) * H]
    if W is None:
        pre = x
    else:
        bi = b_in.clone()
        if kind == 'GRU' and rb is not None:
            bi[:2 * H] += rb[:2 * H]
        pre = bi + mm3(x, W)
    br = gate(rb, 2) if kind == 'GRU' and rb is not None else torch.zeros(H)
    h = cst = torch.zeros(B, R, H)
    out = []
    for t in range(T):
        hu = mm3(h, U)
        if kind == 'GRU':
            z, r = torch.sigmoid(gate(pre[:, t], 0) + gate(hu, 0)), torch.sigmoid(gate(pre[:, t], 1) + gate(hu, 1))
            cand = torch.tanh(gate(pre[:, t], 2) + r * (br + gate(hu, 2)))
            h = z * h + (1 - z) * cand
        else:
            s = pre[:, t] + hu
            cst = torch.sigmoid(gate(s, 1)) * cst + torch.sigmoid(gate(s, 0)) * torch.tanh(gate(s, 2))
            h = torch.sigmoid(gate(s, 3)) * torch.tanh(cst)
        out.append(h)
    return torch.stack(out, dim=1)


def model_backward(c, p, h, cs):
    """(dxp, darec) in fp32 from the saved fp32 forward states h, cs (B,T,R,H): the recurrent pre-activation recomputed from
    h[t-1] and dh[t-1] = direct path + d_arec U^T, both as split-bf16 products; the gate derivatives as the kernels write them."""
    kind, H, G = c['kind'], c['H'], GATES[c['kind']]
    xp, U, gh = p['x'].float(), p['U'].float(), p['gh'].float()
    rb = torch.zeros(G * H) if p['rb'] is None else p['rb'].float()
    B, T, R, _ = xp.shape
    gate = lambda v, g: v[..., g * H:(g + 1) * H]
    zero = torch.zeros(B, R, H)
    dh, dc = zero, zero
    dxp, darec = torch.zeros(B, T, R, G * H), torch.zeros(G, B, T, R, H)
    Ut = U.t().contiguous()
    for t in range(T - 1, -1, -1):
        hp = h[:, t - 1] if t else zero
        ar = rb + mm3(hp, U)
        x = xp[:, t]
        dht = gh[:, t] + dh
        if kind == 'GRU':
            z, r = torch.sigmoid(gate(x, 0) + gate(ar, 0)), torch.sigmoid(gate(x, 1) + gate(ar, 1))
            ah = gate(ar, 2)
            cand = torch.tanh(gate(x, 2) + r * ah)
            dcand = dht * (1 - z) * (1 - cand * cand)
            dz = dht * (hp - cand) * z * (1 - z)
            dr = dcand * ah * r * (1 - r)
            dx, da, direct = [dz, dr, dcand], [dz, dr, dcand * r], dht * z
        else:
            cp = cs[:, t - 1] if t else zero
            s = x + ar
            ig, fg, gg, og = torch.sigmoid(gate(s, 0)), torch.sigmoid(gate(s, 1)), torch.tanh(gate(s, 2)), torch.sigmoid(gate(s, 3))
            tc = torch.tanh(fg * cp + ig * gg)
            dct = dc + dht * og * (1 - tc * tc)
            dx = [dct * gg * ig * (1 - ig), dct * cp * fg * (1 - fg), dct * ig * (1 - gg * gg), dht * tc * og * (1 - og)]
            da, direct, dc = dx, zero, dct * fg
        dxp[:, t] = torch.cat(dx, dim=-1)
        for g in range(G):
            darec[g, :, t] = da[g]
        dh = direct + mm3(torch.cat(da, dim=-1), Ut)
    return dxp, darec


def backward_bounds(c, p):
    """Reference and absolute bound of a backward case: (dxp_ref, darec_ref, allowed_dxp, allowed_darec, model errors), allowed =
    BWD_MARGIN x max|model - fp64 reference| of that tensor.  The model runs on the fp32 evaluation of the forward pass, as the
    kernel runs on the device's exact-fp32 forward."""
    h32, c32 = recurrence(c['kind'], p['x'].float(), p['U'].float(), None if p['rb'] is None else p['rb'].float())
    m_dxp, m_darec = model_backward(c, p, h32, c32)
    dxp, darec = backward_ref(c, p)
    e_dxp, e_darec = float((m_dxp.double() - dxp).abs().max()), float((m_darec.double() - darec).abs().max())
    return dxp, darec, BWD_MARGIN * e_dxp, BWD_MARGIN * e_darec, (e_dxp, e_darec)


def sat_bwd_case(c):
    """The backward case on a saturated forward case's inputs (its widths all have a backward kernel)."""
    H, G = c['H'], GATES[c['kind']]
    return dict(c, fam='bwd', data_of=case_id(c), claims=('bwd64', G) if H == 64 else ('bwd_h', G, H, H < 64))


def sat_gru_masks(c, p):
    """Elements (B,T,R,H) of a saturated GRU case whose output is known exactly in fp32 as in fp64:
      carry   the update gate's input is >= 60 (|h U + rb| <= 4.1 cannot undo it): z = 1, h[t] = h[t-1] bit for bit (zero at t = 0)
      fresh   the update gate's input is <= -60 and the candidate's is beyond +-60: z < 1e-24, h[t] = +-1 exactly
    and the sign of the candidate."""
    assert c.get('sat') and c['kind'] == 'GRU'
    H = c['H']
    xz, xh = p['x'][..., :H], p['x'][..., 2 * H:]
    return xz >= 60, (xz <= -60) & (xh.abs() >= 60), torch.sign(xh)


def bound(ref, tol):
    return tol * max(1.0, float(ref.abs().max()))
