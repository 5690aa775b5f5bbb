"""Shared by tests/test_mpc_solver_math.py (CPU), tests/test_gpu_mpc_objective.py, tests/test_gpu_ce_kernels.py and
tests/test_gpu_mpc_problem.py: fp64 NumPy restatements of the definitions in include/uds_hip.h -- the MPC objective with its
reverse mode (uds_mpc_objective / _backward), the cross-entropy draw (uds_ce_draw, from oracle.dropout_ref.philox4x32_10) and
the cross-entropy update (uds_ce_update: ranking in Python loops) -- and seeded inputs whose values are fp32 numbers."""
import numpy as np

from oracle.dropout_ref import philox4x32_10

U24 = 2.0 ** -24


def f32_exact(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def dense_weights(N, idx, w):
    """Index / weight lists -> the dense (N,) vector (duplicates sum); None for an absent or empty list."""
    if idx is None or len(idx) == 0:
        return None
    out = np.zeros(N)
    np.add.at(out, np.asarray(idx, dtype=np.int64), np.asarray(w, dtype=np.float64))
    return out


def objective_ref(preds, q_in0, w_flood=None, w_out=None, w_smooth=None, gamma=None):
    """(obj (pop,), sum of |term| (pop,)) by the definition; preds (pop, T, N, C), q_in0 (N,) or (pop, N), fp64."""
    preds = np.asarray(preds, dtype=np.float64)
    pop, T, N, C = preds.shape
    q_w, q_in = preds[..., C - 1], preds[..., 1]
    prev = np.concatenate([np.broadcast_to(np.asarray(q_in0, dtype=np.float64), (pop, N))[:, None], q_in[:, :-1]], axis=1)
    gam = np.ones(T) if gamma is None else np.asarray(gamma, dtype=np.float64)
    obj, mag = np.zeros(pop), np.zeros(pop)
    for w, v in ((w_flood, q_w), (w_out, q_in), (w_smooth, np.abs(q_in - prev))):
        if w is not None:
            term = gam[None, :, None] * np.asarray(w, dtype=np.float64)[None, None, :] * v
            obj += term.sum(axis=(1, 2))
            mag += np.abs(term).sum(axis=(1, 2))
    return obj, mag


def objective_grad_ref(preds, q_in0, g, w_flood=None, w_out=None, w_smooth=None, gamma=None):
    """(d_preds of sum_p g[p] obj[p], the sum of |contribution| per element, both (pop, T, N, C)); sign(0) = 0."""
    preds = np.asarray(preds, dtype=np.float64)
    pop, T, N, C = preds.shape
    q_in = preds[..., 1]
    prev = np.concatenate([np.broadcast_to(np.asarray(q_in0, dtype=np.float64), (pop, N))[:, None], q_in[:, :-1]], axis=1)
    gam = np.ones(T) if gamma is None else np.asarray(gamma, dtype=np.float64)
    gg = np.asarray(g, dtype=np.float64)[:, None, None] * gam[None, :, None]              # (pop, T, 1)
    d, mag = np.zeros(preds.shape), np.zeros(preds.shape)

    def add(c, contrib):
        d[..., c] += contrib
        mag[..., c] += np.abs(contrib)
    if w_flood is not None:
        add(C - 1, gg * np.asarray(w_flood)[None, None, :])
    if w_out is not None:
        add(1, gg * np.asarray(w_out)[None, None, :])
    if w_smooth is not None:
        s = gg * np.asarray(w_smooth)[None, None, :] * np.sign(q_in - prev)               # the term of step t, through q_in[t]
        add(1, s)
        back = np.zeros_like(s)
        back[:, :-1] = -s[:, 1:]                                                          # ... and of step t + 1, through q_in[t]
        add(1, back)
    return d, mag


# ---- cross-entropy draw ------------------------------------------------------------------------------------------------------
def ce_normals(seed, j0, pop, n_var):
    """z (pop, n_var) fp64 of candidates j0 .. j0 + pop - 1: Philox counter (j, v), key = seed; u = ((word >> 8) + 0.5) 2^-24 with
    the sum rounded to fp32 as the kernel forms it (exact below 2^23, to even above), then Box-Muller in fp64."""
    j = np.arange(j0, j0 + pop, dtype=np.uint64)[:, None] + np.zeros((1, n_var), dtype=np.uint64)
    v = np.arange(n_var, dtype=np.uint64)[None, :] + np.zeros((pop, 1), dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    counter = np.stack([j & m32, j >> np.uint64(32), v & m32, v >> np.uint64(32)], axis=-1)
    words = philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = lambda w: ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) * U24
    u1, u2 = u(words[..., 0]), u(words[..., 1])
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def ce_draw_ref(mean, std, seed, j0, pop):
    """(the candidates (pop, n_var) fp64, their values before the clip)."""
    raw = np.asarray(mean, dtype=np.float64)[None, :] + np.asarray(std, dtype=np.float64)[None, :] * ce_normals(seed, j0, pop, len(mean))
    return np.clip(raw, 0.0, 1.0), raw


# ---- cross-entropy update ----------------------------------------------------------------------------------------------------
def ce_ranks(obj):
    """rank(p) = #{q: key(q) < key(p) or (key(q) == key(p) and q < p)}, key = obj with every non-finite value +inf."""
    key = [float(o) if np.isfinite(o) else float('inf') for o in obj]
    return [sum(1 for q in range(len(key)) if key[q] < key[p] or (key[q] == key[p] and q < p)) for p in range(len(key))]


def ce_elites(obj, n_elite):
    """Elite candidates in rank order."""
    ranks = ce_ranks(obj)
    order = sorted(range(len(obj)), key=lambda p: ranks[p])
    return [p for p in order if ranks[p] < n_elite and np.isfinite(obj[p])]


def ce_update_ref(y, obj, n_elite, smooth, std_min, mean, std, best_y, best_obj):
    """dict(mean, std, best_y, best_obj, status, elites) after one update, fp64; smooth / std_min enter as the fp32 numbers the
    kernel is handed."""
    y, mean, std = np.asarray(y, dtype=np.float64), np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    smooth, std_min = float(np.float32(smooth)), float(np.float32(std_min))
    el = ce_elites(obj, n_elite)
    out = dict(mean=mean.copy(), std=std.copy(), best_y=np.asarray(best_y, dtype=np.float64).copy(), best_obj=float(best_obj), status=0, elites=el)
    if not el:
        out['status'] = 1
        return out
    m = y[el].mean(axis=0)
    s = np.sqrt(((y[el] - m) ** 2).mean(axis=0))
    out['mean'] = smooth * mean + (1.0 - smooth) * m
    out['std'] = np.maximum(smooth * std + (1.0 - smooth) * s, std_min)
    if float(obj[el[0]]) < out['best_obj']:
        out['best_obj'], out['best_y'] = float(obj[el[0]]), y[el[0]].copy()
    return out


# Error bounds of uds_ce_update against ce_update_ref, for candidates in [0, 1], mean / std in [0, 1], u = 2^-24 per fp32 rounding
# (csrc/kernels_mpc.hpp: the sums are balanced trees of 10 levels whatever K is):
#   m:   10 u sum|x| / K from the tree, u from the division                                         |m' - m| <= 11 u
#   new mean = keep * mean + take * m', take = fl(1 - smooth): u each for take, the two products and the sum  -> 11 u + 4 u = 15 u
#   s:   d = fl(x - m') differs from x - m by delta = m' - m in every leaf, which moves sum d^2 / K by delta^2 only (sum d = 0):
#        below 5e-13, under 0.1 u of the variance once s >= 0.01; rounding d: u, squaring: 2 u + u, tree: 10 u, division: u
#        -> 14.1 u of the variance, so (7.05 + 1) u of s after the root, s <= 0.5                    |s' - s| <= 4.1 u
#   new std = max(keep * std + take * s', std_min): 4 u as above                                     -> 8.1 u, stated as 10 u
#   s < 0.01: the variance is off by at most 14.1 u s^2 + delta^2, and |sqrt(a) - sqrt(b)| <= sqrt(|a - b|), so
#        |s' - s| <= sqrt(14.1 u) s + |delta| <= 9.2e-4 * 0.01 + 6.6e-7 = 9.9e-6; with the 4 u of the smoothing: 1.02e-5 -- the
#        interface's limit of 1e-5 is what is asserted there (it is what a caller may rely on)
CE_MEAN_BOUND = 15 * U24       # 8.9e-7
CE_STD_BOUND = 10 * U24        # 6.0e-7, for a reference s >= 0.01


def ce_std_bound(y, elites):
    """Per variable: CE_STD_BOUND where the elites' reference standard deviation is at least 0.01, else 1e-5."""
    y = np.asarray(y, dtype=np.float64)[list(elites)]
    s = np.sqrt(((y - y.mean(axis=0)) ** 2).mean(axis=0))
    return np.where(s >= 0.01, CE_STD_BOUND, 1e-5)
