"""Model-predictive-control evaluation on the engine: what the reference's `mpc_problem_gr`
runs per candidate control sequence (`surrogate/mpc.py:551-612`) -- expand the decision vector to per-step settings,
predict the horizon with the emulator (chunk by chunk when it is longer than `seq_out`), reduce the prediction to the
scalar objective of the scenario (`envs/scenario/astlingen.py:75-99`), and differentiate it with respect to the decision
vector (the reverse mode runs through the HIP backward kernels).  A whole population is ONE batched forward.

SWMM coupling and scenario configuration stay in the reference; the performance targets are passed as index / weight tensors.

`Problem` is the device-resident form of the same evaluation plus two solvers: the history the population shares is encoded
once (`Emulator.predict_tf_shared`), the objective is one HIP operator (`autograd.MpcObjectiveFn`), and `solve_ce` /
`solve_gr` run a cross-entropy loop and a projected Adam without reading a device value inside their loops.  The reference's
`run_ce` / `run_gr` (`mpc.py:384,641`) are recorded in SURVEY.md in outline only: the sampling and update rules here are this
project's own, as `data.py` states for its window draw.  The GA stays in the reference.
"""
from collections import namedtuple

import torch

from . import _lib
from . import autograd as _ag


def expand_settings(y, n_step, n_act, r_step, horizon_steps):
    """Decision vectors (pop, n_step*n_act) -> per-step settings (pop, horizon_steps, n_act): every control step is held for
    r_step simulation steps and the last one to the end of the evaluation horizon (`mpc.py:552-558`)."""
    s = y.reshape(-1, n_step, n_act).repeat_interleave(r_step, dim=1)
    if s.shape[1] < horizon_steps:
        s = torch.cat([s, s[:, -1:].expand(-1, horizon_steps - s.shape[1], -1)], dim=1)
    return s[:, :horizon_steps]


def predict_horizon(emul, settings, state, runoff, edge_state):
    """`mpc_problem_gr.predict` (`mpc.py:565-582`): `predict_tf` on the whole horizon when it is one chunk, else chunk by
    chunk of seq_out steps, each fed with the previous prediction (flood bit = flooding volume > 0, `:572-574`)."""
    so = emul.seq_out
    n_chunk = settings.shape[1] // so
    if n_chunk <= 1:
        return emul.predict_tf(state, runoff, settings, edge_state)
    state, edge_state = state[:, -emul.seq_in:], edge_state[:, -emul.seq_in:]
    ys, es, perf = [], [], None
    for i in range(n_chunk):
        sl = slice(i * so, (i + 1) * so)
        ri, sett = runoff[:, sl], settings[:, sl]
        if emul.if_flood and i > 0:
            state = torch.cat([state[..., :-1], (perf > 0).float(), state[..., -1:]], dim=-1)
        y, ey = emul.predict_tf(state, ri, sett, edge_state)
        state, perf = torch.cat([y[..., :-2], ri], dim=-1), y[..., -1:]
        edge_state = torch.cat([ey, emul.get_edge_action(sett, True)], dim=-1)
        ys.append(y)
        es.append(ey)
    return torch.cat(ys, dim=1), torch.cat(es, dim=1)


def objective_pred(preds, state, flood_idx, flood_w, outflow_idx=None, outflow_w=None, smooth_idx=None, smooth_w=None, gamma=None):
    """`objective_pred_tf` (`envs/scenario/astlingen.py:75-99`) with the scenario's performance targets as tensors:
    flooding volume q_w at `flood_idx` ('cumflooding' targets), inflow at `outflow_idx` ('cuminflow' at the treatment plant),
    absolute inflow change between steps at `smooth_idx` (the `rough` term), each weighted, discounted by gamma (T,), summed
    over time -> (pop,)."""
    q_w = preds[..., -1]                                                   # (pop, T, N)
    q_in = torch.cat([state[:, -1:, :, 1], preds[..., 1]], dim=1)          # (pop, T+1, N)
    obj = (q_w[..., flood_idx] * flood_w).sum(-1)
    if outflow_idx is not None and len(outflow_idx):
        obj = obj + (q_in[:, 1:, outflow_idx] * outflow_w).sum(-1)
    if smooth_idx is not None and len(smooth_idx):
        obj = obj + ((q_in[:, 1:, smooth_idx] - q_in[:, :-1, smooth_idx]).abs() * smooth_w).sum(-1)
    if gamma is not None:
        obj = obj * gamma
    return obj.sum(-1)


def objective_and_gradient(emul, y, state, runoff, edge_state, n_step, n_act, r_step, targets, gamma=None):
    """`gradient_fn` (`mpc.py:600-610`): objective of every candidate in y (pop, n_step*n_act) and its gradient with respect
    to y.  state (T_in, N, C), runoff (T_h, N, b), edge_state (T_in, E, C) are shared by the population (`pre_state`)."""
    y = y.detach().clone().requires_grad_(True)
    pop = y.shape[0]
    settings = expand_settings(y, n_step, n_act, r_step, runoff.shape[0])
    rep = lambda t: t.unsqueeze(0).expand((pop,) + tuple(t.shape)).contiguous()
    st = rep(state)
    preds = predict_horizon(emul, settings, st, rep(runoff), rep(edge_state))
    obj = objective_pred(preds[0], st, gamma=gamma, **targets)
    (grad,) = torch.autograd.grad(obj.sum(), y)
    return obj.detach(), grad


def hessp(emul, y, p, state, runoff, edge_state, n_step, n_act, r_step, targets, gamma=None, eps=None):
    """`hessp_fn` (`mpc.py:616-624`, the Hessian-vector product `trust-constr` asks for in `run_ntopt`): H(y) p for every
    candidate, y and p (pop, n_step*n_act).  The reference nests two GradientTapes; the HIP backward operators are first-order
    (`torch.autograd.Function`s without a double backward), so the product is the central difference of the GRADIENT along p,
        H p ~ (grad f(y + eps p) - grad f(y - eps p)) / (2 eps),    eps = 1e-2 / max|p|  (settings live in [0, 1]),
    two gradient evaluations = two batched forward + backward passes through the same kernels.  The objective is piecewise
    smooth (relu, |.| of the roughness term, hard gates): like the exact second derivative, the difference is meaningful
    away from the kinks only.  With `use_adj` the adjacency flips there too: a setting within eps * |p| of an integer gives
    the two gradients different adjacencies (the cast to int removes an entry below 1), so the quotient spans the jump.
    Returns (pop, n_step*n_act)."""
    p = p.to(y.dtype)
    if eps is None:
        eps = 1e-2 / max(float(p.abs().max()), 1e-12)
    _, g_hi = objective_and_gradient(emul, y + eps * p, state, runoff, edge_state, n_step, n_act, r_step, targets, gamma)
    _, g_lo = objective_and_gradient(emul, y - eps * p, state, runoff, edge_state, n_step, n_act, r_step, targets, gamma)
    return (g_hi - g_lo) / (2.0 * eps)


Result = namedtuple('Result', 'y obj history')
Result.__doc__ = """What a solver of `Problem` returns: y the decision vector(s), obj their objective, history (iters,) the best
objective found up to each iteration -- all on the problem's device."""


class Problem:
    """One MPC decision problem on the engine: the arguments of `objective_and_gradient`, kept on their device, with the target
    lists scattered once into dense per-node weight vectors (`index_add_`: duplicate indices sum).

    shared_history: the population's common history goes through the emulator once (`Emulator.predict_tf_shared`: chunk 0 of the
    horizon; later chunks are fed with each candidate's own prediction and run replicated, as `predict_horizon` runs them).
    conv=False models have no such split and run replicated.  fused_objective: the objective and its gradient are the HIP
    operator `autograd.MpcObjectiveFn`; off, or on CPU tensors, `objective_pred` runs.  `last_paths` records what the last
    evaluation took: {'prefix': 'shared' | 'replicated', 'objective': 'hip' | 'torch'}.

    `solve_ce` and `solve_gr` are this project's own rules (module docstring), not a port of the reference's drivers."""

    def __init__(self, emul, state, runoff, edge_state, n_step, n_act, r_step, targets, gamma=None, shared_history=True, fused_objective=True):
        for name, t in (('state', state), ('runoff', runoff), ('edge_state', edge_state)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3:
                raise ValueError('%s must be an unbatched 3-d tensor (time, rows, channels), shared by the population' % name)
        N, so = state.shape[1], emul.seq_out
        if runoff.shape[1] != N or state.shape[0] != edge_state.shape[0] or state.shape[0] < 1:
            raise ValueError('state %r, runoff %r and edge_state %r do not describe one network and one history' %
                             (tuple(state.shape), tuple(runoff.shape), tuple(edge_state.shape)))
        if runoff.shape[0] < so or runoff.shape[0] % so:
            raise ValueError('the horizon (%d runoff steps) must be a positive multiple of seq_out = %d' % (runoff.shape[0], so))
        for name, v in (('n_step', n_step), ('n_act', n_act), ('r_step', r_step)):
            if int(v) != v or v < 1:
                raise ValueError('%s must be a positive integer, got %r' % (name, v))
        if gamma is not None and tuple(gamma.shape) != (runoff.shape[0],):
            raise ValueError('gamma must be (%d,), got %r' % (runoff.shape[0], tuple(gamma.shape)))
        if targets.get('flood_idx') is None or targets.get('flood_w') is None:
            raise ValueError("targets needs 'flood_idx' and 'flood_w' (the outflow_* and smooth_* lists are optional)")
        self.emul, self.state, self.runoff, self.edge_state = emul, state, runoff, edge_state
        self.n_step, self.n_act, self.r_step, self.n_var = int(n_step), int(n_act), int(r_step), int(n_step) * int(n_act)
        self.gamma, self.shared_history, self.fused_objective = gamma, bool(shared_history), bool(fused_objective)
        self.targets = {k: v for k, v in targets.items() if v is not None}
        self.weights = {}                     # 'flood' | 'outflow' | 'smooth' -> dense (N,) weights, None where the list is absent
        for key in ('flood', 'outflow', 'smooth'):
            idx, w = targets.get(key + '_idx'), targets.get(key + '_w')
            if (idx is None) != (w is None) or (idx is not None and (idx.dim() != 1 or tuple(w.shape) != tuple(idx.shape))):
                raise ValueError('%s_idx and %s_w must be one-dimensional tensors of one length' % (key, key))
            if idx is None or not len(idx):
                self.weights[key] = None
                continue
            if int(idx.min()) < 0 or int(idx.max()) >= N:
                raise ValueError('%s_idx outside [0, %d)' % (key, N))
            self.weights[key] = torch.zeros(N, dtype=state.dtype, device=state.device).index_add_(0, idx.to(state.device), w.to(state))
        if self.weights['flood'] is None:
            raise ValueError('flood_idx is empty')
        self.last_paths = {'prefix': None, 'objective': None}
        self.ce_state = None                  # after solve_ce: (mean, std) of the sampling distribution it ended with

    # ------------------------------------------------------------------ evaluation
    def _check_y(self, y):
        if not isinstance(y, torch.Tensor) or y.dim() != 2 or y.shape[1] != self.n_var:
            raise ValueError('y must be (pop, n_step * n_act = %d), got %r' % (self.n_var, tuple(getattr(y, 'shape', ()))))

    def predict(self, y):
        """(preds (pop, T_h, N, C), edge_preds) of every candidate of y (pop, n_step * n_act): `predict_horizon` on the settings of
        `expand_settings`, with chunk 0 on the shared history where `shared_history` holds."""
        self._check_y(y)
        em, so, pop = self.emul, self.emul.seq_out, y.shape[0]
        settings = expand_settings(y, self.n_step, self.n_act, self.r_step, self.runoff.shape[0])
        rep = lambda t: t.unsqueeze(0).expand((pop,) + tuple(t.shape))
        shared = self.shared_history and bool(em.conv)
        self.last_paths['prefix'] = 'shared' if shared else 'replicated'
        if not shared:
            return predict_horizon(em, settings, rep(self.state).contiguous(), rep(self.runoff).contiguous(), rep(self.edge_state).contiguous())
        runoff = rep(self.runoff)
        ys, es, state, edge_state, perf = [], [], None, None, None
        for i in range(settings.shape[1] // so):
            sl = slice(i * so, (i + 1) * so)
            ri, sett = runoff[:, sl], settings[:, sl]
            if i == 0:
                yy, ey = em.predict_tf_shared(self.state, self.runoff[sl], sett, self.edge_state)
            else:                                 # as predict_horizon: each candidate's own prediction is its next history
                if em.if_flood:
                    state = torch.cat([state[..., :-1], (perf > 0).float(), state[..., -1:]], dim=-1)
                yy, ey = em.predict_tf(state, ri.contiguous(), sett, edge_state)
            state, perf = torch.cat([yy[..., :-2], ri], dim=-1), yy[..., -1:]
            edge_state = torch.cat([ey, em.get_edge_action(sett, True)], dim=-1)
            ys.append(yy)
            es.append(ey)
        em.last_prefix_batch = 1                  # of the horizon's own history (chunk 0); the fed-back chunks ran at pop
        return (ys[0], es[0]) if len(ys) == 1 else (torch.cat(ys, dim=1), torch.cat(es, dim=1))

    def _objective(self, preds):
        C, T = preds.shape[-1], preds.shape[1]
        hip = self.fused_objective and preds.is_cuda and preds.dtype == torch.float32 and 2 <= C <= 8 and T <= 4096
        self.last_paths['objective'] = 'hip' if hip else 'torch'
        if not hip:
            st = self.state.unsqueeze(0).expand((preds.shape[0],) + tuple(self.state.shape))
            return objective_pred(preds, st, gamma=self.gamma, **self.targets)
        w = self.weights
        q_in0 = self.state[-1, :, 1].contiguous()
        args = (preds, q_in0, w['flood'], w['outflow'], w['smooth'], self.gamma)
        return _ag.MpcObjectiveFn.apply(*args) if _ag.grad_on(preds) else _lib.mpc_objective(preds.contiguous(), *args[1:])

    def objective(self, y):
        """Objective (pop,) of every candidate of y, without autograd."""
        with torch.no_grad():
            return self._objective(self.predict(y)[0])

    def objective_and_gradient(self, y):
        """(objective (pop,), its gradient with respect to y (pop, n_step * n_act)): what the module's
        `objective_and_gradient` returns, to a tolerance (other kernels on the shared half, another summation order)."""
        self._check_y(y)
        with torch.enable_grad():
            y = y.detach().clone().requires_grad_(True)
            obj = self._objective(self.predict(y)[0])
            (grad,) = torch.autograd.grad(obj.sum(), y)
        return obj.detach(), grad

    # ------------------------------------------------------------------ solvers (device only)
    def solve_ce(self, pop, iters, n_elite, mean0=None, std0=0.3, smooth=0.3, std_min=1e-3, seed=0):
        """Cross-entropy method, this project's own rules (`uds_ce_draw` / `uds_ce_update` in include/uds_hip.h state them): per
        iteration draw pop candidates from the clipped normal N(mean, std) (a counter-based Philox stream: the run is a function
        of the seed), evaluate them, rank them, and move mean / std towards the n_elite best with the smoothing `smooth`; std
        never falls below std_min.  mean0: (n_var,) or None (0.5); std0: a number or (n_var,).  Nothing is read from the
        device inside the loop; afterwards ONE read fetches the status and the best objective.  FloatingPointError when an
        iteration had no finite candidate.  -> Result(best y (n_var,), its objective (1,), history (iters,)); `ce_state` keeps
        the (mean, std) the loop ended with."""
        n_var, dev = self.n_var, self.state.device
        if not 2 <= pop <= _lib.CE_MAX or not 1 <= n_var <= _lib.CE_MAX or not 1 <= n_elite <= pop or iters < 1:
            raise ValueError('solve_ce: pop=%r (2 to %d), n_var=%d (at most %d), n_elite=%r (1 to pop), iters=%r (at least 1)' %
                             (pop, _lib.CE_MAX, n_var, _lib.CE_MAX, n_elite, iters))
        if not self.state.is_cuda:
            raise _lib.UdsError('solve_ce runs on the device only: the problem lives on %s' % dev)
        vec = lambda v, fill: (torch.full((n_var,), float(fill if v is None else v), device=dev) if v is None or not isinstance(v, torch.Tensor)
                               else v.detach().to(device=dev, dtype=torch.float32).reshape(n_var).clone())
        mean, std = vec(mean0, 0.5), vec(std0, 0.3)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        y = torch.empty(pop, n_var, device=dev)
        best_y, best_obj = torch.zeros(n_var, device=dev), torch.full((1,), float('inf'), device=dev)
        status, history = torch.zeros(4, dtype=torch.int32, device=dev), torch.empty(iters, device=dev)
        for i in range(iters):
            _lib.ce_draw(mean, std, seed, count, pop, out=y)
            obj = self.objective(y).contiguous()
            _lib.ce_update(y, obj, n_elite, smooth, std_min, mean, std, best_y, best_obj, status)
            history[i:i + 1].copy_(best_obj)
        self.ce_state = (mean, std)
        flag, best = torch.cat([status[:1].to(torch.float32), best_obj]).tolist()          # the one read
        if flag:
            raise FloatingPointError('solve_ce: an iteration had no candidate with a finite objective (best so far %r)' % best)
        return Result(best_y, best_obj, history)

    def solve_gr(self, y0, iters, lr=0.05, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        """Projected Adam on every row of y0 (pop, n_var) at once, this project's own rule: per iteration t = 1 .. iters
            m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  y = clip(y - lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps), 0, 1)
        with g the gradient of `objective_and_gradient` at the current y.  Tensor code (the state is (pop, n_var)); nothing is read
        from the device.  -> Result(the final y (pop, n_var), its objective (pop,), history (iters,)): history[i] is the lowest
        objective of any row at the iterates the first i + 1 iterations evaluated (y0 included, the final y not)."""
        self._check_y(y0)
        if iters < 1:
            raise ValueError('solve_gr: iters=%r (at least 1)' % (iters,))
        y = y0.detach().clone()
        m, v = torch.zeros_like(y), torch.zeros_like(y)
        history, best = torch.empty(iters, device=y.device, dtype=y.dtype), torch.full((), float('inf'), device=y.device, dtype=y.dtype)
        for t in range(1, iters + 1):
            obj, g = self.objective_and_gradient(y)
            best = torch.minimum(best, obj.min().to(y.dtype))
            history[t - 1] = best
            m = beta_1 * m + (1 - beta_1) * g
            v = beta_2 * v + (1 - beta_2) * g * g
            lr_t = lr * (1 - beta_2 ** t) ** 0.5 / (1 - beta_1 ** t)
            y = (y - lr_t * m / (v.sqrt() + epsilon)).clamp_(0.0, 1.0)
        return Result(y, self.objective(y), history)
