"""Device-resident training data: the counterpart of the reference's `DataGenerator` (`surrogate/dataloader.py`) for the part that
runs every epoch.  The reference draws one random batch of sliding windows per epoch in NumPy (`prepare_batch`,
`dataloader.py:106-143`; windows cut as `dataloader.py:93-95,144-169`), normalises five tensors and uploads them
(`main.py:209-232`).  Here the event series are uploaded ONCE (`WindowStore`), a batch of windows is built and normalised by one HIP
launch (`uds_window_batch`), and the window starts are drawn on the device from a counter-based stream (`WindowTable.draw`,
`uds_window_draw`), so a training step uploads nothing.

Layout: fp32, time-major, all events concatenated along time into Ttot rows (`event_len` sums to Ttot):

    states       (Ttot, N, 4)      [h, q_totin, q_ds, r]                      
    flood        (Ttot, N)         flooding volume of the step (the reference's `perfs`), >= 0
    edge_states  (Ttot, E, 4)      [depth, volume, flow, setting]
    settings     (Ttot, n_act)     one column per control action, or None
    tide         (Ttot, N)         second boundary channel (models with `tide`), or None

With t_out = seq_out * max(roll, 1) the window at global start s covers rows s .. s + seq_in + t_out - 1 of ONE event:

    X[t]   row s + t            [h, q_totin - r, q_ds, (1.0 if flood > 0 else 0.0, with if_flood), r]
    B[t]   row s + seq_in + t   [r, (tide)]
    Y[t]   row s + seq_in + t   [h, q_totin - r, q_ds, (flood bit, with if_flood), flood]
    EX[t]  row s + t            the four link channels          EY[t]  row s + seq_in + t   the first three
    A[t]   row s + seq_in + t   settings, never normalised (None without settings)

TWO RULES BELOW ARE THIS PROJECT'S OWN, not restatements: the sampling weights of `WindowTable` (the reference's exact rule,
`dataloader.py:106-143`, was not available; SURVEY.md records only "flood-weighted sampling") and `get_norm` (SURVEY.md Appendix A
records the reference's rule, `dataloader.py:224-266`, only in outline: per-node maxima + 1e-6, min = 0 except head-based
environments).
"""
import numpy as np
import torch

from . import _lib


def _series(t, name, shape, device):
    """A contiguous fp32 copy on `device` owned by the store (a fresh allocation: 16-byte aligned whatever the caller passed)."""
    if t is None:
        return None
    t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t)
    if t.dim() != len(shape) or any(want is not None and want != got for want, got in zip(shape, t.shape)):
        raise ValueError('%s must be %s, got %r' % (name, tuple('*' if s is None else s for s in shape), tuple(t.shape)))
    return t.detach().to(device=device, dtype=torch.float32, copy=True).contiguous()


class WindowStore:
    """The event series on one device, and batches of sliding windows cut from them.

    `batch(starts)` returns `(x, a, b, y, ex, ey)` in `Emulator.fit_eval`'s order: on a CUDA store ONE launch of
    `uds_window_batch`, on a CPU store `batch_torch` -- the route follows the store's device, `last_path` records it ('hip' /
    'torch').  seq_in, seq_out, roll and if_flood come from `emul` or from the keywords; the norms come from `emul._norms` (through
    `Emulator._norm_parts`, so a later `set_norm` is seen) or, without a model, from `set_norm` on the store."""

    def __init__(self, states, flood, edge_states, event_len, settings=None, tide=None, emul=None, device=None, seq_in=None, seq_out=None,
                 roll=None, if_flood=None):
        if device is None:
            device = next(emul.parameters()).device if emul is not None else (states.device if isinstance(states, torch.Tensor) else 'cpu')
        self.device = torch.device(device)
        self.event_len = [int(v) for v in event_len]
        if any(v < 0 for v in self.event_len):
            raise ValueError('event_len has a negative entry')
        self.Ttot = sum(self.event_len)
        self.event_off = [int(v) for v in np.concatenate([[0], np.cumsum(self.event_len)[:-1]])] if self.event_len else []
        self.states = _series(states, 'states', (self.Ttot, None, 4), self.device)
        self.device = self.states.device          # with its index ('cuda' -> 'cuda:0'): what every tensor of the store reports
        self.N = self.states.shape[1]
        self.flood = _series(flood, 'flood', (self.Ttot, self.N), self.device)
        self.edge_states = _series(edge_states, 'edge_states', (self.Ttot, None, 4), self.device)
        self.E = self.edge_states.shape[1]
        self.settings = _series(settings, 'settings', (self.Ttot, None), self.device)
        self.tide = _series(tide, 'tide', (self.Ttot, self.N), self.device)
        self.n_act = 0 if self.settings is None else self.settings.shape[1]
        pick = lambda v, name, default: int(v if v is not None else getattr(emul, name) if emul is not None else default)
        self.seq_in, self.seq_out, self.roll = pick(seq_in, 'seq_in', 6), pick(seq_out, 'seq_out', 1), pick(roll, 'roll', 0)
        self.if_flood = pick(if_flood, 'if_flood', 0)
        if self.seq_in < 1 or self.seq_out < 1:
            raise ValueError('seq_in=%d seq_out=%d' % (self.seq_in, self.seq_out))
        self.emul = emul
        self._norms, self._norm_derived = {}, {}
        self.last_path = None

    # ------------------------------------------------------------------ shapes
    @property
    def t_out(self):
        return self.seq_out * max(self.roll, 1)

    @property
    def cx(self):
        return 5 if self.if_flood else 4

    @property
    def cb(self):
        return 1 if self.tide is None else 2

    # ------------------------------------------------------------------ norms
    def set_norm(self, norm_x, norm_b, norm_y, norm_r, norm_e):
        """The five `[max, min]` arrays for a store without a model (with one, the model's are used)."""
        for k, v in (('x', norm_x), ('b', norm_b), ('y', norm_y), ('r', norm_r), ('e', norm_e)):
            if v is not None:
                self._norms[k] = torch.as_tensor(np.asarray(v), dtype=torch.float32).to(self.device)
        self._norm_derived = {}

    def _norm_parts(self, item, dim):
        """(max - min, min) of the first `dim` channels of norm `item` on the store's device, span formed once: `Emulator._norm_parts`."""
        if self.emul is not None:
            return self.emul._norm_parts(item, dim, self.device)
        hit = self._norm_derived.get((item, dim))
        if hit is None:
            normal = self._norms[item]
            maxi, mini = normal[0, ..., :dim], normal[1, ..., :dim]
            hit = self._norm_derived[(item, dim)] = ((maxi - mini).contiguous(), mini.contiguous())
        return hit

    def get_norm(self, head=False):
        """`(norm_x, norm_b, norm_y, norm_r, norm_e)` for `Emulator.set_norm`, each a `(2, N or E, C)` NumPy array `[max, min]`.
        THE PROJECT'S OWN RULE (the reference's, `dataloader.py:224-266`, is known only in outline): the max is per node (link) and
        channel over ALL rows of the derived channels of X / B / Y / r / EX, plus 1e-6; the min is 0, except with head=True, where
        channel 0 (h) of x and y takes its per-node minimum.  Plain tensor code, run once per data set."""
        h, q, qds, r = self.states.unbind(-1)
        bit = [(self.flood > 0).to(torch.float32)] if self.if_flood else []
        chans = {'x': [h, q - r, qds] + bit + [r], 'b': [r] + ([] if self.tide is None else [self.tide]),
                 'y': [h, q - r, qds] + bit + [self.flood], 'r': [r], 'e': list(self.edge_states.unbind(-1))}
        out = []
        for item in ('x', 'b', 'y', 'r', 'e'):
            v = torch.stack(chans[item], dim=-1)                        # (Ttot, N or E, C)
            maxi = v.max(dim=0).values + 1e-6
            mini = torch.zeros_like(maxi)
            if head and item in ('x', 'y'):
                mini[:, 0] = v[..., 0].min(dim=0).values
            out.append(torch.stack([maxi, mini]).cpu().numpy())
        return tuple(out)

    # ------------------------------------------------------------------ window starts
    def _windows(self, k, t_out, interval=1):
        n = self.event_len[k] - (self.seq_in + t_out)
        if n < 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        return torch.arange(self.event_off[k], self.event_off[k] + n + 1, interval, dtype=torch.int32, device=self.device)

    def event_windows(self, k):
        """Every window start of event k at interval 1 with t_out = seq_out (what `Emulator.simulate` takes): int32, on the device."""
        return self._windows(k, self.seq_out)

    def table(self, events=None, interval=1, flood_weight=1, seed=0):
        return WindowTable(self, events, interval, flood_weight, seed)

    def _checked_starts(self, starts, t_out):
        """A host sequence of starts, each checked to lie inside ONE event, uploaded as int32."""
        host = np.asarray(starts.cpu() if isinstance(starts, torch.Tensor) else starts)
        if host.ndim != 1 or (host.size and not np.issubdtype(host.dtype, np.integer)):
            raise ValueError('starts must be a one-dimensional sequence of integers')
        lo = np.asarray(self.event_off, dtype=np.int64)
        hi = lo + np.asarray(self.event_len, dtype=np.int64)
        for s in host.tolist():
            k = int(np.searchsorted(hi, s, side='right'))            # the event whose rows hold s
            if s < 0 or k >= len(lo) or s + self.seq_in + t_out > hi[k]:
                raise ValueError('window start %d (rows %d .. %d) does not lie inside one event of the store (Ttot=%d)'
                                 % (s, s, s + self.seq_in + t_out - 1, self.Ttot))
        return torch.as_tensor(host.astype(np.int32), device=self.device)

    def _starts(self, starts, t_out):
        if isinstance(starts, torch.Tensor) and starts.device == self.device:
            if starts.dtype != torch.int32 or starts.dim() != 1:
                raise ValueError('device starts must be a one-dimensional int32 tensor, got %s %r' % (starts.dtype, tuple(starts.shape)))
            return starts
        if isinstance(starts, torch.Tensor) and starts.is_cuda:       # never read back silently: only HOST sequences are checked and uploaded
            raise ValueError('starts live on %s, the store on %s' % (starts.device, self.device))
        return self._checked_starts(starts, t_out)

    # ------------------------------------------------------------------ batches
    def batch(self, starts, normalized=True, out=None, t_out=None):
        """`(x, a, b, y, ex, ey)` of the windows at `starts`: an int32 tensor on the store's device (taken as it is: on a CUDA store
        a start outside the series fills its window with NaN, which `fit_eval`'s finite test then refuses), or a host sequence,
        which is checked against the events (ValueError) and uploaded.  normalized=False: raw values (`predict` / `simulate`
        normalise themselves).  out: the tuple of an earlier call, filled again.  t_out: output rows, default seq_out * max(roll, 1)."""
        t_out = self.t_out if t_out is None else int(t_out)
        starts = self._starts(starts, t_out)
        if self.device.type != 'cuda':
            res = self.batch_torch(starts, normalized, t_out)
            if out is not None:
                for dst, src in zip(out, res):
                    if dst is not None:
                        dst.copy_(src)
                res = tuple(out)
            self.last_path = 'torch'
            return res
        norms = None
        if normalized:
            norms = {'x': self._norm_parts('x', self.cx), 'b': self._norm_parts('b', self.cb), 'y': self._norm_parts('y', self.cx),
                     'e': self._norm_parts('e', 4)}
        res = _lib.window_batch(self.states, self.flood, self.edge_states, self.settings, self.tide, starts, self.seq_in, t_out, self.if_flood,
                                norms, out)
        self.last_path = 'hip'
        return res

    def batch_torch(self, starts, normalized=True, t_out=None):
        """The same tuple from indexing, `torch.stack` / `cat` and the `normalize` arithmetic, on any device: the definition the
        kernel is tested against, and what a CPU store runs.  Every start must be valid (indexing raises otherwise)."""
        t_out = self.t_out if t_out is None else int(t_out)
        s = self._starts(starts, t_out).to(torch.int64)
        rows_in = s[:, None] + torch.arange(self.seq_in, device=self.device)                      # (B, seq_in)
        rows_out = s[:, None] + self.seq_in + torch.arange(t_out, device=self.device)             # (B, t_out)

        def node(rows, last):
            h, q, qds, r = self.states[rows].unbind(-1)
            fl = self.flood[rows]
            bit = [(fl > 0).to(torch.float32)] if self.if_flood else []
            return torch.stack([h, q - r, qds] + bit + [r if last == 'r' else fl], dim=-1), r

        x, _ = node(rows_in, 'r')
        y, r_out = node(rows_out, 'flood')
        b = torch.stack([r_out] + ([] if self.tide is None else [self.tide[rows_out]]), dim=-1)
        ex = self.edge_states[rows_in]
        ey = self.edge_states[rows_out][..., :3]
        a = None if self.settings is None else self.settings[rows_out]
        if normalized:
            def norm(v, item):
                span, mini = self._norm_parts(item, v.shape[-1])
                return (v - mini) / span
            x, b, y, ex, ey = norm(x, 'x'), norm(b, 'b'), norm(y, 'y'), norm(ex, 'e'), norm(ey, 'e')
        return x, a, b, y.contiguous(), ex.contiguous(), ey.contiguous()


class WindowTable:
    """The windows of a set of events with integer sampling weights, and a counter-based stream of draws from them.

    For event k (offset o_k, length L_k) the starts are o_k + i * interval, i = 0, 1, ..., while i * interval + seq_in + t_out <= L_k
    (a shorter event contributes none).  THE WEIGHTS ARE THIS PROJECT'S OWN RULE (the reference's flood-weighted sampling,
    `dataloader.py:106-143`, was not available): every window weighs 1, and with flood_weight = w >= 1 a window weighs w if any
    node has flood > 0 in any of its t_out output rows.  `starts` (int32), `weights` (uint32) and `cum` (inclusive 64-bit prefix
    sums) live on the store's device, built once in tensor code.

    Draw j (counting from 0 over the life of the table): Philox4x32-10 with key = seed and counter (j, 0), r = word0 << 32 | word1,
    u = (r * total) >> 64, the window is the smallest k with cum[k] > u.  `count` (one int64 device element) is the next j;
    `state_dict` / `load_state_dict` carry (seed, count), so a resumed run continues the stream."""

    def __init__(self, store, events=None, interval=1, flood_weight=1, seed=0):
        interval, flood_weight = int(interval), int(flood_weight)
        if interval < 1 or flood_weight < 1 or flood_weight >= 1 << 32:
            raise ValueError('interval=%d flood_weight=%d: both must be >= 1' % (interval, flood_weight))
        self.store, self.interval, self.flood_weight, self.seed = store, interval, flood_weight, int(seed)
        self.events = list(range(len(store.event_len))) if events is None else [int(k) for k in events]
        dev, t_out = store.device, store.t_out
        parts = [store._windows(k, t_out, interval) for k in self.events]
        self.starts = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int32, device=dev)
        if self.starts.shape[0] == 0:
            raise ValueError('no window of %d + %d rows fits into events %r (lengths %r)'
                             % (store.seq_in, t_out, self.events, [store.event_len[k] for k in self.events]))
        weights = torch.ones(self.starts.shape[0], dtype=torch.int64, device=dev)
        if flood_weight > 1:
            wet = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), (store.flood > 0).any(dim=1).to(torch.int64).cumsum(0)])
            first = self.starts.to(torch.int64) + store.seq_in
            weights = torch.where(wet[first + t_out] > wet[first], flood_weight, 1).to(torch.int64)
        self.cum = weights.cumsum(0)
        self.weights = weights.to(torch.uint32)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)

    def __len__(self):
        return self.starts.shape[0]

    def draw(self, B, out=None):
        """The next B (1 .. 4096) window starts, int32 on the device (`uds_window_draw`); nothing crosses the bus.  Device only."""
        return _lib.window_draw(self.starts, self.cum, self.seed, self.count, B, out)

    def state_dict(self):
        return {'seed': self.seed, 'count': int(self.count.item())}

    def load_state_dict(self, sd):
        self.seed = int(sd['seed'])
        self.count.fill_(int(sd['count']))
