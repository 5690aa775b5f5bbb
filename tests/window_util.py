"""Shared by tests/test_window_plan.py (CPU), tests/test_gpu_window_batch.py and tests/test_gpu_train_loop.py: a loop-written NumPy
restatement of the window definitions of gnn_uds_amd/data.py (one window, step, node and channel at a time, fp32 throughout, span
formed first), the draw of `WindowTable` restated with oracle.dropout_ref.philox4x32_10 and Python integers, brute-force window
tables / weights / norms, seeded series, and the astlingen model of tests/test_gpu_fit_graph.py (its builder, copied)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

import gnn_uds_amd as U
from oracle.dropout_ref import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PAD = 16                                     # guard floats on either side of a view: a multiple of four, so views stay 16-byte aligned


def make_series(seed, event_len, N, E, n_act=2, tide=True, wet=0.2):
    """dict(states, flood, edge_states, settings, tide) of fp32 arrays; flood > 0 on about `wet` of the rows (whole rows dry else)."""
    rng = np.random.default_rng(seed)
    T = int(sum(event_len))
    wet_row = rng.random(T) < wet
    flood = (rng.random((T, N)) * (rng.random((T, N)) < 0.5) * wet_row[:, None]).astype(F)
    return dict(states=rng.random((T, N, 4)).astype(F), flood=flood, edge_states=(rng.random((T, E, 4)) - 0.3).astype(F),
                settings=rng.random((T, n_act)).astype(F) if n_act else None, tide=rng.random((T, N)).astype(F) if tide else None)


def make_norms(seed, N, E):
    """The five [max, min] arrays with non-zero minima (so the subtraction is exercised): x (N,5), b (N,2), y (N,5), r (N,1), e (E,4)."""
    rng = np.random.default_rng(seed)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), 0.1 * rng.random((rows, c))]).astype(F)
    return mk(N, 5), mk(N, 2), mk(N, 5), mk(N, 1), mk(E, 4)


def windows_ref(series, starts, seq_in, t_out, if_flood, norms=None):
    """(x, a, b, y, ex, ey) by the definitions, element by element.  norms: the five [max, min] arrays or None (raw)."""
    st, fl, es, se, td = (series[k] for k in ('states', 'flood', 'edge_states', 'settings', 'tide'))
    N, E = st.shape[1], es.shape[1]
    n_act = 0 if se is None else se.shape[1]
    cx, cb, B = 5 if if_flood else 4, 1 if td is None else 2, len(starts)
    x, y = np.zeros((B, seq_in, N, cx), F), np.zeros((B, t_out, N, cx), F)
    b, a = np.zeros((B, t_out, N, cb), F), (np.zeros((B, t_out, n_act), F) if n_act else None)
    ex, ey = np.zeros((B, seq_in, E, 4), F), np.zeros((B, t_out, E, 3), F)

    def put(dst, idx, vals, item):
        for c, v in enumerate(vals):
            v = F(v)
            if norms is not None:
                norm = norms[{'x': 0, 'b': 1, 'y': 2, 'e': 4}[item]]
                span = F(norm[0, idx[-1], c] - norm[1, idx[-1], c])
                v = F(F(v - norm[1, idx[-1], c]) / span)
            dst[idx + (c,)] = v

    for w, s in enumerate(starts):
        for t in range(seq_in):
            g = s + t
            for n in range(N):
                h, q, qds, r = st[g, n]
                put(x, (w, t, n), [h, F(q - r), qds] + ([1.0 if fl[g, n] > 0 else 0.0] if if_flood else []) + [r], 'x')
            for e in range(E):
                put(ex, (w, t, e), es[g, e], 'e')
        for t in range(t_out):
            g = s + seq_in + t
            for n in range(N):
                h, q, qds, r = st[g, n]
                put(b, (w, t, n), [r] + ([] if td is None else [td[g, n]]), 'b')
                put(y, (w, t, n), [h, F(q - r), qds] + ([1.0 if fl[g, n] > 0 else 0.0] if if_flood else []) + [fl[g, n]], 'y')
            for e in range(E):
                put(ey, (w, t, e), es[g, e, :3], 'e')
            for j in range(n_act):
                a[w, t, j] = se[g, j]
    return x, a, b, y, ex, ey


def table_ref(event_len, seq_in, t_out, interval, events=None):
    """Window starts by brute force: every candidate row of every event, kept if it is on the interval grid and the window fits."""
    off, starts = 0, []
    for k, L in enumerate(event_len):
        if events is None or k in events:
            for i in range(L):
                if i % interval == 0 and i + seq_in + t_out <= L:
                    starts.append(off + i)
        off += L
    return starts


def weights_ref(flood, starts, seq_in, t_out, w):
    out = []
    for s in starts:
        wet = any(flood[g, n] > 0 for g in range(s + seq_in, s + seq_in + t_out) for n in range(flood.shape[1]))
        out.append(w if wet else 1)
    return out


def draw_ref(starts, weights, seed, j0, count):
    """Draws j0 .. j0 + count - 1 of the stream, in Python integers."""
    cum, total = [], 0
    for w in weights:
        total += int(w)
        cum.append(total)
    counters = np.array([[j & 0xFFFFFFFF, (j >> 32) & 0xFFFFFFFF, 0, 0] for j in range(j0, j0 + count)], dtype=np.uint32)
    out = []
    for words in philox4x32_10(counters, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)):      # one call for all counters
        r = (int(words[0]) << 32) | int(words[1])
        u = (r * total) >> 64
        out.append(starts[next(k for k, c in enumerate(cum) if c > u)])
    return out


def norm_ref(series, if_flood, head=False):
    """get_norm by brute force: per node (link) and channel, a Python loop over the rows."""
    st, fl, es, td = series['states'], series['flood'], series['edge_states'], series['tide']
    T, N, E = st.shape[0], st.shape[1], es.shape[1]

    def rows_of(item, g, n):
        h, q, qds, r = st[g, n]
        bit = [F(1.0 if fl[g, n] > 0 else 0.0)] if if_flood else []
        return {'x': [h, F(q - r), qds] + bit + [r], 'b': [r] + ([] if td is None else [td[g, n]]),
                'y': [h, F(q - r), qds] + bit + [fl[g, n]], 'r': [r]}[item]

    out = []
    for item in ('x', 'b', 'y', 'r', 'e'):
        R = E if item == 'e' else N
        vals = [[list(es[g, n]) if item == 'e' else rows_of(item, g, n) for g in range(T)] for n in range(R)]      # [n][g][c]
        C = len(vals[0][0])
        norm = np.zeros((2, R, C), F)
        for n in range(R):
            for c in range(C):
                col = [vals[n][g][c] for g in range(T)]
                norm[0, n, c] = F(max(col)) + F(1e-6)
                norm[1, n, c] = min(col) if head and item in ('x', 'y') and c == 0 else 0.0
        out.append(norm)
    return tuple(out)


def nan_view(t, dev=None):
    """`t` as a contiguous view in the middle of a NaN-filled parent buffer -> (view, parent); the view stays 16-byte aligned."""
    dev = t.device if dev is None else dev
    parent = torch.full((t.numel() + 2 * PAD,), float('nan'), dtype=t.dtype, device=dev)
    view = parent[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, parent


def guards_intact(parent, n):
    return bool(torch.isnan(parent[:PAD]).all()) and bool(torch.isnan(parent[PAD + n:]).all())


# ---- the model of tests/test_gpu_fit_graph.py::build (copied; that file stays as it is): astlingen, actuated GAT, tide, if_flood = 3
T = 5


def build(dev, recurrent='Conv1D', conv='GAT', **over):
    net = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))['astlingen']
    edges, n, outfall = np.asarray(net['edges']), net['n_node'], np.asarray(net['is_outfall'], dtype=float)
    e = len(edges)
    rng = np.random.default_rng(7)
    args = SimpleNamespace(
        state_shape=(n, 4), edge_state_shape=(e, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3, n_sp_layer=2,
        n_tp_layer=2, activation='relu', if_flood=3, epsilon=0.1, edge_fusion=False, edges=edges, graph=U.DrainageGraph.from_edges(edges, n),
        act=True, act_edges=edges[[1, 4]], conv=conv, resnet=True, recurrent=recurrent, roll=0, model_dir=None, tide=True,
        is_outfall=outfall, hmax=1.0 + rng.random(n), hmin=np.zeros(n), area=0.2 + rng.random(n), learning_rate=1e-3,
        pump=0.1 + rng.random(e), pump_in=rng.random(n) * (rng.random(n) > 0.7), pump_out=rng.random(n) * (rng.random(n) > 0.7),
        offset=rng.random(e) * (rng.random(e) > 0.5), ehmax=0.3 + rng.random(e))
    for k, v in over.items():
        setattr(args, k, v)
    emul = U.Emulator(args.conv, args.resnet, args.recurrent, args, generator=torch.Generator().manual_seed(1)).to(dev)
    mk = lambda rows, c: np.stack([0.5 + rng.random((rows, c)), np.zeros((rows, c))]).astype(np.float32)
    emul.set_norm(mk(n, 5), mk(n, 2), mk(n, 5), mk(n, 1), mk(e, 4))
    return emul, n, e
