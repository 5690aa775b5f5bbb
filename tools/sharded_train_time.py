"""Graph-sharded Emulator TRAINING on ONE GPU: a whole-network `fit_eval` step against the step of the largest part of an
8-way plan.

    python tools/sharded_train_time.py               timing + a kernel-trace child run under rocprofv3
    python tools/sharded_train_time.py --no-profile  timing only

Reports (one JSON line):
  - for the C2-size network (2000 nodes / 2500 links, B = 2, T = 5, actions) and the 200k-node / 240k-link network
    (BASELINE.json config 4, B = 1, T = 4): `Emulator.fit_eval` on the WHOLE network against `ShardedEmulator.fit_eval` of
    the LARGEST part (own + halo rows) with a loopback exchange -- its messages packed (and, in the adjoint, cleared),
    zero messages received and unpacked / accumulated, no wire -- and the identity reduction.  That is the compute of one
    rank of an 8-GPU step (loss, reverse schedule, replicated Adam on the whole model), not the 8-GPU step time;
  - forward and adjoint exchange counts of one step (2L - 1 spatial + 1 flow column each way);
  - launches of uds_halo_pack_clear_all / uds_halo_accumulate_all per step, from a `rocprofv3 --kernel-trace --stats` run
    of a child process (--count-run) doing STEPS sharded C2 steps.
"""
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U                      # noqa: E402
from gnn_uds_amd import dist as D            # noqa: E402

PARTS, L, STEPS = 8, 3, 4
CONFIGS = {'c2': dict(N=2000, E=2500, B=2, T=5, act=True), 'c4': dict(N=200000, E=240000, B=1, T=4, act=False)}


class _Loopback(D.HaloExchangeAll):
    """One rank alone: every message packed as usual, zero messages received (same launches, no peers on the other end)."""

    def __init__(self, base):
        self.__dict__.update(base.__dict__)
        self.calls = 0

    def __call__(self, x, e):
        self.calls += 1
        return super().__call__(x, e)

    def transport(self, msgs):
        for _, _, inc in msgs:
            if inc is not None:
                inc.zero_()


def _setup(dev, cfg):
    N, E, B, T = cfg['N'], cfg['E'], cfg['B'], cfg['T']
    edges = U.synthetic_drainage_network(N, E, 0)
    g = U.DrainageGraph.from_edges(edges)
    a = SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3,
                        n_sp_layer=L, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=g.edges, act=cfg['act'],
                        act_edges=edges[[3, 50, 7]] if cfg['act'] else None, graph=g, model_dir=None, sparse_params=True, learning_rate=1e-3)
    mk = lambda: U.Emulator('GAT', True, 'Conv1D', a, generator=torch.Generator().manual_seed(1)).to(dev)
    norms = [np.stack([np.ones((n, c)), np.zeros((n, c))]) for n, c in ((N, 5), (N, 1), (N, 5), (N, 1), (E, 4))]
    whole, replica = mk(), mk()
    whole.set_norm(*norms)
    replica.set_norm(*norms)
    probs = D.build_partition_plan(g, PARTS)
    big = max(probs, key=lambda p: len(p.nodes) + len(p.links))
    sh = D.shard_emulator(replica, big, dev)
    sh.exchange, sh.flow_exchange = _Loopback(sh.exchange), _Loopback(sh.flow_exchange)
    gen = torch.Generator().manual_seed(2)
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    x, b, ex, y, ey = r(B, T, N, 5), r(B, T, N, 1) * 0.1, r(B, T, E, 4), r(B, T, N, 5), r(B, T, E, 3)
    act = r(B, T, 3) if cfg['act'] else None
    ni, li = torch.as_tensor(big.nodes, device=dev), torch.as_tensor(big.links, device=dev)
    lx, lb, lex, _ = sh.scatter_inputs(x, b, ex)
    local = (lx, act, lb, y.index_select(2, ni).contiguous(), lex, ey.index_select(2, li).contiguous())
    return whole, sh, big, (x, act, b, y, ex, ey), local


def _time(fn, reps=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _measure(dev, name):
    cfg = CONFIGS[name]
    rec = {'network': [cfg['N'], cfg['E']], 'B': cfg['B'], 'T': cfg['T']}
    try:
        whole, sh, big, data, local = _setup(dev, cfg)
        rec.update(largest_part_rows=[len(big.nodes), len(big.links)], largest_part_own_rows=[len(big.own_nodes), len(big.own_links)],
                   largest_part_peers=len(sh.exchange.peers))
        rec['whole_step_ms'] = round(_time(lambda: whole.fit_eval(*data)), 2)
        rec['whole_peak_gib'] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        del whole
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        c0, a0 = sh.exchange.calls + sh.flow_exchange.calls, sh.exchange.adjoint_calls + sh.flow_exchange.adjoint_calls
        sh.fit_eval(*local)
        rec['exchanges_per_step'] = sh.exchange.calls + sh.flow_exchange.calls - c0
        rec['adjoint_exchanges_per_step'] = sh.exchange.adjoint_calls + sh.flow_exchange.adjoint_calls - a0
        rec['largest_part_step_ms'] = round(_time(lambda: sh.fit_eval(*local)), 2)
        rec['largest_part_peak_gib'] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        rec['ratio'] = round(rec['largest_part_step_ms'] / rec['whole_step_ms'], 3)
    except torch.cuda.OutOfMemoryError as exc:
        rec['unmeasured'] = 'out of memory: %s' % str(exc).split('\n')[0][:200]
    torch.cuda.empty_cache()
    return rec


def _count_run():
    dev = torch.device('cuda:0')
    _, sh, _, _, local = _setup(dev, CONFIGS['c2'])
    for _ in range(STEPS):
        sh.loss_and_grad(*local)
    torch.cuda.synchronize()


def _profile():
    out = tempfile.mkdtemp(prefix='sharded_train_prof_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__),
           '--count-run']
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    stats = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if res.returncode != 0 or not stats:
        return {'profile': 'unmeasured (rocprofv3 rc %d)' % res.returncode, 'profile_stderr': res.stderr[-500:]}
    import csv
    calls = {}
    with open(stats[0]) as fh:
        for row in csv.DictReader(fh):
            calls[row['Name']] = calls.get(row['Name'], 0) + int(row['Calls'])
    clear = sum(c for n, c in calls.items() if re.search(r'k_halo_rows_all<true, (true|false), true>', n))
    acc = sum(c for n, c in calls.items() if 'k_halo_accumulate_all' in n)
    pack = sum(c for n, c in calls.items() if re.search(r'k_halo_rows_all<true, (true|false)(, false)?>', n))
    return {'profiled_steps': STEPS, 'pack_clear_all_launches_per_step': clear / STEPS, 'accumulate_all_launches_per_step': acc / STEPS,
            'pack_all_launches_per_step': pack / STEPS}


def main():
    if '--count-run' in sys.argv:
        _count_run()
        return
    dev = torch.device('cuda:0')
    rec = {'tool': 'sharded_train_time', 'parts': PARTS, 'n_sp_layer': L, 'device': torch.cuda.get_device_name(0)}
    for name in CONFIGS:
        rec[name] = _measure(dev, name)
    if '--no-profile' not in sys.argv:
        rec.update(_profile())
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
