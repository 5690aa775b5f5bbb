"""Graph-sharded whole Emulator on ONE GPU: the 8-way plan of the 200k-node / 240k-link network (BASELINE.json config 4).

    python tools/sharded_emulator_time.py               timing + a kernel-trace child run under rocprofv3
    python tools/sharded_emulator_time.py --no-profile  timing only

Reports (one JSON line):
  - predict_tf of the WHOLE network against predict_tf of the LARGEST part (own + halo rows), B = 1, seq_in = seq_out = 4;
    the part runs alone with a loopback exchange (its own send buffer packed, a zero receive buffer unpacked: the two
    launches of every exchange, no wire) -- the compute a rank of an 8-GPU run does, not the 8-GPU step time;
  - kernel launches per sharded forward, from a `rocprofv3 --kernel-trace --stats` run of a child process (--count-run)
    that does FORWARDS sharded forwards: the pack_all / unpack_all launches per forward against the 2L - 1 exchanges,
    whatever the part's number of peers.
"""
import glob
import json
import os
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

N, E, T, PARTS, L, FORWARDS = 200000, 240000, 4, 8, 3, 5


class _Loopback(D.HaloExchangeAll):
    """One rank alone: pack its messages, unpack a zero receive buffer (same launches, no peers on the other end)."""

    def __init__(self, base):
        self.__dict__.update(base.__dict__)

    def __call__(self, x, e):
        if x is None:
            x = e.new_empty((e.shape[0], 0, e.shape[-1]))
        if not self.peers:
            return x, e
        self.pack(x, e)
        self.unpack(torch.zeros(e.shape[0] * self.n_recv[self.peers[-1]][1] * e.shape[-1], device=e.device), x, e)
        return x, e


def _setup(dev):
    g = U.DrainageGraph.from_edges(U.synthetic_drainage_network(N, E, 0))
    a = SimpleNamespace(state_shape=(N, 4), edge_state_shape=(E, 4), seq_in=T, seq_out=T, embed_size=64, hidden_dim=64, kernel_size=3,
                        n_sp_layer=L, n_tp_layer=2, activation='relu', if_flood=3, edge_fusion=True, edges=g.edges, act=False, graph=g,
                        model_dir=None, sparse_params=True)
    emul = U.Emulator('GAT', True, 'Conv1D', a, generator=torch.Generator().manual_seed(1)).to(dev)
    emul.set_norm(*(np.stack([np.ones((n, c)), np.zeros((n, c))]) for n, c in ((N, 5), (N, 1), (N, 5), (N, 1), (E, 4))))
    probs = D.build_partition_plan(g, PARTS)
    big = max(probs, key=lambda p: len(p.nodes) + len(p.links))
    sh = D.shard_emulator(emul, big, dev)
    sh.exchange, sh.flow_exchange = _Loopback(sh.exchange), _Loopback(sh.flow_exchange)
    gen = torch.Generator().manual_seed(2)
    X, B, Ex = torch.rand(1, T, N, 5, generator=gen).to(dev), torch.rand(1, T, N, 1, generator=gen).to(dev) * 0.1, torch.rand(1, T, E, 4, generator=gen).to(dev)
    return emul, sh, big, (X, B, Ex)


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _count_run():
    dev = torch.device('cuda:0')
    emul, sh, big, (X, B, Ex) = _setup(dev)
    lx, lb, le, _ = sh.scatter_inputs(X, B, Ex)
    with torch.no_grad():
        for _ in range(FORWARDS):
            sh.forward(lx, lb, le)
    torch.cuda.synchronize()


def _profile():
    out = tempfile.mkdtemp(prefix='sharded_prof_')
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
    pack = sum(c for n, c in calls.items() if 'k_halo_rows_all<true' in n)
    unpack = sum(c for n, c in calls.items() if 'k_halo_rows_all<false' in n)
    one_time = sum(c for n, c in calls.items() if 'pack_weight' in n or 'plan' in n.lower())
    return {'forwards': FORWARDS, 'exchanges_per_forward': 2 * L - 1, 'pack_all_launches_per_forward': pack / FORWARDS,
            'unpack_all_launches_per_forward': unpack / FORWARDS,
            'launches_per_forward_all_kernels': (sum(calls.values()) - one_time) / FORWARDS}


def main():
    if '--count-run' in sys.argv:
        _count_run()
        return
    dev = torch.device('cuda:0')
    emul, sh, big, (X, B, Ex) = _setup(dev)
    lx, lb, le, _ = sh.scatter_inputs(X, B, Ex)
    with torch.no_grad():
        whole = _time(lambda: emul.predict_tf(X, B, None, Ex))
        part = _time(lambda: sh.predict_tf(lx, lb, None, le))
    rec = {'tool': 'sharded_emulator_time', 'network': [N, E], 'parts': PARTS, 'B': 1, 'seq': T, 'n_sp_layer': L,
           'largest_part_rows': [len(big.nodes), len(big.links)], 'largest_part_own_rows': [len(big.own_nodes), len(big.own_links)],
           'largest_part_peers': len(sh.exchange.peers), 'whole_predict_tf_ms': round(whole, 3), 'largest_part_predict_tf_ms': round(part, 3),
           'ratio': round(part / whole, 3), 'device': torch.cuda.get_device_name(0)}
    if '--no-profile' not in sys.argv:
        rec.update(_profile())
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
