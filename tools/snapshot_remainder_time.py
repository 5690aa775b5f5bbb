"""One spatial layer with a TRAINED dense NodeEdge bias on the five networks the reference ships, S = 4096 snapshots, d = 64 and 128:
ms per layer call of the support-only layer, of the trained layer on the tiled remainder GEMM (SpatialLayer.snapshot_remainder off:
uds_remainder_forward_dense) and of the trained layer on the one-launch snapshot kernel (on: uds_remainder_snapshot_pair).

Each variant is one captured HIP graph; the three graphs are replayed in alternation, ROUNDS windows each of at least WINDOW_S seconds
between device events, and the median window is reported with the spread (max - min) / median of the windows.  The outputs of the two
trained variants are compared on the timed inputs (max |difference| relative to max |output|: both are split-bf16 products of the
same operands, summed in a different order).

    python tools/snapshot_remainder_time.py [out.json]       (default profiles/snapshot_remainder_time.json)
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnn_uds_amd as U  # noqa: E402

S = 4096
ROUNDS = 5
WINDOW_S = 0.25
NETWORKS = ('astlingen', 'shunqing', 'chaohu', 'hague', 'RedChicoSur')


def capture(layer, x, e):
    """(graph, outputs) of one captured layer call."""
    with torch.no_grad():
        for _ in range(3):                       # tile plans, packed weights, LDS attributes, allocator
            layer(x, e)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer(x, e)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(x, e)
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    return g, out


def window(g, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main(path):
    if not torch.cuda.is_available():
        raise SystemExit('snapshot_remainder_time needs the MI355X: no timing without a device')
    dev = torch.device('cuda', 0)
    nets = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'networks.json')))
    rows = []
    for name in NETWORKS:
        net = nets[name]
        gph = U.DrainageGraph.from_edges(np.array(net['edges']), net['n_node'])
        for d in (64, 128):
            gen = torch.Generator().manual_seed(2)
            x = torch.rand(S, gph.n_node, d, generator=gen).to(dev)
            e = torch.rand(S, gph.n_edge, d, generator=gen).to(dev)
            mk = lambda sparse: U.SpatialLayer(gph, d, 'relu', sparse_params=sparse, generator=torch.Generator().manual_seed(1)).to(dev)
            sup, off, on = mk(True), mk(False), mk(False)
            bias = torch.Generator().manual_seed(3)
            for ne in ('node_edge_n', 'node_edge_e'):
                b = torch.randn(getattr(off, ne).bias.shape, generator=bias) * 0.01
                for layer in (off, on):
                    getattr(layer, ne).bias.data = b.to(dev)
            on.snapshot_remainder = True
            graphs, outs = zip(*(capture(layer, x, e) for layer in (sup, off, on)))
            assert off.last_remainder == ('gemm', 'gemm') and off.last_path == on.last_path == 'fused+remainder'
            diff = max(float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(outs[2], outs[1]))
            counts = [max(20, int(WINDOW_S * 1000.0 / window(g, 20)) + 1) for g in graphs]
            times = [[], [], []]
            for _ in range(ROUNDS):
                for i, g in enumerate(graphs):       # alternating: a drift of the machine lands on all three alike
                    times[i].append(window(g, counts[i]))
            med = [statistics.median(t) for t in times]
            spread = [(max(t) - min(t)) / m for t, m in zip(times, med)]
            row = {'network': name, 'nodes': gph.n_node, 'links': gph.n_edge, 'd': d, 'S': S, 'route': on.last_route,
                   'remainder_on': list(on.last_remainder),
                   'support_only_ms': round(med[0], 4), 'trained_gemm_ms': round(med[1], 4), 'trained_snapshot_ms': round(med[2], 4),
                   'ratio_gemm': round(med[1] / med[0], 2), 'ratio_snapshot': round(med[2] / med[0], 2),
                   'snapshot_over_gemm': round(med[2] / med[1], 3), 'spread': [round(s, 3) for s in spread],
                   'replays_per_window': counts, 'windows': ROUNDS, 'max_rel_diff_on_vs_off': diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del graphs, outs, sup, off, on, x, e
            torch.cuda.empty_cache()
    with open(path, 'w') as fh:
        json.dump({'what': 'one SpatialLayer call, captured HIP graph, median of %d alternated windows of >= %.2f s' % (ROUNDS, WINDOW_S),
                   'device': torch.cuda.get_device_name(0), 'rows': rows}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'snapshot_remainder_time.json'))
