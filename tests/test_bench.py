"""bench.py: its command line and the --dump-outputs writer (CPU), and a short plain run of the headline whose dumped last
step is checked against the seeded headline block recomputed here (gpu)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYTHON = [sys.executable] + (['-s'] if sys.flags.no_user_site else [])
BENCH = os.path.join(ROOT, 'bench.py')


def _row_indexed(S, n, d, dtype):
    """(S, n, d) whose flattened row r holds r in every column: a dumped row says which row it is."""
    return torch.arange(S * n, dtype=dtype).repeat_interleave(d).reshape(S, n, d)


def test_dump_outputs_writes_everything_under_the_budget(tmp_path):
    gen = torch.Generator().manual_seed(0)
    x, e = torch.rand(3, 5, 4, generator=gen), torch.rand(3, 7, 4, generator=gen, dtype=torch.float64)
    assert bench.dump_outputs(str(tmp_path), {'nodes': x, 'links': e}) == 1.0
    for name, t in (('nodes', x), ('links', e)):
        a = np.load(tmp_path / (name + '.npy'))
        assert a.dtype == np.float32 and np.array_equal(a, t.reshape(-1, 4).float().numpy())


def test_dump_outputs_samples_the_same_rows_over_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 64 << 10)
    outs = {'nodes': _row_indexed(6, 100, 16, torch.float32), 'links': _row_indexed(6, 150, 16, torch.float64)}
    frac = bench.dump_outputs(str(tmp_path / 'a'), outs)
    assert 0.0 < frac < 1.0 and bench.dump_outputs(str(tmp_path / 'b'), outs) == frac
    total = 0
    for name, t in outs.items():
        a, b = np.load(tmp_path / 'a' / (name + '.npy')), np.load(tmp_path / 'b' / (name + '.npy'))
        assert a.dtype == np.float32 and np.array_equal(a, b)                    # the same sample in every run
        rows = a[:, 0].astype(np.int64)
        assert len(rows) == int(t.shape[0] * t.shape[1] * frac) and np.all(np.diff(rows) > 0)
        assert np.array_equal(a, t.reshape(-1, 16)[torch.from_numpy(rows)].float().numpy())    # whole rows, unchanged
        total += a.nbytes
    assert total <= 64 << 10


def test_dump_budget_leaves_room_for_the_npy_headers():
    assert bench.DUMP_BUDGET_BYTES + 2 * 4096 <= 64 * 10 ** 6


@pytest.mark.parametrize('argv, message', [
    (['--steps', '0'], '--steps must be at least 1'),
    (['--warmup', '-1'], '--warmup at least 0'),
    (['--workload', 'c4', '--dump-outputs', 'out'], '--dump-outputs writes the outputs of the headline workload only'),
])
def test_bench_refuses_bad_arguments(argv, message):
    r = subprocess.run(PYTHON + [BENCH] + argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path):
    """A plain run times the steps asked for, reports ms_per_step, runs none of the --full legs, and its dump is the
    seeded headline block's output (the same fixed sample of rows)."""
    out = tmp_path / 'out'
    r = subprocess.run(PYTHON + [BENCH, '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'graph-steps/s' and line['higher_is_better'] is True and line['dtype'] and line['metric']
    assert not {'c4_partitioned', 'rollout', 'trained_bias', 'cpu_baseline'} & set(line)

    import gnn_uds_amd as U
    args = SimpleNamespace(nodes=10000, links=12000, embed=64, layers=3, snapshots=60, precision='bf16x3')
    _, block, x, e = bench.headline_setup(U, args, torch.device('cuda', 0))
    with torch.no_grad():
        ox, oe = block(x, e)
    torch.cuda.synchronize()
    bench.dump_outputs(str(tmp_path / 'ref'), {'nodes': ox, 'links': oe})
    total = 0
    for name in ('nodes', 'links'):
        got, ref = np.load(out / (name + '.npy')), np.load(tmp_path / 'ref' / (name + '.npy'))
        assert got.dtype == np.float32 and got.shape == ref.shape and got.shape[1] == 64
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
        total += os.path.getsize(out / (name + '.npy'))
    assert total <= 64 * 10 ** 6
