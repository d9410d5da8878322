"""A plain `bench.py --gpus 1 --steps K --warmup W` run (no --full): the headline alone, K timed steps, and --dump-outputs writing what the
last timed step computed -- the same values from run to run with the same arguments."""
import os

import numpy as np
import pytest

from conftest import run_bench

pytestmark = pytest.mark.gpu


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
	lines = {}
	for k in (2, 3):
		out = run_bench(['--gpus', '1', '--steps', str(k), '--warmup', '1', '--dump-outputs', str(tmp_path / str(k))], {})
		assert out['_detail'] == {}  # nothing printed before the contract line
		assert out['steps'] == k and out['warmup'] == 1 and out['n_gpus'] == 1 and out['higher_is_better'] is True
		assert out['metric'] == 'association tests/sec (gene x gene coex)' and out['unit'] == 'tests/s' and out['dtype'].startswith('i8 digits')
		assert out['ms_per_step'] > 0 and abs(out['value'] - 5000 * 4999 // 2 * 1e3 / out['ms_per_step']) <= 1e-6 * out['value']
		assert out['cpu_baseline'] is None and out['end_to_end_pcie_s'] is None and out['extra_workloads'] == {}
		assert out['roofline']['kernel'] == 'k_gram_i8' and out['kernels_ms']['gram'] > 0 and out['guard']['uncertified_pairs'] == 0
		lines[k] = out
	names = sorted(os.listdir(tmp_path / '2'))
	assert names == sorted(os.listdir(tmp_path / '3')) and {'p.npy', 'stat.npy'} <= set(names)
	assert sum(os.path.getsize(tmp_path / '2' / f) for f in names) <= 64 << 20
	for f in names:
		a, b = np.load(tmp_path / '2' / f), np.load(tmp_path / '3' / f)
		assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.array_equal(a, b), f
	p, rows = np.load(tmp_path / '2' / 'p.npy'), np.load(tmp_path / '2' / 'p_rows.npy').astype(np.int64)
	assert p.ndim == 2 and p.shape[0] == len(rows) and p.shape[1] >= 5000 and p.dtype == np.float32 and np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()
