"""bench.py's contract line (no GPU): built from a recorded run's records it stays under 4 KB -- the driver keeps the tail of stdout, and
the round-4 line (14 KB) lost its first extra workloads there --, carries the contract's keys, one summary row per extra workload and
the scaling series; HBM traffic is attached only from the kernel(s) a step actually ran."""
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorded():
	d = json.load(open(os.path.join(ROOT, 'profiles', 'r04_bench_default.json')))
	return d, d.pop('extra_workloads')


def test_contract_line_is_short_and_complete():
	head, extras = _recorded()
	head['scaling_series'] = dict(workload='coex_c5: BASELINE configs[4] per-rank slice, 3750 gene rows per rank x 500000 cells fp64', value=9.2e7, unit='tests/s', ms_per_step=76.2,
								  ranks=1, tests_per_step=7029375, value_per_rank=9.2e7, roofline_frac=0.45, exchange_ms_not_hidden=0.0)
	head['config']['scaling_series'] = 'top-level `scaling_series` = BASELINE configs[4] per-rank slice, the same workload at every N (the headline itself at N > 1)'
	extras['de_c4']['cold_ms'] = 3.1
	extras['broken'] = dict(error='RuntimeError: ' + 'x' * 500)
	line = bench.contract_line(head, extras, 1, head.get('end_to_end_pcie'))
	text = json.dumps(line)
	assert len(text) < 4096, len(text)
	for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline',
			  'scaling_series', 'extra_workloads'):
		assert k in line, k
	assert line['vs_baseline'] is None and line['config']['workload'].startswith('norm.coex') and 'model' not in line['config']
	for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
		assert k in line['roofline'], k
	for k in ('value', 'unit', 'cores', 'kind', 'sample'):
		assert k in line['cpu_baseline'], k
	assert set(line['extra_workloads']) == set(extras) and line['extra_workloads']['de_c4']['cold_ms'] == 3.1 and isinstance(line['extra_workloads']['broken'], str)
	assert line['scaling_series']['ranks'] == 1 and line['scaling_series']['workload'].startswith('coex_c5')


def test_traffic_comes_from_the_kernels_that_ran(tmp_path, monkeypatch):
	pm = {'k_de_sparse<float, true, true>': dict(hbm_bytes_per_launch=3.4e9, effective_clock_ghz=2.1), 'k_s1_stream<float, 5, 8, true, true>': dict(hbm_bytes_per_launch=3.2e9),
		  'k_gram_i8<6>': dict(hbm_bytes_per_launch=1.96e10)}
	f = tmp_path / 'pmc.json'
	f.write_text(json.dumps(pm))
	monkeypatch.setitem(bench.PMC_FILES, 'w', [str(f)])
	roof = dict(kernel='k_de_sparse')
	bench.pmc_traffic('w', roof, kernels=['k_de_sparse', 'k_s1_stream'])
	assert roof['traffic'] == 3.4e9 + 3.2e9 and 'k_de_sparse' in roof['traffic_source'] and 'k_s1_stream' in roof['traffic_source'] and 'k_gram_i8' not in roof['traffic_source']
	roof = dict(kernel='k_de_sparse')
	bench.pmc_traffic('w', roof)
	assert roof['traffic'] == 3.4e9
	roof = dict(kernel='k_fused_new', traffic=1.0, traffic_source='stale')
	bench.pmc_traffic('w', roof)  # no counters for this kernel on file: null, never another kernel's
	assert roof['traffic'] is None and 'traffic_source' not in roof


def test_dump_outputs_float_files_within_the_budget(tmp_path):
	"""--dump-outputs: one float32 / float64 .npy per output, small ones whole, large ones as the same seeded sample of rows on every call
	(indices beside them), everything within the byte limit."""
	import numpy as np
	rng = np.random.default_rng(5)
	big = rng.random((3000, 700)).astype(np.float32)
	arrays = dict(p=big, stat=rng.random((3000, 700)), var=rng.random(3000), net=big > 0.5, flags=np.arange(8, dtype=np.int32), none=None)
	limit = 4 << 20
	shapes = bench.dump_outputs(str(tmp_path / 'a'), arrays, limit=limit)
	assert set(shapes) == {'p', 'stat', 'var', 'net', 'flags'}
	files = {f.name: f for f in (tmp_path / 'a').iterdir()}
	assert sum(f.stat().st_size for f in files.values()) <= limit
	loaded = {f[:-4]: np.load(files[f]) for f in files}
	assert loaded['p'].dtype == np.float32 and loaded['net'].dtype == np.float32 and loaded['stat'].dtype == np.float64 and loaded['flags'].dtype == np.float64
	assert np.array_equal(loaded['var'], arrays['var']) and np.array_equal(loaded['flags'], np.arange(8))  # small enough: whole
	rows = loaded['p_rows'].astype(np.int64)
	assert loaded['p_rows'].dtype == np.float64 and 0 < len(rows) < 3000 and (np.diff(rows) > 0).all()
	assert np.array_equal(loaded['p'], big[rows]) and np.array_equal(loaded['net'], (big > 0.5)[loaded['net_rows'].astype(np.int64)].astype(np.float32))
	bench.dump_outputs(str(tmp_path / 'b'), arrays, limit=limit)  # the same rows again
	assert all(np.array_equal(np.load(tmp_path / 'b' / f), loaded[f[:-4]]) for f in files)
	# a single row above its share: elements of the flattened output are sampled instead
	shapes = bench.dump_outputs(str(tmp_path / 'c'), dict(wide=rng.random((2, 1 << 20))), limit=limit)
	w = np.load(tmp_path / 'c' / 'wide.npy')
	assert w.ndim == 1 and sum(f.stat().st_size for f in (tmp_path / 'c').iterdir()) <= limit
