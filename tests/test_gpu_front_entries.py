"""lcpm, scaling_factor, compute_var, qc_reads, subset and their commands without torch: the front-half whole-problem entries (csrc/nrm_host_front.hip) on the GPU.
One child process in which `import torch` fails (tests/front_entries_child.py) makes every call and runs every command; the tests hold what it wrote against
the reference-held fixtures (G18_front, G18_front_chain, G19_lcpm_sparse, G20_qc) and the numpy restatements of tests/front_numpy.py.  Tolerances are the
project's: integers exact, fp64 quantities close(1e-9, floor=1), scaling factors 1e-12 absolute, fp32 output the fp64 output rounded once, text files
close(1e-6, floor=1).  No bit equality with the torch route is expected (its exp table is numpy's, its pseudo-inverses LAPACK's)."""
import os

import numpy as np
import pytest

import front_entries_child as child
import front_numpy
from cabi_harness import close, start_child

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ok(a, b):
	return close(a, b, 1e-9, floor=1.0)


def near(a, b):
	return close(a, b, 1e-6, floor=1.0)  # (a text file keeps 8 significant digits)


@pytest.fixture(scope='module')
def ran(tmp_path_factory):
	"""(arrays, notes, directory of the command line's files) of the one child run."""
	work = tmp_path_factory.mktemp('front_entries')
	dst = str(work / 'out.npz')
	env = dict(os.environ)
	for k in ('NRM_HOST_ENTRY', 'NRM_DEBUG'):
		env.pop(k, None)
	arr, notes = start_child('front_entries_child.py', [dst, str(work)], dst, env, timeout=600, tail=4000)
	return arr, notes, str(work)


def test_lcpm_dense_without_torch(golden, ran):
	arr, notes, _ = ran
	g, h = golden('G18_front'), golden('G18_front_chain')
	for dt in ('int32', 'int64'):
		k = 'd.{}.'.format(dt)
		lc = arr[k + 'lcpm']
		print(dt, 'lcpm max abs error %.3g' % np.abs(lc - g['lcpm']).max())
		assert lc.dtype == np.float64 and ok(lc, g['lcpm'])
		assert ok(arr[k + 'cov'][[0, 2]], g['cov'][[0, 2]]) and np.array_equal(arr[k + 'cov'][1], g['cov'][1])
		assert ok(arr[k + 'nonorm'], g['nonorm_lcpm']) and ok(arr[k + 'nonorm_cov'][[0, 2]], g['nonorm_cov'][[0, 2]]) and np.array_equal(arr[k + 'nonorm_cov'][1], g['nonorm_cov'][1])
		assert ok(arr[k + 'ntot'], g['ntot_lcpm']) and ok(arr[k + 'ntot_cov'][[0, 2]], g['ntot_cov'][[0, 2]]) and np.array_equal(arr[k + 'ntot_cov'][1], g['ntot_cov'][1])
		assert ok(arr[k + 'nocov'], h['nocov_lcpm']) and notes[k + 'nocov_cov'] == 'None'
		assert ok(arr[k + 'mean'], h['lowmem_mean']) and np.array_equal(arr[k + 'var'], h['lowmem_var']) and arr[k + 'var'].shape == lc.shape
		assert arr[k + 'f32'].dtype == np.float32 and np.array_equal(arr[k + 'f32'], lc.astype(np.float32))
		assert np.abs(arr[k + 'sf'] - g['sf']).max() <= 1e-12
	assert np.array_equal(arr['d.int32.lcpm'], arr['d.int64.lcpm'])
	clipped = np.minimum(g['reads'], 255)
	assert clipped.max() == 255 and (g['reads'] > 255).any()
	ref, rcov = front_numpy.lcpm(clipped)
	assert ok(arr['d.uint8.lcpm'], ref) and ok(arr['d.uint8.cov'][[0, 2]], rcov[[0, 2]]) and np.array_equal(arr['d.uint8.cov'][1], rcov[1])
	assert np.abs(arr['d.uint8.sf'] - front_numpy.scaling_factor(clipped)).max() <= 1e-12
	assert np.abs(arr['d.sf_other'] - g['sf_logtpropmean_min']).max() <= 1e-12
	assert notes['device_out'].startswith('RuntimeError') and notes['varscale'].startswith('NotImplementedError') and notes['huge'].startswith('NotImplementedError')
	assert notes['negative'] == 'ValueError: Negative value in d detected.'
	neg = g['reads'].astype(np.int16)
	neg[5, 7] = -1
	assert np.abs(arr['d.sf_negative'] - front_numpy.scaling_factor(neg)).max() <= 1e-12


def test_lcpm_sparse_without_torch(golden, ran):
	arr, notes, _ = ran
	g = golden('G19_lcpm_sparse')
	for case in ('lo', 'hi'):
		reads = g[case + '_reads']
		assert notes[case + '.stored_zeros'] == 30 and (reads.sum(axis=1) == 0).any()  # stored zeros and an empty gene row
		for form in ('csr', 'coo', 'csc'):
			k = 's.{}.{}.'.format(case, form)
			lc = arr[k + 'lcpm']
			print(case, form, 'lcpm max abs error %.3g' % np.abs(lc - g[case + '_lcpm']).max())
			assert ok(lc, g[case + '_lcpm']) and ok(arr[k + 'cov'][[0, 2]], g[case + '_cov'][[0, 2]]) and np.array_equal(arr[k + 'cov'][1], g[case + '_cov'][1])
			assert ok(arr[k + 'nonorm'], g[case + '_nonorm_lcpm']) and ok(arr[k + 'ntot'], g[case + '_ntot_lcpm']) and ok(arr[k + 'nocov'], g[case + '_nocov_lcpm'])
			assert np.array_equal(arr[k + 'f32'], lc.astype(np.float32))
			assert np.abs(arr[k + 'sf'] - g[case + '_sf']).max() <= 1e-12
			assert np.array_equal(lc, arr['s.{}.csr.lcpm'.format(case)])  # (the three forms are one canonical matrix)
		for dense in ('dense', 'densified'):
			d = arr['s.{}.{}.lcpm'.format(case, dense)]
			assert ok(d, g[case + '_lcpm']) and ok(d, arr['s.{}.coo.lcpm'.format(case)])
		assert np.array_equal(arr['s.{}.dense.lcpm'.format(case)], arr['s.{}.densified.lcpm'.format(case)])
	assert notes['malformed'] == 'ValueError: ' + notes['malformed_text']


def test_smallest_shapes_without_torch(ran):
	"""The shapes at which the entries' own buffer sizing and pitches can go wrong: one element; one row more than a row tile by one cell more than 1024."""
	from normalisr_amd import _lib
	arr, notes, _ = ran
	lib = _lib.load()
	assert int(lib.nrm_lcpm_row_tile()) == child.LCPM_TILE and int(lib.nrm_fitvar_row_tile()) == child.FITVAR_TILE
	ref, rcov = front_numpy.lcpm(np.array([[1]]))
	assert arr['m.one.lcpm'].shape == (1, 1) and ok(arr['m.one.lcpm'], ref) and ok(arr['m.one.cov'], rcov) and notes['m.one.sf'].startswith('AssertionError')
	x = child.small_counts(child.LCPM_TILE + 1, 1025, 23)
	assert (x[3] == 0).all() and (x.sum(axis=0) > 0).all()
	ref, rcov = front_numpy.lcpm(x)
	for k in ('m.tile.', 'm.tile.csr.'):
		assert ok(arr[k + 'lcpm'], ref) and ok(arr[k + 'cov'][[0, 2]], rcov[[0, 2]]) and np.array_equal(arr[k + 'cov'][1], rcov[1])
		assert np.abs(arr[k + 'sf'] - front_numpy.scaling_factor(x)).max() <= 1e-12
	z = child.small_counts(child.LCPM_TILE + 1, 1025, 23, zero_cell=1024)
	ref = front_numpy.lcpm(z, nocov=True)[0]
	for form in ('dense', 'csr'):
		assert notes['m.zero.{}.cov'.format(form)] == 'ValueError: Found cell with no read at all. Please remove.'
		assert ok(arr['m.zero.{}.nocov'.format(form)], ref)


def test_compute_var_without_torch(golden, ran):
	arr, notes, _ = ran
	h = golden('G18_front_chain')
	assert np.linalg.matrix_rank(h['normcov_c']) == 7 and h['normcov_c'].shape[0] == 8
	for steps, key in ((1, 'w1'), (3, 'w3')):
		w = arr['f.w{}'.format(steps)]
		print(steps, 'weights max relative error %.3g' % np.abs(w / h[key] - 1).max(), notes['f.w{}.state'.format(steps)])
		assert w.shape == h[key].shape and w.dtype == np.float64 and w.min() == 1 and ok(w, h[key])
		assert np.array_equal(w, arr['f.w{}.again'.format(steps)])  # two calls, the same bits
		change, taken = notes['f.w{}.state'.format(steps)]
		assert taken == steps and change > 0
	# the first step starts from a scale of ones and its result has minimum 1: its largest relative change is max(scale) - 1 = max(w1) - 1
	assert ok(notes['f.w1.state'][0], h['w1'].max() - 1) and notes['f.w3.state'][0] <= notes['f.w1.state'][0]
	change, taken = notes['f.eps.state']
	assert 1 <= taken < 50 and change <= 0.5  # (the iterations enqueued past the stop leave the state as it is)
	g = golden('G18_front')
	assert ok(arr['f.w1.f32'], front_numpy.compute_var(g['lcpm'].astype(np.float32).astype(np.float64), h['normcov_c']))
	y, c = child.fitvar_small()
	assert ok(arr['f.small'], front_numpy.compute_var(y, c, stepmax=2))
	y, c = child.fitvar_wide()
	ref = front_numpy.compute_var(y.astype(np.float64), c, stepmax=2)
	print('63 covariates: max relative error %.3g' % np.abs(arr['f.wide'] / ref - 1).max())
	assert ok(arr['f.wide'], ref)
	assert notes['f.constant'].startswith('AssertionError')
	assert notes['f.64'].startswith('NotImplementedError') and '63' in notes['f.64'] and notes['f.0'].startswith('NotImplementedError')


def test_qc_reads_without_torch(golden, ran):
	arr, notes, _ = ran
	g = golden('G20_qc')
	for case in 'abc':
		for form in ('dense', 'csr'):
			k = 'q.{}.{}.'.format(case, form)
			assert np.array_equal(arr[k + 'genes'], g[case + '_genes']) and np.array_equal(arr[k + 'cells'], g[case + '_cells']) and arr[k + 'genes'].dtype == np.int64
			assert notes[k + 'iterations'] == int(g[case + '_iterations'])
			assert np.array_equal(np.flatnonzero(arr[k + 'gene_mask']), g[case + '_genes']) and arr[k + 'cell_mask'].dtype == np.bool_
	assert notes['q.all_genes'] == 'RuntimeError: All genes removed in QC.' and notes['q.all_cells'] == 'RuntimeError: All cells removed in QC.'
	assert notes['q.negative'] == 'ValueError: Negative value in reads detected.' and notes['q.bad_param'].startswith('ValueError')
	assert notes['q.device_out'].startswith('RuntimeError')
	x = g['b_reads']
	assert np.array_equal(arr['q.subset'], g['cli_subset']) and np.array_equal(arr['q.subset_csr'], g['cli_subset']) and arr['q.subset'].dtype == x.dtype
	assert np.array_equal(arr['q.subset_f32'], x.astype(np.float32)[g['b_genes'][::-1]])
	assert notes['q.subset_order'].startswith('ValueError') and notes['q.subset_range'].startswith('IndexError')
	assert np.array_equal(arr['q.outlier'], g['w_pass_1e10'])


def test_host_entry_route_with_torch_present(golden, ran, monkeypatch):
	"""NRM_HOST_ENTRY=1 in this process, where torch is importable: the same entries, so the child's arrays bit for bit; and the default torch route agrees with them
	at the project's tolerances."""
	import normalisr_amd.normalisr as norm
	from normalisr_amd import qc
	arr, notes, _ = ran
	g, h, q = golden('G18_front'), golden('G18_front_chain'), golden('G20_qc')
	reads, dc = g['reads'].astype(np.int32), h['normcov_c']
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	lc_t, _, _, cov_t = norm.lcpm(reads)
	w_t = norm.compute_var(g['lcpm'], dc, stepmax=3)
	qc_t = qc.qc_reads(q['a_reads'], *q['a_params'])
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	lc_e, _, _, cov_e = norm.lcpm(reads)
	assert np.array_equal(lc_e, arr['d.int32.lcpm']) and np.array_equal(cov_e, arr['d.int32.cov'])
	assert np.array_equal(norm.scaling_factor(reads), arr['d.int32.sf'])
	w_e = norm.compute_var(g['lcpm'], dc, stepmax=3)
	assert np.array_equal(w_e, arr['f.w3'])
	qc_e = qc.qc_reads(q['a_reads'], *q['a_params'])
	assert np.array_equal(qc_e[0], arr['q.a.dense.genes']) and np.array_equal(qc_e[1], arr['q.a.dense.cells'])
	assert ok(lc_e, lc_t) and ok(cov_e[[0, 2]], cov_t[[0, 2]]) and np.array_equal(cov_e[1], cov_t[1]) and ok(w_e, w_t)
	assert np.array_equal(qc_e[0], qc_t[0]) and np.array_equal(qc_e[1], qc_t[1])


def test_cli_front_commands_without_torch(golden, ran):
	"""qc_reads, subset, lcpm (text and -s from a Matrix Market file), normcov, fitvar and qc_outlier through main([...]) in the child, which asserts at its end that
	torch was never imported."""
	_, _, work = ran
	g, h, q = golden('G18_front'), golden('G18_front_chain'), golden('G20_qc')
	f = lambda name: os.path.join(work, name)
	names = lambda name: [v.strip() for v in open(f(name)) if v.strip()]
	load = lambda name: np.loadtxt(f(name), delimiter='\t', ndmin=2)
	for genes, cells in (('genes_out.txt', 'cells_out.txt'), ('genes_s.txt', 'cells_s.txt')):
		assert names(genes) == list(q['cli_genes_out']) and names(cells) == list(q['cli_cells_out'])
	for sub in ('sub.tsv', 'sub_s.tsv'):
		text = open(f(sub)).read()
		assert '.' not in text and 'E' not in text and np.array_equal(load(sub), q['cli_subset'])
	assert names('wcells_out.txt') == list(q['cli_wcells_out'])
	assert near(load('lcpm.tsv'), g['lcpm']) and near(load('scale.tsv').ravel(), g['sf']) and near(load('cov.tsv'), h['cov_raw'])
	assert (load('var.tsv') == 0).all() and load('var.tsv').shape == g['lcpm'].shape
	assert near(load('lcpm_s.tsv'), g['lcpm']) and near(load('scale_s.tsv').ravel(), g['sf']) and near(load('cov_s.tsv'), g['cov'])
	assert near(load('ncov.tsv'), h['normcov_c']) and near(load('w1.tsv').ravel(), h['w1'])
