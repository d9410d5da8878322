"""CPU-only checks of quality control (normalisr_amd/qc.py, the qc_reads / subset / qc_outlier sub-commands): the parser against the reference's flags and
defaults, argument validation before any device call, qc_outlier (host code) against what the reference returned (golden G20, tests/golden/make_g20.py), the
numpy restatement of tests/qc_numpy.py -- the independent check of the GPU tests' random shapes -- against the same fixture, the name-list files, and the
C-ABI entries.  Everything here is exact: integers, booleans and names."""
import os

import numpy as np
import pytest

import qc_numpy
from conftest import ROOT

CASES = {'a': (4, 185, 374), 'b': (3, 86, 682), 'c': (2, 256, 463)}  # iterations, genes kept, cells kept (verified with the reference by make_g20.py)


def test_parser_accepts_the_quality_control_sub_commands():
	from normalisr_amd.__main__ import build_parser
	p = build_parser()
	ns = vars(p.parse_args(['qc_reads', 'r', 'g', 'c', 'go', 'co']))
	assert ns['cmd'] == 'qc_reads' and (ns['reads_in'], ns['genes_in'], ns['cells_in'], ns['genes_out'], ns['cells_out']) == ('r', 'g', 'c', 'go', 'co')
	assert (ns['n_gene'], ns['nc_gene'], ns['ncp_gene'], ns['n_cell'], ns['nt_cell'], ns['ntp_cell'], ns['sparse']) == (0, 50, 0.02, 500, 100, 0, False)
	assert all(isinstance(ns[k], int) for k in ('n_gene', 'nc_gene', 'n_cell', 'nt_cell')) and all(isinstance(ns[k], float) for k in ('ncp_gene', 'ntp_cell'))
	ns = vars(p.parse_args(['qc_reads', 'r', 'g', 'c', 'go', 'co', '-s', '--gene_read_count', '7', '--gene_cell_count', '8', '--gene_cell_prop', '0.5',
							'--cell_read_count', '9', '--cell_gene_count', '10', '--cell_gene_prop', '0.25']))
	assert (ns['n_gene'], ns['nc_gene'], ns['ncp_gene'], ns['n_cell'], ns['nt_cell'], ns['ntp_cell'], ns['sparse']) == (7, 8, 0.5, 9, 10, 0.25, True)
	ns = vars(p.parse_args(['subset', 'in', 'out']))
	assert ns['cmd'] == 'subset' and (ns['matrix_in'], ns['matrix_out'], ns['r'], ns['c'], ns['nodummy'], ns['sparse']) == ('in', 'out', None, None, False, False)
	ns = vars(p.parse_args(['subset', 'in', 'out', '-r', 'a', 'b', '-c', 'd', 'e', '--nodummy', '-s']))
	assert (ns['r'], ns['c'], ns['nodummy'], ns['sparse']) == (['a', 'b'], ['d', 'e'], True, True)
	ns = vars(p.parse_args(['qc_outlier', 'w', 'c', 'co']))
	assert ns['cmd'] == 'qc_outlier' and (ns['weights_in'], ns['cells_in'], ns['cells_out'], ns['pcut'], ns['outrate']) == ('w', 'c', 'co', 1e-10, 0.02)
	ns = vars(p.parse_args(['qc_outlier', 'w', 'c', 'co', '--pcut', '1e-3', '--outrate', '0.1']))
	assert (ns['pcut'], ns['outrate']) == (1e-3, 0.1)
	from normalisr_amd import run
	assert all(callable(getattr(run, name)) for name in ('qc_reads', 'subset', 'qc_outlier'))


def test_qc_reads_argument_validation_before_any_device_call():
	from normalisr_amd import qc
	x = np.ones((3, 5), dtype=np.int64)
	with pytest.raises(ValueError, match='2 dimensions'):
		qc.qc_reads(x[0], 0, 0, 0, 0, 0, 0)
	for bad in range(6):
		p = [0, 0, 0, 0, 0, 0]
		p[bad] = -1
		with pytest.raises(ValueError, match='non-negative'):
			qc.qc_reads(x, *p)
	for bad in (2, 5):
		p = [0, 0, 0, 0, 0, 0]
		p[bad] = 1.5
		with pytest.raises(ValueError, match='no greater than 1'):
			qc.qc_reads(x, *p)
	with pytest.raises(ValueError, match='Negative'):
		qc.qc_reads(x - 2, 0, 0, 0, 0, 0, 0)
	with pytest.raises(RuntimeError, match='All genes'):
		qc.qc_reads(np.zeros((0, 5), dtype=np.int64), 0, 0, 0, 0, 0, 0)
	with pytest.raises(RuntimeError, match='All cells'):
		qc.qc_reads(np.zeros((4, 0), dtype=np.int64), 0, 0, 0, 0, 0, 0)
	import scipy.sparse
	with pytest.raises(ValueError, match='Negative'):
		qc.qc_reads(scipy.sparse.csr_matrix(x - 2), 0, 0, 0, 0, 0, 0)
	with pytest.raises(ValueError, match='non-negative'):
		qc.qc_reads(scipy.sparse.csr_matrix(x), 0, 0, 0, -1, 0, 0)


def test_subset_argument_validation_before_any_device_call():
	from normalisr_amd import qc
	import scipy.sparse
	x = np.arange(15, dtype=np.int32).reshape(3, 5)
	with pytest.raises(ValueError, match='2 dimensions'):
		qc.subset(x[0])
	with pytest.raises(IndexError):
		qc.subset(x, genes=[0, 3])
	with pytest.raises(IndexError):
		qc.subset(x, cells=[-6])
	with pytest.raises(IndexError):
		qc.subset(x, genes=np.ones(4, dtype=bool))
	with pytest.raises(IndexError):
		qc.subset(x, cells=np.array([0.5]))
	with pytest.raises(ValueError, match='one-dimensional'):
		qc.subset(x, genes=np.zeros((2, 2), dtype=np.int64))
	m = scipy.sparse.csr_matrix(x)
	for sel in (dict(genes=[1, 0]), dict(cells=[0, 2, 2]), dict(genes=[0, 1], cells=[4, 3])):
		with pytest.raises(ValueError, match='increase strictly'):
			qc.subset(m, **sel)
	with pytest.raises(IndexError):
		qc.subset(m, cells=[5])


def test_thresholds_are_the_reference_comparisons():
	"""An integer count t meets a float bound, t >= bound, exactly when t >= ceil(bound): the integer thresholds against the comparison as the reference writes
	it, over the proportions and sizes the comparisons can meet."""
	from normalisr_amd.qc import qc_thresholds
	rng = np.random.default_rng(0)
	for _ in range(300):
		nt, ns = (int(v) for v in rng.integers(1, 3000, 2))
		p = (int(rng.integers(0, 50)), int(rng.integers(0, 50)), float(rng.choice([0, 0.02, 0.05, 0.1, 1 / 3, rng.random(), 1])), int(rng.integers(0, 50)),
			 int(rng.integers(0, 50)), float(rng.choice([0, 0.08, 0.15, 0.3, rng.random(), 1])))
		thr = qc_thresholds(p, nt, ns)
		assert thr == qc_numpy.thresholds(p, nt, ns) and all(isinstance(v, int) and v >= 0 for v in thr)
		t = np.arange(0, max(nt, ns) + 60)
		for i, bound in enumerate((p[0], p[1], p[2] * ns, p[3], p[4], p[5] * nt)):
			assert np.array_equal(t >= bound, t >= thr[i])


def test_numpy_restatement_of_qc_reads_matches_the_reference(golden):
	g = golden('G20_qc')
	for name, (it, ng, nc) in CASES.items():
		genes, cells, n = qc_numpy.qc_reads(g[name + '_reads'], tuple(g[name + '_params']))
		assert np.array_equal(genes, g[name + '_genes']) and np.array_equal(cells, g[name + '_cells'])
		assert n == int(g[name + '_iterations']) == it and (len(genes), len(cells)) == (ng, nc)
		assert g[name + '_genes'].dtype == np.int64
	with pytest.raises(RuntimeError, match='All genes'):
		qc_numpy.qc_reads(g['b_reads'], (10**9, 0, 0, 10**9, 0, 0))


def test_qc_outlier_matches_the_reference(golden):
	from normalisr_amd import qc
	g = golden('G20_qc')
	w = g['w']
	for key, pcut in (('w_pass_1e10', 1e-10), ('w_pass_1e3', 1e-3)):
		got = qc.qc_outlier(w, pcut=pcut)
		assert got.dtype == np.bool_ and got.shape == w.shape and np.array_equal(got, g[key])
		ref, steps, margin = qc_numpy.qc_outlier(w, pcut)
		assert np.array_equal(ref, g[key]) and margin > 1e-6  # (no cell near the cut: rounding cannot change a boolean)
	assert (~g['w_pass_1e10']).sum() == 12 and (~g['w_pass_1e3']).sum() == 25
	import torch
	assert np.array_equal(qc.qc_outlier(torch.from_numpy(w)), g['w_pass_1e10'])  # (a tensor is copied out)
	assert abs(qc._two_sided_z(0.05) - 1.959963984540054) < 1e-12


def test_qc_outlier_errors(golden):
	from normalisr_amd import qc
	w = golden('G20_qc')['w']
	for ka in (dict(pcut=0), dict(pcut=1), dict(pcut=-0.1)):
		with pytest.raises(ValueError, match='pcut'):
			qc.qc_outlier(w, **ka)
	for ka in (dict(outrate=0), dict(outrate=0.5), dict(outrate=0.7)):
		with pytest.raises(ValueError, match='outrate'):
			qc.qc_outlier(w, **ka)
	for bad in (0.0, -1.0):
		v = w.copy()
		v[17] = bad
		with pytest.raises(ValueError, match='Non-positive'):
			qc.qc_outlier(v)
	# more than 2 * outrate of the cells far out on one side: the fit ends with them as outliers and the final check raises
	rng = np.random.default_rng(5)
	v = np.exp(rng.normal(0, 0.05, 2000))
	v[:100] *= 50.0  # 5 % of the cells
	assert (~qc_numpy.qc_outlier(v, pcut=0.5, outrate=0.02)[0]).mean() > 0.04
	with pytest.raises(RuntimeError, match='Fitted outlier rate'):
		qc.qc_outlier(v, pcut=0.5, outrate=0.02)


def test_text_lists_round_trip(tmp_path):
	from normalisr_amd import run
	names = ['GeneA', 'b c', 'ENSG0001.5', 'x']
	f = str(tmp_path / 'names.txt')
	text = run.file_write_txtlist(f, names)
	assert text == os.linesep.join(names) and open(f).read() == text
	got = run.file_read_txtlist(f)
	assert isinstance(got, np.ndarray) and list(got) == names
	with open(f, 'w') as fh:
		fh.write('  one \n\n two\t\n\nthree')
	assert list(run.file_read_txtlist(f)) == ['one', 'two', 'three']
	assert list(got[np.array([True, False, True, False])]) == ['GeneA', 'ENSG0001.5'] and list(got[np.array([3, 0])]) == ['x', 'GeneA']


def test_command_line_checks_before_any_device_call(tmp_path):
	from normalisr_amd import run
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('m.tsv'), np.arange(12).reshape(3, 4), delimiter='\t', fmt='%i')
	run.file_write_txtlist(f('rows.txt'), ['r0', 'r1', 'r2'])
	run.file_write_txtlist(f('cols.txt'), ['c0', 'c1', 'c2', 'c3'])
	run.file_write_txtlist(f('missing.txt'), ['r0', 'nope', 'nada'])
	run.file_write_txtlist(f('twice.txt'), ['r0', 'r0'])
	base = dict(matrix_in=f('m.tsv'), matrix_out=f('out.tsv'), r=None, c=None, nodummy=False, sparse=False)
	with pytest.raises(ValueError, match='row \\(-r\\) or column \\(-c\\)'):
		run.subset(dict(base))
	with pytest.raises(ValueError, match='nodumy'):
		run.subset(dict(base, r=[f('rows.txt'), f('rows.txt')], c=[f('cols.txt'), f('cols.txt')], nodummy=True))
	with pytest.raises(ValueError, match='Subset row names not found: nope,nada'):
		run.subset(dict(base, r=[f('rows.txt'), f('missing.txt')]))
	with pytest.raises(ValueError, match='Subset column names not found'):
		run.subset(dict(base, c=[f('cols.txt'), f('missing.txt')]))
	with pytest.raises(AssertionError):
		run.subset(dict(base, r=[f('cols.txt'), f('rows.txt')]))  # four names for three rows
	with pytest.raises(AssertionError):
		run.subset(dict(base, r=[f('rows.txt'), f('twice.txt')]))
	qc = dict(reads_in=f('m.tsv'), genes_in=f('rows.txt'), cells_in=f('cols.txt'), genes_out=f('go.txt'), cells_out=f('co.txt'), n_gene=0, nc_gene=0, ncp_gene=0,
			  n_cell=0, nt_cell=0, ntp_cell=0, sparse=False)
	with pytest.raises(ValueError, match='Gene count'):
		run.qc_reads(dict(qc, genes_in=f('cols.txt')))
	with pytest.raises(ValueError, match='Cell count'):
		run.qc_reads(dict(qc, cells_in=f('rows.txt')))
	with pytest.raises(ValueError, match='non-negative'):
		run.qc_reads(dict(qc, n_cell=-3))
	np.savetxt(f('w.tsv'), np.ones(5), fmt='%.8G')
	with pytest.raises(ValueError, match='Cell count'):
		run.qc_outlier(dict(weights_in=f('w.tsv'), cells_in=f('cols.txt'), cells_out=f('co.txt'), pcut=1e-10, outrate=0.02))


def test_library_declares_the_qc_entries():
	from normalisr_amd import _lib
	lib = _lib.load()
	names = ('nrm_qc_stats_workspace', 'nrm_qc_stats', 'nrm_qc_csr_stats', 'nrm_qc_decide', 'nrm_subset_dense', 'nrm_subset_csr_count', 'nrm_subset_csr_scan',
			 'nrm_subset_csr_write')
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	for name in names:
		assert name in _lib.exported_symbols() and hasattr(lib, name) and name + '(' in hdr
	assert lib.nrm_qc_stats_workspace(33, 1000) == 2 * 1000 and lib.nrm_qc_stats_workspace(1, 7) == 7
	# argument checks of the entries answer before any launch
	assert lib.nrm_qc_stats(0, _lib.NRM_I32, 4, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0) == _lib.NRM_E_ARG
	assert lib.nrm_subset_dense(8, 3, 4, 4, 4, 0, 4, 0, 4, 8, 4, 0) == _lib.NRM_E_ARG  # three-byte elements
	thr = np.array([0, 0, 0, 0, -1, 0], dtype=np.int64)
	assert lib.nrm_qc_decide(8, 8, 8, 8, 4, 4, thr.ctypes.data, 8, 8, 8, 0) == _lib.NRM_E_ARG


def test_facade_points_at_the_new_module():
	import normalisr_amd.normalisr as norm
	for name in ('qc_reads', 'qc_outlier'):
		with pytest.raises(NotImplementedError, match='normalisr_amd.qc'):
			getattr(norm, name)
	import normalisr_amd.qc as qc
	assert all(callable(getattr(qc, name)) for name in ('qc_reads', 'qc_outlier', 'subset'))
