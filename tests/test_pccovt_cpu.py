"""CPU-only checks of the top-PC covariate (normalisr_amd/gocovt.py, the principal / pccovt sub-commands): the numpy restatement of tests/pc_numpy.py -- the
independent check of the GPU tests -- against what the reference returned (golden G21, tests/golden/make_g21.py: cases on which ten calls of the reference's
randomized SVD agree with the exact component to 1e-11), the principal-gene selection against the reference's lists, every argument error before any device
call, the parser, the facade and the import shim."""
import os

import numpy as np
import pytest

import pc_numpy
from conftest import ROOT
from pc_numpy import g21_case, rel

FP64_CASES = ('c1', 'c2', 'c3', 'c4')


@pytest.mark.parametrize('name', FP64_CASES + ('c5', ))
def test_numpy_restatement_matches_the_reference(golden, name):
	g = golden('G21_pccovt')
	dt, dc, namet, genes, idx, cond, want = g21_case(g, name)
	assert want.shape == (dc.shape[0] + 1, dt.shape[1]) and np.array_equal(want[:-1], dc)
	where = dict(zip(namet, range(len(namet))))
	assert np.array_equal(idx, [where[x] for x in genes])  # (the last of equal names)
	score = pc_numpy.pccovt(dt, dc, idx, condcov=cond)
	err = rel(score, want[-1])
	print(name, 'pc_numpy float64 against the reference: %.3g' % err)
	assert err < (1e-6 if name == 'c5' else 1e-9)
	assert want.dtype == (np.float32 if name == 'c5' else np.float64)


def test_fixture_is_what_the_issue_describes(golden):
	g = golden('G21_pccovt')
	assert g['c1_dt'].shape == (40, 257) and len(g['c1_idx']) == 7 and g['c1_dc'].shape == (8, 257)
	assert g['c2_dt'].shape == (64, 333) and len(g['c2_idx']) == 9 and g['c2_dc'].shape == (0, 333)
	assert g['c3_code'].shape == (300, 2000) and len(g['c3_idx']) == 200 and g['c3_code'].dtype == np.int8
	assert len(g['c4_idx']) == 9 and np.array_equal(g['c4_idx'], g['c5_idx'])
	assert abs(float(g['c1_ratio']) - 0.5) < 0.05 and abs(float(g['c3_ratio']) - 0.1) < 0.02
	assert len(set(g['c1_idx'])) < len(g['c1_idx']) and len(set(g['c1_namet'])) < 40  # a gene twice in genes, a name twice in namet
	dc = g['c3_dc']
	assert np.array_equal(dc[:4].sum(axis=0), np.ones(2000)) and (dc[7] == 1).all()  # one-hot batches beside the intercept: rank deficient


def test_restatement_is_carried_to_the_rounding_of_its_type():
	"""float64 against longdouble on a small case: the distance the GPU tests take their allowance from is of the order of float64's rounding.  The
	restatement iterates from the package's own start vector and resolves genes as the package does, so both are held to the same component."""
	from normalisr_amd import gocovt
	for k in (1, 6, 260):
		assert np.array_equal(gocovt._start_vector(k), pc_numpy.start(k, np.float64))
	assert np.array_equal(gocovt._gene_rows(4, ['a', 'b', 'a', 'c'], ['c', 'a', 'a']), [3, 2, 2]) and np.array_equal(gocovt._gene_rows(4, None, [-1, 0]), [3, 0])
	rng = np.random.default_rng(3)
	n, m = 130, 6
	dc = np.concatenate([rng.normal(size=(2, n)), np.ones((1, n))])
	dt = rng.normal(size=(m, n)) + 0.8 * rng.choice([-1, 1], m)[:, None] * rng.normal(size=n)[None, :] + 5
	idx = np.arange(m)
	a = pc_numpy.pccovt(dt, dc, idx, ft=np.float64)
	b, v, lam, z = pc_numpy.pccovt(dt, dc, idx, ft=np.longdouble, return_all=True)
	assert b.dtype == np.longdouble and rel(a, b.astype(np.float64)) < 1e-13
	top = int(np.argmax(np.abs(v)))
	assert v[top] > 0 and abs(float((b * b).sum()) - float(lam) * n) < 1e-12 * float(lam) * n  # |score|^2 = sigma_1^2
	s = np.linalg.svd(np.asarray(z, dtype=np.float64), full_matrices=False)
	lapack = s[2][0] * s[1][0] * np.sign(s[0][top, 0])
	assert rel(a, lapack) < 1e-12  # (the exact component, by another algorithm)
	# a row of exact zeros changes nothing, and a design of deficient rank is projected off all the same
	dz = np.concatenate([dt, np.zeros((1, n))])
	assert rel(pc_numpy.pccovt(dz, dc[:0], np.arange(m + 1), condcov=False), pc_numpy.pccovt(dt, dc[:0], idx, condcov=False)) < 1e-14
	assert rel(pc_numpy.pccovt(dt, np.concatenate([dc, dc[:1] - 2 * dc[1:2]]), idx), a) < 1e-13


def test_principal_genes_of_the_restatement_match_the_reference(golden):
	from normalisr_amd.gocovt import _select_principal as select_principal
	g = golden('G21_pccovt')
	net = g['net']
	assert net.shape == (97, 97) and net.dtype == np.bool_ and np.array_equal(net, net.T)
	deg = net.sum(axis=1)
	for n in (5, 20, 60):
		want = g['principal_%d' % n]
		assert np.array_equal(pc_numpy.principal(net, n), want) and want.dtype == np.int64
		assert np.array_equal(select_principal(deg, n), want)  # (the package's host selection on the same degrees)
		assert list(g['net_names'][want]) == list(g['principal_names_%d' % n])
		assert len(want) > n  # ties at the threshold are kept
	with pytest.raises(RuntimeError, match='Not enough principal genes'):
		pc_numpy.principal(np.eye(9, dtype=bool)[::-1] & (np.arange(9) < 3)[:, None], 5)
	with pytest.raises(RuntimeError, match='Not enough principal genes'):
		select_principal(np.array([3, 2, 0, 0, 0, 0]), 2)


def test_argument_errors_before_any_device_call(monkeypatch):
	from normalisr_amd import _lib, gocovt

	def no_library():
		raise AssertionError('the library was loaded before the arguments were checked')
	monkeypatch.setattr(_lib, 'load', no_library)
	net = np.zeros((5, 5), dtype=bool)
	for bad in (np.zeros((5, 4), dtype=bool), np.zeros((1, 1), dtype=bool), np.zeros((5, ), dtype=bool), np.zeros((0, 0), dtype=bool)):
		with pytest.raises(ValueError, match='Wrong shape'):
			gocovt.principal_genes(bad, n=2)
	for n in (1, 0, 5, 6):
		with pytest.raises(ValueError, match='Number of principal genes'):
			gocovt.principal_genes(net, n=n)
	dt, dc = np.zeros((4, 6)), np.ones((2, 6))
	names = ['a', 'b', 'c', 'd']
	for empty in (np.zeros((0, 6)), np.zeros((4, 0))):
		with pytest.raises(ValueError, match='Empty normalized expression'):
			gocovt.pccovt(empty, np.ones((2, empty.shape[1])), names[:empty.shape[0]], ['a'])
	with pytest.raises(ValueError, match='Incompatible input shapes'):
		gocovt.pccovt(dt, dc[:, :5], names, ['a'])
	with pytest.raises(ValueError, match='Incompatible input shapes'):
		gocovt.pccovt(dt, dc, names[:3], ['a'])
	with pytest.raises(ValueError, match='Incompatible input shapes'):
		gocovt.pccovt(dt[0], dc, names, ['a'])
	with pytest.raises(ValueError, match='Genes not found: x,y,z,...'):
		gocovt.pccovt(dt, dc, names, ['a', 'x', 'y', 'z', 'w'])
	with pytest.raises(ValueError, match='Genes not found: 4,'):
		gocovt.pccovt(dt, dc, None, [0, 4])
	with pytest.raises(ValueError, match='integer row indices'):
		gocovt.pccovt(dt, dc, None, ['a'])
	for namet, genes in ((names, []), (None, np.zeros(0, dtype=np.int64))):
		with pytest.raises(ValueError, match='No gene'):
			gocovt.pccovt(dt, dc, namet, genes)
	with pytest.raises(ValueError, match='max_iter'):
		gocovt.pccovt(dt, dc, names, ['a'], max_iter=0)


def test_start_vector_is_fixed_and_not_constant():
	from normalisr_amd.gocovt import _start_vector as start_vector
	for m in (1, 2, 7, 260):
		v = start_vector(m)
		assert v.shape == (m, ) and v.dtype == np.float64 and abs((v * v).sum() - 1) < 1e-15 and (v > 0).all() and np.array_equal(v, start_vector(m))
		if m > 1:
			assert len(np.unique(v)) == m and abs((v * np.where(np.arange(m) % 2, -1.0, 1.0)).sum()) > 1e-3  # not orthogonal to alternating loadings


def test_parser_accepts_principal_and_pccovt_and_rejects_gocovt(capsys):
	from normalisr_amd.__main__ import build_parser
	from normalisr_amd import run
	p = build_parser()
	ns = vars(p.parse_args(['principal', 'net', 'genes', 'out']))
	assert (ns['cmd'], ns['net_in'], ns['genes_in'], ns['master_out'], ns['n']) == ('principal', 'net', 'genes', 'out', 100) and isinstance(ns['n'], int)
	assert vars(p.parse_args(['principal', 'net', 'genes', 'out', '-n', '20']))['n'] == 20
	ns = vars(p.parse_args(['pccovt', 'e', 'c', 'g', 'p', 'o']))
	assert (ns['cmd'], ns['exp_in'], ns['cov_in'], ns['genes_in'], ns['pathway_in'], ns['cov_out'], ns['nocond']) == ('pccovt', 'e', 'c', 'g', 'p', 'o', False)
	assert vars(p.parse_args(['pccovt', 'e', 'c', 'g', 'p', 'o', '--nocond']))['nocond'] is True
	with pytest.raises(SystemExit):
		p.parse_args(['gocovt', 'e', 'c', 'n', 'g', 'go', 'goa', 'o'])
	capsys.readouterr()
	text = ' '.join(p.format_help().split())
	assert 'gocovt is not provided' in text and 'principal' in text and 'pccovt' in text and 'goatools' in text
	assert callable(run.principal) and callable(run.pccovt) and not hasattr(run, 'gocovt')


def test_command_line_checks_before_any_device_call(tmp_path):
	from normalisr_amd import run
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('net.tsv'), np.zeros((4, 4), dtype=int), delimiter='\t', fmt='%i')
	run.file_write_txtlist(f('three.txt'), ['a', 'b', 'c'])
	run.file_write_txtlist(f('four.txt'), ['a', 'b', 'c', 'd'])
	with pytest.raises(ValueError, match='Wrong shape'):
		run.principal(dict(net_in=f('net.tsv'), genes_in=f('three.txt'), master_out=f('o.txt'), n=2))
	with pytest.raises(ValueError, match='Number of principal genes'):
		run.principal(dict(net_in=f('net.tsv'), genes_in=f('four.txt'), master_out=f('o.txt'), n=4))
	np.savetxt(f('e.tsv'), np.arange(20.0).reshape(4, 5), delimiter='\t', fmt='%.8G')
	np.savetxt(f('c.tsv'), np.ones((1, 5)), delimiter='\t', fmt='%.8G')
	run.file_write_txtlist(f('path.txt'), ['a', 'q'])
	with pytest.raises(ValueError, match='Genes not found: q,'):
		run.pccovt(dict(exp_in=f('e.tsv'), cov_in=f('c.tsv'), genes_in=f('four.txt'), pathway_in=f('path.txt'), cov_out=f('o.tsv'), nocond=False))
	with pytest.raises(ValueError, match='Incompatible input shapes'):
		run.pccovt(dict(exp_in=f('e.tsv'), cov_in=f('c.tsv'), genes_in=f('three.txt'), pathway_in=f('path.txt'), cov_out=f('o.tsv'), nocond=False))
	assert not os.path.exists(f('o.tsv')) and not os.path.exists(f('o.txt'))


def test_facade_still_raises_and_points_at_the_new_module():
	import normalisr_amd.normalisr as norm
	for name in ('qc_reads', 'qc_outlier', 'gotop', 'pccovt'):
		with pytest.raises(NotImplementedError):
			getattr(norm, name)
	with pytest.raises(NotImplementedError, match='normalisr_amd.gocovt.pccovt'):
		norm.pccovt
	import normalisr_amd.gocovt as gocovt
	assert callable(gocovt.pccovt) and callable(gocovt.principal_genes) and not hasattr(gocovt, 'gotop') and not hasattr(gocovt, 'goe')
	import normalisr_amd
	assert 'gocovt' in normalisr_amd.__all__ and 'qc' in normalisr_amd.__all__


def test_shim_imports_gocovt_and_qc():
	import importlib
	for name in ('gocovt', 'qc'):
		mod = importlib.import_module('normalisr.' + name)
		assert mod is importlib.import_module('normalisr_amd.' + name)
	import normalisr
	assert 'gocovt' in normalisr.__all__ and 'qc' in normalisr.__all__
	from normalisr.gocovt import pccovt, principal_genes  # noqa: F401
	from normalisr.qc import qc_reads  # noqa: F401


def test_library_declares_the_pc_entries():
	from normalisr_amd import _lib
	lib = _lib.load()
	names = ('nrm_net_degree', 'nrm_pc_correlation', 'nrm_pc_power', 'nrm_pc_score_workspace', 'nrm_pc_score')
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	for name in names:
		assert name in _lib.exported_symbols() and hasattr(lib, name) and name + '(' in hdr
	# the score pass splits the genes where the cells alone do not fill the device: scratch = m loadings + splits x n partial sums
	assert lib.nrm_pc_score_workspace(7, 96) == 7 + 1 * 96 and lib.nrm_pc_score_workspace(260, 96) > 260 + 2 * 96 and lib.nrm_pc_score_workspace(0, 5) == 0
	assert (lib.nrm_pc_score_workspace(260, 96) - 260) % 96 == 0 and lib.nrm_pc_score_workspace(40, 10**6) == 40 + 10**6
	# argument checks of the entries answer before any launch
	assert lib.nrm_net_degree(16, 4, 3, 16, 0) == _lib.NRM_E_ARG  # a pitch below the row
	assert lib.nrm_net_degree(0, 4, 4, 16, 0) == _lib.NRM_E_ARG
	assert lib.nrm_pc_correlation(16, 4, 5, 10, 16, 16, 5, 16, 0) == _lib.NRM_E_ARG  # G narrower than m
	assert lib.nrm_pc_power(16, 4, 4, 16, 16, 16, 0, 0) == _lib.NRM_E_ARG  # no steps
	assert lib.nrm_pc_score(16, 7, 3, 7, 16, 16, 16, _lib.NRM_F64, 16, 16, 0) == _lib.NRM_E_ARG  # an odd pitch
	assert lib.nrm_pc_score(24, 8, 3, 7, 16, 16, 16, _lib.NRM_F64, 16, 16, 0) == _lib.NRM_E_ARG  # rows not 16-byte aligned
	assert lib.nrm_pc_score(16, 8, 3, 7, 16, 16, 16, 5, 16, 16, 0) == _lib.NRM_E_ARG  # an output type that does not exist
