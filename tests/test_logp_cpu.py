"""logp=True (ln P from the single=0 sweeps) without a GPU: the new entries exist in the header, the ctypes table and the library;
every caller outside single=0 refuses the keyword before any device call; the command line takes --logp; the text printer writes -inf as numpy.savetxt
does; and the G25 fixtures hold what their generator says they hold."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from normalisr_amd import _lib

ENTRIES = ('nrm_logpvalues_from_r2', 'nrm_assoc_sweep_pk', 'nrm_assoc_sweep_band_pk', 'nrm_assoc_sweep_mirror_pk', 'nrm_de_small_sweep_pk', 'nrm_association_tests_host_pk')


def test_new_entries_in_header_ctypes_table_and_library():
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	lib = ctypes.CDLL(_lib.LIB_PATH)
	for name in ENTRIES:
		assert re.search(r'\bint ' + name + r'\s*\(', hdr), name
		assert name in _lib._SIGNATURES, name
		assert hasattr(lib, name), name
	# one more int (p_kind) than the entry each forwards from, in front of the stream where there is one
	for new, old in (('nrm_assoc_sweep_pk', 'nrm_assoc_sweep'), ('nrm_assoc_sweep_band_pk', 'nrm_assoc_sweep_band'), ('nrm_assoc_sweep_mirror_pk', 'nrm_assoc_sweep_mirror'),
					 ('nrm_de_small_sweep_pk', 'nrm_de_small_sweep')):
		a, b = _lib._SIGNATURES[new][0], _lib._SIGNATURES[old][0]
		assert a == b[:-1] + [ctypes.c_int32] + b[-1:], new
	a, b = _lib._SIGNATURES['nrm_association_tests_host_pk'][0], _lib._SIGNATURES['nrm_association_tests_host'][0]
	assert a == b + [ctypes.c_int32]
	assert _lib._SIGNATURES['nrm_logpvalues_from_r2'] == _lib._SIGNATURES['nrm_pvalues_from_r2']


def test_p_kind_is_validated_before_any_launch():
	lib = _lib.load()
	one = np.ones(1)
	for kind in (2, -1):
		rc = lib.nrm_assoc_sweep_pk(one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, 1, 1, 10, 5.0, 0, 0, one.ctypes.data, one.ctypes.data, 0, 0, _lib.NRM_F64, 1, 0, 0, 0, 0,
									0.0, kind, 0)
		assert rc != 0
		with pytest.raises(Exception, match='p_kind'):
			_lib.check(rc)


def _no_device(monkeypatch):
	"""Any attempt to reach the engine or the library's whole-problem entries fails the test."""
	from normalisr_amd import association, engine

	def boom(*a, **k):
		raise AssertionError('a device call was made')
	monkeypatch.setattr(engine, 'get_engine', boom)
	monkeypatch.setattr(association, '_use_host_entry', boom)
	monkeypatch.setattr(_lib, 'load', boom)


@pytest.mark.parametrize('single', [1, 4, 5])
def test_association_tests_refuses_logp_outside_single0(single, monkeypatch):
	from normalisr_amd.association import association_tests
	from normalisr_amd.de import de
	_no_device(monkeypatch)
	rng = np.random.default_rng(0)
	dx, dy, dc = (rng.random((3, 50)) < 0.2).astype(float), rng.normal(size=(4, 50)), np.ones((1, 50))
	ka = dict(mask=np.ones((3, 4), dtype=bool)) if single == 5 else {}
	with pytest.raises(NotImplementedError, match='single=0'):
		association_tests(dx, dy, dc, single=single, logp=True, **ka)
	if single != 5:
		with pytest.raises(NotImplementedError, match='single=0'):
			de(dx, dy, dc, single=single, logp=True)


def test_plans_levels_and_sharded_entries_refuse_logp(monkeypatch):
	from normalisr_amd import cplan, distributed, levels, single1, single4
	import normalisr
	_no_device(monkeypatch)
	x, y, c = np.ones((2, 8)), np.ones((3, 8)), np.ones((1, 8))
	calls = [lambda: cplan.CoexPlan(y, c, logp=True), lambda: cplan.DePlan(x, y, c, logp=True), lambda: cplan.Single1Plan(x, y, c, logp=True),
			 lambda: cplan.Single4Plan(x, y, c, logp=True), lambda: single1.Single1Plan(x, y, c, logp=True), lambda: single4.Single4Plan(x, y, c, logp=True),
			 lambda: levels.CoexLevels(y, c, logp=True), lambda: levels.coex_levels(y, c, ['a', 'b', 'c'], {}, 0.1, logp=True),
			 lambda: distributed.coex(y, c, logp=True), lambda: distributed.coex_binnet(y, c, 0.1, logp=True), lambda: distributed.de(x, y, c, logp=True),
			 lambda: distributed.CoexPlan(y, c, logp=True), lambda: distributed.DePlan(x, y, c, logp=True),
			 lambda: normalisr.levels.coex_levels(y, c, ['a', 'b', 'c'], {}, 0.1, logp=True)]
	for call in calls:
		with pytest.raises(NotImplementedError, match='logp=True is available for single=0'):
			call()


def test_public_signatures_carry_logp():
	import inspect
	import normalisr
	from normalisr_amd.association import association_tests
	assert inspect.signature(association_tests).parameters['logp'].default is False
	assert normalisr.association.association_tests is association_tests
	for f in (normalisr.coex.coex, normalisr.de.de):
		assert 'logp=True' in f.__doc__
	from normalisr_amd import binnet
	for f in (binnet.bh, binnet.binnet):
		assert 'logarithms' in f.__doc__


def test_cli_parsers_accept_logp():
	from normalisr_amd.__main__ import build_parser, main
	from normalisr_amd import run
	p = build_parser()
	assert vars(p.parse_args(['coex', 'e', 'c', 'p', '--logp']))['logp'] is True
	assert vars(p.parse_args(['coex', 'e', 'c', 'p']))['logp'] is None
	assert vars(p.parse_args(['de', 'd', 'e', 'c', 'p', 'l', '--logp']))['logp'] is True
	assert vars(p.parse_args(['de', 'd', 'e', 'c', 'p', 'l']))['logp'] is None
	for cmd in ('de', 'coex'):
		assert run.COMMANDS[cmd]['options']['logp'] == ('logp', bool)
	with pytest.raises(NotImplementedError, match='one GPU'):
		main(['coex', 'e', 'c', 'p', '--logp', '--gpus', '2'])


def test_text_printer_writes_infinities_as_savetxt_does(tmp_path):
	"""The check that the printer writes -inf as numpy.savetxt does: it did before ln P existed (-INF for '%.8G'), so this test passes without the feature
	too -- it pins what `--logp` relies on, it is not one of the tests that fail without it."""
	import io
	from normalisr_amd import run
	for dtype in (np.float32, np.float64):
		a = np.array([[-np.inf, -9.1e6, -0.0], [-745.5, np.inf, -1e-300 if dtype == np.float64 else -1e-30]], dtype=dtype)
		f = str(tmp_path / ('m%d.tsv' % np.dtype(dtype).itemsize))
		run.file_write_tsv(f, a)
		ref = io.BytesIO()
		np.savetxt(ref, a, delimiter='\t', fmt=run.fmt_float)
		assert open(f, 'rb').read() == ref.getvalue()
		assert b'-INF' in ref.getvalue()
		back = run.file_read_tsv(f)
		assert np.array_equal(back, np.loadtxt(f, delimiter='\t', ndmin=2)) and np.isneginf(back[0, 0]) and np.isposinf(back[1, 1])


def test_logp_assertion_of_de():
	from normalisr_amd.de import _logp_within
	assert _logp_within(np.array([[-np.inf, -9e6, 0.0]]))
	assert not _logp_within(np.array([[-1.0, np.nan]]))
	assert not _logp_within(np.array([[-1.0, 1e-300]]))
	big = np.full((600, 600), -3.0, dtype=np.float32)
	assert _logp_within(big)
	big[599, 599] = np.nan
	assert not _logp_within(big)
	big[599, 599] = -np.inf
	assert _logp_within(big)


def test_fixtures_hold_what_they_say():
	for name in ('G25_logp_grid.npz', 'G25_logp_case.npz'):
		assert os.path.getsize(os.path.join(GOLDEN, name)) < 1000000, name
	g = np.load(os.path.join(GOLDEN, 'G25_logp_grid.npz'))
	r2, dof, lnp = g['r2'], g['dof'], g['lnp']
	assert r2.shape == dof.shape == lnp.shape and r2.size > 500
	assert np.isfinite(lnp).all() and (lnp <= 0).all() and ((r2 > 0) & (r2 < 1)).all()
	assert set(np.unique(dof)) == {16.0, 17.0, 30.0, 100.0, 996.0, 9996.0, 49990.0, 99980.0, 499996.0}
	assert lnp.min() < -8e6 and (lnp < -745.2).sum() > 50  # far beyond where exp() underflows
	for v in (0.5, 0.9, 0.99, 0.999999, 1.0 - 2.0**-52, 1e-300, 5e-324):
		assert (r2 == v).sum() >= 9, v  # (every dof; the alpha u grid may land on one of them as well)
	assert (lnp[(r2 == 1e-300) | (r2 == 5e-324)] == 0).all()  # x = fl(1 - R^2) = 1
	for d in np.unique(dof):
		m = dof == d
		assert (r2[m] < 0.25).any() and (r2[m] > 0.25).any()
		u = -np.log1p(-r2[m])
		assert (u < 1.5).any() and (u > 1.5).any()
	alpha_u = (dof / 2 - 0.25) * -np.log1p(-r2)
	for d in (9996.0, 49990.0, 99980.0, 499996.0):  # the extension beyond G12's alpha u <= 740
		for z in (1e3, 1e4):
			assert (np.abs(alpha_u[dof == d] / z - 1) < 1e-9).any(), (d, z)
	assert (np.abs(alpha_u[dof == 499996.0] / 1e6 - 1) < 1e-9).any() and (np.abs(alpha_u[dof == 99980.0] / 1e5 - 1) < 1e-9).any()
	c = np.load(os.path.join(GOLDEN, 'G25_logp_case.npz'))
	dt, dc, dg, coex, de = c['dt'], c['dc'], c['dg'], c['lnp_coex'], c['lnp_de']
	assert dt.shape == (70, 2100) and dt.dtype == np.float32 and dc.shape == (4, 2100) and dg.shape == (5, 2100)
	assert coex.shape == (70, 70) and de.shape == (5, 70) and int(c['dof']) == 2100 - 1 - 4
	assert (dc[3] == 1).all() and 0 < (dg != 0).mean() <= 1 / 16
	assert np.array_equal(coex, coex.T) and np.isneginf(np.diag(coex)).all()
	off = ~np.eye(70, dtype=bool)
	i, j = c['dup']
	assert np.array_equal(dt[i], dt[j]) and c['r2_coex'][i, j] > 1 - 1e-12
	keep = off.copy()
	keep[i, j] = keep[j, i] = False
	assert np.isfinite(coex[keep]).all() and (coex[keep] <= 0).all() and np.isfinite(de).all() and (de <= 0).all()
	(a0, b0), (a1, b1), (a2, b2) = c['planted_pairs']
	for (a, b), lo, hi in (((a0, b0), 0.5, 0.7), ((a1, b1), 0.85, 0.95)):
		assert lo < c['r2_coex'][a, b] < hi
		assert coex[a, b] < -745.2 and np.exp(coex[a, b]) == 0.0  # the planted linear zeros: P is exactly 0 in double precision, ln P is a number
	assert 0.5e-4 < 1 - c['r2_coex'][a2, b2] < 2e-4
	k = int(c['constant'])
	assert (dt[k] == dt[k, 0]).all() and (np.delete(coex[k], k) == 0).all() and (de[:, k] == 0).all()  # variance 0 -> 1: R^2 = 0, P = 1
	assert ((coex > -3) & off).sum() > 1000 and ((coex < -5) & (coex > -200)).sum() >= 10
