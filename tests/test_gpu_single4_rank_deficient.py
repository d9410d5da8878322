"""GPU: single=4 (`normalisr de -m covariate`) with rank-deficient covariates -- one-hot batches and an intercept, as a high-MOI screen passes
them -- takes the closed form (rows residualised with inv_rank's pseudo-inverse of C C^T, dof = n - nx - rank - dimreduce) instead of the
reference's per-grouping loop, wherever the rank certificate holds: the public call on both design routes, Single4Plan's lean graph, dy=None,
and the torch-free C entry.  Golden G17 holds the reference's own results (tests/golden/make_g17.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from cabi_harness import close, p_close
from cabi_harness import same_bars as _same
from conftest import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_host_loop(monkeypatch):
	"""The reference's per-grouping / per-pair loops on the host raise: a call that passes took the closed form."""
	from normalisr_amd import single4

	def refuse(*a, **k):
		raise AssertionError('the per-grouping algorithm on the host was taken')
	monkeypatch.setattr(single4, '_per_grouping_host', refuse)
	monkeypatch.setattr(single4, '_pairwise_host', refuse)


@pytest.mark.parametrize('route', ['auto', 'force'])
def test_g17_onehot_covariates_take_the_closed_form(golden, route, monkeypatch):
	"""G17 through norm.de / association_tests(single=4) with the host loops switched off: lowmem=False, return_dot both ways, per-gene dimreduce,
	dy=None.  route: the size rule (K1 + the fp64 Gram kernel at this size) or the sparse-design kernels (NRM_DE_SPARSE=force)."""
	import normalisr_amd.normalisr as norm
	from normalisr_amd.association import association_tests
	monkeypatch.setenv('NRM_DE_SPARSE', route)
	g = golden('G17_single4_onehot')
	dg, dt, dc = g['dg'], g['dt'], g['dc']
	with monkeypatch.context() as mp:
		_no_host_loop(mp)
		_same(norm.de(dg, dt, dc, single=4, lowmem=False), g['de_p'], g['de_gamma'], g['de_varg'], g['de_vart'], g['de_alpha'])
		for rd in (1, 0):
			got = association_tests(dg, dt, dc, single=4, lowmem=False, return_dot=bool(rd))
			_same(got, g['at%d_p' % rd], g['at%d_stat' % rd], g['at%d_vx' % rd], g['at%d_vy' % rd], g['at_alpha'])
		_same(norm.de(dg, dt, dc, single=4, dimreduce=g['dr']), g['dr_p'], g['dr_gamma'], g['dr_varg'], g['dr_vart'])
		for rd in (1, 0):
			p, d, a, vx, vy = association_tests(dt[:14], None, dc, single=4, return_dot=bool(rd))
			assert a is None and vx is None
			assert p_close(p, g['sx_p_rd%d' % rd]) and close(d, g['sx_dot_rd%d' % rd], 1e-9, 1e-12) and close(vy, g['sx_vy_rd%d' % rd], 1e-9)
	# covariates near the threshold: the certificate refuses or agrees with the reference.  A kept eigenvalue of C C^T at 2.5 tol x the largest
	# makes the problem itself ill-conditioned (rounding amplified ~1 / (2.5 tol) = 4e7 times, in the reference too): the north-star 1e-6 here
	got = norm.de(dg, dt, g['near_dc'], single=4)
	errs = [relerr(got[1], g['near_gamma'], 1e-12), relerr(got[3], g['near_varg']), relerr(got[4], g['near_vart'])]
	assert p_close(got[0], g['near_p']) and max(errs) < 1e-6, errs
	# a grouping equal to a batch indicator (X~ rank deficient given C) keeps the host loop.  Its own row is rounding noise there (x~ = 0 up to
	# rounding, in the reference too), so the reference's R^2 assertion (association.py:557) may fire on the device's Gram matrices where it did
	# not on the reference's; every other row matches the reference
	from normalisr_amd import single4
	loop, seen = single4._per_grouping_host, []
	monkeypatch.setattr(single4, '_per_grouping_host', lambda *a, **k: seen.append(1) or loop(*a, **k))
	bad = 5
	assert np.array_equal(g['bi_dg'][bad], dc[1])
	try:
		got = norm.de(g['bi_dg'], dt, dc, single=4, lowmem=False)
	except AssertionError as e:
		assert 'R^2 out of range' in str(e)
		got = None
	assert seen
	if got is not None:
		keep = np.arange(dg.shape[0]) != bad
		_same([got[0][keep], got[1][keep], got[2][keep], got[3][keep], got[4][keep]], g['bi_p'][keep], g['bi_gamma'][keep], g['bi_varg'][keep],
			  g['bi_vart'][keep], g['bi_alpha'][keep])


def test_single4_onehot_dense_route_integer_engine(monkeypatch):
	"""The dense route with the integer Gram engine and its guard (NRM_DE_SPARSE=0, fp32 rows, >= 2048 cells) on one-hot covariates: closed form,
	against the oracle's per-grouping loop."""
	from normalisr_amd.association import association_tests
	from normalisr_amd import engine
	monkeypatch.setenv('NRM_DE_SPARSE', '0')
	rng = np.random.default_rng(1717)
	nx, ny, n = 40, 80, 4096
	batch = rng.integers(0, 4, n)
	dc = np.vstack([(batch[None, :] == np.arange(4)[:, None]).astype(np.float64), rng.normal(size=(3, n)), np.ones((1, n))])
	dg = (rng.random((nx, n)) < 0.05).astype(np.float32)
	dt = (rng.normal(size=(ny, n)) + 0.5 * dg[0] + 0.3 * dg[3] + 0.4 * dc[1] - 0.2 * dc[5]).astype(np.float32)
	eng = engine.get_engine()
	assert eng.gram_slices(n) > 0  # (the integer engine takes this size)
	with monkeypatch.context() as mp:
		_no_host_loop(mp)
		got = association_tests(dg, dt, dc, single=4, lowmem=False, return_dot=False)
	want = oracle.association_tests(dg.astype(np.float64), dt.astype(np.float64), dc, single=4, lowmem=False, return_dot=False)
	assert got[0].dtype == np.float32
	ok = want[0] > 1e-30
	assert relerr(got[0][ok], want[0][ok]) < 2e-4 and close(got[1], want[1], 2e-5, 1e-6) and close(got[3], want[3], 2e-6) and close(got[4], want[4], 2e-6)
	assert close(got[2], want[2], 2e-4, 1e-5)


def test_single4_plan_goes_lean_on_onehot_covariates(monkeypatch):
	"""Single4Plan on a configs[3]-shaped sample (100 gRNAs, 45 000 cells, one-hot batches + ones): the first step decides the lean path, later
	steps are one captured graph, check() stands without fallbacks, and every replay is bit-equal to the public call."""
	import torch
	from normalisr_amd.single4 import Single4Plan, association_tests_single4
	rng = np.random.default_rng(1733)
	nx, ny, n = 100, 256, 45000
	batch = rng.integers(0, 5, n)
	dc = np.vstack([(batch[None, :] == np.arange(5)[:, None]).astype(np.float64), rng.normal(size=(2, n)), np.ones((1, n))])
	dx = (rng.random((nx, n)) < 0.01).astype(np.float32)
	dy = (rng.normal(size=(ny, n)) + 0.5 * dx[2] + 0.3 * dc[0]).astype(np.float32)
	d_x, d_y = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
	with monkeypatch.context() as mp:
		_no_host_loop(mp)
		plan = Single4Plan(d_x, d_y, dc, return_dot=False)
		plan.step()
		assert plan.lean is True and plan.dcr == dc.shape[0] - 1
		for k in range(5):
			plan.step()
			assert plan.check() and plan.fallbacks == 0
			if k >= 1:
				assert plan._graph.graph is not None
			if k >= 2:  # (replays of the captured graph)
				got = plan.results()
				pub = association_tests_single4(d_x, d_y, dc, return_dot=False)
				for a, b in zip(got, pub):
					assert (a is None and b is None) or np.array_equal(a, b)
	want = oracle.association_tests(dx[:20].astype(np.float64), dy[:64].astype(np.float64), dc, single=4, return_dot=False)
	# the closed form on a slice against the oracle's per-grouping loop on the same slice
	sub = association_tests_single4(dx[:20], dy[:64], dc, return_dot=False)
	ok = want[0] > 1e-30
	assert relerr(sub[0][ok], want[0][ok]) < 2e-4 and close(sub[1], want[1], 2e-5, 1e-6) and close(sub[4], want[4], 2e-6)


_NO_TORCH_PINV = r"""
import sys
sys.modules['torch'] = None  # `import torch` raises ImportError from here on
sys.path.insert(0, sys.argv[1])
import ctypes
import numpy as np
from normalisr_amd import _lib
from normalisr_amd.association import _prepare_covariates, association_tests
import normalisr_amd.single4 as single4
g = np.load(sys.argv[2])
dg, dt, dc = g['dg'], g['dt'], g['dc']
nx, n = dg.shape
ny, nc = dt.shape[0], dc.shape[0]
dc64, dci, dcr = _prepare_covariates(dc)
dci = np.ascontiguousarray(dci)
lib = _lib.load()
vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
out = {'dcr': dcr}
for rd in (1, 0):
	p, st, vy = (np.empty((nx, ny)) for _ in range(3))
	vx, al = np.empty(nx), np.empty((nx, ny, nc))
	out['rc%d' % rd] = lib.nrm_association_tests_single4_pinv_host(vp(dg), _lib.NRM_F64, nx, vp(dt), _lib.NRM_F64, ny, vp(dc64), _lib.NRM_F64, nc, n, vp(dci), int(dcr), 0, rd,
																	 1e-8, vp(p), vp(st), vp(al), vp(vx), vp(vy), _lib.NRM_F64)
	out['err%d' % rd] = lib.nrm_last_error().decode('utf-8', 'replace') if out['rc%d' % rd] else ''
	out.update({'p%d' % rd: p, 'st%d' % rd: st, 'vx%d' % rd: vx, 'vy%d' % rd: vy, 'al%d' % rd: al})
out['rc_full'] = lib.nrm_association_tests_single4_host(vp(dg), _lib.NRM_F64, nx, vp(dt), _lib.NRM_F64, ny, vp(dc64), _lib.NRM_F64, nc, n, vp(dci), int(dcr), 0, 1,
														1e-8, vp(p), vp(st), vp(al), vp(vx), vp(vy), _lib.NRM_F64)
out['err_full'] = lib.nrm_last_error().decode('utf-8', 'replace')
# the package's torch-free route goes through the new entry: the per-grouping loop is never reached
def refuse(*a, **k):
	raise AssertionError('per-grouping loop')
single4._per_grouping_host = refuse
res = association_tests(dg, dt, dc, single=4, lowmem=False, return_dot=False)
out.update({'pk_p': res[0], 'pk_st': res[1], 'pk_al': res[2], 'pk_vx': res[3], 'pk_vy': res[4]})
assert not any(m == 'torch' or m.startswith('torch.') for m, v in sys.modules.items() if v is not None)
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize('route', ['auto', 'force'])
def test_c_entry_single4_pinv_matches_g17_without_torch(golden, tmp_path, route):
	"""nrm_association_tests_single4_pinv_host from a process that cannot import torch: 0 on G17's one-hot covariates and the reference's results,
	return_dot both ways; the full-rank entry still answers NRM_E_UNSUPPORTED ("full-rank") for them, and association_tests takes the new entry."""
	from normalisr_amd import _lib
	g = golden('G17_single4_onehot')
	env = dict(os.environ, NRM_DE_SPARSE=route)
	r = subprocess.run([sys.executable, '-c', _NO_TORCH_PINV, ROOT, os.path.join(ROOT, 'tests', 'golden', 'G17_single4_onehot.npz'), str(tmp_path / 'out.npz')],
					   capture_output=True, text=True, timeout=600, env=env)
	assert r.returncode == 0, r.stderr[-3000:]
	o = np.load(tmp_path / 'out.npz')
	assert int(o['dcr']) == int(g['rc'])
	for rd in (1, 0):
		assert int(o['rc%d' % rd]) == 0, str(o['err%d' % rd])
		_same([o['p%d' % rd], o['st%d' % rd], o['al%d' % rd], o['vx%d' % rd], o['vy%d' % rd]], g['at%d_p' % rd], g['at%d_stat' % rd], g['at%d_vx' % rd],
			  g['at%d_vy' % rd], g['at_alpha'])
	assert int(o['rc_full']) == _lib.NRM_E_UNSUPPORTED and 'full-rank' in str(o['err_full'])
	_same([o['pk_p'], o['pk_st'], o['pk_al'], o['pk_vx'], o['pk_vy']], g['at0_p'], g['at0_stat'], g['at0_vx'], g['at0_vy'], g['at_alpha'])
