"""The resident coex plan of the C ABI (include/normalisr_hip.h: nrm_coex_plan_*, nrm_covariates_pinv) as far as it goes without a GPU: what is declared is
exported, normalisr_amd.cplan binds it without torch, create refuses bad arguments in the reference's words before any device call, and the library's own
pseudo-inverse of dc dc^T agrees with association.inv_rank on the covariates of the golden fixtures."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from cabi_harness import ROOT, assert_plan_names, binds_without_torch, build_and_run_host_program
from cabi_harness import vp as _vp
from normalisr_amd import _lib
from normalisr_amd.association import inv_rank

PLAN_CALLS = ('create', 'upload', 'step', 'check', 'results', 'device_results', 'stream', 'info', 'time', 'destroy')


def test_c_entry_plan_names_declared_and_exported():
	assert_plan_names('nrm_coex_plan_', PLAN_CALLS, ('nrm_covariates_pinv', 'nrm_cache_bytes'))
	import normalisr
	import normalisr_amd
	assert 'cplan' in normalisr_amd.__all__ and 'cplan' in normalisr.__all__
	assert normalisr.cplan is sys.modules['normalisr_amd.cplan']


def test_cplan_imports_without_torch():
	"""A child in which `import torch` fails: the module, its classes and the library's signatures are all there, and torch was never asked for by name."""
	binds_without_torch(('CoexPlan', 'DeviceMatrix'), (), 'nrm_coex_plan_destroy')
	src = open(os.path.join(ROOT, 'normalisr_amd', 'cplan.py')).read()
	assert not re.search(r'^\s*(import|from)\s+torch', src, re.M)


def _create(dt, ng, n, dc, nc, dci, rank, dimreduce):
	lib = _lib.load()
	h = ctypes.c_void_p()
	rc = lib.nrm_coex_plan_create(ctypes.byref(h), _vp(dt), _lib.NRM_F64, ng, n, n, 0, _vp(dc), _lib.NRM_F64, nc, _vp(dci), rank, dimreduce, _lib.NRM_F64)
	return rc, lib.nrm_last_error().decode(), h


def test_c_entry_plan_create_refuses_bad_arguments_before_any_device_call():
	"""No GPU here: an answer of NRM_E_ARG (not NRM_E_DEVICE) with the reference's words shows the checks come first (association.py:199-216)."""
	n = 12
	dt, dc = np.ones((3, n)), np.vstack([np.ones(n), np.arange(n, dtype=np.float64)])
	dci, rank = inv_rank(dc @ dc.T)
	cases = [
		(_create(dt, 0, n, dc, 2, dci, rank, 0), 'Incorrect dx/dy/dc size.'),  # ng = 0
		(_create(None, 3, n, dc, 2, dci, rank, 0), 'Incorrect dx/dy/dc size.'),  # a null matrix
		(_create(dt, 3, n, dc, 2, dci, 3, 0), 'dcr higher than covariate dimension.'),  # rank > nc
		(_create(dt, 3, n, dc, 2, dci, rank, n - rank - 1), 'Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.'),
		(_create(dt, 3, 3, dc[:, :3].copy(), 2, None, 0, 0), 'Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.'),  # the library's own rank
		(_create(dt, 3, n, dc, 2, dci, -1, 0), 'Negative dcr detected.'),
	]
	for (rc, msg, h), want in cases:
		assert rc == _lib.NRM_E_ARG and msg == want and h.value is None, (rc, msg, want)
	lib = _lib.load()
	assert lib.nrm_coex_plan_destroy(None) == 0  # destroy(NULL) is fine
	for call in ('step', 'upload'):  # a null plan is an argument error, not a crash
		assert getattr(lib, 'nrm_coex_plan_' + call)(None, None) == _lib.NRM_E_ARG
	from normalisr_amd import cplan
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.CoexPlan(dt, dc[:, :5])
	with pytest.raises(ValueError, match='Insufficient number of cells'):
		cplan.CoexPlan(dt[:, :3], dc[:, :3])


def _pinv(dc, tol=1e-8):
	dc = np.ascontiguousarray(dc)
	nc, n = dc.shape
	dci = np.full((nc, nc), -7.)
	rank = ctypes.c_int(-1)
	rc = _lib.load().nrm_covariates_pinv(_vp(dc) if nc else None, _lib.NRM_F64 if dc.dtype == np.float64 else _lib.NRM_F32, nc, n, tol, _vp(dci) if nc else None, ctypes.byref(rank))
	return rc, dci, rank.value


def _covariate_sets(golden):
	g1, g2, g11 = golden('G1_c1'), golden('G2_edge'), golden('G11_i8hard')
	return [('G1 dc', g1['dc'], 2), ('G2 dc', g2['dc'], 3), ('G2 rd_dc', g2['rd_dc'], int(g2['rd_rank'])), ('G11 dc_intercept', g11['dc_intercept'], 1),
			('G11 dc_onehot', g11['dc_onehot'], 4), ('G11 dc_collinear', g11['dc_collinear'], 3)]


def test_c_entry_covariates_pinv_against_inv_rank(golden):
	"""Equal integer ranks, pseudo-inverses within 1e-10 of their largest entry (the two SVDs themselves were measured to differ by at most 1.4e-12, on G11's
	collinear set).  The figures are printed before they are held to the bound."""
	for name, dc, want_rank in _covariate_sets(golden):
		ref, ref_rank = inv_rank(np.matmul(dc, dc.T))
		rc, dci, rank = _pinv(dc)
		err = np.abs(dci - ref).max() / np.abs(ref).max()
		print('{}: rank {} (inv_rank {}), relative error of the pseudo-inverse {:.2e}'.format(name, rank, ref_rank, err))
		assert rc == 0 and rank == ref_rank == want_rank, name
		assert err <= 1e-10, (name, err)
		assert (dci == dci.T).all()


def _g4_covariates(g):
	"""The covariates behind G4's matrices, by the recipe that made them (tests/golden/make_golden.py: g4, seeded), each held to the stored matrix; m3 was
	built from singular values, not from covariates: its symmetric square root stands in."""
	rng = np.random.default_rng(4)
	a = rng.normal(size=(6, 50))
	b = np.vstack([a[:4], a[0] + a[1], 3 * a[2]])
	q, _ = np.linalg.qr(rng.normal(size=(5, 5)))
	a21 = rng.normal(size=(21, 400))
	a21[-1] = 1.
	w, v = np.linalg.eigh(g['m3'])
	root3 = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
	sets = [a, b, np.array([[np.sqrt(2.5)]]), root3, np.ones((3, 1)), a21]
	assert len(sets) == int(g['ncase'])
	for i, dc in enumerate(sets):
		assert np.allclose(dc @ dc.T, g['m%d' % i], rtol=1e-12, atol=1e-15), i
	return sets


def test_c_entry_covariates_pinv_on_the_golden_matrices_of_inv_rank(golden):
	"""G4 (reference inv_rank: m -> mi, rank; every matrix is at most 21 x 21): equal ranks on all six, the golden rank included, and every pseudo-inverse held to a
	bound.  Five of them: 1e-10 of the largest entry, against inv_rank and against the golden mi.  m3 is the fixture's tol-boundary matrix (singular values 1, 1e-3,
	2e-8, 5e-9, 1e-12; the third is the last kept), and 1e-10 is below what two correct answers can agree to there: each side inverts C C^T as ITS fp64 arithmetic
	rounded it -- a sum of nc products, (nc + 1) u of the largest entry at most (u = 2^-53), and LAPACK delivers singular values to a few u of the largest on top --,
	and for matrices of equal rank |A^+ - B^+| <= 3 |A^+| |B^+| |A - B| (Wedin), i.e. relative to |M^+| = 1 / s_kept at most 3 (s_max / s_kept) (nc + 1) u =
	3 x 5e7 x 6 x 1.1e-16 = 1.0e-7.  That is m3's bound, against inv_rank and against the golden mi (measured: 2.3e-9 and 1.7e-8); the Moore-Penrose conditions
	M P M = M and P M P = P are held to it as well, so a pseudo-inverse that is wrong but of rank 3 does not pass.  Figures are printed before they are asserted."""
	g = golden('G4_invrank')
	u = 2.0 ** -53
	for i, dc in enumerate(_g4_covariates(g)):
		m = np.matmul(dc, dc.T)
		ref, ref_rank = inv_rank(m)
		rc, dci, rank = _pinv(dc)
		err = np.abs(dci - ref).max() / np.abs(ref).max()
		err_golden = np.abs(dci - g['mi%d' % i]).max() / np.abs(g['mi%d' % i]).max()
		s = np.linalg.svd(m, compute_uv=False)
		bound = 1e-10 if i != 3 else 3 * (s[0] / s[rank - 1]) * (dc.shape[0] + 1) * u
		mpm = np.abs(m @ dci @ m - m).max() / np.abs(m).max()
		pmp = np.abs(dci @ m @ dci - dci).max() / np.abs(dci).max()
		print('G4 m{}: {} covariates, rank {} (inv_rank {}, golden {}); pseudo-inverse against inv_rank {:.2e}, against the golden {:.2e}, M P M - M {:.2e}, P M P - P {:.2e}; bound {:.2e}'.format(
			i, dc.shape[0], rank, ref_rank, int(g['r%d' % i]), err, err_golden, mpm, pmp, bound))
		assert rc == 0 and rank == ref_rank == int(g['r%d' % i]), i
		assert err <= bound and err_golden <= bound, (i, err, err_golden, bound)
		assert mpm <= max(bound, 1e-10) and pmp <= max(bound, 1e-10), (i, mpm, pmp)
		assert (dci == dci.T).all()


def test_c_entry_covariates_pinv_dtypes_and_limits(golden):
	dc = golden('G2_edge')['rd_dc']
	dc32 = dc.astype(np.float32)
	rc, a, ra = _pinv(dc32)
	rc2, b, rb = _pinv(dc32.astype(np.float64))
	assert rc == 0 and rc2 == 0 and ra == rb and np.array_equal(a, b)  # fp32 covariates: the fp64 answer of the converted values
	rc, dci, rank = _pinv(np.ones((33, 40)))
	assert rc == _lib.NRM_E_UNSUPPORTED and (dci == -7.).all()
	with pytest.raises(NotImplementedError):
		_lib.check(rc)
	rc, dci, rank = _pinv(np.zeros((0, 40)))
	assert rc == 0 and rank == 0  # nothing to write
	rc, dci, rank = _pinv(np.zeros((3, 40)))
	assert rc == 0 and rank == 0 and (dci == 0).all()  # all-zero covariates: rank 0 (association._prepare_covariates)


def test_covariates_pinv_under_address_and_ub_sanitizers(tmp_path):
	"""The new arithmetic of csrc/nrm_host_math.h and its entry in csrc/nrm_small_pinv.hip, built by g++ with -fsanitize=address,undefined beside a program with its own
	main (tests/host/covariates_pinv_sanitize.cpp) and run directly: nothing loaded into python is run under a sanitizer."""
	build_and_run_host_program(tmp_path, ['normalisr_amd/csrc/nrm_small_pinv.hip', 'tests/host/covariates_pinv_sanitize.cpp'], 'covariates pinv ok')
