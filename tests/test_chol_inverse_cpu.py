"""nrm_chol_inverse_host (the host twin of csrc/nrm_chol_inverse.hip: the same blocked algorithm, block boundaries and status rules) and the host helper
norm._fitvar_bases, without a GPU.  Bound of the inverse: column j of N solves M x = e_j by Cholesky, so in extended precision
max |M N - I| / (|M|_inf |N|_inf) <= 4 r^2 u, the normwise bound of Higham, Accuracy and Stability, Thm 10.4, as tests/test_gpu_wide_covariates.py holds
nrm_normvar_chol to it -- a cap, not a target: the observed value is printed."""
import ctypes

import numpy as np
import pytest

from normalisr_amd import _lib
from normalisr_amd.association import inv_rank

U = 2.0**-53
SIZES = (1, 2, 63, 64, 65, 128, 129, 377)


def spd(rng, r, cond):
	"""A seeded positive definite matrix of the given condition, as test_cholesky_kernel_alone builds them."""
	q = np.linalg.qr(rng.normal(size=(r, r)))[0]
	lam = np.exp(-np.log(cond) * rng.permutation(r) / max(r - 1, 1)) * rng.uniform(0.5, 2.0)
	m = (q * lam) @ q.T
	return (m + m.T) / 2


def residual(m, n):
	ml, nl = m.astype(np.longdouble), n.astype(np.longdouble)
	return float(np.abs(ml @ nl - np.eye(m.shape[0])).max() / (np.abs(ml).sum(axis=1).max() * np.abs(nl).sum(axis=1).max()))


def host_inverse(m, ldi=None):
	lib = _lib.load()
	m = np.ascontiguousarray(m, dtype=np.float64)
	r = m.shape[0]
	ldi = ldi or r
	inv = np.full((r, ldi), np.nan)
	status = np.zeros(2, dtype=np.int32)
	before = m.copy()
	_lib.check(lib.nrm_chol_inverse_host(m.ctypes.data, m.strides[0] // 8, r, inv.ctypes.data, ldi, status.ctypes.data))
	assert np.array_equal(m, before, equal_nan=True)  # the input is not modified
	return inv, status


@pytest.mark.parametrize('r', SIZES)
def test_host_inverse_within_the_cholesky_bound(r):
	rng = np.random.default_rng(2300 + r)
	for cond in (1.0, 1e4):
		m = spd(rng, r, cond)
		inv, status = host_inverse(m)
		res = residual(m, inv)
		print('r', r, 'cond', cond, 'residual', res, 'bound', 4 * r * r * U)
		assert list(status) == [0, 0] and np.isfinite(inv).all()
		assert res <= 4 * r * r * U
		assert np.array_equal(inv, inv.T)  # symmetric bits


def test_host_inverse_takes_pitches():
	rng = np.random.default_rng(2310)
	m = spd(rng, 70, 1e4)
	wide = np.full((70, 77), np.nan)
	wide[:, :70] = m
	inv, status = host_inverse(wide[:, :70], ldi=75)
	assert list(status) == [0, 0] and np.isnan(inv[:, 70:]).all()
	assert np.array_equal(inv[:, :70], host_inverse(m)[0])


@pytest.mark.parametrize('r', (2, 65, 129))
def test_host_inverse_status(r):
	rng = np.random.default_rng(2320 + r)
	q = np.linalg.qr(rng.normal(size=(r, r)))[0]
	lam = np.ones(r)
	lam[r // 2] = -0.5
	bad = (q * lam) @ q.T
	inv, status = host_inverse((bad + bad.T) / 2)
	assert list(status) == [1, 0] and (inv == 0).all()  # an indefinite matrix: a pivot that is not positive
	for where in ((0, 0), (r - 1, 0), (r - 1, r - 1), (0, r - 1)):
		m = spd(rng, r, 10.0)
		m[where] = np.nan
		inv, status = host_inverse(m)
		assert list(status) == [0, 1] and (inv == 0).all()
	m = spd(rng, r, 10.0)
	m[r - 1, r - 1] = np.inf
	inv, status = host_inverse(m)
	assert list(status) == [0, 1] and (inv == 0).all()


def test_bad_arguments_before_any_work():
	lib = _lib.load()
	m, inv, status = np.eye(4), np.full((4, 4), 7.0), np.zeros(2, dtype=np.int32)
	p = lambda a: a.ctypes.data
	calls = [(p(m), 4, 0, p(inv), 4, p(status)), (p(m), 4, 1025, p(inv), 1025, p(status)), (p(m), 3, 4, p(inv), 4, p(status)), (p(m), 4, 4, p(inv), 3, p(status)),
			 (None, 4, 4, p(inv), 4, p(status)), (p(m), 4, 4, None, 4, p(status)), (p(m), 4, 4, p(inv), 4, None)]
	for args in calls:
		assert lib.nrm_chol_inverse_host(*args) == _lib.NRM_E_ARG, args
	assert (inv == 7.0).all() and (status == 0).all()
	# the device entry checks its arguments before any device call: no GPU is needed to be refused
	ws = np.zeros(int(lib.nrm_chol_inverse_workspace(4)))
	for args in calls:
		assert lib.nrm_chol_inverse(*args[:5], p(ws), args[5], None) == _lib.NRM_E_ARG, args
	assert lib.nrm_chol_inverse(p(m), 4, 4, p(inv), 4, None, p(status), None) == _lib.NRM_E_ARG
	assert lib.nrm_chol_inverse_workspace(0) == 0 and lib.nrm_chol_inverse_workspace(1025) == 0 and lib.nrm_chol_inverse_workspace(-3) == 0
	assert lib.nrm_chol_inverse_workspace(1) > 0 and lib.nrm_chol_inverse_workspace(1024) >= 2 * 1024 * 1024
	assert lib.nrm_fitvar_wide_workspace(100, 100, 5) == 0 and lib.nrm_fitvar_wide_workspace(2000, 1025, 5) == 0 and lib.nrm_fitvar_wide_workspace(2000, 64, 1026) == 0
	assert lib.nrm_fitvar_wide_workspace(2000, 1024, 1025) > 0


def test_fitvar_bases_on_g22(golden):
	"""The helper's rank is inv_rank's; both bases are orthonormal; B spans the covariates' rows; B1^T B1 is the projector of the second regression."""
	from normalisr_amd.norm import _fitvar_bases, _pinv_gram_unit_rows
	g = golden('G22_wide_covariates')
	for case in ('A', 'B', 'C'):
		dc = g[case + '_dc'].astype(np.float64)
		b, r, hi, lo, b1 = _fitvar_bases(dc)
		assert r == inv_rank(dc @ dc.T)[1] and b.shape == (r, dc.shape[1])
		assert 0 <= lo < 1e-8 <= hi <= 1
		assert np.abs(b @ b.T - np.eye(r)).max() < 1e-12
		assert np.abs(b1 @ b1.T - np.eye(b1.shape[0])).max() < 1e-12
		c1 = np.vstack([dc, np.ones((1, dc.shape[1]))])
		assert np.abs(b1.T @ b1 - c1.T @ _pinv_gram_unit_rows(c1) @ c1).max() < 1e-10
		proj = b.T @ b  # the rows of dc lie in the span of B, as far as the rank rule keeps them: the residual is below sqrt(tol) of the largest row
		assert np.abs(dc - dc @ proj).max() < 1e-3 * np.abs(dc).max()
		assert int(g[case + '_ranks'][0]) == r


def test_plan_refuses_covariates_without_a_certificate(golden):
	"""A covariate row plus noise of another puts an eigenvalue near the rank rule's tolerance: the plan is refused when it is made, before any device call, when
	that eigenvalue lies inside the band (tol / c, c tol) of equal weights, c = WIDE_SAFETY = 4: (2.5e-9, 4e-8) of the largest.
	The case of test_normvar_without_a_certificate_takes_the_reference_path (G22 C, row 3 + 1e-4 noise, seed 2222) has that eigenvalue at 1.60e-9 of the largest:
	inside normvar's band for the spread of w3, but BELOW the band of equal weights -- the reference's rule drops it for sure at u = 1, so the plan is made, and the
	device's per-iteration certificate refuses it from kappa = 2.5e-9 / 1.60e-9 = 1.56 on (tests/test_gpu_compute_var_plan_wide.py runs it).  Twice the noise
	(four times the eigenvalue, 6.4e-9) is inside the band of equal weights and is refused here."""
	from normalisr_amd.norm import ComputeVarPlan, _fitvar_bases, _fitvar_certified
	g = golden('G22_wide_covariates')
	dc = g['C_dc'].astype(np.float64)
	noise = np.random.default_rng(2222).normal(size=dc.shape[1])
	near = np.vstack([dc, dc[3] + 1e-4 * noise])
	b, r, hi, lo, b1 = _fitvar_bases(near)
	print('row + 1e-4 noise: rank', r, 'hi', hi, 'lo', lo)
	assert r == near.shape[0] - 1 and 1e-9 < lo < 2.5e-9
	assert _fitvar_certified(hi, lo, False, 1.0) and not _fitvar_certified(hi, lo, False, 1.6)
	with pytest.raises(ValueError):  # certified for equal weights: the next check is the one for a host array
		ComputeVarPlan(g['C_dt'], near)
	bad = np.vstack([dc, dc[3] + 2e-4 * noise])
	b, r, hi, lo, b1 = _fitvar_bases(bad)
	print('row + 2e-4 noise: rank', r, 'hi', hi, 'lo', lo)
	assert 2.5e-9 <= lo < 1e-8 and not _fitvar_certified(hi, lo, False, 1.0)
	with pytest.raises(NotImplementedError, match='rank is certain'):
		ComputeVarPlan(g['C_dt'], bad)
	b, r, hi, lo, b1 = _fitvar_bases(dc)
	assert _fitvar_certified(hi, lo, r == dc.shape[0], 1.0)
	with pytest.raises(ValueError):  # certified covariates: the next check is the one for a host array
		ComputeVarPlan(g['C_dt'], dc)
