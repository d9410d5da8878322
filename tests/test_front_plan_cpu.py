"""The resident front-half plan of the C ABI (include/normalisr_hip.h: nrm_front_plan_*) as far as it goes without a GPU: what is declared is exported and bound,
normalisr_amd.cplan.FrontPlan binds it without torch, the digamma evaluation of the table kernel (csrc/nrm_digamma.h, one header for host and device) agrees with
scipy's values in golden G18 and with nrm_lcpm_digamma, the constructor and create refuse bad arguments -- create before any device call --, and the argument
checks, normcov's row classification and the reading of the counters run under ASan + UBSan in a program of its own."""
import ctypes

import numpy as np
import pytest

from cabi_harness import assert_plan_names, binds_without_torch, build_and_run_host_program
from cabi_harness import vp as _vp
from normalisr_amd import _lib

PLAN_CALLS = ('create', 'upload', 'step', 'check', 'results', 'device_results', 'stream', 'info', 'time', 'destroy')


def test_front_plan_names_declared_and_exported():
	assert len(assert_plan_names('nrm_front_plan_', PLAN_CALLS)) == 10


def test_front_plan_binds_without_torch():
	binds_without_torch(('FrontPlan', 'DeviceMatrix'), ('step', 'check', 'results', 'weights', 'scaling', 'lcpm', 'normcov', 'device_results', 'update', 'time', 'info', 'close',
														'__enter__', '__exit__'), 'nrm_front_plan_destroy')


def _digamma_header(tmp_path, z):
	"""psi(z) from csrc/nrm_digamma.h, through the host program tests/host/front_digamma_host.cpp."""
	src, dst = tmp_path / 'z.bin', tmp_path / 'psi.bin'
	np.asarray(z, dtype=np.float64).tofile(str(src))
	build_and_run_host_program(tmp_path, ['tests/host/front_digamma_host.cpp'], 'front digamma ok {}'.format(len(z)), args=[str(src), str(dst)])
	return np.fromfile(str(dst), dtype=np.float64)


def test_digamma_header_against_scipy_values_and_the_host_table(golden, tmp_path):
	"""The bar is the one tests/test_front_cpu.py holds nrm_lcpm_digamma to against the same values: |error| <= 1e-14 |psi| + 1e-15."""
	from normalisr_amd.lcpm import digamma_table
	g = golden('G18_front')
	xs, ref, t0s, ref0 = g['psi_x'], g['psi_digamma'], g['psi_t0'], g['psi_t0_digamma']
	psi = _digamma_header(tmp_path, np.concatenate([1.0 + xs, t0s]))
	bar = lambda r: 1e-14 * np.abs(r) + 1e-15
	err = np.abs(psi[:len(xs)] - ref) / bar(ref)
	print('psi(1 + x): worst error / bound = %.3g at x = %d' % (err.max(), xs[err.argmax()]))
	assert err.max() <= 1.0
	err0 = np.abs(psi[len(xs):] - ref0) / bar(ref0)
	print('psi(t0): worst error / bound = %.3g at t0 = %g' % (err0.max(), t0s[err0.argmax()]))
	assert err0.max() <= 1.0
	# the table the host entries fill, at the same arguments
	table, _ = digamma_table(int(xs.max()), 3.0)
	assert (np.abs(psi[:len(xs)] - table[xs]) <= bar(table[xs])).all()
	for t0, v in zip(t0s, psi[len(xs):]):
		_, host = digamma_table(0, float(t0))
		assert abs(v - host) <= 1e-14 * abs(host) + 1e-15, (t0, v, host)


def _problem(n=12, n_cov=2):
	reads = (np.arange(5 * n).reshape(5, n) % 4).astype(np.int32)
	cov = np.vstack([(np.arange(n) % 2).astype(np.float64)] + [np.sin(np.arange(n) * (c + 1.)) for c in range(n_cov - 1)])[:n_cov]
	return reads, np.ascontiguousarray(cov)


def _create(reads, cov, dtype=_lib.NRM_I32, genes=None, n=None, ld=None, on_device=0, n_cov=None, ntot=-1, stepmax=1, eps=1e-6, tol=1e-8, out_dtype=_lib.NRM_F64, cap=256, null_cov=False):
	lib = _lib.load()
	h = ctypes.c_void_p()
	genes = reads.shape[0] if genes is None else genes
	n = reads.shape[1] if n is None else n
	n_cov = cov.shape[0] if n_cov is None else n_cov
	rc = lib.nrm_front_plan_create(ctypes.byref(h), _vp(reads), dtype, genes, n, n if ld is None else ld, on_device, None if (null_cov or not n_cov) else _vp(cov), n_cov, ntot, stepmax,
								   eps, tol, out_dtype, cap)
	return rc, lib.nrm_last_error().decode(), h


def test_front_plan_create_refuses_bad_arguments_before_any_device_call():
	"""No GPU here: NRM_E_ARG / NRM_E_UNSUPPORTED (not NRM_E_DEVICE) shows that every check comes before the first device call."""
	reads, cov = _problem()
	n = reads.shape[1]
	lib = _lib.load()
	top = int(lib.nrm_lcpm_table_cap())
	constant = 'Detected constant covariate. Please only provide full-rank covariate without constant covariate.'
	bad_cov = cov.copy()
	bad_cov[1, n - 1] = np.nan
	flat_cov = cov.copy()
	flat_cov[1] = 3.0
	arg = [
		(_create(None, cov, genes=5, n=n), 'nrm_front_plan_create: null pointer'),
		(_create(reads, cov, null_cov=True, n_cov=2), 'nrm_front_plan_create: null pointer'),
		(_create(reads, cov, n_cov=-1), 'nrm_front_plan_create: null pointer'),
		(_create(reads, cov, genes=0), 'reads must not be empty.'),
		(_create(reads, cov, n=0), 'reads must not be empty.'),
		(_create(reads, cov, dtype=_lib.NRM_F64), 'nrm_front_plan_create: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8'),
		(_create(reads, cov, out_dtype=_lib.NRM_I32), 'nrm_front_plan_create: out_dtype must be NRM_F32 or NRM_F64'),
		(_create(reads, cov, ld=n + 4), 'nrm_front_plan_create: row pitch smaller than the row (a host matrix is contiguous)'),
		(_create(reads, cov, ld=n - 1, on_device=1), 'nrm_front_plan_create: row pitch smaller than the row (a host matrix is contiguous)'),
		(_create(reads, cov, eps=0.), 'eps and stepmax must be positive.'),
		(_create(reads, cov, stepmax=0), 'eps and stepmax must be positive.'),
		(_create(reads, cov, tol=0.), 'nrm_front_plan_create: tol must lie in (0, 1)'),
		(_create(reads, cov, ntot=0), 'ntot must be positive (t0 = ntot + 2 > 2, lcpm.py:95).'),
		(_create(reads, cov, cap=1), 'nrm_front_plan_create: count_cap must lie in [2, {}]'.format(top)),
		(_create(reads, cov, cap=top + 1), 'nrm_front_plan_create: count_cap must lie in [2, {}]'.format(top)),
		(_create(reads, bad_cov), 'array must not contain infs or NaNs'),
		(_create(reads, flat_cov), constant),
	]
	for (rc, msg, h), want in arg:
		assert rc == _lib.NRM_E_ARG and msg == want and h.value is None, (rc, msg, want)
	# the covariate bound is nrm_normvar_device_covariates(): with lcpm's three rows and the constant row, that many less four user rows
	bound = int(lib.nrm_normvar_device_covariates())
	reads, many = _problem(n=40, n_cov=bound - 3)
	rc, msg, h = _create(reads, many)
	assert rc == _lib.NRM_E_UNSUPPORTED and h.value is None and 'the {} covariates'.format(bound) in msg and 'nrm_normvar_device_covariates' in msg, (rc, msg)
	with pytest.raises(NotImplementedError):
		_lib.check(rc)
	assert lib.nrm_front_plan_destroy(None) == 0
	for call in ('step', 'upload', 'check'):  # a null plan is an argument error, not a crash
		assert getattr(lib, 'nrm_front_plan_' + call)(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_front_plan_results(None, None, None, None, None, None, None) == _lib.NRM_E_ARG
	assert lib.nrm_front_plan_device_results(None, None, None, None, None, None) == _lib.NRM_E_ARG
	assert lib.nrm_front_plan_info(None, None) == _lib.NRM_E_ARG and lib.nrm_front_plan_stream(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_front_plan_time(None, 1, None) == _lib.NRM_E_ARG


def test_front_plan_constructor_validation():
	import scipy.sparse
	from normalisr_amd import cplan
	reads, cov = _problem()
	n = reads.shape[1]
	with pytest.raises(ValueError, match='reads must have 2 dimensions.'):
		cplan.FrontPlan(reads[0], cov)
	with pytest.raises(TypeError, match='reads must be an integer matrix.'):
		cplan.FrontPlan(reads.astype(np.float64), cov)
	with pytest.raises(TypeError, match='a sparse reads is not taken here'):
		cplan.FrontPlan(scipy.sparse.csr_matrix(reads), cov)
	with pytest.raises(ValueError, match='reads must not be empty.'):
		cplan.FrontPlan(reads[:0], cov)
	with pytest.raises(ValueError, match='Covariates must have 2 dimensions.'):
		cplan.FrontPlan(reads, cov[0])
	with pytest.raises(ValueError, match='the same cell count'):
		cplan.FrontPlan(reads, cov[:, :5])
	with pytest.raises(ValueError, match='out_dtype must be float32 or float64'):
		cplan.FrontPlan(reads, cov, out_dtype=np.float16)
	with pytest.raises(ValueError, match='eps and stepmax must be positive.'):
		cplan.FrontPlan(reads, cov, eps=0)
	with pytest.raises(ValueError, match='eps and stepmax must be positive.'):
		cplan.FrontPlan(reads, cov, stepmax=0)
	with pytest.raises(ValueError, match='stepmax must be an integer.'):
		cplan.FrontPlan(reads, cov, stepmax=1.5)
	with pytest.raises(ValueError, match='ntot must be a positive integer.'):
		cplan.FrontPlan(reads, cov, ntot=0)
	with pytest.raises(ValueError, match='tol must lie in'):
		cplan.FrontPlan(reads, cov, tol=0)
	with pytest.raises(ValueError, match='count_cap must lie in'):
		cplan.FrontPlan(reads, cov, count_cap=1)
	with pytest.raises(ValueError, match='Detected constant covariate.'):
		cplan.FrontPlan(reads, np.vstack([cov, np.ones((1, n))]))
	with pytest.raises(ValueError, match='infs or NaNs'):
		cplan.FrontPlan(reads, np.vstack([cov, np.full((1, n), np.inf)]))
	with pytest.raises(NotImplementedError, match='nrm_normvar_device_covariates'):
		cplan.FrontPlan(*_problem(n=40, n_cov=5))
	with pytest.raises(NotImplementedError, match='counts below'):
		cplan.FrontPlan(np.full((2, 3), 1 << 24, dtype=np.int64))
	dm = cplan.DeviceMatrix(4096, reads.shape, np.int32)  # (never dereferenced: every refusal below comes before create)
	with pytest.raises(ValueError, match='count_cap must be given for a device matrix'):
		cplan.FrontPlan(dm, cov)
	with pytest.raises(ValueError, match='a device matrix must be int64, int32, int16 or uint8'):
		cplan.FrontPlan(cplan.DeviceMatrix(4096, reads.shape, np.float32), cov, count_cap=256)


def test_front_plan_argument_checks_under_address_and_ub_sanitizers(tmp_path):
	"""csrc/nrm_front_plan_args.h -- every check create makes before a device call, normcov's row classification, the counters read in the reference's order --
	beside tests/host/front_plan_args_sanitize.cpp, a stand-alone program run directly."""
	build_and_run_host_program(tmp_path, ['tests/host/front_plan_args_sanitize.cpp'], 'front plan args ok')
