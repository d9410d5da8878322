"""The resident front-half plan on CSR counts (include/normalisr_hip.h: nrm_front_plan_create_csr, nrm_front_plan_upload_csr; normalisr_amd.cplan.FrontPlanCSR)
as far as it goes without a GPU: the two entries are declared, exported and bound, FrontPlanCSR binds without torch, create_csr refuses bad arguments before any
device call, the constructor refuses what it can see, and the argument checks and the malformed-first reading of the counters run under ASan + UBSan in a
program of its own."""
import ctypes

import numpy as np
import pytest

from cabi_harness import assert_plan_names, binds_without_torch, build_and_run_host_program
from cabi_harness import vp as _vp
from normalisr_amd import _lib

MALFORMED = ('Malformed CSR matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and '
			 'increase strictly (sum duplicates and sort the indices first).')


def test_front_plan_csr_names_declared_and_exported():
	assert len(assert_plan_names('nrm_front_plan_', ('create_csr', 'upload_csr'))) == 2


def test_front_plan_csr_binds_without_torch():
	binds_without_torch(('FrontPlanCSR', 'FrontPlan', 'DeviceCSR'), ('step', 'check', 'results', 'weights', 'scaling', 'lcpm', 'normcov', 'device_results', 'update', 'time', 'info',
																		'close', '__enter__', '__exit__'), 'nrm_front_plan_destroy')


def test_front_plans_share_their_methods():
	"""results, weights, scaling, lcpm, normcov, device_results, check, info and time are one function each for both plans, not copies."""
	from normalisr_amd import cplan
	for m in ('results', 'weights', 'scaling', 'lcpm', 'normcov', 'device_results', 'check', 'info', 'time', 'step', 'close'):
		assert getattr(cplan.FrontPlanCSR, m) is getattr(cplan.FrontPlan, m), m
	assert cplan.FrontPlanCSR.update is not cplan.FrontPlan.update and cplan.FrontPlanCSR._info_fields is cplan.FrontPlan._info_fields


def _problem(n=12, n_cov=2):
	"""5 genes x n cells, two stored entries per gene; cov as tests/test_front_plan_cpu.py makes it."""
	indptr = 2 * np.arange(6, dtype=np.int64)
	indices = np.ravel([[g, g + 6] for g in range(5)]).astype(np.int32)
	data = (1 + np.arange(10) % 3).astype(np.int32)
	cov = np.vstack([(np.arange(n) % 2).astype(np.float64)] + [np.sin(np.arange(n) * (c + 1.)) for c in range(n_cov - 1)])[:n_cov]
	return indptr, indices, data, np.ascontiguousarray(cov)


def _create(indptr, indices, data, cov, dtype=_lib.NRM_I32, genes=5, n=None, nnz=None, nnz_cap=None, on_device=0, n_cov=None, ntot=-1, stepmax=1, eps=1e-6, tol=1e-8,
			out_dtype=_lib.NRM_F64, cap=256, null_cov=False):
	lib = _lib.load()
	h = ctypes.c_void_p()
	n = cov.shape[1] if n is None else n
	nnz = (0 if data is None else data.size) if nnz is None else nnz
	n_cov = cov.shape[0] if n_cov is None else n_cov
	rc = lib.nrm_front_plan_create_csr(ctypes.byref(h), _vp(indptr), _vp(indices), _vp(data), dtype, genes, n, nnz, nnz if nnz_cap is None else nnz_cap, on_device,
									   None if (null_cov or not n_cov) else _vp(cov), n_cov, ntot, stepmax, eps, tol, out_dtype, cap)
	return rc, lib.nrm_last_error().decode(), h


def test_front_plan_create_csr_refuses_bad_arguments_before_any_device_call():
	"""No GPU here: NRM_E_ARG / NRM_E_UNSUPPORTED (not NRM_E_DEVICE) shows that every check comes before the first device call."""
	indptr, indices, data, cov = _problem()
	lib = _lib.load()
	top = int(lib.nrm_lcpm_table_cap())
	who = 'nrm_front_plan_create_csr: '
	sizes = who + '0 <= nnz <= nnz_cap and nnz_cap >= 1 must hold'
	from_one, falling, short = indptr.copy(), indptr.copy(), indptr.copy()
	from_one[0] = 1
	falling[2], falling[3] = 7, 5
	short[5] = 9
	bad_cov, flat_cov = cov.copy(), cov.copy()
	bad_cov[1, -1] = np.nan
	flat_cov[1] = 3.0
	arg = [
		(_create(None, indices, data, cov), who + 'null pointer'),
		(_create(indptr, None, data, cov, nnz=10), who + 'null pointer'),
		(_create(indptr, indices, None, cov, nnz=10), who + 'null pointer'),
		(_create(indptr, indices, data, cov, null_cov=True, n_cov=2), who + 'null pointer'),
		(_create(indptr, indices, data, cov, n_cov=-1), who + 'null pointer'),
		(_create(indptr, indices, data, cov, nnz=-1, nnz_cap=10), sizes),
		(_create(indptr, indices, data, cov, nnz=10, nnz_cap=9), sizes),
		(_create(indptr, indices, data, cov, nnz=0, nnz_cap=0), sizes),
		(_create(indptr, indices, data, cov, nnz=-1, nnz_cap=10, on_device=1), sizes),
		(_create(indptr, indices, data, cov, nnz=10, nnz_cap=9, on_device=1), sizes),
		(_create(indptr, indices, data, cov, genes=0), 'reads must not be empty.'),
		(_create(indptr, indices, data, cov, n=0), 'reads must not be empty.'),
		(_create(indptr, indices, data, cov, n_cov=0, n=1 << 31), who + 'at most 2097120 genes and 2^31 - 1 cells'),
		(_create(indptr, indices, data, cov, genes=(1 << 31), on_device=1), who + 'at most 2097120 genes and 2^31 - 1 cells'),
		(_create(indptr, indices, data, cov, dtype=_lib.NRM_F64), who + 'counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8'),
		(_create(indptr, indices, data, cov, out_dtype=_lib.NRM_I32), who + 'out_dtype must be NRM_F32 or NRM_F64'),
		(_create(from_one, indices, data, cov), MALFORMED),
		(_create(falling, indices, data, cov), MALFORMED),
		(_create(short, indices, data, cov), MALFORMED),
		(_create(indptr, indices, data, cov, nnz=9, nnz_cap=10), MALFORMED),
		(_create(indptr, indices, data, cov, eps=0.), 'eps and stepmax must be positive.'),
		(_create(indptr, indices, data, cov, stepmax=0), 'eps and stepmax must be positive.'),
		(_create(indptr, indices, data, cov, tol=0.), who + 'tol must lie in (0, 1)'),
		(_create(indptr, indices, data, cov, ntot=0), 'ntot must be positive (t0 = ntot + 2 > 2, lcpm.py:95).'),
		(_create(indptr, indices, data, cov, cap=1), who + 'count_cap must lie in [2, {}]'.format(top)),
		(_create(indptr, indices, data, cov, cap=top + 1), who + 'count_cap must lie in [2, {}]'.format(top)),
		(_create(indptr, indices, data, bad_cov), 'array must not contain infs or NaNs'),
		(_create(indptr, indices, data, flat_cov), 'Detected constant covariate. Please only provide full-rank covariate without constant covariate.'),
	]
	for (rc, msg, h), want in arg:
		assert rc == _lib.NRM_E_ARG and msg == want and h.value is None, (rc, msg, want)
	with pytest.raises(ValueError, match='Malformed CSR matrix'):
		_lib.check(_create(short, indices, data, cov)[0])
	# the covariate bound is nrm_normvar_device_covariates(), as for the dense plan
	bound = int(lib.nrm_normvar_device_covariates())
	many = _problem(n=40, n_cov=bound - 3)[3]
	rc, msg, h = _create(indptr, indices, data, many)
	assert rc == _lib.NRM_E_UNSUPPORTED and h.value is None and 'the {} covariates'.format(bound) in msg and 'nrm_normvar_device_covariates' in msg, (rc, msg)
	with pytest.raises(NotImplementedError):
		_lib.check(rc)
	# a null plan is an argument error, not a crash
	assert lib.nrm_front_plan_upload_csr(None, _vp(indptr), _vp(indices), _vp(data), 10) == _lib.NRM_E_ARG
	assert lib.nrm_front_plan_create_csr(None, _vp(indptr), _vp(indices), _vp(data), _lib.NRM_I32, 5, 12, 10, 10, 0, None, 0, -1, 1, 1e-6, 1e-8, _lib.NRM_F64, 256) == _lib.NRM_E_ARG


def test_front_plan_csr_constructor_validation():
	import scipy.sparse
	from normalisr_amd import cplan
	indptr, indices, data, cov = _problem()
	n = cov.shape[1]
	reads = scipy.sparse.csr_matrix((data, indices, indptr), shape=(5, n))
	with pytest.raises(TypeError, match='reads must be a scipy.sparse matrix or a cplan.DeviceCSR'):
		cplan.FrontPlanCSR(reads.toarray(), cov)
	with pytest.raises(TypeError, match='reads must be an integer matrix.'):
		cplan.FrontPlanCSR(reads.astype(np.float64), cov)
	with pytest.raises(ValueError, match='the same cell count'):
		cplan.FrontPlanCSR(reads, cov[:, :5])
	with pytest.raises(ValueError, match='nnz_cap = 9 is below the 10 stored entries'):
		cplan.FrontPlanCSR(reads, cov, nnz_cap=9)
	with pytest.raises(ValueError, match='nnz_cap must be an integer.'):
		cplan.FrontPlanCSR(reads, cov, nnz_cap=10.5)
	with pytest.raises(ValueError, match='Negative value in d detected.'):
		cplan.FrontPlanCSR(-reads, cov)
	with pytest.raises(ValueError, match='out_dtype must be float32 or float64'):
		cplan.FrontPlanCSR(reads, cov, out_dtype=np.float16)
	with pytest.raises(ValueError, match='eps and stepmax must be positive.'):
		cplan.FrontPlanCSR(reads, cov, stepmax=0)
	with pytest.raises(ValueError, match='ntot must be a positive integer.'):
		cplan.FrontPlanCSR(reads, cov, ntot=0)
	with pytest.raises(ValueError, match='count_cap must lie in'):
		cplan.FrontPlanCSR(reads, cov, count_cap=1)
	with pytest.raises(ValueError, match='Detected constant covariate.'):
		cplan.FrontPlanCSR(reads, np.vstack([cov, np.ones((1, n))]))
	with pytest.raises(NotImplementedError, match='nrm_normvar_device_covariates'):
		cplan.FrontPlanCSR(scipy.sparse.csr_matrix((data, indices, indptr), shape=(5, 40)), _problem(n=40, n_cov=5)[3])
	with pytest.raises(NotImplementedError, match='FrontPlanCSR tabulates'):
		cplan.FrontPlanCSR(scipy.sparse.csr_matrix(np.full((2, 3), 1 << 24, dtype=np.int64)))
	# a DeviceCSR (its addresses are never dereferenced: every refusal below comes before create)
	dev = cplan.DeviceCSR(4096, 8192, 12288, (5, n), 10, np.int32)
	for kw in (dict(), dict(count_cap=256), dict(nnz_cap=10)):
		with pytest.raises(ValueError, match='count_cap and nnz_cap must be given for a DeviceCSR'):
			cplan.FrontPlanCSR(dev, cov, **kw)
	with pytest.raises(ValueError, match='nnz_cap = 9 is below the 10 stored entries'):
		cplan.FrontPlanCSR(dev, cov, count_cap=256, nnz_cap=9)
	for dtype in (np.float32, np.float64):
		with pytest.raises(ValueError, match='a DeviceCSR of read counts must be int64, int32, int16 or uint8'):
			cplan.FrontPlanCSR(cplan.DeviceCSR(4096, 8192, 12288, (5, n), 10, dtype), cov, count_cap=256, nnz_cap=10)
	with pytest.raises(ValueError, match='has indices and data'):
		cplan.FrontPlanCSR(cplan.DeviceCSR(4096, 8192, None, (5, n), 10, np.int32), cov, count_cap=256, nnz_cap=10)
	with pytest.raises(ValueError, match='DeviceCSR: data must be'):
		cplan.DeviceCSR(4096, 8192, 12288, (5, n), 10, np.uint16)
	# the other plans keep to their own kind: a design is float, FrontPlan is dense
	with pytest.raises(ValueError, match='the data of a design must be float32 or float64'):
		cplan.DePlan(dev, np.zeros((3, n)), cov)
	for sparse in (reads, dev):
		with pytest.raises(TypeError, match='a sparse reads is not taken here'):
			cplan.FrontPlan(sparse, cov, count_cap=256)


def test_front_plan_csr_argument_checks_under_address_and_ub_sanitizers(tmp_path):
	"""csrc/nrm_front_plan_args.h -- every check create_csr and upload_csr make before a device call, and the counters read with the malformed word first --
	beside tests/host/front_plan_csr_args_sanitize.cpp, a stand-alone program run directly."""
	build_and_run_host_program(tmp_path, ['tests/host/front_plan_csr_args_sanitize.cpp'], 'front plan csr args ok')
