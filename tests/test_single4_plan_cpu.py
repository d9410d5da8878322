"""The resident single=4 plan of the C ABI (include/normalisr_hip.h: nrm_single4_plan_*) as far as it goes without a GPU: what is declared is exported,
normalisr_amd.cplan.Single4Plan binds it without torch, the constructor and create refuse bad arguments -- create before any device call, in the reference's words --,
the checks run under ASan + UBSan in a program of its own, and every screen tests/test_gpu_single4_plan.py builds is held, in numpy and the oracle, to the conditions
those tests rely on."""
import ctypes

import numpy as np
import pytest

from cabi_harness import assert_plan_names, binds_without_torch, build_and_run_host_program
from cabi_harness import vp as _vp
from normalisr_amd import _lib

PLAN_CALLS = ('create', 'design', 'upload', 'step', 'check', 'results', 'device_results', 'stream', 'info', 'time', 'destroy')


def test_single4_plan_names_declared_and_exported():
	assert len(assert_plan_names('nrm_single4_plan_', PLAN_CALLS)) == 11


def test_single4_plan_binds_without_torch():
	binds_without_torch(('Single4Plan', ), ('step', 'check', 'results', 'qvalues', 'device_results', 'update', 'set_design', 'time', 'info', 'close', '__enter__', '__exit__'), 'nrm_single4_plan_destroy')


def _problem(n=12, nc=2):
	dg = np.zeros((4, n))
	dg[np.arange(4), np.arange(4) % n] = 1.
	dt = np.ones((3, n))
	dc = np.vstack([np.ones(n), np.arange(n, dtype=np.float64)] + [np.sin(np.arange(n) * (c + 1.)) for c in range(nc - 2)])[:nc]
	return dg, dt, np.ascontiguousarray(dc)


def _create(dg, dt, dc, dci=None, rank=0, dimreduce=0, tol=1e-8, ng0=4, nt=3, n=None, ldg=None, ldt=None, dg_dtype=_lib.NRM_F64, dt_dtype=_lib.NRM_F64, c_dtype=_lib.NRM_F64,
			out_dtype=_lib.NRM_F64, form=0, indptr=None, indices=None, nnz=0, nc=None, null_dc=False):
	lib = _lib.load()
	h = ctypes.c_void_p()
	n = dt.shape[1] if n is None else n
	nc = dc.shape[0] if nc is None else nc
	rc = lib.nrm_single4_plan_create(ctypes.byref(h), form, _vp(dg), dg_dtype, n if ldg is None else ldg, _vp(indptr), _vp(indices), nnz, 0, ng0, _vp(dt), dt_dtype, nt, n,
									 n if ldt is None else ldt, 0, None if (null_dc or not nc) else _vp(dc), c_dtype, nc, _vp(dci), rank, dimreduce, out_dtype, 0, 0, tol)
	return rc, lib.nrm_last_error().decode(), h


def test_single4_plan_create_refuses_bad_arguments_before_any_device_call():
	"""No GPU here: NRM_E_ARG / NRM_E_UNSUPPORTED (not NRM_E_DEVICE) shows that every check comes before the first device call."""
	dg, dt, dc = _problem()
	n = dt.shape[1]
	size, unmatching, dtype = 'Incorrect dx/dy/dc size.', 'Unmatching dx/dy/dc dimensions.', 'nrm_single4_plan_create: bad dtype'
	pitch = 'nrm_single4_plan_create: row pitch smaller than the row (a host matrix is contiguous)'
	tol = 'nrm_single4_plan_create: tol must be a positive number below 1'
	dci = np.zeros((2, 2))
	arg = [
		(_create(None, dt, dc), size),  # a null design
		(_create(dg, None, dc, n=n), size),  # a null expression matrix
		(_create(dg, dt, dc, ng0=0), size),
		(_create(dg, dt, dc, nt=0), size),
		(_create(dg, dt, dc, n=0), size),
		(_create(dg, dt, dc, form=1), size),  # CSR without indptr
		(_create(dg, dt, dc, null_dc=True), unmatching),  # covariates counted and not given
		(_create(dg, dt, dc, nc=-1), unmatching),
		(_create(dg, dt, dc, dg_dtype=7), dtype),
		(_create(dg, dt, dc, dt_dtype=3), dtype),
		(_create(dg, dt, dc, c_dtype=5), dtype),
		(_create(dg, dt, dc, out_dtype=16), dtype),
		(_create(dg, dt, dc, dimreduce=-1), 'dimreduce must be a non-negative integer.'),
		(_create(dg, dt, dc, ng0=2 ** 31), 'nrm_single4_plan_create: more than 2^31 - 1 rows or cells'),
		(_create(dg, dt, dc, nt=2 ** 31), 'nrm_single4_plan_create: more than 2^31 - 1 rows or cells'),
		(_create(dg, dt, dc, n=2 ** 31), 'nrm_single4_plan_create: more than 2^31 - 1 rows or cells'),
		(_create(dg, dt, dc, ldg=n - 1), pitch),  # a host design is contiguous
		(_create(dg, dt, dc, ldg=n + 4), pitch),
		(_create(dg, dt, dc, ldt=n + 4), pitch),  # ... and so is a host expression matrix
		(_create(dg, dt, dc, ldt=n - 1), pitch),
		(_create(dg, dt, dc, form=2), 'nrm_single4_plan_create: the design is dense (0) or canonical CSR (1)'),
		(_create(dg, dt, dc, form=1, indptr=np.zeros(5, np.int64), nnz=3), size),  # CSR entries without indices
		(_create(dg, dt, dc, form=1, indptr=np.zeros(5, np.int64), indices=np.zeros(4, np.int32), nnz=4 * n + 4), 'nrm_single4_plan_create: more stored entries than the matrix has cells'),
		(_create(dg, dt, dc, tol=0.), tol),
		(_create(dg, dt, dc, tol=-1e-8), tol),
		(_create(dg, dt, dc, tol=float('nan')), tol),
		(_create(dg, dt, dc, tol=1.), tol),
		(_create(dg, dt, dc, dci, 3), 'dcr higher than covariate dimension.'),
		(_create(dg, dt, dc, dci, -1), 'Negative dcr detected.'),
	]
	for (rc, msg, h), want in arg:
		assert rc == _lib.NRM_E_ARG and msg == want and h.value is None, (rc, msg, want)
	# covariates of rank 0, and 33 covariates -- without a pseudo-inverse, and with one (beyond the sparse-design kernel)
	rc, msg, h = _create(dg, dt, dc, dci, 0)
	assert rc == _lib.NRM_E_UNSUPPORTED and h.value is None and 'covariates of rank 0' in msg, (rc, msg)
	dg, dt, dc33 = _problem(n=40, nc=33)
	for dci33 in (None, np.zeros((33, 33))):
		rc, msg, h = _create(dg, dt, dc33, dci33, 2)
		assert rc == _lib.NRM_E_UNSUPPORTED and h.value is None and 'at most 32 covariates' in msg, (rc, msg)
		with pytest.raises(NotImplementedError):
			_lib.check(rc)
	lib = _lib.load()
	assert lib.nrm_single4_plan_destroy(None) == 0
	for call in ('step', 'upload'):  # a null plan is an argument error, not a crash
		assert getattr(lib, 'nrm_single4_plan_' + call)(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single4_plan_design(None, 0, None, _lib.NRM_F64, 0, None, None, 0, 0) == _lib.NRM_E_ARG
	assert lib.nrm_single4_plan_check(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single4_plan_results(None, None, None, None, None, None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single4_plan_info(None, None) == _lib.NRM_E_ARG and lib.nrm_single4_plan_stream(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single4_plan_time(None, 1, None) == _lib.NRM_E_ARG


def test_single4_plan_constructor_validation():
	import scipy.sparse
	from normalisr_amd import cplan
	dg, dt, dc = _problem()
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.Single4Plan(dg, dt, dc[:, :5])
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.Single4Plan(dg[:, :5], dt, dc)
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.Single4Plan(scipy.sparse.csr_matrix(dg[:, :5]), dt, dc)
	with pytest.raises(ValueError, match='dimreduce must be an integer.'):
		cplan.Single4Plan(dg, dt, dc, dimreduce=1.5)
	with pytest.raises(ValueError, match='dimreduce must be a non-negative integer.'):
		cplan.Single4Plan(dg, dt, dc, dimreduce=-1)
	with pytest.raises(NotImplementedError, match='one dimreduce for all genes'):
		cplan.Single4Plan(dg, dt, dc, dimreduce=np.zeros(3, dtype=np.int64))
	with pytest.raises(ValueError, match='out_dtype must be float32 or float64'):
		cplan.Single4Plan(dg, dt, dc, out_dtype=np.float16)
	with pytest.raises(ValueError, match="pinv must be 'numpy' or 'library'"):
		cplan.Single4Plan(dg, dt, dc, pinv='lapack')
	with pytest.raises(ValueError, match='tol must be a positive number below 1'):
		cplan.Single4Plan(dg, dt, dc, pinv='library', tol=0)
	with pytest.raises(TypeError, match='a sparse dt is not taken here'):
		cplan.Single4Plan(dg, scipy.sparse.csr_matrix(dt), dc)
	with pytest.raises(TypeError, match='a sparse dc is not taken here'):
		cplan.Single4Plan(dg, dt, scipy.sparse.csr_matrix(dc))
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.Single4Plan(dg[0], dt, dc)
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.Single4Plan(dg, dt[0], dc)
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.Single4Plan(dg, dt, dc[0])
	with pytest.raises(NotImplementedError, match='covariates of rank 0'):
		cplan.Single4Plan(dg, dt, np.zeros_like(dc))
	dg33, dt33, dc33 = _problem(n=40, nc=33)
	with pytest.raises(NotImplementedError, match='at most 32 covariates'):
		cplan.Single4Plan(dg33, dt33, dc33)


def test_single4_plan_argument_checks_under_address_and_ub_sanitizers(tmp_path):
	"""csrc/nrm_single4_plan_args.h -- every check create makes before a device call, the library's own pseudo-inverse included -- beside
	tests/host/single4_plan_args_sanitize.cpp: a program with its own main, built by g++ with -fsanitize=address,undefined and run directly.  Nothing loaded into
	python runs under a sanitizer."""
	build_and_run_host_program(tmp_path, ['normalisr_amd/csrc/nrm_small_pinv.hip', 'tests/host/single4_plan_args_sanitize.cpp'], 'single4 plan args ok')


def _residuals(rows, dc):
	"""The rows residualised against the covariates with the pseudo-inverse of C C^T (numpy)."""
	if not dc.shape[0]:
		return rows
	return rows - rows @ dc.T @ np.linalg.pinv(dc @ dc.T) @ dc


def _de_asserts(res):
	p, gam, _, vx, vy = res
	assert np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all() and np.isfinite(gam).all()
	assert np.isfinite(vx).all() and (vx >= 0).all() and np.isfinite(vy).all() and (vy >= 0).all()


def test_single4_plan_gpu_screens_are_well_posed():
	"""Every screen tests/test_gpu_single4_plan.py builds, in numpy and the oracle: de's filter keeps the expected 65 rows; lambda_min / lambda_max of A A^T >= 1e-3, so
	the certificates are never the thing under test; every design and expression row keeps >= 0.9 of its squared norm against the covariates -- but the planted
	gene, which keeps < 1e-4; dof > 0; the oracle's results pass de's assertions; rho(I - M~ diag(M~)^-1) > 1 without covariates and < 0.5 with, so both starts of
	the Newton-Schulz iteration are exercised."""
	import oracle
	import single4_plan_child as child
	from normalisr_amd import cplan
	kept = child.kept_rows()

	def held(dg, dt, dc, planted=None, rho=None):
		keep = cplan.varying_rows(dg)
		assert keep.sum() == 65 and (np.nonzero(~keep)[0] == [child.ZERO_ROW, child.ONES_ROW]).all()
		x = dg[kept]
		nc = dc.shape[0]
		rank = np.linalg.matrix_rank(dc) if nc else 0
		assert child.N - 65 - rank > 0
		a = np.vstack([x, dc])
		ev = np.linalg.eigvalsh(a @ a.T)[(nc - rank):]  # (the directions inv_rank drops from rank-deficient covariates are not A A^T's to keep)
		assert ev[0] / ev[-1] >= 1e-3, ev[0] / ev[-1]
		xr, yr = _residuals(x, dc), _residuals(dt.astype(np.float64), dc)
		assert ((xr ** 2).sum(axis=1) >= 0.9 * (x ** 2).sum(axis=1)).all()
		ratio = (yr ** 2).sum(axis=1) / (dt.astype(np.float64) ** 2).sum(axis=1)
		others = np.ones(len(ratio), dtype=bool)
		if planted is not None:
			others[planted] = False
			assert ratio[planted] < 1e-4, ratio[planted]
		assert (ratio[others] >= 0.9).all(), ratio[others].min()
		m = xr @ xr.T
		r = np.abs(np.linalg.eigvals(np.eye(65) - m / np.diag(m)[None, :])).max()
		if rho is not None:
			assert (r > 1) if rho == 'diverges' else (r < 0.5), r
		return r

	for nc in child.NCS:
		dg, dt, dc = child.screen(nc)
		r = held(dg, dt, dc, rho='diverges' if nc == 0 else 'converges')
		print(nc, r)
		_de_asserts(oracle.association_tests(dg[kept], dt, dc, single=4, return_dot=False, lowmem=False))
	dg2, dt2, dc2 = child.second_screen(3)
	held(dg2, dt2, dc2, rho='converges')
	assert not np.array_equal(dg2, child.screen(3)[0]) and not np.array_equal(dt2, child.screen(3)[1])
	held(*child.screen(3, np.float32))
	dg, dt, dc = child.handback_screen()
	held(dg, dt, dc, planted=child.PLANTED_GENE)
	_de_asserts(oracle.association_tests(dg[kept], dt, dc, single=4, return_dot=False, lowmem=False))
	# the refusals: the good design on three one-hot batches and an intercept is well posed; the two refused designs are singular given the covariates
	dg, dt, _ = child.screen(3)
	dc, refused = child.refused_designs()
	assert np.linalg.matrix_rank(dc) == 3 and child.covariates_pinv(dc)[2] == 3
	held(dg, dt, dc)
	for name, d in refused.items():
		assert cplan.varying_rows(d).sum() == 65
		xr = _residuals(d[kept], dc)
		ev = np.linalg.eigvalsh(xr @ xr.T)
		assert ev[0] < 1e-9 * ev[-1], (name, ev[0] / ev[-1])
