"""The resident de plan of the C ABI (include/normalisr_hip.h: nrm_de_plan_*) as far as it goes without a GPU: what is declared is exported, normalisr_amd.cplan
binds it without torch, the constructor and create refuse bad arguments -- create before any device call, in the reference's words --, the varying-row rule the
plan's kernels decide by is held to de's own on its edge cases, and the host arithmetic of the checks runs under ASan + UBSan in a program of its own."""
import ctypes

import numpy as np
import pytest

from cabi_harness import assert_plan_names, binds_without_torch, build_and_run_host_program
from cabi_harness import vp as _vp
from normalisr_amd import _lib
from normalisr_amd.association import inv_rank

PLAN_CALLS = ('create', 'design', 'upload', 'step', 'check', 'results', 'device_results', 'stream', 'info', 'time', 'destroy')
TOO_FEW = 'Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.'


def test_de_plan_names_declared_and_exported():
	assert_plan_names('nrm_de_plan_', PLAN_CALLS)


def test_de_plan_binds_without_torch():
	binds_without_torch(('DePlan', 'DeviceCSR', 'varying_rows'), (), 'nrm_de_plan_destroy')


def _problem(n=12, nc=2):
	dg = np.zeros((4, n))
	dg[np.arange(4), np.arange(4) % n] = 1.
	dt = np.ones((3, n))
	dc = np.vstack([np.ones(n), np.arange(n, dtype=np.float64)] + [np.sin(np.arange(n) * (c + 1.)) for c in range(nc - 2)])[:nc]
	return dg, dt, np.ascontiguousarray(dc)


def _create(dg, dt, dc, dci, rank, dimreduce=0, ng0=None, nt=None, n=None, dg_dtype=_lib.NRM_F64, dt_dtype=_lib.NRM_F64, out_dtype=_lib.NRM_F64, form=0, indptr=None, indices=None, nnz=0):
	lib = _lib.load()
	h = ctypes.c_void_p()
	n = dt.shape[1] if n is None else n
	nc = dc.shape[0]
	rc = lib.nrm_de_plan_create(ctypes.byref(h), form, _vp(dg), dg_dtype, n, _vp(indptr), _vp(indices), nnz, 0, 4 if ng0 is None else ng0, _vp(dt), dt_dtype, 3 if nt is None else nt, n, n,
								0, _vp(dc) if nc else None, _lib.NRM_F64, nc, _vp(dci), rank, dimreduce, out_dtype, 0, 0)
	return rc, lib.nrm_last_error().decode(), h


def test_de_plan_create_refuses_bad_arguments_before_any_device_call():
	"""No GPU here: NRM_E_ARG / NRM_E_UNSUPPORTED (not NRM_E_DEVICE) shows that every check comes before the first device call (association.py:199-216)."""
	dg, dt, dc = _problem()
	n = dt.shape[1]
	dci, rank = inv_rank(dc @ dc.T)
	dci = np.ascontiguousarray(dci)
	arg = [
		(_create(None, dt, dc, dci, rank), 'Incorrect dx/dy/dc size.'),  # a null design
		(_create(dg, None, dc, dci, rank, n=n), 'Incorrect dx/dy/dc size.'),  # a null expression matrix
		(_create(dg, dt, dc, dci, rank, ng0=0), 'Incorrect dx/dy/dc size.'),
		(_create(dg, dt, dc, dci, rank, form=1), 'Incorrect dx/dy/dc size.'),  # CSR without indptr
		(_create(dg, dt, dc, dci, rank, dg_dtype=7), 'nrm_de_plan_create: bad dtype'),
		(_create(dg, dt, dc, dci, rank, dt_dtype=3), 'nrm_de_plan_create: bad dtype'),
		(_create(dg, dt, dc, dci, rank, out_dtype=16), 'nrm_de_plan_create: bad dtype'),
		(_create(dg, dt, dc, dci, 3), 'dcr higher than covariate dimension.'),
		(_create(dg, dt, dc, dci, -1), 'Negative dcr detected.'),
		(_create(dg, dt, dc, dci, rank, dimreduce=n - rank - 1), TOO_FEW),
		(_create(dg[:, :3].copy(), dt[:, :3].copy(), dc[:, :3].copy(), None, 0), TOO_FEW),  # the library's own rank: 3 cells, rank 2
	]
	for (rc, msg, h), want in arg:
		assert rc == _lib.NRM_E_ARG and msg == want and h.value is None, (rc, msg, want)
	# 33 covariates: without a pseudo-inverse, and with one (beyond the sparse-design kernel)
	dg, dt, dc33 = _problem(n=40, nc=33)
	for dci33 in (None, np.zeros((33, 33))):
		rc, msg, h = _create(dg, dt, dc33, dci33, 2)
		assert rc == _lib.NRM_E_UNSUPPORTED and h.value is None and 'covariates' in msg, (rc, msg)
		with pytest.raises(NotImplementedError):
			_lib.check(rc)
	lib = _lib.load()
	assert lib.nrm_de_plan_destroy(None) == 0
	for call in ('step', 'upload'):  # a null plan is an argument error, not a crash
		assert getattr(lib, 'nrm_de_plan_' + call)(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_de_plan_design(None, 0, None, _lib.NRM_F64, 0, None, None, 0, 0) == _lib.NRM_E_ARG
	assert lib.nrm_de_plan_check(None, None) == _lib.NRM_E_ARG


def test_de_plan_constructor_validation():
	import scipy.sparse
	from normalisr_amd import cplan
	dg, dt, dc = _problem()
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.DePlan(dg, dt, dc[:, :5])
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.DePlan(dg[:, :5], dt, dc)
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.DePlan(scipy.sparse.csr_matrix(dg[:, :5]), dt, dc)
	with pytest.raises(ValueError, match='dimreduce must be an integer.'):
		cplan.DePlan(dg, dt, dc, dimreduce=1.5)
	with pytest.raises(ValueError, match='out_dtype must be float32 or float64'):
		cplan.DePlan(dg, dt, dc, out_dtype=np.float16)
	with pytest.raises(TypeError, match='a sparse dt is not taken here'):
		cplan.DePlan(dg, scipy.sparse.csr_matrix(dt), dc)
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.DePlan(dg[0], dt, dc)
	with pytest.raises(ValueError, match="pinv must be 'numpy' or 'library'"):
		cplan.DePlan(dg, dt, dc, pinv='lapack')
	with pytest.raises(ValueError, match='Insufficient number of cells'):
		cplan.DePlan(dg[:, :3], dt[:, :3], dc[:, :3])
	with pytest.raises(ValueError, match='Insufficient number of cells'):
		cplan.DePlan(scipy.sparse.csr_matrix(dg[:, :3]), dt[:, :3], dc[:, :3], pinv='library')


def _rule_cases():
	"""(name, dense rows (r, n)) for the rule: all zeros, all ones, all NaN, NaN and a value, a full row of two values, a full row of one value that is not 1,
	a row with some cells set, NaN among zeros."""
	nan = np.nan
	n = 6
	rows = np.array([
		[0, 0, 0, 0, 0, 0],
		[1, 1, 1, 1, 1, 1],
		[nan, nan, nan, nan, nan, nan],
		[nan, 2, nan, nan, nan, nan],
		[2, 2, 3, 2, 2, 2],
		[2.5, 2.5, 2.5, 2.5, 2.5, 2.5],
		[0, 0, 1, 0, 1, 0],
		[0, nan, 0, 0, 0, 0],
		[nan, nan, nan, nan, nan, 0],
	], dtype=np.float64)
	assert rows.shape[1] == n
	return rows, np.array([False, False, False, True, True, False, True, True, True])


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int64])
def test_varying_row_rule_against_de(dtype):
	"""The rule the plan's kernels decide by (cplan.varying_rows: k entries among n cells, values compared with NaNs equal), on de's edge cases, against
	de._varying_rows (dense), de._varying_rows_scipy (canonical CSR) and the expected answers spelled out."""
	import scipy.sparse
	from normalisr_amd import cplan, de, de_sparse
	rows, want = _rule_cases()
	if dtype == np.int64:
		keep = ~np.isnan(rows).any(axis=1)
		rows, want = rows[keep].astype(np.int64), want[keep]
	else:
		rows = rows.astype(dtype)
	assert (de._varying_rows(rows) == want).all()
	assert (cplan.varying_rows(rows) == want).all()
	indptr, indices, data = de_sparse.canonical_design_csr(scipy.sparse.csr_matrix(rows))
	m = scipy.sparse.csr_matrix((data, indices, indptr), shape=rows.shape)
	assert (de._varying_rows_scipy(m) == want).all()
	assert (cplan.varying_rows(m) == want).all()


def test_varying_row_rule_stored_zeros_and_one_cell():
	import scipy.sparse
	from normalisr_amd import cplan, de
	# stored zeros are not entries: a full row of stored values of which one is zero holds two values; a row of stored zeros only is constant
	n = 5
	data = np.array([3., 3., 0., 3., 3., 0., 0., 4., 4., 4., 4., 4.])
	indices = np.array([0, 1, 2, 3, 4, 1, 3, 0, 1, 2, 3, 4], dtype=np.int32)
	indptr = np.array([0, 5, 7, 12], dtype=np.int64)
	m = scipy.sparse.csr_matrix((data, indices, indptr), shape=(3, n))
	want = np.array([True, False, False])
	assert (cplan.varying_rows(m) == want).all()
	assert (de._varying_rows(m.toarray()) == want).all()
	assert (cplan.varying_rows(m.toarray()) == want).all()
	# n = 1: no row varies, whatever it holds
	one = np.array([[0.], [1.], [np.nan]])
	assert not de._varying_rows(one).any() and not cplan.varying_rows(one).any()
	assert not cplan.varying_rows(scipy.sparse.csr_matrix(np.array([[0.], [1.]]))).any()
	assert not de._varying_rows_scipy(scipy.sparse.csr_matrix(np.array([[0.], [1.]]))).any()


def test_varying_row_rule_on_seeded_designs():
	import scipy.sparse
	from normalisr_amd import cplan, de
	rng = np.random.default_rng(5)
	for n in (1, 2, 3, 70, 300):
		dg = (rng.random((40, n)) < 0.2) * rng.integers(1, 3, (40, n)).astype(np.float64)
		dg[3] = 0
		dg[4] = 2
		dg[5, rng.random(n) < 0.5] = np.nan
		want = de._varying_rows(dg)
		assert (cplan.varying_rows(dg) == want).all(), n
		m = scipy.sparse.csr_matrix(dg)
		m.eliminate_zeros()
		assert (cplan.varying_rows(m) == want).all(), n


def test_de_plan_argument_checks_under_address_and_ub_sanitizers(tmp_path):
	"""csrc/nrm_de_plan_args.h -- every check create and design make before a device call, the library's own pseudo-inverse included -- built by g++ with
	-fsanitize=address,undefined beside a program with its own main (tests/host/de_plan_args_sanitize.cpp) and run directly: nothing loaded into python runs
	under a sanitizer."""
	build_and_run_host_program(tmp_path, ['normalisr_amd/csrc/nrm_small_pinv.hip', 'tests/host/de_plan_args_sanitize.cpp'], 'de plan args ok')
