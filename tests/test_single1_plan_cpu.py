"""The resident single=1 plan of the C ABI (include/normalisr_hip.h: nrm_single1_plan_*) as far as it goes without a GPU: what is declared is exported,
normalisr_amd.cplan.Single1Plan binds it without torch, the constructor and create refuse bad arguments -- create before any device call, in the reference's words --,
and the host arithmetic of the checks runs under ASan + UBSan in a program of its own."""
import ctypes

import numpy as np
import pytest

from cabi_harness import assert_plan_names, binds_without_torch, build_and_run_host_program
from cabi_harness import vp as _vp
from normalisr_amd import _lib

PLAN_CALLS = ('create', 'design', 'upload', 'step', 'check', 'results', 'device_results', 'stream', 'info', 'time', 'destroy')


def test_single1_plan_names_declared_and_exported():
	assert len(assert_plan_names('nrm_single1_plan_', PLAN_CALLS)) == 11


def test_single1_plan_binds_without_torch():
	binds_without_torch(('Single1Plan', ), ('step', 'check', 'results', 'qvalues', 'device_results', 'update', 'set_design', 'time', 'info', 'close', '__enter__', '__exit__'), 'nrm_single1_plan_destroy')


def _problem(n=12, nc=2):
	dg = np.zeros((4, n))
	dg[np.arange(4), np.arange(4) % n] = 1.
	dt = np.ones((3, n))
	dc = np.vstack([np.ones(n), np.arange(n, dtype=np.float64)] + [np.sin(np.arange(n) * (c + 1.)) for c in range(nc - 2)])[:nc]
	return dg, dt, np.ascontiguousarray(dc)


def _create(dg, dt, dc, dimreduce=0, ng0=4, nt=3, n=None, ldg=None, ldt=None, dg_dtype=_lib.NRM_F64, dt_dtype=_lib.NRM_F64, c_dtype=_lib.NRM_F64, out_dtype=_lib.NRM_F64, form=0,
			indptr=None, indices=None, nnz=0, nc=None, null_dc=False):
	lib = _lib.load()
	h = ctypes.c_void_p()
	n = dt.shape[1] if n is None else n
	nc = dc.shape[0] if nc is None else nc
	rc = lib.nrm_single1_plan_create(ctypes.byref(h), form, _vp(dg), dg_dtype, n if ldg is None else ldg, _vp(indptr), _vp(indices), nnz, 0, ng0, _vp(dt), dt_dtype, nt, n,
									 n if ldt is None else ldt, 0, None if (null_dc or not nc) else _vp(dc), c_dtype, nc, dimreduce, out_dtype, 0, 0)
	return rc, lib.nrm_last_error().decode(), h


def test_single1_plan_create_refuses_bad_arguments_before_any_device_call():
	"""No GPU here: NRM_E_ARG / NRM_E_UNSUPPORTED (not NRM_E_DEVICE) shows that every check comes before the first device call."""
	dg, dt, dc = _problem()
	n = dt.shape[1]
	size, unmatching, dtype = 'Incorrect dx/dy/dc size.', 'Unmatching dx/dy/dc dimensions.', 'nrm_single1_plan_create: bad dtype'
	pitch = 'nrm_single1_plan_create: row pitch smaller than the row (a host matrix is contiguous)'
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
		(_create(dg, dt, dc, ng0=2 ** 31), 'nrm_single1_plan_create: more than 2^31 - 1 rows or cells'),
		(_create(dg, dt, dc, nt=2 ** 31), 'nrm_single1_plan_create: more than 2^31 - 1 rows or cells'),
		(_create(dg, dt, dc, n=2 ** 31), 'nrm_single1_plan_create: more than 2^31 - 1 rows or cells'),
		(_create(dg, dt, dc, ldg=n - 1), pitch),  # a host design is contiguous
		(_create(dg, dt, dc, ldg=n + 4), pitch),
		(_create(dg, dt, dc, ldt=n + 4), pitch),  # ... and so is a host expression matrix
		(_create(dg, dt, dc, ldt=n - 1), pitch),
		(_create(dg, dt, dc, form=2), 'nrm_single1_plan_create: the design is dense (0) or canonical CSR (1)'),
		(_create(dg, dt, dc, form=1, indptr=np.zeros(5, np.int64), nnz=3), size),  # CSR entries without indices
		(_create(dg, dt, dc, form=1, indptr=np.zeros(5, np.int64), indices=np.zeros(4, np.int32), nnz=4 * n + 4), 'nrm_single1_plan_create: more stored entries than the matrix has cells'),
	]
	for (rc, msg, h), want in arg:
		assert rc == _lib.NRM_E_ARG and msg == want and h.value is None, (rc, msg, want)
	# 33 covariates: beyond the kernels
	dg, dt, dc33 = _problem(n=40, nc=33)
	rc, msg, h = _create(dg, dt, dc33)
	assert rc == _lib.NRM_E_UNSUPPORTED and h.value is None and 'up to 32 covariates' in msg, (rc, msg)
	with pytest.raises(NotImplementedError):
		_lib.check(rc)
	lib = _lib.load()
	assert lib.nrm_single1_plan_destroy(None) == 0
	for call in ('step', 'upload'):  # a null plan is an argument error, not a crash
		assert getattr(lib, 'nrm_single1_plan_' + call)(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single1_plan_design(None, 0, None, _lib.NRM_F64, 0, None, None, 0, 0) == _lib.NRM_E_ARG
	assert lib.nrm_single1_plan_check(None) == _lib.NRM_E_ARG
	assert lib.nrm_single1_plan_results(None, None, None, None, None, None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single1_plan_info(None, None) == _lib.NRM_E_ARG and lib.nrm_single1_plan_stream(None, None) == _lib.NRM_E_ARG
	assert lib.nrm_single1_plan_time(None, 1, None) == _lib.NRM_E_ARG


def test_single1_plan_constructor_validation():
	import scipy.sparse
	from normalisr_amd import cplan
	dg, dt, dc = _problem()
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.Single1Plan(dg, dt, dc[:, :5])
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.Single1Plan(dg[:, :5], dt, dc)
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions.'):
		cplan.Single1Plan(scipy.sparse.csr_matrix(dg[:, :5]), dt, dc)
	with pytest.raises(ValueError, match='dimreduce must be an integer.'):
		cplan.Single1Plan(dg, dt, dc, dimreduce=1.5)
	with pytest.raises(ValueError, match='dimreduce must be a non-negative integer.'):
		cplan.Single1Plan(dg, dt, dc, dimreduce=-1)
	with pytest.raises(NotImplementedError, match='one dimreduce for all genes'):
		cplan.Single1Plan(dg, dt, dc, dimreduce=np.zeros(3, dtype=np.int64))
	with pytest.raises(ValueError, match='out_dtype must be float32 or float64'):
		cplan.Single1Plan(dg, dt, dc, out_dtype=np.float16)
	with pytest.raises(TypeError, match='a sparse dt is not taken here'):
		cplan.Single1Plan(dg, scipy.sparse.csr_matrix(dt), dc)
	with pytest.raises(TypeError, match='a sparse dc is not taken here'):
		cplan.Single1Plan(dg, dt, scipy.sparse.csr_matrix(dc))
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.Single1Plan(dg[0], dt, dc)
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.Single1Plan(dg, dt[0], dc)
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size.'):
		cplan.Single1Plan(dg, dt, dc[0])
	dg33, dt33, dc33 = _problem(n=40, nc=33)
	with pytest.raises(NotImplementedError, match='up to 32 covariates'):
		cplan.Single1Plan(dg33, dt33, dc33)


def _sanitized_program(tmp_path, name, says):
	"""tests/host/NAME.cpp -- a program with its own main over csrc/nrm_single1_plan_args.h -- beside csrc/nrm_small_pinv.hip (cabi_harness.build_and_run_host_program)."""
	build_and_run_host_program(tmp_path, ['normalisr_amd/csrc/nrm_small_pinv.hip', 'tests/host/{}.cpp'.format(name)], says)


def test_single1_plan_argument_checks_under_address_and_ub_sanitizers(tmp_path):
	"""csrc/nrm_single1_plan_args.h -- every check create makes before a device call -- beside tests/host/single1_plan_args_sanitize.cpp."""
	_sanitized_program(tmp_path, 'single1_plan_args_sanitize', 'single1 plan args ok')


def test_single1_status_under_address_and_ub_sanitizers(tmp_path):
	"""nrm_single1_status, the one reading of single=1's counters for the whole-problem entry and the plan (tests/host/single1_status_sanitize.cpp): all 32
	combinations of counters [0..4] give the status and message of [2] over [4] over [3] over [0] / [1], and NRM_OK for none."""
	_sanitized_program(tmp_path, 'single1_status_sanitize', 'single1 status ok')


def test_single1_plan_gpu_screens_are_well_posed():
	"""Every (seed, covariate count) tests/test_gpu_single1_plan.py builds a screen from, on the CPU through the oracle's per-grouping loop on the rows de keeps: its
	own assertions (each kept grouping takes more than one value on its selected cells, association.py:917-918) and dof > 0 hold, every P-value is finite, and de's
	filter drops exactly the two rows added."""
	import oracle
	import single1_plan_child as child
	from normalisr_amd import cplan
	for seed, nc in child.screens_used():
		dg, dt, dc = child.screen(seed, np.float64, nc)
		keep = cplan.varying_rows(dg)
		assert (np.nonzero(~keep)[0] == [child.ZERO_ROW, child.ONES_ROW]).all()
		assert dg.max() == 1 and dg.min() == 0 and 0 < child.exclusive_cells(dg) < child.N
		p, gam, _, vx, vy = oracle.association_tests(dg[keep], dt, dc, single=1, return_dot=False)
		assert p.shape == (child.NX, child.NY) and np.isfinite(p).all() and np.isfinite(gam).all() and (vx > 0).all() and (vy > 0).all(), (seed, nc)
	for nc in child.ENTRY_NCS:  # the screen of test_single1_plan_c_entry_same_bytes_as_the_host_entry
		dg, dt, dc = child.entry_screen(np.float64, nc)
		keep = cplan.varying_rows(dg)
		assert (np.nonzero(~keep)[0] == [child.ENTRY_CONST_ROW]).all()
		p, gam, _, vx, vy = oracle.association_tests(dg[keep], dt, dc, single=1, return_dot=False)
		assert p.shape == (6, 37) and np.isfinite(p).all() and np.isfinite(gam).all() and (vx > 0).all() and (vy > 0).all(), nc
	dg, dg2 = child.screen(child.SEEDS['replays'], np.float64, 3)[0], child.screen(child.SEEDS['replays'] + 1, np.float64, 3)[0]
	assert child.exclusive_cells(dg) != child.exclusive_cells(dg2)  # (set_design changes the size of the stream kernel's transposed output)
