"""Resident co-expression through the library's own plan handle (include/normalisr_hip.h: nrm_coex_plan_*): numpy, ctypes and libnormalisr_hip.so -- this module
never imports torch.  The matrix stays in HBM, a step is K1 -> K2 -> K3 as one HIP graph inside the library, and `results()` is `coex`'s contract:

	with cplan.CoexPlan(dt, dc) as plan:
		plan.step()
		p, dot, var = plan.results()      # == normalisr.coex(dt, dc)
		plan.update(dt2); plan.step()     # same shape, new values: no allocation, one graph launch

DePlan (nrm_de_plan_*) is the same for de(dg, dt, dc) with single=0 on the sparse-design kernels: the design dense or sparse, de's row filter, re-inflation and
assertions and, on request, alpha and Benjamini-Hochberg q-values on the device; `results()` is `de`'s contract.  Single1Plan (nrm_single1_plan_*) is the same
for single=1, a low-MOI screen: the row filter runs in front of the cell selection, the variances are per grouping.  Single4Plan (nrm_single4_plan_*) is the same
for single=4, a high-MOI screen in closed form: what depends on the design alone is computed when the design is set, not in a step.
FrontPlan (nrm_front_plan_*) is the front half in front of them: read counts in, normvar's (dtn, dcn) out -- lcpm, normcov, compute_var, scaling_factor and normvar
with the reference's defaults as one graph --, whose output matrix a CoexPlan or DePlan of the same process adopts.  FrontPlanCSR (nrm_front_plan_create_csr)
is the same plan on sparse counts: canonical CSR in HBM, never densified.
"""
import ctypes

import numpy as np

from . import _lib, _opts

_vp, _i64, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
INFO_FIELDS = ('engine', 'captured', 'steps', 'reruns', 'rank', 'dof', 'bytes')


class DeviceMatrix:
	"""A (rows, cols) fp32 / fp64 matrix in device-visible memory by its address, row pitch `ld` in elements: what a caller with a pointer and no array library hands
	to CoexPlan to be adopted (it is exposed as __cuda_array_interface__)."""

	def __init__(self, ptr, shape, dtype, ld=None):
		self.ptr, self.shape, self.dtype = int(ptr), (int(shape[0]), int(shape[1])), np.dtype(dtype)
		self.ld = self.shape[1] if ld is None else int(ld)

	@property
	def __cuda_array_interface__(self):
		return dict(shape=self.shape, typestr=self.dtype.str, data=(self.ptr, False), version=3, strides=(self.ld * self.dtype.itemsize, self.dtype.itemsize))


def _code(dtype):
	return _lib.NRM_F64 if np.dtype(dtype) == np.float64 else _lib.NRM_F32


def _adopt(dt):
	"""(pointer, (ng, n), numpy dtype, ld) of a device matrix: a tensor (data_ptr / stride / dtype by name) or anything with __cuda_array_interface__; None for host data."""
	if hasattr(dt, '__cuda_array_interface__') and not hasattr(dt, 'data_ptr'):
		d = dt.__cuda_array_interface__
		dtype, shape, strides = np.dtype(d['typestr']), tuple(d['shape']), d.get('strides')
		if len(shape) != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		if strides is None:
			strides = (shape[1] * dtype.itemsize, dtype.itemsize)
		if strides[1] != dtype.itemsize or strides[0] % dtype.itemsize:
			raise ValueError('CoexPlan: a device matrix must have contiguous rows')
		return int(d['data'][0]), shape, dtype, strides[0] // dtype.itemsize
	if hasattr(dt, 'data_ptr'):
		if not getattr(dt, 'is_cuda', True):
			return None
		shape = tuple(dt.shape)
		if len(shape) != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		dtype = np.dtype(str(dt.dtype).replace('torch.', ''))
		stride = tuple(dt.stride())
		if stride[1] != 1:
			raise ValueError('CoexPlan: a device matrix must have contiguous rows')
		return int(dt.data_ptr()), shape, dtype, int(stride[0])
	return None


def _matrix(dt, cls):
	"""(the array to keep alive, pointer, shape, numpy dtype, row pitch, adopted) of a plan's matrix: a host array made fp32 / fp64 and contiguous, or a device matrix as
	_adopt finds it; cls: the plan's class, for what it says of a device matrix."""
	dev = _adopt(dt)
	if dev is None:
		dt = np.asarray(dt)
		if dt.ndim != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		if dt.dtype not in (np.float32, np.float64):
			dt = dt.astype(np.float64)
		dt = np.ascontiguousarray(dt)
		return dt, dt.ctypes.data, dt.shape, dt.dtype, dt.shape[1], False
	ptr, shape, dtype, ld = dev
	if dtype not in (np.float32, np.float64):
		raise ValueError(cls + ': a device matrix must be float32 or float64')
	return dt, ptr, shape, dtype, ld, True


def _covariates(dc, pinv):
	"""(dc contiguous, its pseudo-inverse or None, its rank) as nrm_coex_plan_create and nrm_de_plan_create take them."""
	if pinv == 'numpy':
		from .association import _prepare_covariates
		dc, dci, dcr = _prepare_covariates(dc)
		dci = np.ascontiguousarray(dci, dtype=np.float64)
	else:
		dc = dc if dc.dtype in (np.float32, np.float64) else dc.astype(np.float64)
		dci, dcr = None, 0
	return np.ascontiguousarray(dc), dci, int(dcr)


class _Plan:
	"""What the plans share: the handle and its entries.  A class names its entries' prefix and the fields of its info()."""
	_prefix = None
	_info_fields = None
	_create = 'create'  # the entry that makes the handle

	def __init__(self):
		self._h = self._keep = None
		self._lib = _lib.load()

	def _set_out_dtype(self, out_dtype):
		self.out_dtype = np.dtype(self.dtype if out_dtype is None else out_dtype)
		if self.out_dtype not in (np.float32, np.float64):
			raise ValueError('out_dtype must be float32 or float64')

	def _open(self, device, keep, *args):
		"""The handle from the create entry, on `device` when one is named; keep: the matrix as _matrix returned it."""
		if device is not None:
			_lib.check(self._lib.nrm_set_device(int(device)))
		h = _vp()
		_lib.check(getattr(self._lib, self._prefix + self._create)(ctypes.byref(h), *args))
		self._h = h
		self._keep = keep if self.adopted else None  # (an adopted matrix lives as long as the plan reads it)

	def _handle(self):
		if self._h is None:
			raise ValueError(type(self).__name__ + ': the plan is closed')
		return self._h

	def _call(self, entry, *args):
		_lib.check(getattr(self._lib, self._prefix + entry)(self._handle(), *args))

	def step(self, stream=None):
		"""One step on the matrices as they stand, queued on `stream` (a hipStream_t as an integer; None: the plan's own).  Does not wait."""
		self._call('step', stream)
		return self

	def update(self, dt):
		"""New values of the same shape and dtype into the plan's own copy of dt (ValueError for an adopted matrix: its owner rewrites it in place)."""
		if self.adopted:
			raise ValueError(type(self).__name__ + '.update: the plan adopted a device matrix; its owner rewrites it in place')
		dt = np.ascontiguousarray(np.asarray(dt), dtype=self.dtype)
		if dt.shape != self.shape[-2:]:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		self._call('upload', dt.ctypes.data)
		return self

	def time(self, steps):
		"""Milliseconds per step over `steps` steps, between two device events on the plan's stream."""
		ms = _dbl(0.)
		self._call('time', int(steps), ctypes.byref(ms))
		return float(ms.value)

	def info(self):
		"""The plan's counters by name (the class's docstring says which)."""
		v = (_i64 * 8)()
		self._call('info', v)
		return dict(zip(self._info_fields, (int(x) for x in v)))

	def close(self):
		h, self._h = self._h, None
		if h is not None:
			_lib.check(getattr(self._lib, self._prefix + 'destroy')(h))
		self._keep = None

	def __enter__(self):
		return self

	def __exit__(self, *exc):
		self.close()
		return False

	def __del__(self):
		try:
			self.close()
		except Exception:  # noqa: BLE001 -- interpreter shutdown
			pass


class CoexPlan(_Plan):
	"""coex(dt, dc) resident on the GPU.  dt: a numpy array (the plan keeps its own device copy; `update` re-uploads) or a device matrix -- anything with data_ptr() or
	__cuda_array_interface__, fp32 / fp64 with contiguous rows -- which is adopted: never copied, rewritten in place by its owner between steps.  dc (nc, n) covariates.
	out_dtype: dt's by default, as coex.  device: GPU index (nrm_set_device), default the process's.  pinv='numpy' takes the pseudo-inverse and rank of dc dc^T from
	association._prepare_covariates, the function coex calls; pinv='library' leaves both to the library (nrm_covariates_pinv: no LAPACK, at most 32 covariates).
	info(): engine (0: fp64 kernel, 5 / 6: digit planes of the integer engine), captured, steps, reruns, rank, dof, bytes."""
	_prefix, _info_fields = 'nrm_coex_plan_', INFO_FIELDS

	def __init__(self, dt, dc, dimreduce=0, out_dtype=None, device=None, pinv='numpy', logp=False):
		_opts.refuse_logp(logp, 'cplan.CoexPlan')
		super().__init__()
		if pinv not in ('numpy', 'library'):
			raise ValueError("pinv must be 'numpy' or 'library'")
		if np.ndim(dimreduce) != 0 or int(dimreduce) != dimreduce:
			raise ValueError('dimreduce must be an integer.')
		dt, ptr, shape, dtype, ld, self.adopted = _matrix(dt, 'CoexPlan')
		dc = np.asarray(dc)
		if dc.ndim != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		if dc.shape[1] != shape[1]:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		self.shape, self.dtype = (int(shape[0]), int(shape[1])), np.dtype(dtype)
		self._set_out_dtype(out_dtype)
		nc = dc.shape[0]
		dc, dci, dcr = _covariates(dc, pinv)
		self._open(device, dt, ptr, _code(dtype), shape[0], shape[1], ld, 1 if self.adopted else 0, dc.ctypes.data if nc else None, _code(dc.dtype), nc,
				   None if dci is None or not nc else dci.ctypes.data, dcr, int(dimreduce), _code(self.out_dtype))

	def check(self):
		"""Waits for the queued steps and tests what they counted: AssertionError for the reference's assertions; (guard_hits, guard_worst) otherwise -- guard_hits > 0:
		the integer engine could not certify that many pairs and the step was redone on the fp64 kernel before returning."""
		hits, worst = _i64(0), _dbl(0.)
		self._call('check', ctypes.byref(hits), ctypes.byref(worst))
		return int(hits.value), float(worst.value)

	def results(self):
		"""(P-values (ng, ng), dot (ng, ng), var (ng,)) of the last step as numpy arrays of out_dtype: coex's return value."""
		ng = self.shape[0]
		p, dot, var = np.empty((ng, ng), self.out_dtype), np.empty((ng, ng), self.out_dtype), np.empty(ng, self.out_dtype)
		self._call('results', p.ctypes.data, dot.ctypes.data, var.ctypes.data)
		return p, dot, var

	def device_results(self):
		"""dict(p=, dot=, var= device addresses, ld= row pitch in elements, dtype=, stream= the plan's own stream): for a consumer queued behind the step, such as nrm_binnet."""
		p, dot, var, st, ld = _vp(), _vp(), _vp(), _vp(), _i64(0)
		self._call('device_results', ctypes.byref(p), ctypes.byref(dot), ctypes.byref(var), ctypes.byref(ld))
		self._call('stream', ctypes.byref(st))
		return dict(p=p.value, dot=dot.value, var=var.value, ld=int(ld.value), dtype=self.out_dtype, stream=st.value)


DE_INFO_FIELDS = ('route', 'captured', 'steps', 'reruns', 'rank', 'dof', 'bytes', 'rows_kept')


class DeviceCSR:
	"""A canonical CSR matrix in device-visible memory by its three addresses: indptr (rows + 1) int64, indices (nnz) int32 -- the cell of every stored entry,
	strictly increasing inside a row --, data (nnz) of `dtype`.  A design (n_grouping, n_cell) for DePlan: float32 / float64, or None for all ones.  Read counts
	(n_gene, n_cell) for FrontPlanCSR: int64 / int32 / int16 / uint8; nnz then only has to lie within the plan's nnz_cap, every step reads indptr[rows].  What a
	caller without an array library hands over; the library checks the structure (ValueError for a malformed matrix)."""

	def __init__(self, indptr, indices, data, shape, nnz, dtype=np.float64):
		self.indptr, self.indices, self.data = int(indptr), int(indices) if indices else None, int(data) if data else None
		self.shape, self.nnz, self.dtype = (int(shape[0]), int(shape[1])), int(nnz), np.dtype(dtype)
		if self.dtype not in (np.float32, np.float64) and str(self.dtype) not in ('int64', 'int32', 'int16', 'uint8'):
			raise ValueError('DeviceCSR: data must be float32 or float64 (a design), or int64, int32, int16 or uint8 (read counts)')
		if self.nnz < 0 or (self.nnz > 0 and self.indices is None):
			raise ValueError('DeviceCSR: indices are missing')


def varying_rows(dg):
	"""The rows of a design that de tests (de.py:93: more than one distinct value, NaNs equal), stated as the plan's kernels decide it.  dg: a dense matrix, or a
	scipy.sparse matrix in CSR form whose stored zeros are not entries.  k entries among n cells: 0 < k < n varies, k == 0 does not, k == n varies when the values
	differ; with n < 2 no row varies."""
	from . import de_sparse
	if de_sparse._is_scipy_sparse(dg):
		m = dg.tocsr()
		rows, n = m.shape
		out = np.zeros(rows, dtype=bool)
		for i in range(rows):
			v = np.asarray(m.data[m.indptr[i]:m.indptr[i + 1]], dtype=np.float64)
			v = v[v != 0]  # (a NaN != 0: an entry)
			k = v.size
			full = k == n and n > 1 and bool(((v != v[0]) & ~(np.isnan(v) & np.isnan(v[0]))).any())
			out[i] = (0 < k < n) or full
		return out
	dg = np.asarray(dg)
	rows, n = dg.shape
	if n < 2:
		return np.zeros(rows, dtype=bool)
	first = dg[:, :1]
	diff = dg != first
	if dg.dtype.kind == 'f':
		diff &= ~(np.isnan(dg) & np.isnan(first))
	return diff.any(axis=1)


def _design(dg):
	"""The arguments nrm_de_plan_create / nrm_de_plan_design take for a design, its shape, and what must stay alive while the library reads it."""
	from . import de_sparse
	if isinstance(dg, DeviceCSR):
		if dg.dtype not in (np.float32, np.float64):
			raise ValueError('DeviceCSR: the data of a design must be float32 or float64')
		return (1, dg.data, _code(dg.dtype), 0, dg.indptr, dg.indices, dg.nnz, 1), dg.shape, dg
	csr = de_sparse.as_design_csr(dg)
	if csr is not None:
		from . import engine as _engine
		indptr, indices, data, code, nnz = csr._ready(_engine.get_engine(csr.device.index))
		return (1, None if data is None else data.data_ptr(), code, 0, indptr.data_ptr(), indices.data_ptr() if nnz else None, nnz, 1), tuple(csr.shape), (indptr, indices, data)
	if de_sparse._is_scipy_sparse(dg):
		if len(dg.shape) != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		indptr, indices, data = (np.ascontiguousarray(a) for a in de_sparse.canonical_design_csr(dg))
		return (1, data.ctypes.data, _code(data.dtype), 0, indptr.ctypes.data, indices.ctypes.data, int(indices.size), 0), tuple(int(v) for v in dg.shape), (indptr, indices, data)
	dev = _adopt(dg)
	if dev is not None:
		ptr, shape, dtype, ld = dev
		if dtype not in (np.float32, np.float64):
			raise ValueError('DePlan: a device matrix must be float32 or float64')
		return (0, ptr, _code(dtype), ld, None, None, 0, 1), (int(shape[0]), int(shape[1])), dg
	dg = np.asarray(dg)
	if dg.ndim != 2:
		raise ValueError('Incorrect dx/dy/dc size.')
	if dg.dtype.kind not in 'iufb':
		raise TypeError('the design matrix must hold real numbers.')
	if dg.dtype not in (np.float32, np.float64):
		dg = dg.astype(np.float64)
	dg = np.ascontiguousarray(dg)
	return (0, dg.ctypes.data, _code(dg.dtype), dg.shape[1], None, None, 0, 0), dg.shape, dg


class _DesignPlan(_Plan):
	"""What DePlan, Single1Plan and Single4Plan share: a design beside the matrix, de's five results and the q-values."""

	def _problem(self, dg, dt, dc, lowmem, q, out_dtype):
		"""The constructors' common part: sets shape, dtype, adopted, out_dtype, nc, lowmem and q; returns the design's arguments, the matrix as _matrix returns it
		without `adopted`, and dc as an array."""
		from . import de_sparse
		de_sparse.refuse_sparse(dt, 'dt')
		de_sparse.refuse_sparse(dc, 'dc')
		dt, ptr, shape, dtype, ld, self.adopted = _matrix(dt, type(self).__name__)
		dc = np.asarray(dc)
		if dc.ndim != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		gargs, gshape, gkeep = _design(dg)  # (gkeep lives until create has read the design: the caller holds gargs no longer than that)
		if dc.shape[1] != shape[1] or gshape[1] != shape[1]:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		self.shape, self.dtype = (int(gshape[0]), int(shape[0]), int(shape[1])), np.dtype(dtype)
		self._set_out_dtype(out_dtype)
		self.nc = int(dc.shape[0])
		self.lowmem, self.q = bool(lowmem), bool(q)
		return (gargs, gkeep), (dt, ptr, shape, dtype, ld), dc

	def _fetch(self, want_q):
		ng0, nt, _ = self.shape
		o = self.out_dtype
		if want_q:
			qv = np.empty((ng0, nt), o)
			self._call('results', None, None, None, None, None, qv.ctypes.data)
			return qv
		p, gam, varg, vart = np.empty((ng0, nt), o), np.empty((ng0, nt), o), np.empty(ng0, o), np.empty((ng0, nt), o)
		alpha = None if self.lowmem else np.zeros((ng0, nt, self.nc), o)
		self._call('results', p.ctypes.data, gam.ctypes.data, alpha.ctypes.data if (alpha is not None and self.nc) else None, varg.ctypes.data, vart.ctypes.data, None)
		return p, gam, alpha, varg, vart

	def results(self):
		"""(P-values (n_group, n_gene), gamma (n_group, n_gene), alpha (n_group, n_gene, n_cov) | None, varg (n_group,), vart (n_group, n_gene)) of the last step as numpy
		arrays of out_dtype: de's return value."""
		return self._fetch(False)

	def qvalues(self):
		"""The Benjamini-Hochberg q-values (n_group, n_gene) of the last step's P-values: binnet.bh of them, bit for bit (a plan created with q=True)."""
		if not self.q:
			raise ValueError(type(self).__name__ + '.qvalues: the plan was created without q=True')
		return self._fetch(True)

	def device_results(self):
		"""dict(p=, gamma=, alpha=, varg=, q= full-size device addresses (None for what the plan was created without), vart= the genes' variances -- (n_gene) for DePlan,
		full-size (n_group, n_gene) for Single1Plan and Single4Plan --, mask= one byte per grouping (1: tested), ld= row pitch in elements, dtype=, stream= the plan's own stream): for a
		consumer queued behind the step."""
		v = [_vp() for _ in range(7)]
		st, ld = _vp(), _i64(0)
		self._call('device_results', *[ctypes.byref(x) for x in v], ctypes.byref(ld))
		self._call('stream', ctypes.byref(st))
		out = dict(zip(('p', 'gamma', 'alpha', 'varg', 'q', 'vart', 'mask'), (x.value for x in v)))
		out.update(ld=int(ld.value), dtype=self.out_dtype, stream=st.value)
		return out

	def set_design(self, dg):
		"""Another design of the same shape, in any of the forms the constructor takes: the row filter, the compaction and the lists (for Single1Plan the cell selection
		too) again, and a new graph from the second step on it."""
		gargs, gshape, gkeep = _design(dg)
		if tuple(int(v) for v in gshape) != (self.shape[0], self.shape[2]):
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		self._call('design', *gargs)
		del gkeep
		return self


class DePlan(_DesignPlan):
	"""de(dg, dt, dc) with single=0 resident on the GPU, on the sparse-design kernels whatever the size (include/normalisr_hip.h: nrm_de_plan_*):

		with cplan.DePlan(dg, dt, dc, lowmem=False, q=True) as plan:
			plan.step()
			p, gamma, alpha, varg, vart = plan.results()   # == normalisr.de(dg, dt, dc, lowmem=False)
			q = plan.qvalues()                              # == binnet.bh(p)
			plan.update(dt2); plan.step()                   # same shape, new values: one graph launch
			plan.set_design(dg2); plan.step()               # another design of the same shape

	dg: a numpy matrix, a scipy.sparse matrix (canonicalised by de_sparse.canonical_design_csr), a de_sparse.DesignCSR, a DeviceCSR, or a dense device matrix (anything
	CoexPlan adopts); it is read when it is set and not kept.  dt: a numpy array (the plan keeps its own device copy; `update` re-uploads) or a device matrix, adopted
	and rewritten in place by its owner.  lowmem=False adds alpha; q=True adds the q-values of all P-values to every step.  out_dtype: dt's by default, as de.
	pinv as for CoexPlan.
	info(): route (0: the sparse-design kernels, 1: K1 and the fp64 Gram kernel after a hand-back), captured, steps, reruns, rank, dof, bytes, rows_kept."""
	_prefix, _info_fields = 'nrm_de_plan_', DE_INFO_FIELDS

	def __init__(self, dg, dt, dc, dimreduce=0, lowmem=True, q=False, out_dtype=None, device=None, pinv='numpy', logp=False):
		_opts.refuse_logp(logp, 'cplan.DePlan')
		super().__init__()
		if pinv not in ('numpy', 'library'):
			raise ValueError("pinv must be 'numpy' or 'library'")
		if np.ndim(dimreduce) != 0 or int(dimreduce) != dimreduce:
			raise ValueError('dimreduce must be an integer.')
		(gargs, gkeep), (dt, ptr, shape, dtype, ld), dc = self._problem(dg, dt, dc, lowmem, q, out_dtype)
		nc = self.nc
		dc, dci, dcr = _covariates(dc, pinv)
		self._open(device, dt, *gargs, self.shape[0], ptr, _code(dtype), shape[0], shape[1], ld, 1 if self.adopted else 0, dc.ctypes.data if nc else None, _code(dc.dtype), nc,
				   None if dci is None or not nc else dci.ctypes.data, dcr, int(dimreduce), _code(self.out_dtype), 0 if self.lowmem else 1, 1 if self.q else 0)
		del gkeep  # (the design was read inside create)

	def check(self):
		"""Waits for the queued steps and tests what they counted: AssertionError for the reference's assertions (association.py:248,252; de.py:124-131).  Returns the rows
		handed back since the last check -- > 0: rows all but inside the covariates' span; the step was redone on K1 and the fp64 Gram kernel before returning, and the
		plan stays on that route until set_design."""
		back = _i64(0)
		self._call('check', ctypes.byref(back))
		return int(back.value)


S1_INFO_FIELDS = ('route', 'captured', 'steps', 'cells_kept', 'covariates', 'reserved', 'bytes', 'rows_kept')


class Single1Plan(_DesignPlan):
	"""de(dg, dt, dc, single=1) -- a low-MOI screen: every grouping tested on the cells that carry no other grouping -- resident on the GPU (include/normalisr_hip.h:
	nrm_single1_plan_*):

		with cplan.Single1Plan(dg, dt, dc, lowmem=False, q=True) as plan:
			plan.step()
			p, gamma, alpha, varg, vart = plan.results()   # == normalisr.de(dg, dt, dc, single=1, lowmem=False)
			q = plan.qvalues()                              # == binnet.bh(p)
			plan.update(dt2); plan.step()                   # same shape, new values: one graph launch
			plan.set_design(dg2); plan.step()               # another design of the same shape

	dg, dt, lowmem, q and out_dtype as DePlan takes them.  The design's entries are >= 0 with the largest equal to 1 and at most a quarter of them set, dc has at most
	32 covariates (NotImplementedError otherwise); dimreduce is a scalar.  The pseudo-inverses are per grouping and taken on the device: there is no `pinv`.
	info(): route (0), captured, steps, cells_kept (cells that carry exactly one grouping), covariates, reserved (0), bytes, rows_kept."""
	_prefix, _info_fields = 'nrm_single1_plan_', S1_INFO_FIELDS

	def __init__(self, dg, dt, dc, dimreduce=0, lowmem=True, q=False, out_dtype=None, device=None, logp=False):
		_opts.refuse_logp(logp, 'cplan.Single1Plan')
		super().__init__()
		if np.ndim(dimreduce) != 0:
			raise NotImplementedError('Single1Plan: one dimreduce for all genes (association_tests(..., single=1) takes one per gene)')
		if int(dimreduce) != dimreduce:
			raise ValueError('dimreduce must be an integer.')
		(gargs, gkeep), (dt, ptr, shape, dtype, ld), dc = self._problem(dg, dt, dc, lowmem, q, out_dtype)
		nc = self.nc
		dc = np.ascontiguousarray(dc if dc.dtype in (np.float32, np.float64) else dc.astype(np.float64))
		self._open(device, dt, *gargs, self.shape[0], ptr, _code(dtype), shape[0], shape[1], ld, 1 if self.adopted else 0, dc.ctypes.data if nc else None, _code(dc.dtype), nc,
				   int(dimreduce), _code(self.out_dtype), 0 if self.lowmem else 1, 1 if self.q else 0)
		del gkeep  # (the design was read inside create)

	def check(self):
		"""Waits for the queued steps and tests what they counted, as the reference would have raised it: AssertionError for a grouping with a single value on the cells
		selected for it (association.py:917-918) and for the result assertions (association.py:248,252; de.py:124-131), ValueError for covariates that are not finite,
		RuntimeError for too few cells."""
		self._call('check')


class Single4Plan(_DesignPlan):
	"""de(dg, dt, dc, single=4) -- a high-MOI screen: every grouping tested with all the others as covariates, in closed form -- resident on the GPU
	(include/normalisr_hip.h: nrm_single4_plan_*):

		with cplan.Single4Plan(dg, dt, dc, lowmem=False, q=True) as plan:
			plan.step()
			p, gamma, alpha, varg, vart = plan.results()   # == normalisr.de(dg, dt, dc, single=4, lowmem=False)
			q = plan.qvalues()                              # == binnet.bh(p)
			plan.update(dt2); plan.step()                   # same shape, new values: one graph launch
			plan.set_design(dg2); plan.step()               # another design of the same shape: the design side again, once

	dg, dt, lowmem, q, out_dtype and pinv as DePlan takes them; dimreduce is a scalar.  Everything that depends on the design and the covariates alone -- M~, its
	inverse, the design scalars, the rank decision at `tol` -- is computed when the design is set, not in a step.  NotImplementedError where the closed form has no
	certificate (design rows dependent given the covariates, covariates of rank 0, more covariates than the sparse-design kernel takes): normalisr.de(..., single=4)
	covers those.
	info(): route (0: the sparse-design kernels, 1: K1 and the fp64 Gram kernel after a hand-back), captured, steps, reruns, rank, dof, bytes, rows_kept."""
	_prefix, _info_fields = 'nrm_single4_plan_', DE_INFO_FIELDS

	def __init__(self, dg, dt, dc, dimreduce=0, lowmem=True, q=False, out_dtype=None, device=None, pinv='numpy', tol=1e-8, logp=False):
		_opts.refuse_logp(logp, 'cplan.Single4Plan')
		super().__init__()
		if pinv not in ('numpy', 'library'):
			raise ValueError("pinv must be 'numpy' or 'library'")
		if np.ndim(dimreduce) != 0:
			raise NotImplementedError('Single4Plan: one dimreduce for all genes (association_tests(..., single=4) takes one per gene)')
		if int(dimreduce) != dimreduce:
			raise ValueError('dimreduce must be an integer.')
		(gargs, gkeep), (dt, ptr, shape, dtype, ld), dc = self._problem(dg, dt, dc, lowmem, q, out_dtype)
		nc = self.nc
		if pinv == 'numpy' and nc:  # the reference's own pseudo-inverse and rank of dc dc^T at `tol` (association.py:527-528)
			from .association import inv_rank
			dc = np.ascontiguousarray(dc, dtype=np.float64)
			if (dc != 0).any():
				dci, dcr = inv_rank(np.matmul(dc, dc.T), tol=tol)
			else:
				dci, dcr = np.zeros((nc, nc)), 0
			dci = np.ascontiguousarray(dci, dtype=np.float64)
		else:
			dc, dci, dcr = _covariates(dc, 'library')
		self._open(device, dt, *gargs, self.shape[0], ptr, _code(dtype), shape[0], shape[1], ld, 1 if self.adopted else 0, dc.ctypes.data if nc else None, _code(dc.dtype), nc,
				   None if dci is None or not nc else dci.ctypes.data, int(dcr), int(dimreduce), _code(self.out_dtype), 0 if self.lowmem else 1, 1 if self.q else 0, float(tol))
		del gkeep  # (the design was read inside create)

	def check(self):
		"""Waits for the queued steps and tests what they counted.  Returns the expression rows handed back since the last check -- > 0: rows all but inside the
		covariates' span; the design side and the step were redone on K1 and the fp64 Gram kernel before returning, and the plan stays on that route until
		set_design.  AssertionError for the reference's assertions on what then stands (association.py:557; de.py:124-131)."""
		back = _i64(0)
		self._call('check', ctypes.byref(back))
		return int(back.value)


FRONT_INFO_FIELDS = ('captured', 'steps', 'cv_steps', 'max_count', 'count_cap', 'covariates', 'bytes', 'near_constant')
_COUNT_CODES = {'int64': _lib.NRM_I64, 'int32': _lib.NRM_I32, 'int16': _lib.NRM_I16, 'uint8': _lib.NRM_U8}


class _FrontPlan(_Plan):
	"""What FrontPlan and FrontPlanCSR share: the checks of the options, check() and everything that reads a step's results."""
	_prefix, _info_fields = 'nrm_front_plan_', FRONT_INFO_FIELDS

	def _options(self, cov, stepmax, eps, ntot, out_dtype):
		"""The options both constructors take, checked; self.shape is set.  -> cov as a contiguous float64 matrix (n_cov, n_cell)."""
		self.out_dtype = np.dtype(out_dtype)
		if self.out_dtype not in (np.float32, np.float64):
			raise ValueError('out_dtype must be float32 or float64')
		if eps <= 0 or stepmax <= 0:
			raise ValueError('eps and stepmax must be positive.')
		if int(stepmax) != stepmax:
			raise ValueError('stepmax must be an integer.')
		cov = np.zeros((0, self.shape[1])) if cov is None else np.asarray(cov)
		if cov.ndim != 2:
			raise ValueError('Covariates must have 2 dimensions.')
		if cov.shape[1] != self.shape[1]:
			raise ValueError('reads and cov must have the same cell count.')
		if cov.dtype.kind not in 'iufb':
			raise TypeError('cov must hold real numbers.')
		cov = np.ascontiguousarray(cov, dtype=np.float64)
		self.n_cov = int(cov.shape[0])
		self.covariates = self.n_cov + 4  # lcpm's three rows and the constant row
		if ntot is not None and (int(ntot) != ntot or ntot <= 0):
			raise ValueError('ntot must be a positive integer.')
		return cov

	def _set_count_cap(self, count_cap, values):
		"""count_cap as given, or (None, host input) the next power of two above the largest of `values`, 256 at the least."""
		if count_cap is None:
			top = int(values.max()) if values.size else 0
			if top >= int(self._lib.nrm_lcpm_table_cap()):
				raise NotImplementedError('{} tabulates psi(1 + count) for counts below {}; the largest count here is {}.'.format(type(self).__name__, int(self._lib.nrm_lcpm_table_cap()), top))
			count_cap = max(256, 1 << max(top, 0).bit_length())
		if int(count_cap) != count_cap:
			raise ValueError('count_cap must be an integer.')
		self.count_cap = int(count_cap)

	def _tail(self, cov, ntot, stepmax, eps, tol):
		"""The arguments both create entries end in."""
		return (cov.ctypes.data if self.n_cov else None, self.n_cov, -1 if ntot is None else int(ntot), int(stepmax), float(eps), float(tol), _code(self.out_dtype), self.count_cap)

	def check(self):
		"""Waits for the queued steps and tests what they counted, in the order the reference would meet it: ValueError for a negative entry, AssertionError for a
		matrix without a read, ValueError for a cell without a read, NotImplementedError for a count at or beyond count_cap, ValueError for a constant covariate,
		AssertionError for compute_var's, scaling_factor's and normvar's assertions, RuntimeError for zero-rank covariates.  Returns the rows normcov would warn about
		as near constant since the last check, under the same RuntimeWarning."""
		near = _i64(0)
		self._call('check', ctypes.byref(near))
		if near.value:
			import warnings
			warnings.warn('Detected near constant covariate. Results may be error-prone.', RuntimeWarning)
		return int(near.value)

	def _fetch(self, **want):
		ng, n = self.shape
		shapes = dict(dtn=((ng, n), self.out_dtype), dcn=((self.covariates, n), np.float64), w=((n, ), np.float64), wt=((ng, ), np.float64), lcpm=((ng, n), self.out_dtype),
					  cov=((self.covariates, n), np.float64))
		out = {k: np.empty(*shapes[k]) for k in shapes if want.get(k)}
		self._call('results', *[out[k].ctypes.data if k in out else None for k in ('dtn', 'dcn', 'w', 'wt', 'lcpm', 'cov')])
		return out

	def results(self):
		"""[dtn (n_gene, n_cell) of out_dtype, dcn (n_cov + 4, n_cell) float64] of the last step: normvar's return value."""
		out = self._fetch(dtn=True, dcn=True)
		return [out['dtn'], out['dcn']]

	def weights(self):
		"""compute_var's weights (n_cell,) of the last step."""
		return self._fetch(w=True)['w']

	def scaling(self):
		"""scaling_factor's result (n_gene,) of the last step."""
		return self._fetch(wt=True)['wt']

	def lcpm(self):
		"""lcpm (n_gene, n_cell) of out_dtype of the last step."""
		return self._fetch(lcpm=True)['lcpm']

	def normcov(self):
		"""normcov([cov; lcpm's three rows]) with the constant row, (n_cov + 4, n_cell) float64, of the last step."""
		return self._fetch(cov=True)['cov']

	def device_results(self):
		"""dict(dtn=, lcpm= DeviceMatrix objects of out_dtype -- what CoexPlan and DePlan adopt --, dcn= the device address of the scaled covariates (n_cov + 4, n_cell)
		float64, ld= row pitch in elements, dtype=, stream= the plan's own stream)."""
		dtn, dcn, lc, st, ld = _vp(), _vp(), _vp(), _vp(), _i64(0)
		self._call('device_results', ctypes.byref(dtn), ctypes.byref(dcn), ctypes.byref(lc), ctypes.byref(ld), ctypes.byref(st))
		return dict(dtn=DeviceMatrix(dtn.value, self.shape, self.out_dtype, ld.value), lcpm=DeviceMatrix(lc.value, self.shape, self.out_dtype, ld.value), dcn=dcn.value,
					ld=int(ld.value), dtype=self.out_dtype, stream=st.value)


class FrontPlan(_FrontPlan):
	"""Read counts to normalised expression resident on the GPU (include/normalisr_hip.h: nrm_front_plan_*): lcpm -> normcov -> compute_var -> scaling_factor ->
	normvar with the reference's default options as one HIP graph, nothing decided on the host in between:

		with cplan.FrontPlan(reads, cov=batches, stepmax=1) as front:
			front.step()
			dtn, dcn = front.results()                      # == normvar(lcpm(reads)[0], normcov(vstack([batches, lcpm(reads)[3]])), w, scaling_factor(reads))
			coex = cplan.CoexPlan(front.device_results()['dtn'], dcn)   # adopts the matrix where it lies
			front.update(reads2); front.step()              # same shape and dtype, new counts: one graph launch

	reads (n_gene, n_cell): a numpy integer array (int64 / int32 / int16 / uint8 as they are, other integer types as int64; the plan keeps its own device copy and
	`update` re-uploads) or a device matrix of one of those four dtypes -- anything with data_ptr() or __cuda_array_interface__, such as a DeviceMatrix -- which is
	adopted and rewritten in place by its owner.  cov (n_cov, n_cell): the raw covariate rows stacked in front of lcpm's three before normcov (None: none); with
	lcpm's three and the constant row there may be nrm_normvar_device_covariates() in all (NotImplementedError beyond).  stepmax, eps: compute_var's; ntot: lcpm's;
	tol: normvar's; out_dtype: float64 (the reference's) or float32 for lcpm and dtn.  count_cap: the tables hold counts below it; None for host input: the next
	power of two above the matrix's maximum, 256 at the least; an adopted matrix must name one.  A step whose largest count reaches the cap is refused by check().
	Not covered: the non-default options of lcpm / normcov / scaling_factor / normvar, qc_outlier and subset between fitvar and normvar (weights() is there for a
	caller who wants them).  Sparse counts are FrontPlanCSR's.
	info(): captured, steps, cv_steps (iterations compute_var took in the last step checked), max_count (of that step), count_cap, covariates, bytes, near_constant."""

	def __init__(self, reads, cov=None, stepmax=1, eps=1e-6, ntot=None, tol=1e-8, out_dtype=np.float64, count_cap=None, device=None):
		super().__init__()
		if hasattr(reads, 'tocsr') or isinstance(reads, DeviceCSR):
			raise TypeError('FrontPlan: a sparse reads is not taken here (FrontPlanCSR takes one).')
		dev = _adopt(reads)
		if dev is None:
			reads = np.asarray(reads)
			if reads.ndim != 2:
				raise ValueError('reads must have 2 dimensions.')
			if reads.dtype.kind not in 'iub':
				raise TypeError('reads must be an integer matrix.')
			if str(reads.dtype) not in _COUNT_CODES:
				reads = reads.astype(np.int64)
			reads = np.ascontiguousarray(reads)
			ptr, shape, dtype, ld, self.adopted = reads.ctypes.data, reads.shape, reads.dtype, reads.shape[1], False
		else:
			ptr, shape, dtype, ld = dev
			self.adopted = True
			if str(dtype) not in _COUNT_CODES:
				raise ValueError('FrontPlan: a device matrix must be int64, int32, int16 or uint8')
			if count_cap is None:
				raise ValueError('FrontPlan: count_cap must be given for a device matrix (its maximum is not looked at here)')
		self.shape, self.dtype = (int(shape[0]), int(shape[1])), np.dtype(dtype)
		cov = self._options(cov, stepmax, eps, ntot, out_dtype)
		self._set_count_cap(count_cap, reads)
		self._open(device, reads, ptr, _COUNT_CODES[str(self.dtype)], self.shape[0], self.shape[1], ld, 1 if self.adopted else 0, *self._tail(cov, ntot, stepmax, eps, tol))


class FrontPlanCSR(_FrontPlan):
	"""FrontPlan on sparse read counts (nrm_front_plan_create_csr): canonical CSR over the genes resident in HBM, the same step as one HIP graph, and no
	(n_gene, n_cell) matrix of counts anywhere -- the plan is CSR whatever the density.

		with cplan.FrontPlanCSR(scipy.sparse.csr_matrix(reads), cov=batches, nnz_cap=2 * reads.nnz) as front:
			front.step()
			dtn, dcn = front.results()
			front.update(reads2); front.step()              # same shape and dtype, any pattern with at most nnz_cap stored entries: one graph launch

	reads (n_gene, n_cell): any scipy.sparse matrix of an integer dtype, canonicalised on the host (lcpm.canonical_csr: duplicates summed, columns sorted, zeros
	dropped; int64 / int32 / int16 / uint8 data as they are, other integer types as int64), of which the plan keeps its own three device arrays of nnz_cap entries
	(None: the matrix's own count) that `update` rewrites; or a cplan.DeviceCSR of one of those four dtypes, which is adopted: its owner rewrites the three arrays in
	place, the pattern included, every step reads the number of stored entries from indptr[n_gene], and count_cap and nnz_cap (the elements indices and data hold)
	must be named.  The other arguments, the methods and info() are FrontPlan's.  check() raises ValueError for a malformed matrix -- indptr not rising from 0 to at
	most nnz_cap, a column outside [0, n_cell) or not above the one before it -- in front of FrontPlan's exceptions; no step reads outside the arrays for one."""
	_create = 'create_csr'

	def __init__(self, reads, cov=None, stepmax=1, eps=1e-6, ntot=None, tol=1e-8, out_dtype=np.float64, count_cap=None, nnz_cap=None, device=None):
		super().__init__()
		self.adopted = isinstance(reads, DeviceCSR)
		if self.adopted:
			if str(reads.dtype) not in _COUNT_CODES:
				raise ValueError('FrontPlanCSR: a DeviceCSR of read counts must be int64, int32, int16 or uint8')
			if count_cap is None or nnz_cap is None:
				raise ValueError('FrontPlanCSR: count_cap and nnz_cap must be given for a DeviceCSR (its arrays are not looked at here)')
			if reads.indices is None or reads.data is None:
				raise ValueError('FrontPlanCSR: a DeviceCSR of read counts has indices and data')
			self.shape, self.dtype = reads.shape, reads.dtype
			ptrs, nnz, values = (reads.indptr, reads.indices, reads.data), reads.nnz, None
		else:
			arrays = self._host_csr(reads, None)
			self.shape, self.dtype = (int(reads.shape[0]), int(reads.shape[1])), arrays[2].dtype
			ptrs, nnz, values = tuple(a.ctypes.data for a in arrays), int(arrays[2].size), arrays[2]
		cov = self._options(cov, stepmax, eps, ntot, out_dtype)
		self._set_count_cap(count_cap, values)
		if nnz_cap is None:
			nnz_cap = max(nnz, 1)  # (a matrix without a stored entry still gets arrays: check() then says that it holds no read)
		if int(nnz_cap) != nnz_cap:
			raise ValueError('nnz_cap must be an integer.')
		self.nnz_cap = int(nnz_cap)
		if self.nnz_cap < max(nnz, 1):
			raise ValueError('FrontPlanCSR: nnz_cap = {} is below the {} stored entries of reads (and 1 at the least)'.format(self.nnz_cap, nnz))
		self._open(device, reads, ptrs[0], ptrs[1], ptrs[2], _COUNT_CODES[str(self.dtype)], self.shape[0], self.shape[1], nnz, self.nnz_cap, 1 if self.adopted else 0,
				   *self._tail(cov, ntot, stepmax, eps, tol))

	@staticmethod
	def _host_csr(reads, dtype):
		"""(indptr int64, indices int32, data) of a scipy.sparse count matrix, canonical and contiguous; data in the plan's dtype (None: the one FrontPlan would keep
		the input in)."""
		if not hasattr(reads, 'tocsr'):
			raise TypeError('FrontPlanCSR: reads must be a scipy.sparse matrix or a cplan.DeviceCSR (FrontPlan takes a dense matrix).')
		if len(reads.shape) != 2:
			raise ValueError('reads must have 2 dimensions.')
		if reads.dtype.kind not in 'iub':
			raise TypeError('reads must be an integer matrix.')
		want = reads.dtype if str(reads.dtype) in _COUNT_CODES else np.dtype(np.int64)
		if dtype is not None and want != dtype:
			raise ValueError('FrontPlanCSR.update: reads of dtype {}, the plan holds {}'.format(want, dtype))
		from .lcpm import canonical_csr  # (imports without torch)
		indptr, indices, data = canonical_csr(reads)
		return np.ascontiguousarray(indptr), np.ascontiguousarray(indices), np.ascontiguousarray(data.astype(want))

	def update(self, reads):
		"""New counts of the same shape and dtype, of any pattern with at most nnz_cap stored entries, into the plan's own arrays (ValueError beyond nnz_cap, before
		any device call, and for an adopted matrix: its owner rewrites it in place)."""
		if self.adopted:
			raise ValueError('FrontPlanCSR.update: the plan adopted a device matrix; its owner rewrites it in place')
		indptr, indices, data = self._host_csr(reads, self.dtype)
		if tuple(int(v) for v in reads.shape) != self.shape:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		if data.size > self.nnz_cap:
			raise ValueError('FrontPlanCSR.update: {} stored entries, beyond the plan\'s nnz_cap = {}'.format(int(data.size), self.nnz_cap))
		self._call('upload_csr', indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, int(data.size))
		return self


assert __name__ != "__main__"
