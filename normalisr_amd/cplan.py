"""Resident co-expression through the library's own plan handle (include/normalisr_hip.h: nrm_coex_plan_*): numpy, ctypes and libnormalisr_hip.so -- this module
never imports torch.  The matrix stays in HBM, a step is K1 -> K2 -> K3 as one HIP graph inside the library, and `results()` is `coex`'s contract:

	with cplan.CoexPlan(dt, dc) as plan:
		plan.step()
		p, dot, var = plan.results()      # == normalisr.coex(dt, dc)
		plan.update(dt2); plan.step()     # same shape, new values: no allocation, one graph launch
"""
import ctypes

import numpy as np

from . import _lib

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


class CoexPlan:
	"""coex(dt, dc) resident on the GPU.  dt: a numpy array (the plan keeps its own device copy; `update` re-uploads) or a device matrix -- anything with data_ptr() or
	__cuda_array_interface__, fp32 / fp64 with contiguous rows -- which is adopted: never copied, rewritten in place by its owner between steps.  dc (nc, n) covariates.
	out_dtype: dt's by default, as coex.  device: GPU index (nrm_set_device), default the process's.  pinv='numpy' takes the pseudo-inverse and rank of dc dc^T from
	association._prepare_covariates, the function coex calls; pinv='library' leaves both to the library (nrm_covariates_pinv: no LAPACK, at most 32 covariates)."""

	def __init__(self, dt, dc, dimreduce=0, out_dtype=None, device=None, pinv='numpy'):
		self._h = None
		lib = self._lib = _lib.load()
		if pinv not in ('numpy', 'library'):
			raise ValueError("pinv must be 'numpy' or 'library'")
		if np.ndim(dimreduce) != 0 or int(dimreduce) != dimreduce:
			raise ValueError('dimreduce must be an integer.')
		dev = _adopt(dt)
		if dev is None:
			dt = np.asarray(dt)
			if dt.ndim != 2:
				raise ValueError('Incorrect dx/dy/dc size.')
			if dt.dtype not in (np.float32, np.float64):
				dt = dt.astype(np.float64)
			dt = np.ascontiguousarray(dt)
			ptr, shape, dtype, ld = dt.ctypes.data, dt.shape, dt.dtype, dt.shape[1]
		else:
			ptr, shape, dtype, ld = dev
			if dtype not in (np.float32, np.float64):
				raise ValueError('CoexPlan: a device matrix must be float32 or float64')
		dc = np.asarray(dc)
		if dc.ndim != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		if dc.shape[1] != shape[1]:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		self.shape, self.dtype, self.adopted = (int(shape[0]), int(shape[1])), np.dtype(dtype), dev is not None
		self.out_dtype = np.dtype(dtype if out_dtype is None else out_dtype)
		if self.out_dtype not in (np.float32, np.float64):
			raise ValueError('out_dtype must be float32 or float64')
		nc = dc.shape[0]
		if pinv == 'numpy':
			from .association import _prepare_covariates
			dc, dci, dcr = _prepare_covariates(dc)
			dci = np.ascontiguousarray(dci, dtype=np.float64)
		else:
			dc = dc if dc.dtype in (np.float32, np.float64) else dc.astype(np.float64)
			dci, dcr = None, 0
		dc = np.ascontiguousarray(dc)
		if device is not None:
			_lib.check(lib.nrm_set_device(int(device)))
		h = _vp()
		_lib.check(lib.nrm_coex_plan_create(ctypes.byref(h), ptr, _code(dtype), shape[0], shape[1], ld, 1 if self.adopted else 0, dc.ctypes.data if nc else None, _code(dc.dtype),
											nc, None if dci is None or not nc else dci.ctypes.data, int(dcr), int(dimreduce), _code(self.out_dtype)))
		self._h = h
		self._keep = dt if self.adopted else None  # (an adopted matrix lives as long as the plan reads it)

	def _handle(self):
		if self._h is None:
			raise ValueError('CoexPlan: the plan is closed')
		return self._h

	def step(self, stream=None):
		"""One coex on the matrix as it stands, queued on `stream` (a hipStream_t as an integer; None: the plan's own).  Does not wait."""
		_lib.check(self._lib.nrm_coex_plan_step(self._handle(), stream))
		return self

	def check(self):
		"""Waits for the queued steps and tests what they counted: AssertionError for the reference's assertions; (guard_hits, guard_worst) otherwise -- guard_hits > 0:
		the integer engine could not certify that many pairs and the step was redone on the fp64 kernel before returning."""
		hits, worst = _i64(0), _dbl(0.)
		_lib.check(self._lib.nrm_coex_plan_check(self._handle(), ctypes.byref(hits), ctypes.byref(worst)))
		return int(hits.value), float(worst.value)

	def results(self):
		"""(P-values (ng, ng), dot (ng, ng), var (ng,)) of the last step as numpy arrays of out_dtype: coex's return value."""
		ng = self.shape[0]
		p, dot, var = np.empty((ng, ng), self.out_dtype), np.empty((ng, ng), self.out_dtype), np.empty(ng, self.out_dtype)
		_lib.check(self._lib.nrm_coex_plan_results(self._handle(), p.ctypes.data, dot.ctypes.data, var.ctypes.data))
		return p, dot, var

	def device_results(self):
		"""dict(p=, dot=, var= device addresses, ld= row pitch in elements, dtype=, stream= the plan's own stream): for a consumer queued behind the step, such as nrm_binnet."""
		p, dot, var, st, ld = _vp(), _vp(), _vp(), _vp(), _i64(0)
		_lib.check(self._lib.nrm_coex_plan_device_results(self._handle(), ctypes.byref(p), ctypes.byref(dot), ctypes.byref(var), ctypes.byref(ld)))
		_lib.check(self._lib.nrm_coex_plan_stream(self._handle(), ctypes.byref(st)))
		return dict(p=p.value, dot=dot.value, var=var.value, ld=int(ld.value), dtype=self.out_dtype, stream=st.value)

	def update(self, dt):
		"""New values of the same shape and dtype into the plan's own copy of the matrix (ValueError for an adopted matrix: its owner rewrites it in place)."""
		if self.adopted:
			raise ValueError('CoexPlan.update: the plan adopted a device matrix; its owner rewrites it in place')
		dt = np.ascontiguousarray(np.asarray(dt), dtype=self.dtype)
		if dt.shape != self.shape:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		_lib.check(self._lib.nrm_coex_plan_upload(self._handle(), dt.ctypes.data))
		return self

	def time(self, steps):
		"""Milliseconds per step over `steps` steps, between two device events on the plan's stream."""
		ms = _dbl(0.)
		_lib.check(self._lib.nrm_coex_plan_time(self._handle(), int(steps), ctypes.byref(ms)))
		return float(ms.value)

	def info(self):
		"""engine (0: fp64 kernel, 5 / 6: digit planes of the integer engine), captured, steps, reruns, rank, dof, bytes."""
		v = (_i64 * 8)()
		_lib.check(self._lib.nrm_coex_plan_info(self._handle(), v))
		return dict(zip(INFO_FIELDS, (int(x) for x in v)))

	def close(self):
		h, self._h = self._h, None
		if h is not None:
			_lib.check(self._lib.nrm_coex_plan_destroy(h))
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


assert __name__ != "__main__"
