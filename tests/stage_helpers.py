"""What the kernel-level GPU files (test_gpu_s1_stages.py, test_gpu_s4_stages.py) share -- TEST INFRASTRUCTURE ONLY: device buffers that show a write outside the
logical array (Buf), the record of the worst error-to-bound ratios (note) and the run-twice rule (twice).  torch is imported on first use, so the module loads
on a machine without a GPU."""
import functools

import numpy as np

import k3_reference as k3

F64, F32 = np.float64, np.float32
I32, I64 = np.int32, np.int64


@functools.lru_cache(maxsize=None)
def _torch():
	import torch
	return torch


def tdt(dtype):
	torch = _torch()
	return {np.dtype(F64): torch.float64, np.dtype(F32): torch.float32, np.dtype(I32): torch.int32, np.dtype(I64): torch.int64}[np.dtype(dtype)]


class Buf:
	"""A device array of `shape` at row pitch `pitch` (elements; the last axis is the row), pre-filled with NaN (integers: -7) -- or holding `data` with the
	pre-fill in the padding --, `skip` elements into its allocation (a misaligned pointer) and followed by a 1024-byte tail."""

	def __init__(self, shape, dtype, pitch=None, data=None, skip=0):
		torch = _torch()
		self.shape = tuple(int(v) for v in (shape if isinstance(shape, tuple) else (shape, )))
		self.dtype = np.dtype(dtype)
		self.cols = self.shape[-1] if len(self.shape) > 1 else int(np.prod(self.shape))
		self.rows = int(np.prod(self.shape[:-1])) if len(self.shape) > 1 else 1
		self.pitch = int(pitch or self.cols)
		assert self.pitch >= self.cols
		self.skip, self.size = skip, self.rows * self.pitch
		self.fill = float('nan') if self.dtype.kind == 'f' else -7
		self.t = torch.full((skip + self.size + 1024 // self.dtype.itemsize, ), self.fill, dtype=tdt(dtype), device='cuda')
		if data is not None and self.size:
			h = np.full((self.rows, self.pitch), self.fill, dtype=self.dtype)
			h[:, :self.cols] = np.asarray(data, dtype=self.dtype).reshape(self.rows, self.cols)
			self.t[skip:skip + self.size].copy_(torch.from_numpy(h.ravel()))

	@property
	def ptr(self):
		return self.t.data_ptr() + self.skip * self.dtype.itemsize

	def _untouched(self, a):
		return np.isnan(a) if self.dtype.kind == 'f' else a == self.fill

	def raw(self):
		"""The (rows, pitch) matrix; the elements in front of it and the tail must be untouched."""
		a = self.t.cpu().numpy()
		assert self._untouched(a[:self.skip]).all() and self._untouched(a[self.skip + self.size:]).all(), 'written outside the buffer'
		return a[self.skip:self.skip + self.size].reshape(self.rows, self.pitch)

	def get(self):
		"""The logical array; the pitch padding must be untouched too."""
		a = self.raw()
		assert self._untouched(a[:, self.cols:]).all(), 'written into the pitch padding'
		return a[:, :self.cols].reshape(self.shape).copy()

	def clean(self):
		return bool(self._untouched(self.raw()).all())


def note(table, kernel, ws, case):
	"""Print every output's worst error-to-bound ratio, keep the worst of the run in `table`, then assert that none is above 1."""
	for name, w in ws.items():
		print('%-36s %-12s worst error / bound %.3g at %s  (%s; %s)' % (kernel, name, w.ratio, w.where, w.what, case))
		if w.ratio > table.get((kernel, name), (-1.0, ''))[0]:
			table[(kernel, name)] = (w.ratio, case)
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (kernel, case, bad)


def same(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.dtype == b.dtype and a.shape == b.shape and bool(k3.same_bits(a, b).all())


def twice(run):
	"""Every kernel is run twice on the same inputs into fresh buffers: identical bits (the fixed summation orders the comments promise)."""
	one, two = run(), run()
	for k in one:
		if isinstance(one[k], np.ndarray):
			assert same(one[k], two[k]), 'run to run: %s differs' % k
		else:
			assert one[k] == two[k], 'run to run: %s differs' % k
	return one
