"""Binarisation of co-expression P-value networks (mirror of the reference's binnet module, binnet.py).
`binnet` runs on the device (csrc/nrm_binnet.hip), and so does `bh` for P-values that lie in HBM or on request (csrc/nrm_bh.hip); `nodiag`, `rediag` are
small host utilities."""
import logging

import numpy as np

from . import engine as _engine


def nodiag(d, split=False):
	"""Off-diagonal entries of a 2-D matrix, row by row (binnet.py:4-34)."""
	d = np.asarray(d)
	assert d.ndim == 2
	k = min(d.shape)
	rows = [np.concatenate([d[i, :i], d[i, i + 1:]]) for i in range(k)] + list(d[k:])
	return rows if split else np.concatenate(rows)


def rediag(d, fill=0, shape=None):
	"""Inverse of nodiag(split=False) with `fill` on the diagonal (binnet.py:37-74)."""
	d = np.asarray(d)
	if shape is None:
		t = int(np.sqrt(d.size)) + 1
		assert t * (t - 1) == d.size
		shape = (t, t)
	assert len(shape) == 2 and shape[0] * shape[1] - min(shape) == d.size
	m = np.full(shape, fill, dtype=d.dtype)
	k = min(shape)
	off = np.ones(shape, dtype=bool)
	off[np.arange(k), np.arange(k)] = False
	m[off] = d
	return m


def _bh_host(pv, weight=None):
	"""Benjamini-Hochberg q-values with ties and optional weights (binnet.py:77-131), numpy on the host."""
	pv = np.asarray(pv)
	assert pv.ndim == 1 and pv.size > 0
	assert np.isfinite(pv).all() and pv.min() >= 0 and pv.max() <= 1
	if weight is None:
		weight = np.ones(pv.size)
	else:
		weight = np.asarray(weight)
		assert weight.shape == pv.shape
		assert np.isfinite(weight).all() and weight.min() >= 0 and weight.max() > 0
	u, ids = np.unique(pv, return_inverse=True)
	if u.size == 1:
		logging.warning('Identical p-value in all entries.')
	w = np.zeros(u.size, dtype=pv.dtype)
	np.add.at(w, ids, weight.astype(pv.dtype))
	w = np.cumsum(w)
	w /= w[-1]
	with np.errstate(divide='ignore', invalid='ignore'):
		q = u / w
	q[~np.isfinite(q)] = 1
	q = np.maximum(np.minimum(q, 1), 0)  # the reference's two steps (:126-127), not np.clip: the maximum with 0 turns the q of a -0.0 entry into +0.0, as the reference's does
	q = np.minimum.accumulate(q[::-1])[::-1]
	return q[ids].astype(pv.dtype, copy=False)


_BH_INVALID = 'P-values must be finite and within [0,1] (binnet.py:104).'


def bh(pv, weight=None, on_device=None):
	"""Benjamini-Hochberg q-values with ties and optional weights (binnet.py:77-131).

	A numpy vector with on_device None or False: numpy on the host.  A torch CUDA tensor of fp32 or fp64 -- 1-D, or 2-D with contiguous rows, flattened row-major:
	association_tests(..., device_out=True)[0], a plan's result -- takes the device path (csrc/nrm_bh.hip: a radix sort of the P-values' bit patterns, tie-aware ranks, a suffix
	minimum, a look-up) and comes back as a tensor of the same shape and dtype in HBM: q-values over ALL its entries, bit for bit the reference's (beyond 2^24 fp32
	entries the reference's fp32 count stalls; the device's stays exact).  on_device=True sends a numpy array (1-D or 2-D) the same way: upload, nrm_bh, download --
	or, in a process on the library's whole-problem entries (no torch; NRM_HOST_ENTRY=1), nrm_bh_host.  Any other dtype runs the host code and raises what it raises.
	weight is not None ALWAYS runs the host code (a device tensor is downloaded and the result uploaded again): the reference adds the weights up sequentially, in
	the order of the entries, and no parallel sum reproduces that order's rounding.
	pv holds P-values, not their logarithms: the result of a logp=True call is refused by the assertion 0 <= p <= 1 (q-values on ln P are a follow-up)."""
	is_dev = hasattr(pv, 'is_cuda') and pv.is_cuda
	native = str(getattr(pv, 'dtype', '')).replace('torch.', '') in ('float32', 'float64')
	if weight is not None or (is_dev and not native):
		if not is_dev:
			return _bh_host(pv, weight)
		eng = _engine.get_engine()
		w = weight if weight is None or not hasattr(weight, 'cpu') else weight.cpu().numpy().ravel()
		q = _bh_host(pv.cpu().numpy().ravel(), w)
		return eng.upload(q).reshape(pv.shape)
	if not is_dev and not (on_device and native):
		return _bh_host(pv, None)
	return _bh_device(pv, is_dev)


def _bh_device(pv, is_dev):
	import ctypes
	from . import _lib
	from .association import _use_host_entry, _result
	assert pv.ndim in (1, 2) and int(np.prod(pv.shape)) > 0
	if not is_dev and _use_host_entry():
		# no torch in this process (or NRM_HOST_ENTRY=1): the library's whole-problem entry, numpy buffers in and out
		hp = np.ascontiguousarray(pv)
		out = _result(hp.shape, hp.dtype)
		same = ctypes.c_int32(0)
		_lib.check(_lib.load().nrm_bh_host(hp.ctypes.data_as(ctypes.c_void_p), _engine.dtype_code(hp), hp.size, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(same)))
		if same.value:
			logging.warning('Identical p-value in all entries.')
		return out
	eng = _engine.get_engine()
	with eng.lock:  # one call at a time per device (the workspace is the engine's)
		torch = eng.torch
		with torch.cuda.device(eng.device):
			d_p = pv if is_dev else eng.upload(np.ascontiguousarray(pv))
			pitched = d_p.dim() == 2 and d_p.shape[0] > 1  # rows with a pitch of their own (a column slice of a wider result) are read where they lie
			if (d_p.stride(1) != 1 or d_p.stride(0) < d_p.shape[1]) if pitched else not d_p.is_contiguous():
				d_p = d_p.contiguous()
			n = d_p.numel()
			rows, cols, ldp = (d_p.shape[0], d_p.shape[1], d_p.stride(0)) if pitched else (1, n, n)
			out = torch.empty(d_p.shape, dtype=d_p.dtype, device=eng.device)
			code = _engine.dtype_code(d_p)
			nbytes = int(eng.lib.nrm_bh_workspace_bytes(n, code))
			if nbytes < 0:
				_lib.check(nbytes)
			work = eng.bh_work(nbytes)
			flags = torch.empty(2, dtype=torch.int32, device=eng.device)  # (zeroed by the call)
			_lib.check(eng.lib.nrm_bh(d_p.data_ptr(), code, rows, cols, ldp, out.data_ptr(), cols, work.data_ptr(), work.numel(), flags.data_ptr(), eng._stream()))
			invalid, distinct = flags.tolist()  # the one read-back
			if invalid:
				raise AssertionError(_BH_INVALID)
			if not distinct:
				logging.warning('Identical p-value in all entries.')
			return out if is_dev else eng.download(out)


def binnet(net, qcut):
	"""Binarise a symmetric co-expression P-value matrix: per-row BH q-values over the off-diagonal entries,
	thresholded at qcut (binnet.py:134-173).  Returns a boolean (n_gene, n_gene) matrix, diagonal False.
	A torch CUDA tensor is accepted (and then returned) so that coex -> binnet can stay in HBM.
	net holds P-values, not their logarithms: coex(..., logp=True)[0] is refused by the assertion 0 <= p <= 1 (a follow-up)."""
	from . import _lib
	on_device = hasattr(net, 'is_cuda') and net.is_cuda  # torch tensor already in HBM (e.g. coex(..., device_out=True)[0])
	if not on_device:
		net = np.asarray(net)
	assert net.ndim == 2
	nt = net.shape[0]
	if net.shape[1] != nt or nt <= 1:
		raise ValueError('Wrong shape of net or namet.')
	if qcut <= 0 or qcut >= 1:
		raise ValueError('Q-value cutoff must be between 0 and 1.')
	from .association import _use_host_entry
	if not on_device and _use_host_entry():
		# no torch in this process (or NRM_HOST_ENTRY=1): the library's whole-problem entry, numpy buffers in and out
		import ctypes
		hp = _engine.as_input(net)
		from .association import _result
		out = _result((nt, nt), np.uint8)
		total = ctypes.c_int64(-1)
		_lib.check(_lib.load().nrm_binnet_host(hp.ctypes.data_as(ctypes.c_void_p), _engine.dtype_code(hp), nt, float(qcut),
											   out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(total)))
		if total.value == 0:
			raise RuntimeError('Empty binary network.')
		return out.view(np.bool_)
	eng = _engine.get_engine()
	with eng.lock:  # one call at a time per device (engine scratch, streams and guard state are shared)
		torch = eng.torch
		with torch.cuda.device(eng.device):
			d_p = net.contiguous() if on_device else eng.upload(_engine.as_input(net))
			if d_p.dtype not in (torch.float32, torch.float64):
				d_p = d_p.to(torch.float64)
			out = torch.empty((nt, nt), dtype=torch.uint8, device=eng.device)
			total = torch.zeros(1, dtype=torch.int64, device=eng.device)
			flags = torch.zeros(2, dtype=torch.int32, device=eng.device)
			_lib.check(eng.lib.nrm_binnet(d_p.data_ptr(), _engine.dtype_code(d_p), nt, d_p.stride(0),
										  float(qcut), out.data_ptr(), out.stride(0), total.data_ptr(), flags.data_ptr(), eng._stream()))
			if int(flags[0].item()):
				raise AssertionError('P-values must be finite and within [0,1] (binnet.py:151-152).')
			if int(total.item()) == 0:
				raise RuntimeError('Empty binary network.')
			return out.view(torch.bool) if on_device else eng.download(out).view(np.bool_)  # the kernel writes exact 0/1 bytes: a view, no pass over the mask


assert __name__ != "__main__"
