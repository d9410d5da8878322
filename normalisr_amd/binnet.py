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


def _lnp_within(lnp):
	"""Every entry is ln of a P-value: <= 0 and no NaN (-inf, the exact zero of the linear form, included)."""
	lnp = np.asarray(lnp)
	return lnp.dtype.kind == 'f' and bool((lnp <= 0).all())


def _bh_host_log(lnp, weight=None):
	"""ln q from ln P, numpy on the host, fp64 arithmetic for every input dtype: over the distinct values u with c(u) = #{entries <= u},
	ln q(u) = min(0, u + (ln N - ln c(u))), then the minimum over u' >= u.  With weights: ln q(u) = min(0, u - ln(W(u) / W)), W(u) the weights of the entries
	<= u added up in fp64, W their total.  -inf stays -inf, both zeros are ln 1 and come back as +0.0."""
	lnp = np.asarray(lnp)
	assert lnp.ndim == 1 and lnp.size > 0
	assert _lnp_within(lnp), _BH_LOG_INVALID
	u, ids, cnt = np.unique(lnp + lnp.dtype.type(0), return_inverse=True, return_counts=True)
	if u.size == 1:
		logging.warning('Identical p-value in all entries.')
	u = u.astype(np.float64)
	with np.errstate(divide='ignore', invalid='ignore'):
		if weight is None:
			shift = np.log(np.float64(lnp.size)) - np.log(np.cumsum(cnt).astype(np.float64))
		else:
			weight = np.asarray(weight)
			assert weight.shape == lnp.shape
			assert np.isfinite(weight).all() and weight.min() >= 0 and weight.max() > 0
			w = np.zeros(u.size, dtype=np.float64)
			np.add.at(w, ids, weight.astype(np.float64))
			w = np.cumsum(w)
			shift = -np.log(w / w[-1])  # (+inf where no weight lies at or below u: ln q = 0 there, as q = 1 in the linear form -- unless u = -inf, which stays)
		lq = u + shift
	lq[np.isnan(lq)] = -np.inf  # (-inf + inf: a zero P-value without weight is still a zero)
	lq = np.where(lq < 0, lq, 0.0)
	lq = np.minimum.accumulate(lq[::-1])[::-1]
	return lq[ids].astype(lnp.dtype, copy=False)


_BH_INVALID = 'P-values must be finite and within [0,1] (binnet.py:104).'
_BH_LOG_INVALID = 'ln P-values must be <= 0 and no NaN.'


def bh(pv, weight=None, on_device=None, logp=False):
	"""Benjamini-Hochberg q-values with ties and optional weights (binnet.py:77-131).

	A numpy vector with on_device None or False: numpy on the host.  A torch CUDA tensor of fp32 or fp64 -- 1-D, or 2-D with contiguous rows, flattened row-major:
	association_tests(..., device_out=True)[0], a plan's result -- takes the device path (csrc/nrm_bh.hip: a radix sort of the P-values' bit patterns, tie-aware ranks, a suffix
	minimum, a look-up) and comes back as a tensor of the same shape and dtype in HBM: q-values over ALL its entries, bit for bit the reference's (beyond 2^24 fp32
	entries the reference's fp32 count stalls; the device's stays exact).  on_device=True sends a numpy array (1-D or 2-D) the same way: upload, nrm_bh, download --
	or, in a process on the library's whole-problem entries (no torch; NRM_HOST_ENTRY=1), nrm_bh_host.  Any other dtype runs the host code and raises what it raises.
	weight is not None ALWAYS runs the host code (a device tensor is downloaded and the result uploaded again): the reference adds the weights up sequentially, in
	the order of the entries, and no parallel sum reproduces that order's rounding.
	pv holds P-values, not their logarithms, unless logp=True: without it the result of a logp=True call is refused by the assertion 0 <= p <= 1.
	logp=True: pv holds ln P -- de(..., logp=True)[0], association_tests(..., logp=True)[0] -- and the result is ln q, finite where q underflows to 0 (DESIGN.md
	section 4g): over the distinct values u with c(u) = #{entries <= u}, ln q(u) = min(0, u + (ln N - ln c(u))), then the minimum over u' >= u, in fp64 for both
	dtypes, an fp32 result rounded once.  Valid entries are <= 0 and no NaN; -inf (an exact zero) stays -inf.  The routes are the same (nrm_bh_pk, nrm_bh_host_pk with
	p_kind = 1; numpy without on_device and every weighted call: _bh_host_log); nothing is bit-for-bit the reference's here, which has no such form."""
	host = _bh_host_log if logp else _bh_host
	is_dev = hasattr(pv, 'is_cuda') and pv.is_cuda
	native = str(getattr(pv, 'dtype', '')).replace('torch.', '') in ('float32', 'float64')
	if weight is not None or (is_dev and not native):
		if not is_dev:
			return host(pv, weight)
		eng = _engine.get_engine()
		w = weight if weight is None or not hasattr(weight, 'cpu') else weight.cpu().numpy().ravel()
		q = host(pv.cpu().numpy().ravel(), w)
		return eng.upload(q).reshape(pv.shape)
	if not is_dev and not (on_device and native):
		return host(pv, None)
	return _bh_device(pv, is_dev, 1 if logp else 0)


def _bh_device(pv, is_dev, p_kind=0):
	import ctypes
	from . import _lib
	from .association import _use_host_entry, _result
	assert pv.ndim in (1, 2) and int(np.prod(pv.shape)) > 0
	if not is_dev and _use_host_entry():
		# no torch in this process (or NRM_HOST_ENTRY=1): the library's whole-problem entry, numpy buffers in and out
		hp = np.ascontiguousarray(pv)
		out = _result(hp.shape, hp.dtype)
		same = ctypes.c_int32(0)
		_lib.check(_lib.load().nrm_bh_host_pk(hp.ctypes.data_as(ctypes.c_void_p), _engine.dtype_code(hp), hp.size, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(same),
											  p_kind))
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
			_lib.check(eng.lib.nrm_bh_pk(d_p.data_ptr(), code, rows, cols, ldp, out.data_ptr(), cols, work.data_ptr(), work.numel(), flags.data_ptr(), p_kind, eng._stream()))
			invalid, distinct = flags.tolist()  # the one read-back
			if invalid:
				raise AssertionError(_BH_LOG_INVALID if p_kind else _BH_INVALID)
			if not distinct:
				logging.warning('Identical p-value in all entries.')
			return out if is_dev else eng.download(out)


def binnet(net, qcut, logp=False):
	"""Binarise a symmetric co-expression P-value matrix: per-row BH q-values over the off-diagonal entries,
	thresholded at qcut (binnet.py:134-173).  Returns a boolean (n_gene, n_gene) matrix, diagonal False.
	A torch CUDA tensor is accepted (and then returned) so that coex -> binnet can stay in HBM.
	net holds P-values, not their logarithms, unless logp=True: without it coex(..., logp=True)[0] is refused by the assertion 0 <= p <= 1.
	logp=True: net holds ln P -- coex(..., logp=True)[0], on the host or in HBM -- and row i's edges are { j != i : lnp_ij <= tau* },
	tau* = max{ v : v + (ln m - ln c_v) <= ln qcut } with m = n_gene - 1 and c_v = #{off-diagonal entries <= v}, evaluated in fp64 for both dtypes
	(DESIGN.md section 4g): the network of the linear form wherever that form can tell the P-values apart.  Valid entries are <= 0 and no NaN; -inf (the diagonal,
	an exact zero) is one."""
	p_kind = 1 if logp else 0
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
		_lib.check(_lib.load().nrm_binnet_host_pk(hp.ctypes.data_as(ctypes.c_void_p), _engine.dtype_code(hp), nt, float(qcut),
												  out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(total), p_kind))
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
			_lib.check(eng.lib.nrm_binnet_pk(d_p.data_ptr(), _engine.dtype_code(d_p), nt, d_p.stride(0),
											 float(qcut), out.data_ptr(), out.stride(0), total.data_ptr(), flags.data_ptr(), p_kind, eng._stream()))
			if int(flags[0].item()):
				raise AssertionError(_BH_LOG_INVALID if p_kind else 'P-values must be finite and within [0,1] (binnet.py:151-152).')
			if int(total.item()) == 0:
				raise RuntimeError('Empty binary network.')
			return out.view(torch.bool) if on_device else eng.download(out).view(np.bool_)  # the kernel writes exact 0/1 bytes: a view, no pass over the mask


assert __name__ != "__main__"
