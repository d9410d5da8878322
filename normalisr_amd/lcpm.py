"""Bayesian logCPM and the variance-normalisation scaling factor (mirror of the reference's lcpm.lcpm / lcpm.scaling_factor, lcpm.py:21-283) on the device.

With varscale == 0 the posterior expectation is a function of the count alone, so lcpm is a table lookup,
    lcpm[g,k] = T[reads[g,k]] - t1[k],    T[x] = psi(1 + x) - psi(sum(reads) + 2),    t1[k] = ln sum_g exp(T[reads[g,k]]) - ln 1e6 ,
and csrc/nrm_lcpm.hip streams the count matrix three times: integer totals (which are also the covariates and scaling_factor's zero counts),
the per-cell sums of exp(T) from a second table, and the pass that writes the result.  The tables come from the library's own digamma
(nrm_lcpm_digamma: no scipy on this path).  Counts up to nrm_lcpm_table_cap() - 1 (2**24 - 1); NotImplementedError beyond."""
import ctypes
import logging

import numpy as np

from . import _lib
from . import _opts
from . import engine as _engine

_WARN_LCPM = "Modifying keyword arguments other than nth or seed is neither recommended nor supported for function 'lcpm'. Do so at your own risk."
_WARN_SF = "Modifying keyword arguments is neither recommended nor supported for function 'scaling_factor'. Do so at your own risk."



def _is_sparse(a):
	try:
		import scipy.sparse
	except ImportError:
		return False
	return scipy.sparse.issparse(a)


def digamma_table(xmax, t0):
	"""(psi(1 + x) for x = 0 .. xmax, psi(t0)) from the library (host code: csrc/nrm_lcpm.hip)."""
	xmax = int(xmax)
	if xmax >= int(_lib.load().nrm_lcpm_table_cap()):
		raise NotImplementedError('lcpm on the device tabulates psi(1 + count) for counts below {}; the largest count here is {}.'.format(
			int(_lib.load().nrm_lcpm_table_cap()), xmax))
	psi = np.empty(xmax + 1, dtype=np.float64)
	psi_t0 = ctypes.c_double()
	_lib.check(_lib.load().nrm_lcpm_digamma(xmax, float(t0), psi.ctypes.data, ctypes.addressof(psi_t0)))
	return psi, psi_t0.value


def _host_counts(d):
	"""A host count matrix as a C-contiguous int32 / int64 array: (array, has a negative entry).  Floats hold integer values (lcpm.py:138-139 casts them)."""
	d = np.asarray(d)
	if d.dtype == np.bool_:
		d = d.astype(np.int32)
	if d.dtype.kind not in 'iuf':
		raise TypeError('reads must be an integer (or integer-valued floating-point) matrix.')
	neg = bool(d.size and d.dtype.kind != 'u' and d.min() < 0)
	if d.dtype.kind == 'f' or d.dtype.itemsize > 4 or d.dtype == np.uint32:
		big = bool(d.size) and d.max() > np.iinfo(np.int32).max
		d = d.astype(np.int64 if big else np.int32)
	elif d.dtype != np.int32:
		d = d.astype(np.int32)
	return np.ascontiguousarray(d), neg


MALFORMED_CSR = ('Malformed CSR matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and '
				 'increase strictly (sum duplicates and sort the indices first).')
_CODES = {'torch.int64': _lib.NRM_I64, 'torch.int32': _lib.NRM_I32, 'torch.int16': _lib.NRM_I16, 'torch.uint8': _lib.NRM_U8}

# A scipy.sparse input takes the CSR kernels (csrc/nrm_lcpm_sparse.hip) up to this share of stored entries and today's dense route above it.
# A PLACEHOLDER from byte counts, not a measured crossing: tools/time_front_sparse.py measures both routes per density and writes the crossing
# (from_host_threshold) into profiles/front_half_sparse.json; no such record exists yet.  NRM_DEBUG lcpm_sparse=0 | force overrides
# it; a DeviceCSR always takes the CSR kernels.
SPARSE_MAX_DENSITY = 0.25


def canonical_csr(m):
	"""A scipy.sparse matrix of counts as canonical CSR over its rows, in O(stored entries): (indptr int64, indices int32, data), duplicates summed, columns
	sorted, zeros dropped, data in the narrowest of uint8 / int16 / int32 / int64 that holds its maximum.  Floats hold integer values and are cast as
	_host_counts casts them (lcpm.py:138-139); ValueError for a negative value."""
	kind = m.dtype.kind
	if kind not in 'iufb':
		raise TypeError('reads must be an integer (or integer-valued floating-point) matrix.')
	if m.shape[1] > np.iinfo(np.int32).max:
		raise NotImplementedError('sparse reads with more than 2**31 - 1 cells.')
	c = m.tocsr()
	if c is m:
		c = c.copy()
	if c.data.size and kind not in 'ub' and c.data.min() < 0:
		raise ValueError('Negative value in d detected.')
	c.sum_duplicates()  # (sorts the columns of every row as well)
	if kind in 'fb':
		c.data = c.data.astype(np.int64)
	if c.data.size and (c.data == 0).any():
		c.eliminate_zeros()
	top = int(c.data.max()) if c.data.size else 0
	dtype = np.uint8 if top <= 255 else np.int16 if top <= 32767 else np.int32 if top <= np.iinfo(np.int32).max else np.int64
	return c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data.astype(dtype)


class DeviceCSR:
	"""A sparse count matrix in HBM, canonical CSR over genes: indptr (rows + 1), indices (the cell of every stored entry, strictly increasing inside a row),
	data (the counts; stored zeros are legal), all 1-D torch CUDA tensors of integer dtype, shape = (n_gene, n_cell).  lcpm and scaling_factor take it as it
	is -- nothing is sorted or merged: the count kernel checks the structure and a malformed matrix is a ValueError."""
	is_cuda, ndim = True, 2

	def __init__(self, indptr, indices, data, shape):
		shape = tuple(int(v) for v in shape)
		if len(shape) != 2 or min(shape) < 0:
			raise ValueError('DeviceCSR: shape must be (n_gene, n_cell).')
		for name, t in (('indptr', indptr), ('indices', indices), ('data', data)):
			if not hasattr(t, 'data_ptr') or t.dim() != 1:
				raise ValueError('DeviceCSR: {} must be a 1-D torch tensor.'.format(name))
		for name, t in (('indptr', indptr), ('indices', indices)):
			if t.dtype.is_floating_point or t.dtype.is_complex or str(t.dtype) == 'torch.bool':
				raise ValueError('DeviceCSR: {} must have an integer dtype.'.format(name))
		if data.dtype.is_complex:
			raise ValueError('DeviceCSR: data must hold counts.')
		if indptr.numel() != shape[0] + 1:
			raise ValueError('DeviceCSR: indptr must have n_gene + 1 = {} entries, not {}.'.format(shape[0] + 1, indptr.numel()))
		if indices.numel() != data.numel():
			raise ValueError('DeviceCSR: indices and data must have the same length.')
		if shape[1] > np.iinfo(np.int32).max:
			raise NotImplementedError('DeviceCSR with more than 2**31 - 1 cells.')
		if not (indptr.is_cuda and indices.is_cuda and data.is_cuda) or not (indptr.device == indices.device == data.device):
			raise ValueError('DeviceCSR: indptr, indices and data must be CUDA tensors on one device.')
		self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape

	@property
	def device(self):
		return self.data.device

	@classmethod
	def from_scipy(cls, m, device=None):
		"""Canonicalise a scipy.sparse matrix on the host (canonical_csr) and upload its three arrays."""
		eng = _engine.get_engine(device)
		return cls(*[eng.upload(a) for a in canonical_csr(m)], m.shape)


class _Csr:
	"""What the CSR kernels read: indptr int64, indices int32, data of a dtype in _CODES, all contiguous."""

	def __init__(self, indptr, indices, data, shape):
		self.indptr, self.indices, self.data, self.shape, self.code, self.nnz = indptr, indices, data, shape, _CODES[str(data.dtype)], int(data.numel())

	def args(self):
		return (self.indptr.data_ptr(), self.indices.data_ptr(), self.data.data_ptr(), self.code, self.shape[0], self.shape[1], self.nnz)


def _as_device_csr(d):
	"""The device forms of a sparse matrix -- a DeviceCSR, a torch tensor of layout torch.sparse_csr in HBM -- as a DeviceCSR; None for anything else."""
	if isinstance(d, DeviceCSR):
		return d
	if _engine.is_dev(d) and str(getattr(d, 'layout', '')) == 'torch.sparse_csr':
		return DeviceCSR(d.crow_indices(), d.col_indices(), d.values(), d.shape)
	return None


def _takes_csr(d):
	"""Whether a scipy.sparse matrix goes through the CSR kernels (True) or is densified as before (False)."""
	mode = _opts.debug('lcpm_sparse', 'auto')
	if mode in ('0', 'force'):
		return mode == 'force'
	return d.nnz <= SPARSE_MAX_DENSITY * d.shape[0] * d.shape[1]


_NP_CODES = {'int64': _lib.NRM_I64, 'int32': _lib.NRM_I32, 'int16': _lib.NRM_I16, 'uint8': _lib.NRM_U8}


def _entry_counts(d, check=True):
	"""A host count matrix as the whole-problem entries read it (include/normalisr_hip.h: nrm_lcpm_host, nrm_qc_reads_host and their CSR forms): the three arrays
	of canonical_csr for a scipy.sparse matrix that takes the CSR kernels (_takes_csr), else a C-contiguous dense array of int64 / int32 / int16 / uint8 -- those
	four as they are, anything else through _host_counts.  ValueError for a negative entry seen here (check=False: a dense matrix is not looked at, as
	scaling_factor does not look: lcpm.py:258 counts zeros whatever else the matrix holds)."""
	if _is_sparse(d):
		if _takes_csr(d):
			return canonical_csr(d)
		if check and d.data.size and d.dtype.kind not in 'ub' and d.data.min() < 0:
			raise ValueError('Negative value in d detected.')
		d = d.toarray()  # (densified on the host, as lcpm.py:134-137 does)
	d = np.asarray(d)
	if str(d.dtype) in _NP_CODES:
		return np.ascontiguousarray(d)
	d, neg = _host_counts(d)
	if neg and check:
		raise ValueError('Negative value in d detected.')
	return d


def _vp(a):
	return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _lcpm_host_entry(d, shape, normalize=True, ntot=None, otype=None, nocov=True, want_zero=False):
	"""lcpm and scaling_factor's zero counts through nrm_lcpm_host / nrm_lcpm_csr_host: host buffers in and out, no torch, one upload for both.  d: what
	_entry_counts returns; otype None: the integer pass alone.  Returns (lcpm or None, cov or None, zero entries per gene or None, sum, maximum)."""
	lib = _lib.load()
	nt, ns = (int(v) for v in shape)
	out = None
	if otype is not None:
		from .association import _result
		out = _result((nt, ns), otype)  # (page-locked, recycled)
	cov = None if nocov else np.empty((3, ns), dtype=np.float64)
	zero = np.empty(nt, dtype=np.int64) if want_zero else None
	info = np.zeros(2, dtype=np.int64)
	tail = (1 if normalize else 0, -1 if ntot is None else int(ntot), _vp(out), _engine.dtype_code(np.float64 if otype is None else otype), _vp(cov), _vp(zero), _vp(info))
	if isinstance(d, tuple):
		indptr, indices, data = d
		_lib.check(lib.nrm_lcpm_csr_host(_vp(indptr), _vp(indices), _vp(data), _NP_CODES[str(data.dtype)], nt, ns, int(data.size), *tail))
	else:
		_lib.check(lib.nrm_lcpm_host(_vp(d), _NP_CODES[str(d.dtype)], nt, ns, *tail))
	return out, cov, zero, int(info[0]), int(info[1])


def _ready_csr(eng, c):
	"""(_Csr, has a negative entry on this side) of a DeviceCSR: index tensors cast on the device to the widths the kernels read, the values to a count dtype."""
	torch = eng.torch
	neg, data = False, c.data
	if data.dtype.is_floating_point:
		neg = bool(data.numel() and (data < 0).any().item())
		data = data.to(torch.int64)
	elif str(data.dtype) not in _CODES:
		data = data.to(torch.int32 if data.dtype in (torch.int8, torch.bool) else torch.int64)
	return _Csr(c.indptr.to(torch.int64).contiguous(), c.indices.to(torch.int32).contiguous(), data.contiguous(), c.shape), neg


def _device_counts(eng, d):
	"""The count matrix in HBM as the kernels read it -- a dense tensor with unit column stride, or a _Csr for the CSR kernels: (matrix, dtype code, has a
	negative entry on the host side)."""
	torch = eng.torch
	neg = False
	if isinstance(d, DeviceCSR):
		x, neg = _ready_csr(eng, d)
		return x, x.code, neg
	if not _engine.is_dev(d):
		if _is_sparse(d):
			if _takes_csr(d):
				x = _Csr(*[eng.upload(a) for a in canonical_csr(d)], d.shape)  # (three arrays of the stored entries: no dense matrix on either side)
				return x, x.code, False
			neg = bool(d.data.size and d.data.min() < 0)
			d = d.toarray()  # (densified on the host, as lcpm.py:134-137 does)
		d, neg2 = _host_counts(d)
		neg = neg or neg2
		d = eng.upload(d)
	else:
		if d.dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
			neg = bool((d < 0).any().item())
			d = d.to(torch.int64)
		elif str(d.dtype) not in _CODES:
			d = d.to(torch.int32 if d.dtype in (torch.int8, torch.bool) else torch.int64)
		if d.stride(1) != 1:
			d = d.contiguous()
	return d, _CODES[str(d.dtype)], neg


class _Counts:
	"""The integer pass over a count matrix (nrm_lcpm_count, or nrm_lcpm_csr_count for a _Csr): per-cell totals and non-zero counts, per-gene zero counts, grand
	total, maximum, negative flag; for a _Csr the structure check as well (ValueError for a malformed matrix)."""

	def __init__(self, eng, d, code):
		torch = eng.torch
		nt, ns = d.shape
		buf = eng.zeros((2 * ns + nt + 4, ), torch.int64)
		self.cell_total, self.cell_nnz, self.gene_zero, self.info = buf[:ns], buf[ns:2 * ns], buf[2 * ns:2 * ns + nt], buf[2 * ns + nt:]
		out = (self.cell_total.data_ptr(), self.cell_nnz.data_ptr(), self.gene_zero.data_ptr(), self.info.data_ptr())
		if isinstance(d, _Csr):
			part = torch.empty((int(eng.lib.nrm_lcpm_csr_workspace(nt, ns)), ), dtype=torch.int64, device=eng.device)
			_lib.check(eng.lib.nrm_lcpm_csr_count(*d.args(), *out, part.data_ptr(), eng._stream()))
		else:
			part = torch.empty((int(eng.lib.nrm_lcpm_count_workspace(nt, ns)), ), dtype=torch.int64, device=eng.device)
			_lib.check(eng.lib.nrm_lcpm_count(d.data_ptr(), code, nt, ns, d.stride(0), *out, part.data_ptr(), eng._stream()))
		h = buf.cpu().numpy()  # (one small read-back: 2 n_cell + n_gene + 4 integers)
		self.h_cell_total, self.h_cell_nnz, self.h_gene_zero = h[:ns], h[ns:2 * ns], h[2 * ns:2 * ns + nt]
		self.total, self.max, self.negative = int(h[-4]), int(h[-3]), bool(h[-2])
		if h[-1]:
			raise ValueError(MALFORMED_CSR)


def lcpm(reads, normalize=True, nth=0, ntot=None, varscale=0, seed=None, lowmem=True, nocov=False, device_out=False, out_dtype=None, _scale=False):
	"""Bayesian logCPM from raw read counts, same contract as reference lcpm.py:21-208: returns (lcpm, mean, var, cov).
	reads: (n_gene, n_cell) counts -- a numpy array of any integer dtype (or floats holding integers), a scipy.sparse matrix (densified on the host) or a torch
	CUDA integer tensor already in HBM.  nth and seed are accepted for compatibility and ignored.  varscale != 0 resamples from numpy's global random stream in
	the reference and is not provided: NotImplementedError.
	out_dtype: None / numpy.float64 (the reference's) or numpy.float32 (the fp64 value rounded once, at the store).  device_out=True leaves lcpm (and mean, var)
	in HBM as torch tensors -- what compute_var and normvar take next; cov is always a (3, n_cell) numpy array (None with nocov).
	Host input in a process without torch (or with NRM_HOST_ENTRY=1, or from the command line) goes through the library's whole-problem entries (nrm_lcpm_host,
	nrm_lcpm_csr_host): numpy and the library suffice.  _scale=True (the command line, on that route only) appends scaling_factor(reads) from the same call."""
	d = _as_device_csr(reads) or reads
	if d.ndim != 2:
		raise ValueError('reads must have 2 dimensions.')
	if varscale < 0:
		raise ValueError('varscale must be non-negative.')
	otype = np.dtype(np.float64 if out_dtype is None else out_dtype)
	if otype not in (np.dtype(np.float32), np.dtype(np.float64)):
		raise ValueError('out_dtype must be numpy.float32 or numpy.float64.')
	if not _engine.is_dev(d) and not _is_sparse(d):
		d, neg = _host_counts(d)
		if neg:
			raise ValueError('Negative value in d detected.')
	elif _is_sparse(d) and d.data.size and d.data.min() < 0:
		raise ValueError('Negative value in d detected.')
	if not normalize or ntot is not None or varscale != 0:
		logging.warning(_WARN_LCPM)
	if varscale != 0:
		raise NotImplementedError('lcpm with varscale != 0 draws its resampling noise from numpy\'s global random stream (lcpm.py:126-127); '
								  'only the posterior expectation (varscale=0) is provided on the device.')
	nt, ns = d.shape
	if ntot is None:
		assert nt * ns > 0  # t0 > 2 (lcpm.py:95): an empty matrix has no reads
	else:
		assert ntot + 2 > 2
		if nt * ns == 0:
			raise ValueError('reads must not be empty.')
	if not _engine.is_dev(d):
		from .association import _use_host_entry
		if _use_host_entry():
			# no torch in this process (or the command line / NRM_HOST_ENTRY=1): the library's whole-problem entries, numpy buffers in and out
			if device_out:
				raise RuntimeError('device_out=True returns torch tensors: torch is needed for it.')
			raw = reads if not _is_sparse(reads) and str(getattr(reads, 'dtype', '')) in _NP_CODES else d  # (int16 and uint8 counts go as they are)
			dtn, dcov, zeros = _lcpm_host_entry(_entry_counts(raw), (nt, ns), normalize, ntot, otype, nocov, want_zero=_scale)[:3]
			ans = (dtn, None, None, dcov) if lowmem else (dtn, dtn.copy(), np.zeros((nt, ns), dtype=otype), dcov)
			return ans + (_rescale(zeros / float(ns), 0, 'max', nt), ) if _scale else ans
	eng = _engine.get_engine(d.device.index if _engine.is_dev(d) else None)
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			x, code, neg = _device_counts(eng, d)
			csr = isinstance(x, _Csr)
			if neg:
				raise ValueError('Negative value in d detected.')
			cnt = _Counts(eng, x, code)
			if cnt.negative:
				raise ValueError('Negative value in d detected.')
			t0 = cnt.total + 2 if ntot is None else ntot + 2
			assert t0 > 2
			psi, psi_t0 = digamma_table(cnt.max, t0)
			tab = psi - psi_t0  # T[x] (lcpm.py:107)
			d_tab = eng.upload(tab)
			d_t1 = None
			if normalize:
				etab = np.exp(tab)  # exp() once per table entry: the per-cell sums of lcpm.py:158 are sums of table entries
				d_exp = eng.upload(etab)
				d_t1 = torch.empty((ns, ), dtype=torch.float64, device=eng.device)
				if csr:
					# sum over the stored entries of E[x] - E[0] <= x * unit, in fixed point scaled by the cell's total (csrc/nrm_lcpm_sparse.hip)
					unit = float(((etab[1:] - etab[0]) / np.arange(1, etab.size)).max()) if etab.size > 1 else 0.0
					part = torch.empty((int(eng.lib.nrm_lcpm_csr_workspace(nt, ns)), ), dtype=torch.int64, device=eng.device)
					with _engine._Span(eng, 'lcpm_csr_colsum'):
						_lib.check(eng.lib.nrm_lcpm_csr_colsum(*x.args(), d_exp.data_ptr(), tab.size, unit, cnt.cell_total.data_ptr(), part.data_ptr(), d_t1.data_ptr(),
															   eng._stream()))
				else:
					tiles = -(-nt // int(eng.lib.nrm_lcpm_row_tile()))
					part = torch.empty((tiles, ns), dtype=torch.float64, device=eng.device)
					with _engine._Span(eng, 'lcpm_colsum'):
						_lib.check(eng.lib.nrm_lcpm_colsum(x.data_ptr(), code, nt, ns, x.stride(0), d_exp.data_ptr(), tab.size, part.data_ptr(), d_t1.data_ptr(), eng._stream()))
				del part
			out = torch.empty((nt, ns), dtype=torch.float64 if otype == np.float64 else torch.float32, device=eng.device)
			tail = (d_tab.data_ptr(), tab.size, 0 if d_t1 is None else d_t1.data_ptr(), out.data_ptr(), _engine.dtype_code(otype),
					out.stride(0), eng._stream())
			if csr:
				with _engine._Span(eng, 'lcpm_csr_write'):
					_lib.check(eng.lib.nrm_lcpm_csr_write(*x.args(), *tail))
			else:
				with _engine._Span(eng, 'lcpm_write'):
					_lib.check(eng.lib.nrm_lcpm_write(x.data_ptr(), code, nt, ns, x.stride(0), *tail))
			if nocov:
				dcov = None
			else:
				if (cnt.h_cell_total == 0).any():
					raise ValueError('Found cell with no read at all. Please remove.')
				t1 = np.log(cnt.h_cell_total)
				dcov = np.array([t1, nt - cnt.h_cell_nnz, t1**2])
				assert dcov.shape == (3, ns) and np.isfinite(dcov).all()
			# every table entry is finite, so is every per-cell sum of positive entries: the reference's isfinite assertions (lcpm.py:203-206) hold by construction
			assert np.isfinite(tab).all()
			dtn = out if device_out else eng.download(out)
			if lowmem:
				dmean = dvar = None
			elif device_out:
				dmean, dvar = out.clone(), eng.zeros((nt, ns), out.dtype)  # (varscale == 0: the mean is the estimate, its variance scaled by 0: lcpm.py:176,184-186)
			else:
				dmean, dvar = dtn.copy(), np.zeros((nt, ns), dtype=otype)
	return (dtn, dmean, dvar, dcov)


def scaling_factor(dt, varname='nt0mean', v0=0, v1='max'):
	"""Scaling factor of variance normalisation for every gene, same contract as reference lcpm.py:211-283.
	dt: the read-count matrix, a numpy array or a torch CUDA integer tensor.  The default variable (the share of zero entries per gene) is counted on the
	device (nrm_lcpm_count; for host input without torch through nrm_lcpm_host / nrm_lcpm_csr_host); the other four are whole-matrix numpy expressions and run on
	the host, without torch for host input."""
	dt = _as_device_csr(dt) or dt
	if dt.ndim != 2:
		raise ValueError('dt must have 2 dimensions.')
	if v0 != 0 or v1 != 'max' or varname != 'nt0mean':
		logging.warning(_WARN_SF)
	if varname not in ('logtpropmean', 'logtmeanprop', 'nt0mean', 'lognt0mean', 'log1-nt0mean'):
		raise ValueError('Unknown varname: {}'.format(varname))
	if varname == 'nt0mean':
		from .association import _use_host_entry
		if not _engine.is_dev(dt) and dt.shape[0] * dt.shape[1] > 0 and _use_host_entry():
			zeros = _lcpm_host_entry(_entry_counts(dt, check=False), dt.shape, want_zero=True)[2]  # (the integer pass alone)
		else:
			eng = _engine.get_engine(dt.device.index if _engine.is_dev(dt) else None)
			with eng.lock, eng.torch.cuda.device(eng.device):
				x, code, _ = _device_counts(eng, dt)
				zeros = _Counts(eng, x, code).h_gene_zero
		d = zeros / float(dt.shape[1])  # (dt == 0).mean(axis=1)
	else:
		if isinstance(dt, DeviceCSR):  # (these four are whole-matrix numpy expressions: dense on the host)
			import scipy.sparse
			dt = scipy.sparse.csr_matrix((dt.data.cpu().numpy(), dt.indices.cpu().numpy(), dt.indptr.cpu().numpy()), shape=dt.shape)
		h = dt.cpu().numpy() if _engine.is_dev(dt) else (dt.toarray() if _is_sparse(dt) else np.asarray(dt))
		with np.errstate(divide='ignore', invalid='ignore'):
			if varname == 'logtpropmean':
				d = h.mean(axis=1)
				d = np.log(d / d.sum())
			elif varname == 'logtmeanprop':
				d = h / h.sum(axis=0)
				d = np.log(d.mean(axis=1))
			elif varname == 'lognt0mean':
				d = np.log((h == 0).mean(axis=1))
			else:
				d = np.log(1 - (h == 0).mean(axis=1))
	return _rescale(d, v0, v1, dt.shape[0])


def _rescale(d, v0, v1, nt):
	"""scaling_factor's variable d (n_gene,) mapped linearly so that v0 -> 0 and v1 -> 1 ('max' / 'min': of d; lcpm.py:268-283)."""
	ans = []
	for v in [v0, v1]:
		if isinstance(v, str) and v == 'max':
			ans.append(d.max())
		elif isinstance(v, str) and v == 'min':
			ans.append(d.min())
		else:
			ans.append(float(v))
	v0, v1 = ans
	assert v1 != v0
	ans = (d - v0) / (v1 - v0)
	assert ans.shape == (nt, )
	assert np.isfinite(ans).all()
	return ans


assert __name__ != "__main__"
