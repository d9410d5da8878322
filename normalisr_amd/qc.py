"""Quality control (mirror of the reference's normalisr.qc, qc.py:4-154) and the subsetting that follows it, on a count matrix that stays in HBM.

qc_reads bounds genes and cells from below by their read totals and by how many cells / genes they are seen in, again and again until nothing changes.  The
matrix is never rewritten between the iterations: two byte masks say what is left, and an iteration is one masked statistics pass (nrm_qc_stats over a
dense matrix, nrm_qc_csr_stats over canonical CSR -- a sparse input is never densified), one small kernel that holds the thresholds against the statistics
and clears the masks (nrm_qc_decide), and one read-back of the two alive counts.  subset then cuts the survivors out: a gather for dense matrices of any of
the six dtypes (nrm_subset_dense), count / scan / write for CSR (nrm_subset_csr_*).  Everything is integer arithmetic: the results are exact and the same on
every run.  qc_outlier works on one vector of cell weights and runs on the host.  Kernels: csrc/nrm_qc.hip.

These functions are reached as normalisr_amd.qc.<name> and through the command line; the facade normalisr_amd.normalisr does not export them yet."""
import ctypes
import logging
import math

import numpy as np

from . import _lib
from . import engine as _engine
from . import lcpm as _lcpm
from .lcpm import DeviceCSR


def _check_qc_reads_args(ndim, params):
	if ndim != 2:
		raise ValueError('reads must have 2 dimensions.')
	if any(not v >= 0 for v in params):
		raise ValueError('All parameters must be non-negative.')
	if any(not v <= 1 for v in (params[2], params[5])):
		raise ValueError('Proportional parameters must be no greater than 1.')


def _counts_on_device(eng, d):
	"""The count matrix in HBM as the kernels read it: a dense integer tensor with unit column stride, or lcpm's _Csr.  A scipy.sparse matrix is uploaded as
	canonical CSR whatever its density.  ValueError for a negative entry seen on the host side."""
	if _lcpm._is_sparse(d):
		return _lcpm._Csr(*[eng.upload(a) for a in _lcpm.canonical_csr(d)], d.shape)  # (raises for a negative value)
	if not _engine.is_dev(d):
		d, neg = _lcpm._host_counts(d)
		if neg:
			raise ValueError('Negative value in reads detected.')
	x, _, neg = _lcpm._device_counts(eng, d)
	if neg:
		raise ValueError('Negative value in reads detected.')
	return x


class _Stats:
	"""The buffers of the QC loop on one matrix and its two launches."""

	def __init__(self, eng, x):
		torch = eng.torch
		self.eng, self.x, self.csr = eng, x, isinstance(x, _lcpm._Csr)
		nt, ns = (int(v) for v in x.shape)
		self.nt, self.ns = nt, ns
		self.gene_alive = torch.ones((nt, ), dtype=torch.uint8, device=eng.device)
		self.cell_alive = torch.ones((ns, ), dtype=torch.uint8, device=eng.device)
		buf = torch.empty((2 * nt + 2 * ns + 4, ), dtype=torch.int64, device=eng.device)
		self.gene_total, self.gene_nnz, self.cell_total, self.cell_nnz = buf[:nt], buf[nt:2 * nt], buf[2 * nt:2 * nt + ns], buf[2 * nt + ns:2 * nt + 2 * ns]
		self.tail = buf[2 * nt + 2 * ns:]  # alive genes, alive cells, negative entry, malformed matrix: what the host reads back
		self.work = torch.empty((int(eng.lib.nrm_qc_stats_workspace(nt, ns)), ), dtype=torch.int64, device=eng.device)

	def stats(self):
		eng, x = self.eng, self.x
		out = (self.gene_alive.data_ptr(), self.cell_alive.data_ptr(), self.gene_total.data_ptr(), self.gene_nnz.data_ptr(), self.cell_total.data_ptr(),
			   self.cell_nnz.data_ptr(), self.tail[2:].data_ptr(), self.work.data_ptr(), eng._stream())
		if self.csr:
			_lib.check(eng.lib.nrm_qc_csr_stats(*x.args(), *out))
		else:
			_lib.check(eng.lib.nrm_qc_stats(x.data_ptr(), _lcpm._CODES[str(x.dtype)], self.nt, self.ns, x.stride(0), *out))

	def decide(self, thresholds):
		eng = self.eng
		thr = (ctypes.c_int64 * 6)(*[int(v) for v in thresholds])
		_lib.check(eng.lib.nrm_qc_decide(self.gene_total.data_ptr(), self.gene_nnz.data_ptr(), self.cell_total.data_ptr(), self.cell_nnz.data_ptr(), self.nt, self.ns,
										 ctypes.addressof(thr), self.gene_alive.data_ptr(), self.cell_alive.data_ptr(), self.tail.data_ptr(), eng._stream()))
		h = self.tail.cpu().numpy()  # (the one read-back of an iteration: four integers)
		if h[3]:
			raise ValueError(_lcpm.MALFORMED_CSR)
		if h[2]:
			raise ValueError('Negative value in reads detected.')
		return int(h[0]), int(h[1])


def qc_thresholds(params, nt, ns):
	"""The six integer thresholds of one iteration on nt genes x ns cells.  A count t is an integer, so the reference's t >= bound with a float bound
	(qc.py:56-71) is t >= ceil(bound); the proportional bounds are taken of the CURRENT numbers of cells and genes, in Python floats as the reference writes
	them.  A disabled criterion (0) gives 0, which no count misses."""
	n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell = params
	return (math.ceil(n_gene), math.ceil(nc_gene), math.ceil(ncp_gene * ns), math.ceil(n_cell), math.ceil(nt_cell), math.ceil(ntp_cell * nt))


def _qc_reads_host_entry(d, params, return_info):
	"""qc_reads through nrm_qc_reads_host / nrm_qc_reads_csr_host (include/normalisr_hip.h): host buffers in and out, no torch.  d: a dense count array as
	_host_counts leaves it, or a scipy.sparse matrix (canonical CSR whatever its density, never densified)."""
	lib = _lib.load()
	nt_all, ns_all = (int(v) for v in d.shape)
	gm, cm = np.empty(nt_all, dtype=np.uint8), np.empty(ns_all, dtype=np.uint8)
	info = np.zeros(3, dtype=np.int64)
	vp = _lcpm._vp
	tail = tuple(float(v) for v in params) + (vp(gm), vp(cm), vp(info))
	if _lcpm._is_sparse(d):
		indptr, indices, data = _lcpm.canonical_csr(d)
		_lib.check(lib.nrm_qc_reads_csr_host(vp(indptr), vp(indices), vp(data), _lcpm._NP_CODES[str(data.dtype)], nt_all, ns_all, int(data.size), *tail))
	else:
		_lib.check(lib.nrm_qc_reads_host(vp(d), _lcpm._NP_CODES[str(d.dtype)], nt_all, ns_all, *tail))
	it, nt, ns = (int(v) for v in info)
	if nt == 0:
		raise RuntimeError('All genes removed in QC.')
	if ns == 0:
		raise RuntimeError('All cells removed in QC.')
	gm, cm = gm != 0, cm != 0
	genes, cells = np.flatnonzero(gm).astype(np.int64), np.flatnonzero(cm).astype(np.int64)
	logging.info('Removed {}/{} genes and {}/{} cells in QC.'.format(nt_all - nt, nt_all, ns_all - ns, ns_all))
	if return_info:
		return (genes, cells, dict(iterations=it, gene_mask=gm, cell_mask=cm))
	return (genes, cells)


def qc_reads(reads, n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell, device_out=False, return_info=False):
	"""Quality control by lower bounds on read counts, same contract as reference qc.py:4-85: returns (genes_select, cells_select), the int64 indices of the
	genes and cells that pass.  A gene needs n_gene reads, nc_gene expressing cells and the share ncp_gene of the cells expressing it; a cell needs n_cell
	reads, nt_cell expressed genes and the share ntp_cell of the genes; genes and cells are judged on the same statistics, and the whole is repeated on what is
	left until nothing is removed.  0 disables a criterion.
	reads: (n_gene, n_cell) counts in any form lcpm takes -- a numpy array, a torch CUDA integer tensor, a scipy.sparse matrix, a torch.sparse_csr tensor in
	HBM or a lcpm.DeviceCSR; the sparse forms go through the CSR kernel and are never densified.
	device_out=True returns the two index arrays as torch CUDA tensors.  return_info=True appends a dict: iterations (passes over the matrix), gene_mask and
	cell_mask (the final boolean masks, numpy or torch as the indices).
	Deviation from the reference: a negative entry raises ValueError (the reference sums it silently; lcpm rejects such a matrix anyway).
	RuntimeError when no gene or no cell is left, genes checked first (qc.py:78-81).
	Host input in a process without torch (or with NRM_HOST_ENTRY=1, or from the command line) goes through the library's whole-problem entries
	nrm_qc_reads_host / nrm_qc_reads_csr_host: numpy and the library suffice."""
	d = _lcpm._as_device_csr(reads) or reads
	params = (n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell)
	_check_qc_reads_args(d.ndim, params)
	nt_all, ns_all = (int(v) for v in d.shape)
	if not _engine.is_dev(d):  # (what the host can see is refused before anything touches the device)
		if _lcpm._is_sparse(d):
			neg = bool(d.nnz and d.dtype.kind not in 'ub' and d.data.min() < 0)
		else:
			d, neg = _lcpm._host_counts(d)
		if neg:
			raise ValueError('Negative value in reads detected.')
	if nt_all == 0 or ns_all == 0:  # (the reference's loop on an empty matrix, qc.py:49,78-81)
		if nt_all or ns_all:
			raise RuntimeError('All genes removed in QC.' if nt_all == 0 else 'All cells removed in QC.')
		sel = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
		if device_out:
			eng = _engine.get_engine()
			sel = tuple(eng.upload(v) for v in sel)
		mask = sel[0] != 0
		return sel + ((dict(iterations=0, gene_mask=mask, cell_mask=mask), ) if return_info else ())
	if not _engine.is_dev(d):
		from .association import _use_host_entry
		if _use_host_entry():
			# no torch in this process (or the command line / NRM_HOST_ENTRY=1): the library's whole-problem entries, numpy buffers in and out
			if device_out:
				raise RuntimeError('device_out=True returns torch tensors: torch is needed for it.')
			return _qc_reads_host_entry(d, params, return_info)
	eng = _engine.get_engine(d.device.index if _engine.is_dev(d) else None)
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			st = _Stats(eng, _counts_on_device(eng, d))
			nt, ns, nt0, ns0, it = nt_all, ns_all, 0, 0, 0
			while nt0 != nt or ns0 != ns:
				nt0, ns0, it = nt, ns, it + 1
				with _engine._Span(eng, 'qc_stats'):
					st.stats()
				nt, ns = st.decide(qc_thresholds(params, nt, ns))
				if nt == 0:
					raise RuntimeError('All genes removed in QC.')
				if ns == 0:
					raise RuntimeError('All cells removed in QC.')
			gm, cm = st.gene_alive != 0, st.cell_alive != 0
			if device_out:
				genes, cells = torch.nonzero(gm).flatten(), torch.nonzero(cm).flatten()
			else:
				gm, cm = gm.cpu().numpy(), cm.cpu().numpy()
				genes, cells = np.flatnonzero(gm).astype(np.int64), np.flatnonzero(cm).astype(np.int64)
	logging.info('Removed {}/{} genes and {}/{} cells in QC.'.format(nt_all - nt, nt_all, ns_all - ns, ns_all))
	if return_info:
		return (genes, cells, dict(iterations=it, gene_mask=gm, cell_mask=cm))
	return (genes, cells)


# ---- subset -----------------------------------------------------------------------------------------------------------------------------------------------

def _selection(sel, size, what):
	"""An index array or a boolean mask over an axis of `size`, on the host or in HBM, as (int64 numpy index array or None, torch index tensor or None).
	None: the whole axis.  Negative indices count from the end, as numpy's; IndexError outside the axis."""
	if sel is None:
		return None, None
	if hasattr(sel, 'data_ptr'):
		t = sel
		if t.dim() != 1:
			raise ValueError('{} must be one-dimensional.'.format(what))
		if str(t.dtype) == 'torch.bool':
			if t.numel() != size:
				raise IndexError('{}: a boolean mask of length {} for an axis of length {}.'.format(what, t.numel(), size))
			t = t.nonzero().flatten()
		elif t.dtype.is_floating_point or t.dtype.is_complex:
			raise IndexError('{} must hold integers or booleans.'.format(what))
		t = t.to(dtype=_engine._torch().int64)
		if t.numel():
			lo, hi = int(t.min().item()), int(t.max().item())
			if lo < -size or hi >= size:
				raise IndexError('{}: index out of range for an axis of length {}.'.format(what, size))
			if lo < 0:
				t = t + (t < 0) * size
		return (None, t.contiguous()) if t.is_cuda else (t.numpy(), None)
	a = np.asarray(sel)
	if a.ndim != 1:
		raise ValueError('{} must be one-dimensional.'.format(what))
	if a.dtype == np.bool_:
		if a.size != size:
			raise IndexError('{}: a boolean mask of length {} for an axis of length {}.'.format(what, a.size, size))
		return np.flatnonzero(a).astype(np.int64), None
	if a.dtype.kind not in 'iu':
		if a.size:
			raise IndexError('{} must hold integers or booleans.'.format(what))
		a = a.astype(np.int64)
	a = a.astype(np.int64)
	if a.size and (a.min() < -size or a.max() >= size):
		raise IndexError('{}: index out of range for an axis of length {}.'.format(what, size))
	return np.where(a < 0, a + size, a), None


def _increasing_mask(eng, sel, size, what):
	"""A selection of a sparse matrix as a byte mask in HBM (and how many it keeps); ValueError unless it increases strictly."""
	torch = eng.torch
	h, t = sel
	if h is None and t is None:
		return torch.ones((size, ), dtype=torch.uint8, device=eng.device), size
	if h is not None:
		if h.size > 1 and not (np.diff(h) > 0).all():
			raise ValueError('{} of a sparse matrix must increase strictly.'.format(what))
		m = np.zeros(size, dtype=np.uint8)
		m[h] = 1
		return eng.upload(m), int(h.size)
	if t.numel() > 1 and not bool((t[1:] > t[:-1]).all().item()):
		raise ValueError('{} of a sparse matrix must increase strictly.'.format(what))
	m = torch.zeros((size, ), dtype=torch.uint8, device=eng.device)
	m[t] = 1
	return m, int(t.numel())


def _subset_csr(eng, c, genes, cells):
	"""The CSR subset of a DeviceCSR by two selections: a DeviceCSR (indptr int64, indices int32, data of the input's count dtype)."""
	torch = eng.torch
	nt, ns = c.shape
	gmask, ng = _increasing_mask(eng, genes, nt, 'genes')
	cmask, nc = _increasing_mask(eng, cells, ns, 'cells')
	if nt == 0 or ns == 0 or ng == 0 or nc == 0:
		z = lambda n, dt: torch.zeros((n, ), dtype=dt, device=eng.device)
		return DeviceCSR(z(ng + 1, torch.int64), z(0, torch.int32), z(0, c.data.dtype), (ng, nc))
	x, neg = _lcpm._ready_csr(eng, c)
	rowc = torch.empty((nt, ), dtype=torch.int64, device=eng.device)
	indptr = torch.empty((nt + 1, ), dtype=torch.int64, device=eng.device)
	cmap = torch.empty((ns, ), dtype=torch.int32, device=eng.device)
	tail = torch.empty((5, ), dtype=torch.int64, device=eng.device)  # rows kept, cells kept, stored entries kept | negative (unused), malformed
	stream = eng._stream()
	_lib.check(eng.lib.nrm_subset_csr_count(x.indptr.data_ptr(), x.indices.data_ptr(), nt, ns, x.nnz, gmask.data_ptr(), cmask.data_ptr(), rowc.data_ptr(),
											tail[3:].data_ptr(), stream))
	_lib.check(eng.lib.nrm_subset_csr_scan(rowc.data_ptr(), nt, gmask.data_ptr(), cmask.data_ptr(), ns, indptr.data_ptr(), cmap.data_ptr(), tail.data_ptr(), stream))
	h = tail.cpu().numpy()  # (one small read-back: the size of the result)
	if h[4]:
		raise ValueError(_lcpm.MALFORMED_CSR)
	assert int(h[0]) == ng and int(h[1]) == nc
	nnz = int(h[2])
	oidx = torch.empty((nnz, ), dtype=torch.int32, device=eng.device)
	odat = torch.empty((nnz, ), dtype=x.data.dtype, device=eng.device)
	_lib.check(eng.lib.nrm_subset_csr_write(x.indptr.data_ptr(), x.indices.data_ptr(), x.data.data_ptr(), x.data.element_size(), nt, ns, x.nnz, gmask.data_ptr(),
											cmask.data_ptr(), rowc.data_ptr(), cmap.data_ptr(), oidx.data_ptr(), odat.data_ptr(), nnz, stream))
	return DeviceCSR(indptr[:ng + 1], oidx, odat, (ng, nc))


def _subset_dense(eng, x, genes, cells):
	"""x[genes][:, cells] of a 2-D device tensor with unit column stride, through the gather."""
	torch = eng.torch
	nt, ns = (int(v) for v in x.shape)
	idx = []
	for h, t in (genes, cells):
		idx.append(eng.upload(h) if h is not None else t)
	no = [int(i.numel()) if i is not None else size for i, size in zip(idx, (nt, ns))]
	out = torch.empty((no[0], no[1]), dtype=x.dtype, device=eng.device)
	if no[0] == 0 or no[1] == 0:
		return out
	if nt == 0 or ns == 0:
		raise IndexError('index out of range for an empty axis.')
	_lib.check(eng.lib.nrm_subset_dense(x.data_ptr(), x.element_size(), nt, ns, x.stride(0), 0 if idx[0] is None else idx[0].data_ptr(), no[0],
										0 if idx[1] is None else idx[1].data_ptr(), no[1], out.data_ptr(), out.stride(0), eng._stream()))
	return out


def _subset_host(m, rows, cols, sparse_in):
	"""subset of a host matrix by numpy / scipy indexing, for a process without torch: the same checks, errors and results as the device route (a scipy matrix
	goes through canonical_csr first, as there).  rows, cols: int64 index arrays already checked by _selection, None = the whole axis."""
	rows = slice(None) if rows is None else rows
	cols = slice(None) if cols is None else cols
	if sparse_in:
		import scipy.sparse
		indptr, indices, data = _lcpm.canonical_csr(m)
		out = scipy.sparse.csr_matrix((data, indices, indptr), shape=m.shape)[rows][:, cols].tocsr()
		out.sort_indices()
		return out.astype(m.dtype, copy=False)
	a = np.ascontiguousarray(m)
	if a.dtype.itemsize not in (1, 2, 4, 8) or a.dtype.kind not in 'biuf':
		raise TypeError('subset copies integer and floating-point elements of 1, 2, 4 or 8 bytes.')
	return np.ascontiguousarray(a[rows][:, cols])


def subset(m, genes=None, cells=None, device_out=False):
	"""m[genes][:, cells] on the device: what follows qc_reads and qc_outlier in the pipeline.
	m: a dense (n_gene, n_cell) matrix -- a numpy array or a torch CUDA tensor of int64, int32, int16, uint8, float32 or float64 (any dtype of 1, 2, 4 or 8
	bytes is copied bit for bit) -- or a sparse count matrix: scipy.sparse, torch.sparse_csr in HBM, lcpm.DeviceCSR.
	genes, cells: index arrays (any order, repeats allowed, negative indices from the end) or boolean masks, numpy or torch; None keeps the axis.  For a sparse
	matrix both selections must increase strictly -- what qc_reads returns -- and ValueError otherwise; the result is canonical CSR and stored zeros stay
	stored.
	Returns the input's kind: numpy for numpy, a torch tensor for a torch tensor, scipy CSR for scipy, torch.sparse_csr for torch.sparse_csr, DeviceCSR for
	DeviceCSR.  device_out=True leaves the result in HBM instead: a torch tensor, or a DeviceCSR for every sparse form.
	Host input with host selections in a process without torch (or with NRM_HOST_ENTRY=1, or from the command line) is indexed on the host by numpy / scipy,
	with the same checks, errors and results; it needs no device."""
	d = _lcpm._as_device_csr(m)
	sparse_in = d is not None or _lcpm._is_sparse(m)
	src = d if d is not None else m
	if src.ndim != 2:
		raise ValueError('m must have 2 dimensions.')
	nt, ns = (int(v) for v in src.shape)
	sel = (_selection(genes, nt, 'genes'), _selection(cells, ns, 'cells'))
	if sparse_in:  # (the order is checked before anything touches the device)
		for (h, t), what in zip(sel, ('genes', 'cells')):
			if h is not None and h.size > 1 and not (np.diff(h) > 0).all():
				raise ValueError('{} of a sparse matrix must increase strictly.'.format(what))
	if not _engine.is_dev(src) and not device_out and all(t is None for _, t in sel):
		from .association import _have_torch
		if _lib.host_entry_preferred() or not _have_torch():
			return _subset_host(m, sel[0][0], sel[1][0], sparse_in)  # (no torch in this process, or the command line: indexing on the host needs no device)
	eng = _engine.get_engine(src.device.index if _engine.is_dev(src) else None)
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			if sparse_in:
				if d is None:
					kind = m.dtype
					d = DeviceCSR(*[eng.upload(a) for a in _lcpm.canonical_csr(m)], m.shape)
				out = _subset_csr(eng, d, *sel)
				if device_out or isinstance(m, DeviceCSR):
					return out
				if _engine.is_dev(m):
					return torch.sparse_csr_tensor(out.indptr, out.indices.to(torch.int64), out.data.to(m.values().dtype), size=out.shape)
				import scipy.sparse
				return scipy.sparse.csr_matrix((out.data.cpu().numpy().astype(kind, copy=False), out.indices.cpu().numpy(), out.indptr.cpu().numpy()), shape=out.shape)
			if _engine.is_dev(m):
				x = m if m.stride(1) == 1 else m.contiguous()
				if x.element_size() not in (1, 2, 4, 8) or x.dtype.is_complex:
					raise TypeError('subset copies elements of 1, 2, 4 or 8 bytes.')
				return _subset_dense(eng, x, *sel)
			a = np.ascontiguousarray(m)
			if a.dtype.itemsize not in (1, 2, 4, 8) or a.dtype.kind not in 'biuf':
				raise TypeError('subset copies integer and floating-point elements of 1, 2, 4 or 8 bytes.')
			code = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]  # (copied bit for bit, as integers of the same width)
			out = _subset_dense(eng, eng.upload(a.view(code)), *sel)
			if device_out:
				tdt = {'int64': torch.int64, 'int32': torch.int32, 'int16': torch.int16, 'uint8': torch.uint8, 'float32': torch.float32, 'float64': torch.float64,
					   'int8': torch.int8, 'bool': torch.bool, 'float16': torch.float16}.get(str(a.dtype))
				if tdt is None:
					raise TypeError('no torch dtype for {}: use device_out=False.'.format(a.dtype))
				return out.view(tdt)
			return eng.download(out).view(a.dtype)


# ---- qc_outlier ---------------------------------------------------------------------------------------------------------------------------------------------

def _two_sided_z(q):
	"""The z >= 0 with erfc(z / sqrt 2) = q, 0 < q < 1: the point where the two-sided normal P-value equals q.  Bisection on math.erfc, which falls strictly in
	z: 200 halvings of [0, 40] end far below the spacing of doubles (erfc(40 / sqrt 2) < 1e-300)."""
	lo, hi = 0.0, 40.0
	for _ in range(200):
		mid = 0.5 * (lo + hi)
		if math.erfc(mid / math.sqrt(2.0)) > q:
			lo = mid
		else:
			hi = mid
	return lo


def qc_outlier(dw, pcut=1E-10, outrate=0.02):
	"""Quality control of cells by their fitted variance, same contract as reference qc.py:88-154: a normal distribution is fitted to the inverse-sqrt-variance
	weights of the cells that are not outliers, outliers are the cells whose two-sided P-value under it is below pcut / n_cell, and the two steps alternate
	from a start that sets the share outrate aside on either side, until an assignment comes back (at least 3 times and in a tenth of the steps).  Returns the
	boolean vector of the cells that pass.  RuntimeError when more than 2 * outrate of the cells end up as outliers.
	dw: (n_cell,) positive weights, a numpy array or a torch tensor (for instance ComputeVarPlan.w; it is copied to the host: this is one vector).
	Runs on the host in numpy, without scipy: the reference's 2 * min(sf(t), cdf(t)) >= pcut / n_cell is erfc(|t| / sqrt 2) >= pcut / n_cell, that is
	|t| <= z for the one z with erfc(z / sqrt 2) = pcut / n_cell, found by bisection."""
	if pcut <= 0 or pcut >= 1:
		raise ValueError('Parameter pcut should be between 0 and 1 (exclusive).')
	if outrate <= 0 or outrate >= 0.5:
		raise ValueError('Parameter outrate and outrate should be between 0 and 0.5 (exclusive).')
	if hasattr(dw, 'data_ptr'):
		dw = dw.detach().cpu().numpy()
	dw = np.asarray(dw)
	if dw.ndim != 1:
		raise ValueError('dw must have 1 dimension.')
	if dw.min() <= 0:
		raise ValueError('Non-positive cell weight found..')
	ns = len(dw)
	z = _two_sided_z(pcut / ns)
	lo, hi = int(np.ceil(outrate * ns)), int(np.floor((1 - outrate) * ns))
	part = np.partition(dw, [lo, hi])
	fit = (dw >= part[lo]) & (dw <= part[hi])  # the start: the share outrate set aside on either side
	samples = np.ones(ns, dtype=bool)
	seen = []  # every assignment so far, the all-pass one first
	step = 0
	while True:
		step += 1
		seen.append(samples)
		if step > 1:
			fit = samples
		mean = dw[fit].mean()
		sd = np.sqrt(((dw[fit] - mean)**2).mean())
		samples = np.abs((dw - mean) / sd) <= z
		logging.debug('Step {}, outlier count/rate: {}/{}'.format(step, (~samples).sum(), (~samples).mean()))
		same = np.array([np.array_equal(samples, s) for s in seen])
		if same.mean() >= 0.1 and same.sum() >= 3:
			break
	if (~samples).mean() > 2 * outrate:
		raise RuntimeError('Fitted outlier rate {}>{}.'.format((~samples).mean(), 2 * outrate))
	logging.info('Removed {}/{} cells due to variance outlier'.format((~samples).sum(), samples.size))
	return samples


assert __name__ != "__main__"
