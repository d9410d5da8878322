"""Differential expression: all genes against all groupings (mirror of the reference's de module)."""
import numpy as np

from .association import association_tests
from . import engine as _engine


def _varying_rows(dg):
	"""Rows with more than one distinct value (de.py:93 uses len(np.unique(x)) > 1; NaNs compare equal there).
	Column blocks of growing width, only over the rows still undecided: a row is settled by its first value that differs
	from its first entry, so a 0/1 incidence matrix costs far less than one pass."""
	rows, n = dg.shape
	varying = np.zeros(rows, dtype=bool)
	if n < 2:
		return varying
	isf = dg.dtype.kind == 'f'
	todo = np.arange(rows)
	c0, width = 1, 256
	while todo.size and c0 < n:
		c1 = min(n, c0 + width)
		whole = todo.size == rows
		blk = dg[:, c0:c1] if whole else dg[todo, c0:c1]
		first = dg[:, :1] if whole else dg[todo, :1]
		diff = blk != first
		if isf:
			diff &= ~(np.isnan(blk) & np.isnan(first))
		hit = diff.any(axis=1)
		varying[todo[hit]] = True
		todo = todo[~hit]
		c0, width = c1, width * 4
	return varying


def _full_row_varies(v):
	"""Whether the values of a row with every cell set are not all equal (NaNs compare equal, as for np.unique)."""
	return bool(((v != v[0]) & ~(np.isnan(v) & np.isnan(v[0]))).any())


def _varying_rows_entries(k, n, full_varies):
	"""_varying_rows from the entries of a sparse design: k[i] = non-zero entries of row i among n cells.  No entry: constant (all zeros); some cells
	set, some not: two values; every cell set: full_varies(i) looks at the values."""
	k = np.asarray(k)
	varying = (k > 0) & (k < n)
	for i in np.nonzero((k == n) & (n > 1))[0]:  # (the exceptional rows)
		varying[i] = full_varies(int(i))
	return varying


def _varying_rows_scipy(m):
	"""_varying_rows(m.toarray()) of a canonical scipy CSR matrix (no stored zeros, no duplicates) in O(stored entries)."""
	ip = m.indptr
	data = m.data if m.data.dtype.kind == 'f' else m.data.astype(np.float64)
	return _varying_rows_entries(np.diff(ip), m.shape[1], lambda i: _full_row_varies(data[ip[i]:ip[i + 1]]))


def _varying_rows_device(design):
	"""_varying_rows of a DesignCSR (stored zeros are not entries): one read-back -- indptr and the non-zero entries before every row -- and, for a row with
	every cell set, a torch min / max on its segment.  The structure is checked first (torch indexing does not clamp)."""
	design.check()
	import torch
	ip = design.indptr.to(torch.int64)
	if design.data is None:
		h = ip.cpu().numpy()
		k = np.diff(h)
	else:
		nz = torch.cat([torch.zeros(1, dtype=torch.int64, device=ip.device), torch.cumsum(design.data != 0, 0)])  # (NaN != 0: an entry)
		h = torch.stack([ip, nz[ip]]).cpu().numpy()
		k, h = np.diff(h[1]), h[0]

	def full(i):
		if design.data is None:
			return False
		v = design.data[int(h[i]):int(h[i + 1])]
		v = v[v != 0].to(torch.float64)
		nan = torch.isnan(v)
		if bool(nan.any()):
			return not bool(nan.all())
		return bool(v.min() != v.max())
	return _varying_rows_entries(k, design.shape[1], full), h


def _device_rows(design, gid, h):
	"""The rows gid (a boolean mask) of a DesignCSR as a new DesignCSR: a gather of the kept rows' segments on the device.  h: indptr on the host."""
	import torch
	from . import de_sparse
	dev = design.indptr.device
	lens = np.diff(h)[gid]
	new_ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
	shift = torch.from_numpy((h[:-1][gid] - new_ip[:-1]).astype(np.int64)).to(dev)
	src = torch.repeat_interleave(shift, torch.from_numpy(lens.astype(np.int64)).to(dev)) + torch.arange(int(new_ip[-1]), dtype=torch.int64, device=dev)
	return de_sparse.DesignCSR(torch.from_numpy(new_ip).to(dev), design.indices[src], None if design.data is None else design.data[src], (int(gid.sum()), design.shape[1]))


def _de_sparse_design(dg, dt, dc, bs, ka):
	"""de for a sparse design (scipy.sparse, de_sparse.DesignCSR, a torch.sparse_csr CUDA tensor): the row filter of de.py:93 from the entries, the rows kept
	as a sparse matrix again -- no dense design on the host."""
	from . import de_sparse
	de_sparse.refuse_sparse(dt, 'dt')
	de_sparse.refuse_sparse(dc, 'dc')
	dt, dc = np.asarray(dt), np.asarray(dc)
	if dg.ndim != 2 or dt.ndim != 2 or dc.ndim != 2:
		raise ValueError('Incorrect dx/dy/dc size.')
	design = de_sparse.as_design_csr(dg)
	if design is None:
		import scipy.sparse
		m = scipy.sparse.csr_matrix((de_sparse.canonical_design_csr(dg)[2::-1]), shape=dg.shape)  # (data, indices, indptr)
		gid = _varying_rows_scipy(m)
		sub = m if gid.all() else m[gid]
	else:
		gid, h = _varying_rows_device(design)
		sub = design if gid.all() else _device_rows(design, gid, h)
	res = association_tests(sub, dt, dc, bsx=bs, bsy=bs, return_dot=False, **ka)
	return _inflate(gid, res, dg.shape[0], dt, dc.shape[0], logp=bool(ka.get('logp', False)))


def _logp_within(a):
	"""The assertion on P-values for their logarithms (logp=True): no NaN and nothing above 0; -inf is a value (P = 0 that is no underflow)."""
	if a.size == 0:
		return True
	if a.size >= (1 << 18) and a.dtype in (np.float32, np.float64) and a.flags.c_contiguous:
		from . import _lib
		out = np.empty(3)
		_lib.check(_lib.load().nrm_host_minmax(a.ctypes.data, _engine.dtype_code(a), a.size, 0, out.ctypes.data))
		return bool(out[2] == 0 and out[1] <= 0)
	return bool(a.max() <= 0)  # (a NaN anywhere makes the maximum NaN and the comparison False)


def _inflate(gid, res, ng0, dt, nc, logp=False):
	"""The results of the tested rows put back among all groupings (de.py:107-122) and the reference's assertions on them (de.py:124-131).
	logp: the first array holds ln P -- rows that were not tested get ln 1 = 0, and the assertion on it is "no NaN and <= 0"."""
	p_ok = _logp_within if logp else (lambda a: _finite_within(a, 0, 1))
	p, gam, alpha, varg, vart = res
	nt = dt.shape[0]
	odt = dt.dtype if dt.dtype in (np.float32, np.float64) else np.dtype(np.float64)
	if bool(gid.all()) and p.dtype == odt:  # nothing to re-inflate (de.py:107-122 is the identity then)
		P, G, A, VG = p, gam, alpha, varg
		VT = vart if np.ndim(vart) == 2 else np.broadcast_to(vart, (ng0, nt)).copy()  # single=0: (n_gene,) for every row
		assert p_ok(P) and _finite_within(G) and _finite_within(VG, 0) and _finite_within(VT, 0)
		return (P, G, A, VG, VT)
	P = np.zeros((ng0, nt), dtype=odt) if logp else np.ones((ng0, nt), dtype=odt)
	P[gid] = p
	G = np.zeros((ng0, nt), dtype=odt)
	G[gid] = gam
	A = None
	if alpha is not None:
		A = np.zeros((ng0, nt, nc), dtype=odt)
		A[gid] = alpha
	VG = np.zeros((ng0, ), dtype=odt)
	VG[gid] = varg
	VT = np.zeros((ng0, nt), dtype=odt)
	VT[gid] = vart  # (n_gene,) for single=0 broadcasts to every tested row
	assert p_ok(P) and _finite_within(G) and _finite_within(VG, 0) and _finite_within(VT, 0)
	return (P, G, A, VG, VT)


def _finite_within(a, lo=None, hi=None):
	"""np.isfinite(a).all() and (a >= lo).all() and (a <= hi).all() (the reference's assertions on its results, de.py:124-131) from the
	array's minimum, maximum and NaN count: one threaded pass in the library for large arrays (numpy's min and max for small ones: a NaN
	anywhere makes both NaN and every comparison False) instead of up to five numpy passes with temporaries (the assertions were 12 ms
	of an 85 ms de call at BASELINE configs[3] size, 35 ms of a 50 ms normvar call)."""
	if a.size == 0:
		return True
	if a.size >= (1 << 18) and a.dtype in (np.float32, np.float64) and a.flags.c_contiguous:
		# one threaded pass in the library (numpy's NaN-propagating min / max of 400 MB of fp64 take 35 ms)
		from . import _lib
		out = np.empty(3)
		_lib.check(_lib.load().nrm_host_minmax(a.ctypes.data, _engine.dtype_code(a), a.size, 0, out.ctypes.data))
		if out[2] > 0:
			return False
		mn, mx = float(out[0]), float(out[1])
	else:
		mn, mx = float(a.min()), float(a.max())
	return bool(np.isfinite(mn) and np.isfinite(mx) and (lo is None or mn >= lo) and (hi is None or mx <= hi))


def de(dg, dt, dc, bs=0, **ka):
	"""Differential expression of every gene (rows of dt) against every grouping (rows of dg) with
	covariates dc: Y = gamma*X + alpha*C + eps, H0: gamma = 0.  Same contract as reference de.py:4-132.

	Returns (P-values (n_group,n_gene), gamma (n_group,n_gene), alpha (n_group,n_gene,n_cov)|None,
	varg (n_group,), vart (n_group,n_gene)).  Keyword arguments single, lowmem, nth, dimreduce, tol, ...
	are passed to association_tests.  Single-valued grouping rows are not tested and come back with
	p=1, gamma=0, alpha=0, varg=0, vart=0 (de.py:107-122).
	logp=True (single=0 only): the first result holds ln P, finite wherever P is a number other than an exact 0; rows that are not
	tested come back with ln P = 0.
	dg may be sparse -- a scipy.sparse matrix, a de_sparse.DesignCSR or a torch.sparse_csr CUDA tensor: the results are those of the densified
	matrix, and the dense matrix is never formed on the host (DESIGN.md section 4c says which routes scatter it on the device).
	"""
	from . import de_sparse
	if ka.get('logp', False) and ka.get('single', 0) != 0:  # (before the row filter, which for a design in HBM runs on the device)
		raise NotImplementedError('logp=True is available for single=0 only (single=1, 4 and 5 return P-values).')
	if de_sparse.is_sparse_design(dg):
		return _de_sparse_design(dg, dt, dc, bs, ka)
	dg0 = np.asarray(dg)
	dt = np.asarray(dt)
	dc = np.asarray(dc)
	if dg0.ndim != 2 or dt.ndim != 2 or dc.ndim != 2:
		raise ValueError('Incorrect dx/dy/dc size.')
	gid = _varying_rows(dg0)
	allrows = bool(gid.all())
	res = association_tests(dg0 if allrows else dg0[gid], dt, dc, bsx=bs, bsy=bs, return_dot=False, **ka)
	return _inflate(gid, res, dg0.shape[0], dt, dc.shape[0], logp=bool(ka.get('logp', False)))


assert __name__ != "__main__"
