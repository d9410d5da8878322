"""de with a sparse design matrix (a CRISPR screen's gRNA incidence): csrc/nrm_de_sparse.hip.

The reference multiplies residualised design and expression rows densely (association.py:224-235).  Because a residual is orthogonal to
the covariates, y~ . x~ = y . x - (y C^T) . b_x: a design row with few cells set needs the expression values at those cells only.  This
module decides whether a call qualifies, has the library turn the design matrix into the kernel's ELL lists (csrc/nrm_design_lists.hip),
takes the design rows' own statistics from those entries, runs the one-pass kernels on the raw expression rows, and K3 as always."""
import os

import numpy as np

from . import _lib, _opts
from ._lib import ROW_TILE
from . import engine as _engine

MAX_DENSITY = 1.0 / 16  # (break-even against K1 + the integer Gram engine is near one entry in ten)



def candidate(eng, dx, dy, dc, samexy):
	"""Cheap conditions that need no look at the data."""
	mode = os.environ.get('NRM_DE_SPARSE', '1')
	if samexy or dy is None or mode == '0' or eng._force_f64:  # (_force_f64: the call is being redone after a guard hit)
		return False
	nx, n = dx.shape
	if mode == 'force':  # (tests: small shapes through this path)
		return dc.shape[0] <= int(eng.lib.nrm_de_sparse_max_covariates())
	return nx >= 32 and dc.shape[0] <= int(eng.lib.nrm_de_sparse_max_covariates()) and dy.shape[0] >= 64 and n >= 2048 and nx * n >= (1 << 22)


MALFORMED_DESIGN_CSR = ('Malformed CSR design matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and '
						'increase strictly (sum duplicates and sort the indices first).')
_DENSE_WAY = 'a sparse {} is not taken here: pass a dense array (DesignCSR.dense() / toarray() give one).'


def _is_scipy_sparse(a):
	import sys
	sps = sys.modules.get('scipy.sparse')  # (whoever holds a scipy.sparse matrix has imported it: every dense call is spared the import)
	return sps is not None and sps.issparse(a)


def canonical_design_csr(m):
	"""A scipy.sparse design matrix of any format as canonical CSR over its rows, in O(stored entries): (indptr int64, indices int32, data), duplicates summed,
	columns sorted, zeros dropped (a NaN is kept: it is an entry).  data is fp32 for fp32 input and fp64 for everything else (integers, bools, other floats)."""
	if m.dtype.kind not in 'iufb':
		raise TypeError('the design matrix must hold real numbers.')
	if m.shape[1] > np.iinfo(np.int32).max:
		raise NotImplementedError('a sparse design with more than 2**31 - 1 cells.')
	c = m.tocsr()
	if c is m:
		c = c.copy()
	c.sum_duplicates()  # (in the matrix's own dtype, as toarray() adds them; sorts the columns of every row as well)
	if c.dtype not in (np.float32, np.float64):
		c = c.astype(np.float64)
	if c.data.size and (c.data == 0).any():
		c.eliminate_zeros()
	return c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data


class DesignCSR:
	"""A sparse design matrix (gRNA incidence) in HBM, canonical CSR over groupings: indptr (rows + 1) and indices (the cell of every stored entry, strictly
	increasing inside a row) 1-D torch CUDA tensors of integer dtype, data the values (floating, integer or bool; stored zeros are legal and are not entries) or
	None for all ones, shape = (n_grouping, n_cell).  de and association_tests take it as it is -- nothing is sorted or merged: the count kernel
	(csrc/nrm_design_csr.hip) checks the structure and a malformed matrix is a ValueError."""
	is_cuda, ndim = True, 2

	def __init__(self, indptr, indices, data, shape):
		shape = tuple(int(v) for v in shape)
		if len(shape) != 2 or min(shape) < 0:
			raise ValueError('DesignCSR: shape must be (n_grouping, n_cell).')
		for name, t in (('indptr', indptr), ('indices', indices)) + ((('data', data), ) if data is not None else ()):
			if not hasattr(t, 'data_ptr') or t.dim() != 1:
				raise ValueError('DesignCSR: {} must be a 1-D torch tensor.'.format(name))
		for name, t in (('indptr', indptr), ('indices', indices)):
			if t.dtype.is_floating_point or t.dtype.is_complex or str(t.dtype) == 'torch.bool':
				raise ValueError('DesignCSR: {} must have an integer dtype.'.format(name))
		if data is not None and data.dtype.is_complex:
			raise ValueError('DesignCSR: data must hold real numbers.')
		if indptr.numel() != shape[0] + 1:
			raise ValueError('DesignCSR: indptr must have n_grouping + 1 = {} entries, not {}.'.format(shape[0] + 1, indptr.numel()))
		if data is not None and indices.numel() != data.numel():
			raise ValueError('DesignCSR: indices and data must have the same length.')
		if shape[1] > np.iinfo(np.int32).max:
			raise NotImplementedError('DesignCSR with more than 2**31 - 1 cells.')
		parts = [indptr, indices] + ([data] if data is not None else [])
		if not all(t.is_cuda for t in parts) or not all(t.device == indptr.device for t in parts):
			raise ValueError('DesignCSR: indptr, indices and data must be CUDA tensors on one device.')
		self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape
		self._dense = self._checked = None

	@property
	def device(self):
		return self.indptr.device

	@property
	def dtype(self):
		"""The torch dtype the design is computed in: fp32 for fp32 data, else fp64 (what dense() gives by default)."""
		import torch
		return torch.float32 if (self.data is not None and self.data.dtype == torch.float32) else torch.float64

	@property
	def _version(self):
		"""In-place writes to any of the three tensors (torch counts them) make it another matrix for the caches."""
		return (self.indptr._version, self.indices._version, -1 if self.data is None else self.data._version)

	@classmethod
	def from_scipy(cls, m, device=None):
		"""Canonicalise a scipy.sparse matrix on the host (canonical_design_csr) and upload its three arrays."""
		eng = _engine.get_engine(device)
		return cls(*[eng.upload(a) for a in canonical_design_csr(m)], m.shape)

	def _ready(self, eng):
		"""(indptr int64, indices int32, data fp32 / fp64 or None, dtype code, stored entries) as the kernels read them: cast on the device where they are not."""
		torch = eng.torch
		data = self.data
		if data is not None:
			if data.dtype not in (torch.float32, torch.float64):
				data = data.to(torch.float64)
			data = data.contiguous()
		return (self.indptr.to(torch.int64).contiguous(), self.indices.to(torch.int32).contiguous(), data,
				_lib.NRM_F32 if data is None else _engine.dtype_code(data), int(self.indices.numel()))

	def check(self, eng=None):
		"""The structure check of nrm_design_csr_count by itself (once per state of the tensors): ValueError for a malformed matrix.  What looks at the arrays
		with anything but the library's kernels (torch indexing does not clamp) calls this first."""
		if self._checked == self._version:
			return self
		eng = eng or _engine.get_engine(self.device.index)
		torch = eng.torch
		nx, n = self.shape
		if nx == 0 or n == 0:
			raise ValueError('Dimensions in na==0 detected.')
		with eng.lock, torch.cuda.device(eng.device):
			indptr, indices, data, code, nnz = self._ready(eng)
			nslots = _engine.round_up(nx, 64)
			nch = (n + int(eng.lib.nrm_de_sparse_chunk()) - 1) // int(eng.lib.nrm_de_sparse_chunk())
			cnt = torch.empty((nch, nslots), dtype=torch.int32, device=eng.device)
			info = torch.empty(8, dtype=torch.int64, device=eng.device)
			_lib.check(eng.lib.nrm_design_csr_count(indptr.data_ptr(), _engine.ptr(indices), _engine.ptr(data), code, nx, n, nnz, cnt.data_ptr(), nslots, info.data_ptr(), eng._stream()))
			if int(info.cpu()[_lib.DESIGN_CSR_BAD]):
				raise ValueError(MALFORMED_DESIGN_CSR)
		self._checked = self._version
		return self

	def dense(self, dtype=None):
		"""The design as a dense (n_grouping, n_cell) tensor in HBM (nrm_design_csr_dense: a zero fill and a scatter on the device), for the routes that read a
		matrix; kept until one of the three tensors is written to.  dtype: torch.float32 / torch.float64; None: fp32 for fp32 data, else fp64 -- what the
		same design handed over dense would be computed in."""
		eng = _engine.get_engine(self.device.index)
		torch = eng.torch
		if dtype is None:
			dtype = self.dtype
		if dtype not in (torch.float32, torch.float64):
			raise ValueError('DesignCSR.dense: dtype must be torch.float32 or torch.float64.')
		hit = self._dense
		if hit is not None and hit[0] == self._version and hit[1].dtype == dtype:
			return hit[1]
		self.check(eng)
		nx, n = self.shape
		with eng.lock, torch.cuda.device(eng.device):
			indptr, indices, data, code, _ = self._ready(eng)
			out = torch.empty((nx, n), dtype=dtype, device=eng.device)
			_lib.check(eng.lib.nrm_design_csr_dense(indptr.data_ptr(), _engine.ptr(indices), _engine.ptr(data), code, nx, n, out.data_ptr(), _engine.dtype_code(out), out.stride(0),
													eng._stream()))
		import weakref
		out._nrm_design_csr = weakref.ref(self)  # (lists_for: the lists of this tensor come from the entries it was written from)
		self._dense = (self._version, out)
		return out


def as_design_csr(d):
	"""The device forms of a sparse design -- a DesignCSR, a torch tensor of layout torch.sparse_csr in HBM -- as a DesignCSR (the same one for the same tensor:
	the list caches go by identity); None for anything else."""
	if isinstance(d, DesignCSR):
		return d
	if _engine.is_dev(d) and str(getattr(d, 'layout', '')) == 'torch.sparse_csr':
		hit = getattr(d, '_nrm_design', None)
		if hit is None:
			hit = DesignCSR(d.crow_indices(), d.col_indices(), d.values(), d.shape)
			try:
				d._nrm_design = hit
			except AttributeError:
				pass
		return hit
	return None


def is_sparse_design(d):
	"""A design in one of the sparse forms de / association_tests take: a scipy.sparse matrix, a DesignCSR, a torch.sparse_csr CUDA tensor."""
	return isinstance(d, DesignCSR) or _is_scipy_sparse(d) or (_engine.is_dev(d) and str(getattr(d, 'layout', '')) == 'torch.sparse_csr')


def refuse_sparse(d, what):
	"""TypeError for a sparse matrix where only the design of de / association_tests may be one."""
	if is_sparse_design(d) or str(getattr(d, 'layout', 'torch.strided')) != 'torch.strided':
		raise TypeError(_DENSE_WAY.format(what))


class Lists:
	"""The design matrix as the kernels read it, built by the library's own kernels (csrc/nrm_design_lists.hip: two passes over the matrix, a
	counting rank per chunk, two prefix sums -- no torch / rocPRIM kernel, one small device-to-host copy for the sizes):
	  CSR   row_ptr (nx + 1), cells (int32), row_vals (fp64 or None): the entries row by row, cells ascending (design_stats, single=1's selection);
	  ELL   for every chunk of cells and every 64 positions of k_de_sparse's lanes (the design rows are dealt to the positions chunk by chunk,
	        sorted by their number of entries in the chunk), the entries of the 64 rows side by side, padded to the longest (ell=False: not built).
	max_density: the largest share of entries set for which the lists are built at all (ok = False beyond it, and for an empty design).
	Lists.from_csr builds the same lists -- the same bytes -- from a DesignCSR (csrc/nrm_design_csr.hip: two walks over the stored entries)."""

	def __init__(self, eng, d_x, ell=True, max_density=MAX_DENSITY):
		torch = eng.torch
		nx, n = d_x.shape
		if d_x.dtype not in (torch.float32, torch.float64):
			d_x = d_x.to(torch.float64)
		if d_x.stride(1) != 1:
			d_x = d_x.contiguous()
		code = _engine.dtype_code(d_x)
		count = lambda cnt, nslots, info, st: eng.lib.nrm_design_count(d_x.data_ptr(), code, nx, n, d_x.stride(0), cnt, nslots, info, st)
		fill = lambda nslots, *rest: eng.lib.nrm_design_fill(d_x.data_ptr(), code, nx, n, d_x.stride(0), nslots, *rest)
		self._build(eng, nx, n, ell, max_density, count, fill)

	@classmethod
	def from_csr(cls, eng, csr, ell=True, max_density=MAX_DENSITY):
		"""The lists of a DesignCSR (or a torch.sparse_csr CUDA tensor): the same fields, the same single read-back between plan and fill; ValueError
		(MALFORMED_DESIGN_CSR) for a matrix that is not canonical CSR.  No dense matrix is formed."""
		csr = as_design_csr(csr)
		nx, n = csr.shape
		if nx == 0 or n == 0:
			raise ValueError('Dimensions in na==0 detected.')
		indptr, indices, data, code, nnz = csr._ready(eng)
		head = (indptr.data_ptr(), _engine.ptr(indices), _engine.ptr(data), code, nx, n)
		count = lambda cnt, nslots, info, st: eng.lib.nrm_design_csr_count(*head, nnz, cnt, nslots, info, st)
		fill = lambda nslots, *rest: eng.lib.nrm_design_csr_fill(*head, nslots, *rest)
		self = cls.__new__(cls)
		self._build(eng, nx, n, ell, max_density, count, fill)
		csr._checked = csr._version
		return self

	def _build(self, eng, nx, n, ell, max_density, count, fill):
		torch = eng.torch
		ch = int(eng.lib.nrm_de_sparse_chunk())
		nslots = _engine.round_up(nx, 64)
		nch = (n + ch - 1) // ch
		self.ngroups = nslots // 64
		i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=eng.device)
		st = eng._stream()
		cnt, coff = i32(nch, nslots), i32(nch, nslots)
		info = torch.empty(8, dtype=torch.int64, device=eng.device)
		self.row_ptr = torch.empty(nx + 1, dtype=torch.int64, device=eng.device)
		self.slot2x = i32(nslots)
		sig = pos = w = base = None
		if ell:
			sig, pos, w = i32(nch, nslots), i32(nch, nslots), i32(nch * self.ngroups)
			base = torch.empty(nch * self.ngroups, dtype=torch.int64, device=eng.device)
		_lib.check(count(cnt.data_ptr(), nslots, info.data_ptr(), st))
		_lib.check(eng.lib.nrm_design_plan(cnt.data_ptr(), nx, n, nslots, _engine.ptr(sig), _engine.ptr(pos), _engine.ptr(w), _engine.ptr(base), self.row_ptr.data_ptr(), coff.data_ptr(),
										   self.slot2x.data_ptr(), info.data_ptr(), st))
		h = info.cpu().numpy()  # the one synchronisation: the sizes of what follows
		if h[_lib.DESIGN_CSR_BAD]:
			raise ValueError(MALFORMED_DESIGN_CSR)
		self.nnz, self.padded, self.bits = int(h[0]), int(h[1]), int(h[2])
		self.binary = not (self.bits & _lib.DESIGN_NOTONE)
		self.ok = 0 < self.nnz <= max_density * nx * n
		if not self.ok:
			return
		self.cells = i32(max(self.nnz, 1))
		self.row_vals = None if self.binary else torch.empty(max(self.nnz, 1), dtype=torch.float64, device=eng.device)
		self.ell = self.vals = None
		if ell:
			self.ell = torch.empty(max(self.padded, 8), dtype=torch.int16, device=eng.device)
			self.vals = None if self.binary else torch.empty(max(self.padded, 8), dtype=torch.float64, device=eng.device)
		_lib.check(fill(nslots, _engine.ptr(pos), _engine.ptr(w), _engine.ptr(base), self.row_ptr.data_ptr(), coff.data_ptr(),
						_engine.ptr(self.ell), _engine.ptr(self.vals), self.cells.data_ptr(), _engine.ptr(self.row_vals), 1 if self.binary else 0, st))
		self.sig, self.base, self.w = sig, base, w


def design_source(d_x):
	"""What the lists of d_x are built from: the DesignCSR itself, the DesignCSR a dense tensor was written from (DesignCSR.dense(), still in that state), or None."""
	csr = as_design_csr(d_x)
	if csr is not None:
		return csr
	ref = getattr(d_x, '_nrm_design_csr', None)
	src = ref() if ref is not None else None
	if src is not None and src._dense is not None and src._dense[1] is d_x and src._dense[0] == src._version:
		return src
	return None


def cached_lists(eng, slot, d_x, **ka):
	"""Lists of d_x (a dense device tensor, a DesignCSR or a torch.sparse_csr CUDA tensor), kept in eng.<slot> for the next call on the SAME object as long as
	it has not been written to (torch counts in-place writes in ._version; a weak reference: the cache keeps no design alive, and a new tensor at an old
	address is not the same object)."""
	import weakref
	key = as_design_csr(d_x) or d_x
	hit = getattr(eng, slot, None)
	if hit is not None and hit[0]() is key and hit[1] == key._version:
		return hit[2]
	src = design_source(d_x)
	lists = Lists(eng, d_x, **ka) if src is None else Lists.from_csr(eng, src, **ka)
	setattr(eng, slot, (weakref.ref(key), key._version, lists))
	return lists


def lists_for(eng, d_x):
	"""Lists of the design for single=0 / single=4 -- a resident screen analysed again and again pays for its lists once (cached_lists)."""
	return cached_lists(eng, '_sparse_lists', d_x)


class DesignRows:
	"""What the sweep and alpha need of the design rows: their sums of squares and coefficients (the fields of engine.Residualized they read)."""

	def __init__(self, ss, coef):
		self.ss, self.coef = ss, coef


def design_stats(eng, lists, d_c, d_dci, rank, nx, nc, flags=None):
	"""|x~_i|^2 and b_i of every design row from its entries (csrc/nrm_de_sparse.hip: k_design_stats) -- K1 would sweep n cells twice
	for rows that have a few hundred entries.  flags: the call's device counters; [2] counts design rows too close to the span of the
	covariates for that difference (the caller redoes such a call on the dense path)."""
	torch = eng.torch
	ncu = nc if (rank > 0 and nc > 0) else 0
	ss = eng.zeros((_engine.round_up(nx, ROW_TILE), ), torch.float64)
	coef = eng.zeros((nx, nc), torch.float64) if nc else eng.zeros((nx, 1), torch.float64)[:, :0]  # (covariates of rank 0: the coefficients stay zero)
	with _engine._Span(eng, 'design_stats'):
		_lib.check(eng.lib.nrm_design_stats(lists.row_ptr.data_ptr(), lists.cells.data_ptr(), 0 if lists.row_vals is None else lists.row_vals.data_ptr(),
											d_c.data_ptr() if ncu else 0, d_c.stride(0) if ncu else 0, ncu, d_dci.data_ptr() if ncu else 0, nx, ss.data_ptr(),
											coef.data_ptr() if ncu else 0, 0 if flags is None else flags.data_ptr(), eng._stream()))
	return DesignRows(ss, coef)


def run(eng, d_x, lists, dy, d_c, d_dci, rank, nx, ny, n, nc, want_coef, flags=None):
	"""The design rows' statistics from their entries, the one-pass kernels on the expression rows.
	Returns (dot (nx_pad, ny_pad) fp64 with dot[i, y] = x~_i . y~_y, rx, ssy, coefy); rx.yraw = the raw rows' |y|^2."""
	rx = design_stats(eng, lists, d_c, d_dci, rank, nx, nc, flags)
	dot, ssy, coefy, common = products(eng, lists, dy, d_c, d_dci, rank, rx.coef, nx, ny, n, nc, want_coef, False, flags)
	rx.yraw = common[-1]  # |y|^2 of the raw rows (flagged_rows)
	return dot, rx, ssy, coefy


def flagged_rows(eng, ssy, yraw, ny):
	"""Indices (device, int64) of the expression rows k_de_sparse counted into flags[2]: |y~|^2 < 1e-4 |y|^2 (the kernel's own test, on what it
	stored).  Only looked at after the counter came back non-zero -- the exceptional path, a few torch launches."""
	torch = eng.torch
	s, q = ssy[:ny], yraw[:ny]
	return torch.nonzero(~(s >= 1e-4 * q) & (q > 0)).reshape(-1)


def products(eng, lists, dy, d_c, d_dci, rank, bx, nx, ny, n, nc, want_coef, by_gene, flags=None):
	"""x~_i . y~_y for every design row and expression row from the RAW expression rows (csrc/nrm_de_sparse.hip), |y~|^2 and, on request,
	the expression rows' coefficients b_y.  by_gene: the products as (ny_pad, nx_pad) (single=4 reads them so), else (nx_pad, ny_pad).
	flags: the call's device counters (engine.new_flags); [2] counts rows too close to the span of the covariates for these differences."""
	torch = eng.torch
	active = rank > 0 and nc > 0
	d_y = dy if not isinstance(dy, np.ndarray) else eng.upload(_engine.as_input(dy))
	nxp, nyp = _engine.round_up(nx, ROW_TILE), _engine.round_up(ny, ROW_TILE)
	dot = eng.zeros((nyp, nxp), torch.float64) if by_gene else torch.empty((nxp, nyp), dtype=torch.float64, device=eng.device)
	ssy = torch.empty((nyp, ), dtype=torch.float64, device=eng.device)
	ncu = nc if active else 0  # (covariates of rank 0 -- all zero -- leave the rows as they are: association.py:899-903)
	coefy = eng.zeros((ny, nc), torch.float64) if want_coef else None
	ycode = _engine.dtype_code(d_y)
	common = torch.empty((ncu + 1, ny), dtype=torch.float64, device=eng.device)
	# The rows' products with the covariates and their sums of squares: inside the gather kernel, on the fp64 matrix cores, from the chunk of rows
	# it holds in LDS anyway -- one pass over the expression matrix -- for up to 8 covariates besides a constant one (csrc/nrm_de_sparse.hip);
	# beyond that (or NRM_DE_SPARSE_SUMS=stream) the stream kernel of single=1 takes them first, every cell "common": a second pass.
	ci, cval = eng.constant_row(d_c) if ncu else (-1, 0.0)
	fused = ncu - (1 if ci >= 0 else 0) <= int(eng.lib.nrm_de_sparse_fused_covariates()) and _opts.debug('de_sparse_sums', 'inside') != 'stream'
	ct = None
	if fused:
		ct = torch.empty((int(eng.lib.nrm_de_sparse_ct_doubles(n, ncu, ci)), ), dtype=torch.float64, device=eng.device)
	else:
		code = getattr(eng, '_all_common', None)
		if code is None or code.numel() < n:
			code = eng._all_common = torch.empty((n, ), dtype=torch.int32, device=eng.device)
			_lib.check(eng.lib.nrm_fill_i32(code.data_ptr(), _lib.NRM_S1_COMMON, n, eng._stream()))
		with _engine._Span(eng, 'row_sums'):
			_lib.check(eng.lib.nrm_single1_stream(d_y.data_ptr(), ycode, d_y.stride(0), d_c.data_ptr() if ncu else 0, d_c.stride(0) if ncu else n, ncu, code.data_ptr(), n, ny,
												  common.data_ptr(), common.data_ptr(), _engine.round_up(ny, 8), eng._stream()))  # (no cell keeps its values: the last buffer is not written)
	with _engine._Span(eng, 'de_sparse'):
		_lib.check(eng.lib.nrm_de_sparse(d_y.data_ptr(), ycode, ny, n, d_y.stride(0), common.data_ptr(), ncu, d_dci.data_ptr() if ncu else 0, lists.ell.data_ptr(),
										 0 if lists.vals is None else lists.vals.data_ptr(), lists.base.data_ptr(), lists.w.data_ptr(), lists.sig.data_ptr(), lists.ngroups,
										 lists.slot2x.data_ptr(), bx.data_ptr() if ncu else 0, max(nc, 1), dot.data_ptr(), dot.stride(0), 1 if by_gene else 0, ssy.data_ptr(),
										 coefy.data_ptr() if (coefy is not None and ncu) else 0, 0 if flags is None else flags.data_ptr(),
										 d_c.data_ptr() if ncu else 0, d_c.stride(0) if ncu else n, ci, float(cval), 0 if ct is None else ct.data_ptr(), eng._stream()))
	return dot, ssy, coefy, common


assert __name__ != "__main__"
