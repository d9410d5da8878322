"""The co-expression loop of the reference's example (examples/GSE123139/code/cmd_coex.sh:37-46: coex -> binnet -> gocovt, once per level, each level appending
the top pathway's principal component as a covariate) with the problem resident in HBM.

Between two levels the expression matrix does not change and the covariates grow by one row.  Let q be the new covariate with everything in the span of the
present covariates removed, scaled to unit length.  The Gram matrix of the residualised genes G = X (I - P) X^T (association.py:224-235) then changes by a rank-one
term, G' = G - a a^T with a_i = x_i . q taken on the RAW row (Frisch-Waugh: q is orthogonal to the covariates), the sums of squares to ss' = ss - a^2 and the
degrees of freedom by one.  A level after the first costs one read of the expression matrix (nrm_coex_project), one pass over G (nrm_coex_downdate) and the existing
K3 sweep; K1 and K2 run at construction and at a rebuild only.  Kernels: csrc/nrm_coex_levels.hip.  DESIGN.md section 6l has the identity, the rules below and
their derivations.

  rank rule    the rank after an append is _prepare_covariates' on the enlarged covariates, the function coex itself calls.  rho = |q|^2 / |v|^2 of every new row v is
               taken against the basis B of the present covariates (and, for several rows at once, the rows accepted before it, in order).  The update runs only when the rank grows by exactly the number of rows with rho >= RHO_MIN and
               every other row has rho <= RHO_SPAN (it lies in the span and changes nothing); anything else is rebuilt from scratch.
  guard        the downdate counts the genes whose sum of squares fell to less than 2^-10 of what it was at the last from-scratch build, and those whose sum is no
               longer finite and positive; either count rebuilds from scratch on the enlarged covariates, which refreshes the reference sums.
"""
import logging

import numpy as np

from .association import _check_dimreduce, _prepare_covariates
from . import _opts
from . import engine as _engine

RHO_MIN = 1e-6    # a new row keeping at least this part of its squared length outside the span is a new direction
RHO_SPAN = 1e-12  # a new row keeping at most this part lies in the span
_PROJECT_ROWS = 8  # directions per launch of nrm_coex_project


class NonFiniteCovariates(AssertionError, ValueError):
	"""Covariates with a NaN or an infinity.  coex answers them with ValueError('array must not contain infs or NaNs') from inv_rank (the reference: scipy's
	check_finite, association.py:66); the class is an AssertionError as well, which is what a caller of append is told to expect."""



def _host(a):
	return np.asarray(a.cpu() if hasattr(a, 'data_ptr') else a)


def _check_problem(dt_shape, dc, dimreduce):
	"""coex's argument checks (association.py:199-216 as association_tests applies them), on shapes and the covariates alone: returns (dc64, dci, rank, dimreduce)."""
	if len(dt_shape) != 2 or dc.ndim != 2:
		raise ValueError('Incorrect dx/dy/dc size.')
	dimreduce = _check_dimreduce(dimreduce)
	n = int(dt_shape[1])
	if dc.shape[1] != n:
		raise ValueError('Unmatching dx/dy/dc dimensions.')
	if dt_shape[0] == 0:
		raise AssertionError('No association test to perform.')
	if dc.dtype.kind not in 'biuf' or not np.isfinite(dc).all():
		raise NonFiniteCovariates('array must not contain infs or NaNs')
	if dc.shape[0] == 0:
		logging.warning('No covariate dc input.')
	dc64, dci, dcr = _prepare_covariates(dc)
	if n <= dcr + dimreduce + 1:
		raise ValueError('Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.')
	return dc64, dci, int(dcr), dimreduce


def covariate_basis(dc, tol=1E-8):
	"""(B, rank): orthonormal rows (rank, n_cell), fp64, spanning what coex removes for the covariates dc -- the eigenvectors of dc dc^T whose eigenvalue reaches tol x the
	largest, the rule of inv_rank (association.py:77-80), carried to the cells and orthonormalised once more."""
	dc64 = np.asarray(dc, dtype=np.float64)
	nc, n = dc64.shape
	if nc == 0 or not (dc64 != 0).any():
		return np.zeros((0, n)), 0
	_, s, vh = np.linalg.svd(np.matmul(dc64, dc64.T))
	r = int(nc - np.searchsorted(s[::-1], tol * s[0]))
	b0 = np.matmul(vh[:r], dc64) / np.sqrt(s[:r])[:, None]
	q, _ = np.linalg.qr(b0.T)
	return np.ascontiguousarray(q.T), r


def _off_span(b, v):
	"""v - B^T B v, applied twice (what the first pass leaves along B is removed by the second, as pccovt does)."""
	for _ in range(2):
		if b.shape[0]:
			v = v - np.matmul(np.matmul(b, v), b)
	return v


def plan_append(b, dc, rows, rank=None):
	"""The decision of CoexLevels.append, a pure function of the present basis b (rank, n_cell), the present covariates dc and the new rows (k, n_cell): a dict with
	rank (of the enlarged covariates, by _prepare_covariates unless given), rho (k), update (bool: the rank-one path may run) and q (m, n_cell), the orthonormal new directions
	in the order of their rows (m = 0: every row lies in the span)."""
	rows = np.asarray(rows, dtype=np.float64)
	if rank is None:  # (append hands over the rank it has already taken for coex's checks: the SVD behind it is the host's largest cost with hundreds of covariates)
		rank = int(_prepare_covariates(np.concatenate([np.asarray(dc, dtype=np.float64), rows], axis=0))[2])
	rho = np.zeros(rows.shape[0])
	qs = []
	ok = True
	for i, v in enumerate(rows):
		vv = float(np.dot(v, v))
		if vv == 0:
			continue
		q = _off_span(b, v)
		if qs:
			q = _off_span(np.array(qs), q)  # and off the directions accepted before it, in order: k rows at once are k single appends
		left = float(np.dot(q, q))
		rho[i] = left / vv
		if rho[i] >= RHO_MIN:
			qs.append(q / np.sqrt(left))
		elif rho[i] > RHO_SPAN:
			ok = False
	update = bool(ok and rank - b.shape[0] == len(qs))
	return dict(rank=rank, rho=rho, update=update, q=np.array(qs).reshape(len(qs), rows.shape[1]) if update else np.zeros((0, rows.shape[1])))


class CoexLevels:
	"""coex(dt, dc) that stays in HBM while covariates are appended.
	dt: (n_gene, n_cell) fp32 or fp64, numpy or a torch CUDA tensor, as coex takes it; dc: (n_cov, n_cell) numpy.  Construction is the from-scratch build (K1 and the
	fp64 Gram kernel); it keeps G (n_gene^2 x 8 bytes), the sums of squares, their copy from the build and dt resident, and on the host an orthonormal basis of the
	covariates' row space.
	results(device_out=False) -> (p, dot, var) under the contract and types of coex(dt, self.dc, dimreduce=dimreduce, device_out=...); one sweep per level, cached.
	append(rows) -> self: rows (n_cell, ) or (k, n_cell); every check of coex on the enlarged covariates before any state changes.
	Attributes: level (appends so far), dc (all rows so far), rank, dof, rebuilt (one bool per append), info (the last append's rho and counters).
	A dt tensor written in place after construction (torch counts such writes) makes the next append or results rebuild from its current content."""

	def __init__(self, dt, dc, dimreduce=0, device=None, logp=False):
		_opts.refuse_logp(logp, 'CoexLevels')
		dev = _engine.is_dev(dt)
		if not dev:
			dt = np.asarray(dt)
		dc = _host(dc)
		dc64, dci, dcr, self.dimreduce = _check_problem(tuple(dt.shape), dc, dimreduce)
		self._eng = _engine.get_engine(dt.device.index if dev else device)
		self.nt, self.ns = (int(v) for v in dt.shape)
		if dev:
			self.out_dtype = np.dtype(np.float32 if 'float32' in str(dt.dtype) else np.float64)
		else:
			self.out_dtype = dt.dtype if dt.dtype in (np.float32, np.float64) else np.dtype(np.float64)
		self._src = dt if dev else None  # the caller's tensor: its ._version tells an in-place rewrite
		self._x = None if dev else self._eng.upload(_engine.as_input(dt))
		self.dc = dc
		self.level, self.rebuilt, self.info = 0, [], dict(rho=np.zeros(0), counters=(0, 0))
		self._cache = None
		with self._eng.lock:
			self._build(dc64, dci, dcr)

	# ---- state ---------------------------------------------------------------------------------------------------------------------------------------------------
	@property
	def dof(self):
		return self.ns - 1 - self.rank - self.dimreduce

	def _rows(self):
		"""The expression as the kernels read it: fp32 or fp64 with unit column stride.  The caller's tensor itself whenever it already is."""
		if self._src is None:
			return self._x
		torch = self._eng.torch
		x = self._src if self._src.dtype in (torch.float32, torch.float64) else self._src.to(torch.float64)
		return x if x.stride(1) == 1 and x.stride(0) >= self.ns else x.contiguous()

	def _stale(self):
		return self._src is not None and self._src._version != self._version

	def _build(self, dc64, dci, dcr):
		"""From scratch on the covariates dc64: K1, the fp64 Gram kernel; the fp64 residual rows are freed."""
		eng = self._eng
		with eng.torch.cuda.device(eng.device):
			if self._src is not None:
				self._version = self._src._version
				self._x = self._rows()
			d_c, d_dci = eng.covariates(dc64, dci)
			rx = eng.residualize(self._x, d_c, d_dci, dcr, nslices=0, keep_fp64=True)
			self._g = eng.gram(rx, rx, True, nslices=0)
			self._ss = rx.ss
			self._ss_ref = rx.ss.clone()
			del rx
		self._b, r = covariate_basis(dc64)
		assert r == dcr, (r, dcr)
		self.rank = int(dcr)
		self._cache = None

	def _rebuild(self):
		self._build(*_prepare_covariates(self.dc))

	# ---- results -------------------------------------------------------------------------------------------------------------------------------------------------
	def results(self, device_out=False):
		eng = self._eng
		with eng.lock:
			if self._stale():
				self._rebuild()
			if self._cache is None:
				p, stat, _, _, flags = eng.sweep(self._g, self._ss, self._ss, self.nt, self.nt, self.ns, self.dof, True, 0, self.out_dtype)
				eng.check_flags(flags)
				self._cache = (p, stat, eng.variances(self._ss, self.nt, self.ns, self.out_dtype))
			p, stat, var = self._cache
			if device_out:
				return p, stat, var.copy()
			return eng.download(p), eng.download(stat), var.copy()

	# ---- append --------------------------------------------------------------------------------------------------------------------------------------------------
	def append(self, rows):
		rows = _host(rows)
		if rows.ndim == 1:
			rows = rows.reshape(1, -1)
		if rows.ndim != 2:
			raise ValueError('Incorrect dx/dy/dc size.')
		if rows.shape[1] != self.ns:
			raise ValueError('Unmatching dx/dy/dc dimensions.')
		alld = np.concatenate([self.dc, rows], axis=0)
		dc64, dci, dcr, _ = _check_problem((self.nt, self.ns), alld, self.dimreduce)
		eng = self._eng
		with eng.lock:
			stale = self._stale()
			plan = plan_append(self._b, self.dc, rows, rank=dcr) if not stale else dict(rank=dcr, rho=np.full(rows.shape[0], np.nan), update=False)
			assert plan['rank'] == dcr
			counters = (0, 0)
			rebuilt = not plan['update']
			if plan['update'] and plan['q'].shape[0]:
				counters = self._downdate(plan['q'])
				rebuilt = counters[0] > 0 or counters[1] > 0
			self.dc = alld
			self.level += 1
			self.info = dict(rho=plan['rho'], counters=counters)
			self.rebuilt.append(bool(rebuilt))
			if rebuilt:
				self._build(dc64, dci, dcr)
				if counters[0] > 0:
					self.results(device_out=True)  # (a sum of squares that is still not finite raises here what coex raises)
			elif plan['q'].shape[0]:
				self._b = np.concatenate([self._b, plan['q']], axis=0)
				self.rank = dcr
				self._cache = None
		return self

	def _downdate(self, q):
		"""G -= a a^T and ss -= a^2 for the orthonormal directions q (m, n_cell); returns the two counters."""
		from . import _lib
		eng = self._eng
		torch = eng.torch
		m = q.shape[0]
		with torch.cuda.device(eng.device):
			d_q = eng.upload(np.ascontiguousarray(q, dtype=np.float64))
			a = torch.empty((m, self.nt), dtype=torch.float64, device=eng.device)
			counters = eng.zeros((2, ), torch.int32)
			x = self._x
			stream = eng._stream()
			with _engine._Span(eng, 'coex_project'):
				for k0 in range(0, m, _PROJECT_ROWS):
					k = min(_PROJECT_ROWS, m - k0)
					_lib.check(eng.lib.nrm_coex_project(x.data_ptr(), _engine.dtype_code(x), self.nt, self.ns, x.stride(0),
														d_q[k0:].data_ptr(), k, d_q.stride(0), a[k0:].data_ptr(), a.stride(0), stream))
			with _engine._Span(eng, 'coex_downdate'):
				_lib.check(eng.lib.nrm_coex_downdate(self._g.data_ptr(), self.nt, self._g.stride(0), self._ss.data_ptr(), self._ss_ref.data_ptr(), a.data_ptr(), m,
													 a.stride(0), counters.data_ptr(), stream))
			c = counters.cpu().numpy()  # (the one read-back of an append)
		return int(c[0]), int(c[1])


def _iter_levels(dt, dc, namet, sets, qcut, lvmax, n, nmin, dimreduce, condcov, keep, device_out):
	"""The records of coex_levels one by one, as they complete; a step's known failure ends the sequence with a record that holds `stopped` and `error`."""
	from . import binnet as _binnet, enrich as _enrich, gocovt
	keep = tuple(keep)
	for k in keep:
		if k not in ('p', 'dot', 'var', 'net'):
			raise ValueError('keep names p, dot, var and net only.')
	if int(lvmax) != lvmax or lvmax < 0:
		raise ValueError('lvmax must be a non-negative integer.')
	if qcut <= 0 or qcut >= 1:
		raise ValueError('Q-value cutoff must be between 0 and 1.')
	if not _engine.is_dev(dt):
		dt = np.asarray(dt)
	dc = _host(dc)
	_check_problem(tuple(dt.shape), dc, dimreduce)
	namet = np.asarray(namet)
	if namet.ndim != 1 or namet.shape[0] != dt.shape[0] or dt.shape[0] <= 1:
		raise ValueError('Wrong shape for net or namet.')
	gocovt._check_principal_args((int(dt.shape[0]), int(dt.shape[0])), n)
	bound = sets if isinstance(sets, _enrich.BoundSets) else sets.bind(namet)
	lv = CoexLevels(dt, dc, dimreduce=dimreduce)
	eng = lv._eng
	x = lv._src if lv._src is not None else lv._x  # pccovt reads the resident rows
	host = lambda t: eng.download(t.view(eng.torch.uint8)).view(np.bool_) if t.dtype == eng.torch.bool else eng.download(t)
	give = (lambda t: t) if device_out else host
	for level in range(int(lvmax) + 1):
		rec = dict(level=level, cov=lv.dc)
		try:
			p, dot, var = lv.results(device_out=True)
			for k, v in (('p', p), ('dot', dot)):
				if k in keep:
					rec[k] = give(v)
			if 'var' in keep:
				rec['var'] = var
			net = _binnet.binnet(p, qcut)
			if 'net' in keep:
				rec['net'] = give(net)
			principals, res, top, genes = _enrich.top_pathway(net, namet, bound, n=n, nmin=nmin)
			rec.update(principals=principals, result=res, top=top, genes=genes)
			cov_next = gocovt.pccovt(x, lv.dc, namet, genes, condcov=condcov)
			lv.append(cov_next[-1])
			rec.update(cov_next=cov_next, rebuilt=lv.rebuilt[-1])
		except (RuntimeError, ValueError) as e:
			known = isinstance(e, RuntimeError) and (str(e) == 'Empty binary network.' or str(e).startswith('Not enough principal genes'))
			known = known or (isinstance(e, ValueError) and str(e) == 'No GO enrichment found for given criteria.')
			if not known:
				raise
			rec.update(stopped=str(e), error=e)
			yield rec
			return
		yield rec


def coex_levels(dt, dc, namet, sets, qcut, lvmax=5, n=100, nmin=5, dimreduce=0, condcov=True, keep=('net', ), strict=True, device_out=False, logp=False):
	"""The loop of the reference's co-expression example (cmd_coex.sh:37-46) on a resident problem: for level 0 .. lvmax, co-expression given the covariates so far
	(CoexLevels.results), the binary network (binnet.binnet at qcut), the principal genes and their top gene set (enrich.top_pathway with n, nmin; sets: a GeneSets,
	bound once, or a BoundSets), the top principal component of that set's genes as one more covariate (gocovt.pccovt with condcov), appended.  Between levels only
	the score vector, the covariates and the small records cross PCIe.
	Returns one dict per level: level, cov (the covariates used), principals, top (the set's name), genes, result (the EnrichResult), cov_next, rebuilt, and whichever
	of p, dot, var, net keep names (numpy, or with device_out=True torch CUDA tensors; var is numpy).
	strict=True raises what a step raises (RuntimeError 'Empty binary network.' / 'Not enough principal genes...', ValueError 'No GO enrichment found for given
	criteria.'); strict=False ends the loop there and returns the completed levels and a last record with what that level had produced and stopped=<message>."""
	_opts.refuse_logp(logp, 'coex_levels')
	out = []
	for rec in _iter_levels(dt, dc, namet, sets, qcut, lvmax, n, nmin, dimreduce, condcov, keep, device_out):
		err = rec.pop('error', None)
		if err is not None and strict:
			raise err
		out.append(rec)
	return out


assert __name__ != "__main__"
