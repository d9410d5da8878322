"""The covariate of the top principal component of chosen genes (mirror of the numerical parts of the reference's normalisr.gocovt, gocovt.py:257-266 and
:271-321), on an expression matrix that may stay in HBM.

principal_genes takes the row degrees of a binary co-expression network (nrm_net_degree) and keeps every gene whose degree reaches that of the n-th ranked
one: the selection inside the reference's gotop.  The GO enrichment that follows it there (goe: goatools and a web service) is not part of this build; a user
runs it with any tool on the list of names and hands the pathway's genes to pccovt -- or with normalisr_amd.enrich, which does that step's arithmetic on the
device from local gene-set files.

pccovt removes the covariates and the mean from the chosen rows, brings every row to mean square 1, takes the top principal component over the cells and
appends it as a covariate row.  The reference takes the component from a randomized SVD (sklearn's TruncatedSVD: 5 power iterations from an unseeded
sketch), which approximates it and differs from call to call; here it is the exact component to rounding, and the same bits on every run:
  gather        the m chosen rows (nrm_subset_dense on a resident matrix; a host matrix is cut before its upload)
  K1            nrm_residualize against the design [dc; 1] (the constant row alone without conditioning), applied twice -- the second pass removes what the
                normal equations of the first leave along the covariates --: fp64 residual rows Zres and their sums of squares
  K2            nrm_gram_f64, symmetric: G = Zres Zres^T
  correlation   nrm_pc_correlation: a_g = 1 / (sqrt(ss_g / n) + 1e-200), R = diag(a) G diag(a) / n; a row of exact zeros gives a zero row of R
  power         nrm_pc_power: v <- R v / |R v| from a fixed start; the host reads (lambda, |R v - lambda v|) back every 16 steps and stops at
                |R v - lambda v| <= 16 m u lambda (u = 2^-53), or at max_iter with a RuntimeWarning
  score         nrm_pc_score: the sign rule of sklearn's svd_flip (the loading of largest magnitude is positive, the first of equals), then
                score[j] = sum_g v_g a_g Zres[g, j] -- Z^T v with Z the scaled rows, |score|^2 = sigma_1^2
Kernels: csrc/nrm_pc.hip.  Arithmetic is fp64 whatever the input's type."""
import logging
import warnings

import numpy as np

from . import engine as _engine

_POWER_BLOCK = 16  # power steps between two read-backs of (lambda, residual)
_UNIT = 2.0**-53
_K1_PASSES = 2  # applications of K1 to the chosen rows (see pccovt)



def _check_principal_args(shape, n):
	if len(shape) != 2 or shape[0] != shape[1] or shape[0] <= 1:
		raise ValueError('Wrong shape for net or namet.')
	if n <= 1 or n >= shape[0]:
		raise ValueError('Number of principal genes must be from 1 to the number of all genes (exclusive).')


def _select_principal(deg, n):
	"""The reference's selection on the degrees (gocovt.py:258-265): the genes whose degree reaches that of the gene ranked n (0-based, descending), in rising
	order.  RuntimeError when that degree is 0."""
	deg = np.asarray(deg)
	thr = np.sort(deg)[::-1][n]
	if thr == 0:
		raise RuntimeError('Not enough principal genes that have co-expression')
	sel = np.flatnonzero(deg >= thr).astype(np.int64)
	assert n <= len(sel) < len(deg)
	return sel


def net_degree(net, device_out=False):
	"""Row sums of a binary network on the device: net (n_gene, n_gene), a numpy array or a torch CUDA tensor of bool or uint8 (what binnet returns; any
	non-zero byte counts once; a pitch larger than the row is allowed).  int64, numpy or -- device_out=True -- a torch CUDA tensor."""
	from . import _lib
	if len(net.shape) != 2 or net.shape[0] != net.shape[1] or net.shape[0] < 1:
		raise ValueError('Wrong shape for net or namet.')
	ng = int(net.shape[0])
	eng = _engine.get_engine(net.device.index if _engine.is_dev(net) else None)
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			if _engine.is_dev(net):
				x = net
				if x.dtype not in (torch.bool, torch.uint8):
					raise TypeError('net must be bool or uint8.')
				if x.stride(1) != 1 or x.stride(0) < ng:
					x = x.contiguous()
			else:
				a = np.asarray(net)
				if a.dtype != np.bool_ and a.dtype != np.uint8:
					a = a != 0
				x = eng.upload(np.ascontiguousarray(a).view(np.uint8))
			deg = torch.empty((ng, ), dtype=torch.int64, device=eng.device)
			with _engine._Span(eng, 'net_degree'):
				_lib.check(eng.lib.nrm_net_degree(x.data_ptr(), ng, x.stride(0), deg.data_ptr(), eng._stream()))
			return deg if device_out else deg.cpu().numpy()


def principal_genes(net, n=100, device_out=False):
	"""The principal genes of a binary co-expression network, the selection of the reference's gotop (gocovt.py:249-265): the genes with the most co-expressed
	genes -- every gene whose degree reaches that of the gene ranked n.  Returns their int64 row indices in rising order, at least n and fewer than n_gene.
	net: (n_gene, n_gene) bool or uint8, a numpy array or a torch CUDA tensor as binnet(..., device_out=True) returns.  The degrees are taken on the device
	(nrm_net_degree), the selection over n_gene integers on the host.  device_out=True returns the indices as a torch CUDA tensor.
	ValueError for a net that is not square or has one gene, and for n <= 1 or n >= n_gene; RuntimeError when the gene ranked n has no co-expressed gene."""
	_check_principal_args(tuple(net.shape), n)
	sel = _select_principal(net_degree(net), n)
	if device_out:
		return _engine.get_engine(net.device.index if _engine.is_dev(net) else None).upload(sel)
	return sel


def _start_vector(m):
	"""The start of the power iteration for m genes: v0[g] = 1 + ((2654435761 g) mod 2^32) / 2^32, scaled to unit length.  Fixed and free of any seed; not
	constant, so a component whose loadings add up to zero is not orthogonal to it; positive, so neither is a common factor."""
	g = np.arange(m, dtype=np.uint64)
	v = 1.0 + ((g * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / 2.0**32
	return v / np.sqrt((v * v).sum())


def _gene_rows(nt, namet, genes):
	"""The row of every entry of genes: through the names (the last of equal names wins, gocovt.py:316), or, with namet None, the integers themselves."""
	if namet is None:
		idx = np.asarray(genes.cpu() if hasattr(genes, 'data_ptr') else genes)
		if idx.ndim != 1 or (idx.size and idx.dtype.kind not in 'iu'):
			raise ValueError('Without namet, genes must be a one-dimensional list of integer row indices.')
		idx = idx.astype(np.int64)
		if idx.size and (idx.min() < -nt or idx.max() >= nt):
			raise ValueError('Genes not found: {},...'.format(','.join(str(int(v)) for v in idx[(idx < -nt) | (idx >= nt)][:3])))
		return np.where(idx < 0, idx + nt, idx)
	if len(namet) != nt:
		raise ValueError('Incompatible input shapes.')
	where = dict(zip(namet, range(len(namet))))
	genes = list(genes)
	missing = [x for x in dict.fromkeys(genes) if x not in where]
	if missing:
		raise ValueError('Genes not found: {},...'.format(','.join(str(x) for x in missing[:3])))
	return np.array([where[x] for x in genes], dtype=np.int64)


def _check_pccovt_args(dt_shape, dc, namet, genes):
	"""The reference's checks (gocovt.py:296-304) and this build's, before anything touches the device: returns the int64 rows of the chosen genes."""
	if len(dt_shape) != 2 or dc.ndim != 2:
		raise ValueError('Incompatible input shapes.')
	nt, ns = (int(v) for v in dt_shape)
	if nt == 0 or ns == 0:
		raise ValueError('Empty normalized expression.')
	if dc.shape[1] != ns:
		raise ValueError('Incompatible input shapes.')
	idx = _gene_rows(nt, namet, genes)
	if idx.size == 0:
		raise ValueError('No gene to take the principal component of.')
	return idx


def _design(dc, ns, conditioned):
	"""The rows that are projected off, fp64, and the pseudo-inverse of their Gram matrix: [dc; 1] when conditioning (the reference's StandardScaler +
	LinearRegression(fit_intercept=True), gocovt.py:306-314, is the orthogonal projection off that span, whatever its rank), the constant row alone otherwise
	(pc1's centring, gocovt.py:20)."""
	from .norm import _pinv_gram_unit_rows
	one = np.ones((1, ns))
	c1 = np.concatenate([np.asarray(dc, dtype=np.float64), one], axis=0) if conditioned else one
	return np.ascontiguousarray(c1), _pinv_gram_unit_rows(c1)


def pccovt(dt, dc, namet, genes, condcov=True, device_out=False, max_iter=4096, return_info=False):
	"""An extra covariate from the top principal component of the chosen genes, same contract as reference gocovt.py:271-321: returns the (n_cov + 1, n_cell)
	covariate matrix, dc with the component's score over the cells as its last row.
	dt: (n_gene, n_cell) normalised expression, fp32 or fp64, a numpy array or a torch CUDA tensor already in HBM (normvar(..., device_out=True)); a pitch larger
	than the row is allowed.  dc: (n_cov, n_cell) numpy, n_cov = 0 allowed.  namet: the gene names of dt's rows and genes the names to use (a name repeated in
	genes repeats its row; of equal names in namet the last one is taken); with namet=None, genes holds integer row indices -- the resident form, no names needed.
	condcov: remove dc (and the intercept) from the rows first; without it, and with n_cov = 0, the rows are centred only.
	The chosen rows are residualised, scaled to mean square 1 (a row of exact zeros stays zero) and their top principal component over the cells is found by power
	iteration on their m x m correlation matrix: exact to rounding, the same bits on every run, where the reference's randomized SVD approximates it and varies
	from call to call.  Sign: the loading of largest magnitude is positive (the first of equals), sklearn's rule.  One gene (m = 1) gives its standardised row.
	max_iter bounds the power steps: RuntimeWarning ('top principal component not separated') when they end unconverged, which needs two top singular values
	equal to about 1 part in 1e3; the current iterate is returned.
	The result's dtype is np.result_type(dc.dtype, float64 if conditioned else dt's dtype), what the reference's concatenation yields; arithmetic is fp64.
	device_out=True returns a torch CUDA tensor.  return_info=True appends a dict: iterations, eigenvalue (sigma_1^2 / n_cell), residual, converged, top (the
	position in genes of the loading of largest magnitude) and sign.
	ValueError for an empty expression matrix, incompatible shapes, names that are not found ('Genes not found: a,b,c,...') and an empty genes."""
	from . import _lib
	dev = _engine.is_dev(dt)
	if not dev:
		dt = np.asarray(dt)
	dc = np.asarray(dc.cpu() if hasattr(dc, 'data_ptr') else dc)
	idx = _check_pccovt_args(tuple(dt.shape), dc, namet, genes)
	if int(max_iter) < 1:
		raise ValueError('max_iter must be positive.')
	nt, ns = (int(v) for v in dt.shape)
	nc, m = dc.shape[0], int(idx.size)
	conditioned = bool(condcov) and nc > 0
	fp32 = str(dt.dtype) in ('torch.float32', 'float32')
	score_np = np.dtype(np.float32 if fp32 and not conditioned else np.float64)  # (pc1 returns its input's type, gocovt.py:23; the residuals are fp64, :314)
	out_np = np.result_type(dc.dtype, score_np)
	c1, mi = _design(dc, ns, conditioned)
	eng = _engine.get_engine(dt.device.index if dev else None)
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			f64 = dict(dtype=torch.float64, device=eng.device)
			with _engine._Span(eng, 'pc_gather'):
				if dev:
					src = dt if dt.dtype in (torch.float32, torch.float64) else dt.to(torch.float64)
					d_idx = eng.upload(idx)
					if src.stride(1) != 1:  # (a transposed view: only the chosen rows are laid out again, not the matrix)
						x = src.index_select(0, d_idx).contiguous()
					else:
						x = torch.empty((m, ns), dtype=src.dtype, device=eng.device)
						_lib.check(eng.lib.nrm_subset_dense(src.data_ptr(), src.element_size(), nt, ns, src.stride(0), d_idx.data_ptr(), m, 0, ns, x.data_ptr(),
															x.stride(0), eng._stream()))
				else:
					x = eng.upload(_engine.as_input(dt[idx]))  # (only the chosen rows cross PCIe)
			d_c, d_mi = eng.upload(c1), eng.upload(np.ascontiguousarray(mi, dtype=np.float64))
			# K1 twice: the projection goes through the pseudo-inverse of the design's Gram matrix, which leaves about 1e-14 of the row's size along the covariates
			# (measured against longdouble: 2e-14 of max |score| at m = 1, three times the allowance 64 m u); a second pass over the m residual rows removes it
			res = eng.residualize(x, d_c, d_mi, c1.shape[0])
			for _ in range(1, _K1_PASSES):
				res = eng.residualize(res.data[:m, :ns], d_c, d_mi, c1.shape[0])
			dot = eng.gram(res, res, True)
			r = torch.empty((m, m), **f64)
			a = torch.empty((m, ), **f64)
			v = eng.upload(_start_vector(m))
			w = torch.empty((m, ), **f64)
			stat = torch.empty((3, ), **f64)
			stream = eng._stream()
			with _engine._Span(eng, 'pc_correlation'):
				_lib.check(eng.lib.nrm_pc_correlation(dot.data_ptr(), dot.stride(0), m, ns, res.ss.data_ptr(), r.data_ptr(), r.stride(0), a.data_ptr(), stream))
			done, lam, resid, converged = 0, 0.0, 0.0, False
			with _engine._Span(eng, 'pc_power'):
				while done < max_iter and not converged:
					step = min(_POWER_BLOCK, int(max_iter) - done)
					_lib.check(eng.lib.nrm_pc_power(r.data_ptr(), r.stride(0), m, v.data_ptr(), w.data_ptr(), stat.data_ptr(), step, stream))
					done += step
					lam, resid = (float(t) for t in stat.cpu().numpy()[:2])  # (the one read-back of a block of steps)
					converged = resid <= 16 * m * _UNIT * lam
					if not (np.isfinite(lam) and np.isfinite(resid)):
						break
			if not converged:
				warnings.warn('top principal component not separated after {} power iterations (residual {:.3g} of eigenvalue {:.3g}).'.format(done, resid, lam),
							  RuntimeWarning)
			score = torch.empty((ns, ), dtype=torch.float64 if score_np == np.float64 else torch.float32, device=eng.device)
			work = torch.empty((int(eng.lib.nrm_pc_score_workspace(m, ns)), ), **f64)
			sign = torch.empty((2, ), dtype=torch.int64, device=eng.device)
			with _engine._Span(eng, 'pc_score'):
				_lib.check(eng.lib.nrm_pc_score(res.data.data_ptr(), res.data.stride(0), m, ns, v.data_ptr(), a.data_ptr(), score.data_ptr(),
												_engine.dtype_code(score_np), work.data_ptr(), sign.data_ptr(), stream))
			info = None
			if return_info:
				top, sg = (int(t) for t in sign.cpu().numpy())
				info = dict(iterations=done, eigenvalue=lam, residual=resid, converged=bool(converged), top=top, sign=sg)
			if device_out:
				tdt = {'float32': torch.float32, 'float64': torch.float64}.get(str(out_np))
				if tdt is None:
					raise TypeError('no torch dtype for {}: use device_out=False.'.format(out_np))
				out = torch.empty((nc + 1, ns), dtype=tdt, device=eng.device)
				if nc:
					out[:nc] = eng.upload(np.ascontiguousarray(dc.astype(out_np, copy=False)))
				out[nc] = score.to(tdt)
			else:
				out = np.concatenate([dc, score.cpu().numpy().reshape(1, ns)], axis=0)
				assert out.dtype == out_np
	assert tuple(out.shape) == (nc + 1, ns)
	logging.debug('pccovt: {} genes, {} power iterations, eigenvalue {}.'.format(m, done, lam))
	return (out, info) if return_info else out


assert __name__ != "__main__"
