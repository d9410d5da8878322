"""Variance normalisation (mirror of the reference's norm.normvar / normvar1, norm.py:131-289) on the device.

normvar multiplies gene g by w**wt[g] and removes the covariates dc * w**wt[g] from it -- a different small OLS
per gene.  The reference loops over genes (one (n_cov, n_cov) SVD and two skinny matmuls each); here the per-gene
Gram matrices and moment vectors are rows of two Gram contractions on the fp64 matrix cores,
    M_g = sum_k e_gk^2 C_k C_k^T = (U P^T)_g        a_g = sum_k e_gk^2 y_gk C_k = (V C^T)_g ,
with U = e^2, V = e^2 y, P = the pairwise products of covariate rows; the pseudo-inverses (integer ranks) are a
batched SVD on the host, and two HBM-bound element-wise kernels (csrc/nrm_normvar.hip) do the rest.

normcov (norm.py:4-53) standardises the continuous covariate rows: a (covariates, cells) matrix, numpy on the host.
compute_var (norm.py:56-128) fits the per-cell weights normvar takes: the reference's two regressions are used for their fitted values only, so
each iteration is two orthogonal projections -- the gene rows onto the weighted covariates, in three streaming passes of csrc/nrm_fitvar.hip that
never store the residual, and the per-cell log-RMS onto span(covariates, 1), O(cells x covariates) on the host."""
import logging
import os

import numpy as np

from . import _lib, _opts
from . import engine as _engine
from ._lib import ROW_TILE, K_TILE
from .association import inv_rank
from .de import _finite_within  # (np.isfinite(a).all() from the array's minimum and maximum: one pass each, no temporary)



def normvar1(dt, dc, w2=None):
	"""Remove covariates from every row of dt (norm.py:131-163).  w2 (n_gene, n_cell): row g uses dc * w2[g]."""
	dt, dc = np.asarray(dt), np.asarray(dc)
	if w2 is not None:
		return _normvar1_weighted(dt, dc, np.asarray(w2))
	dc64 = np.asarray(dc, dtype=np.float64)
	mi, r = inv_rank(np.matmul(dc64, dc64.T))
	if r <= 0:
		raise RuntimeError('Zero-rank covariates found.')
	eng = _engine.get_engine()
	with eng.lock:  # one call at a time per device (engine scratch, streams and guard state are shared)
		d_c, d_mi = eng.covariates(dc64, mi)
		res = eng.residualize(_engine.as_input(dt), d_c, d_mi, r)
		out = eng.download(res.data[:dt.shape[0], :dt.shape[1]].contiguous())
		assert _finite_within(out)
		return out.astype(np.result_type(dt.dtype, dc.dtype, np.float32), copy=False)


def _normvar1_weighted(dt, dc, w2, tol=1E-8):
	"""normvar1 with w2 (norm.py:150-153): gene g against dc * w2[g].  The per-gene Gram matrices sum_k w2_gk^2 C_k C_k^T and moment
	vectors sum_k w2_gk y_gk C_k are rows of two contractions on the fp64 matrix cores, the pseudo-inverses (integer ranks) a batched
	SVD on the host as in normvar, the residuals one element-wise kernel (nrm_normvar_apply_w2)."""
	nt, ns = dt.shape
	nc = dc.shape[0]
	if w2.shape != (nt, ns):
		raise ValueError('w2 must have the shape of dt.')
	if nc == 0 or nc > 63:
		raise NotImplementedError('normvar1 on the device takes 1 to 63 covariates.')
	out_dtype = np.dtype(np.float32) if np.result_type(dt.dtype, dc.dtype, w2.dtype, np.float32) == np.float32 else np.dtype(np.float64)
	eng = _engine.get_engine()
	with eng.lock:  # one call at a time per device (engine scratch, streams and guard state are shared)
		torch = eng.torch
		iu = np.triu_indices(nc)
		npair = len(iu[0])
		with torch.cuda.device(eng.device):
			y = eng.upload(_engine.as_input(dt))
			d_w = eng.upload(np.asarray(w2, dtype=np.float64))
			d_c = eng.upload(np.asarray(dc, dtype=np.float64))
			rp, kp = _engine.round_up(nt, ROW_TILE), _engine.round_up(ns, K_TILE)
			u = torch.zeros((rp, kp), dtype=torch.float64, device=eng.device)
			v = torch.zeros((rp, kp), dtype=torch.float64, device=eng.device)
			u[:nt, :ns] = d_w * d_w
			v[:nt, :ns] = d_w * y.to(torch.float64)
			pr = torch.zeros((_engine.round_up(npair, ROW_TILE), kp), dtype=torch.float64, device=eng.device)
			pr[:npair, :ns] = d_c[torch.as_tensor(iu[0], device=eng.device)] * d_c[torch.as_tensor(iu[1], device=eng.device)]
			cp = torch.zeros((_engine.round_up(nc, ROW_TILE), kp), dtype=torch.float64, device=eng.device)
			cp[:nc, :ns] = d_c
			R = _engine.Residualized
			gm = eng.gram(R(nt, ns, u, None, None), R(npair, ns, pr, None, None), False)[:nt, :npair].cpu().numpy()
			ga = eng.gram(R(nt, ns, v, None, None), R(nc, ns, cp, None, None), False)[:nt, :nc].cpu().numpy()
			m = np.zeros((nt, nc, nc))
			m[:, iu[0], iu[1]] = gm
			m[:, iu[1], iu[0]] = gm
			from .association import small_pinv
			mi, rk = small_pinv(m, tol)  # per-gene pseudo-inverse by the rank rule of inv_rank (association.py:77), threaded in the library
			if (np.asarray(rk) <= 0).any():
				raise RuntimeError('Zero-rank covariates found.')
			b = np.einsum('gcd,gd->gc', mi, ga)  # b_g = M_g^+ a_g
			tdt = torch.float64 if out_dtype == np.float64 else torch.float32
			out = torch.empty((nt, ns), dtype=tdt, device=eng.device)
			d_b = eng.upload(b)
			_lib.check(eng.lib.nrm_normvar_apply_w2(y.data_ptr(), _engine.dtype_code(y), nt, ns, y.stride(0), d_w.data_ptr(),
													d_w.stride(0), d_c.data_ptr(), nc, d_c.stride(0), d_b.data_ptr(), out.data_ptr(),
													_engine.dtype_code(out_dtype), ns, eng._stream()))
			dtn = eng.download(out)
		assert _finite_within(dtn)
		return dtn



def _scaled_covariates(dc, w, cat):
	"""Continuous covariate rows (and, cat=1, the intercept; cat=2: every row) are scaled by w (norm.py:261-273)."""
	if cat == 2:
		return dc * w
	dcn = dc.copy()
	t0 = ((dc != 0) & (dc != 1)).any(axis=1)
	if cat == 1:
		t0 |= (dc == 1).all(axis=1)
	dcn = dcn.astype(np.result_type(dc.dtype, w.dtype), copy=False)
	dcn[t0] = dc[t0] * w
	return dcn


def _normvar_host_entry(dt, dc, w, wt, dextra, cat, keepvar, tol, out_dtype):
	"""normvar through nrm_normvar_host (include/normalisr_hip.h): host buffers in and out, no torch -- what `normalisr normvar` needs in a process that
	has numpy and the library only.  NotImplementedError beyond the entry's covariate count (the caller then takes the package's Gram-launch form)."""
	import ctypes
	lib = _lib.load()
	y = _engine.as_input(dt)
	nt, ns = y.shape
	nc = dc.shape[0]
	c64 = np.ascontiguousarray(dc, dtype=np.float64)
	lnw = np.log(np.asarray(w, dtype=np.float64))
	wt64 = np.ascontiguousarray(wt, dtype=np.float64)
	from .association import _result
	out = _result((nt, ns), out_dtype)  # (page-locked, recycled: 400 MB of fresh numpy memory per call cost more than the kernels)
	zero = ctypes.c_int64(0)
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	code = _engine.dtype_code
	_lib.check(lib.nrm_normvar_host(vp(y), code(y), nt, ns, vp(lnw), vp(wt64), vp(c64), nc, float(tol), 1 if keepvar else 0, vp(out), code(out), ctypes.byref(zero)))
	if zero.value:
		raise RuntimeError('Zero-rank covariates found.')
	dcn = _scaled_covariates(dc, w, cat)
	assert _finite_within(out) and _finite_within(dcn)
	ans = [out, dcn]
	if dextra is not None:
		dextran = dextra * w
		assert _finite_within(dextran)
		ans.append(dextran)
	return ans


WIDE_SAFETY = 4.0  # c of the rank certificate below: the margin for the rounding of the computed eigenvalues ("normvar with hundreds of covariates")


def wide_covariates():
	"""The largest covariate count of compute_var and normvar (nrm_wide_covariates(): the constant lives in the library)."""
	return int(_lib.load().nrm_wide_covariates())


def _check_wide(what, nc, ns):
	"""More than 63 covariates: more cells than covariates (with as many covariates as cells there is no residual to fit and the reference divides by zero) and
	at most nrm_wide_covariates() of them.  NotImplementedError before any device call."""
	if ns <= nc:
		raise NotImplementedError('{} on the device takes more than 63 covariates only with more cells than covariates ({} covariates, {} cells).'.format(what, nc, ns))
	lim = wide_covariates()
	if nc > lim:
		raise NotImplementedError('{} on the device takes 1 to {} covariates.'.format(what, lim))


def _wide_basis(dc, w, wt, tol=1E-8, safety=WIDE_SAFETY):
	"""(B, r, certified, gaps) for normvar with many covariates.  B (r, n_cell) = Lambda_r^-1/2 U_r^T dc from the eigen-decomposition of dc dc^T, r by the
	rule of inv_rank (eigenvalues >= tol x the largest): an orthonormal basis of the covariates' row space.  diag(e_g) is invertible (e_gk = w_k^wt_g > 0), so
	B diag(e_g) spans what dc diag(e_g) spans: one basis serves every gene, and M_g = B diag(e_g^2) B^T is positive definite with condition <= kappa.
	certified: every gene's matrix dc diag(e_g^2) dc^T has rank r under the reference's own rule (norm.py:154-159 through association.py:77).  By Ostrowski's
	theorem its eigenvalues lie in [e_min^2 lambda_i, e_max^2 lambda_i], so with kappa = (e_max / e_min)^2 over all genes and cells (e = 1 where wt_g = 0) and
	the margin c = safety for the rounding of the computed lambda, it is enough that
	    lambda_r / lambda_1 >= c tol kappa      and      lambda_{r+1} / lambda_1 < tol / (c kappa).
	False means "no certificate" (nearly collinear covariates, extreme weights), never "rank deficient"; gaps = (lambda_r / lambda_1, lambda_{r+1} / lambda_1, kappa)."""
	c64 = np.asarray(dc, dtype=np.float64)
	nc = c64.shape[0]
	lam, u = np.linalg.eigh(np.matmul(c64, c64.T))
	lam, u = lam[::-1], u[:, ::-1]
	assert np.isfinite(lam).all() and lam[0] > 0  # (the reference: 0 / 0 in inv_rank for covariates that are all zero, infs or NaNs refused)
	r = int((lam >= tol * lam[0]).sum())
	w, wt = np.asarray(w, dtype=np.float64), np.asarray(wt, dtype=np.float64)
	lw = np.log(np.array([w.min(), w.max()]))
	ex = wt[wt != 0]
	le = np.outer(np.array([ex.min(), ex.max()]), lw).ravel() if ex.size else np.zeros(1)
	if (wt == 0).any():
		le = np.append(le, 0.0)
	with np.errstate(over='ignore'):
		kappa = float(np.exp(2 * (le.max() - le.min())))
	hi = float(lam[r - 1] / lam[0])
	lo = float(max(lam[r], 0.0) / lam[0]) if r < nc else 0.0
	certified = bool(np.isfinite(kappa) and hi >= safety * tol * kappa and (r == nc or lo < tol / (safety * kappa)))
	b = (u[:, :r] / np.sqrt(lam[:r])).T @ c64
	return b, r, certified, (hi, lo, kappa)


def _fitvar_bases(dc, tol=1E-8):
	"""(B, r, hi, lo, B1) for ComputeVarPlan with many covariates.  B (r, n_cell) as in _wide_basis, from the eigen-decomposition of dc dc^T with r by the rule of
	inv_rank on that matrix -- the rank inv_rank(cu cu^T) gives at u = 1 -- and hi = lambda_r / lambda_1, lo = lambda_{r+1} / lambda_1 (0 for r = n_cov): what the
	rank certificate of _wide_basis needs beside kappa = (u_max / u_min)^2, which only the device knows (nrm_fitvar_wide_design evaluates it per iteration).
	B1 (r1, n_cell): an orthonormal basis of the directions of [dc; 1] that _pinv_gram_unit_rows keeps (the Gram matrix of the rows scaled to unit length, the rule
	of inv_rank on it), so that B1^T B1 is the projector of the second regression, c1^T _pinv_gram_unit_rows(c1) c1."""
	c64 = np.asarray(dc, dtype=np.float64)
	nc, ns = c64.shape
	lam, u = np.linalg.eigh(np.matmul(c64, c64.T))
	lam, u = lam[::-1], u[:, ::-1]
	assert np.isfinite(lam).all() and lam[0] > 0  # (the reference: 0 / 0 in inv_rank for covariates that are all zero, infs or NaNs refused)
	r = int((lam >= tol * lam[0]).sum())
	hi = float(lam[r - 1] / lam[0])
	lo = float(max(lam[r], 0.0) / lam[0]) if r < nc else 0.0
	b = (u[:, :r] / np.sqrt(lam[:r])).T @ c64
	c1 = np.concatenate([c64, np.ones((1, ns))], axis=0)
	d = np.sqrt(np.einsum('ij,ij->i', c1, c1))
	xs = c1 * (1 / np.where(d > 0, d, 1.0))[:, None]
	lam1, u1 = np.linalg.eigh(np.matmul(xs, xs.T))
	lam1, u1 = lam1[::-1], u1[:, ::-1]
	r1 = int((lam1 >= tol * lam1[0]).sum())
	b1 = (u1[:, :r1] / np.sqrt(lam1[:r1])).T @ xs
	return b, r, hi, lo, b1


def _fitvar_certified(hi, lo, full, kappa, tol=1E-8, safety=WIDE_SAFETY):
	"""The rank certificate of _wide_basis for weights of spread kappa = (u_max / u_min)^2 (nrm_fitvar_wide_design holds the same expression)."""
	return bool(hi >= safety * tol * kappa and (full or lo < tol / (safety * kappa)))


def _normvar_wide_reference(dt, dc, w, wt, keepvar, tol=1E-8):
	"""The reference's per-gene algorithm (norm.py:150-163,244-259) in host numpy with inv_rank: one (nc, nc) pseudo-inverse per gene.  What normvar does for
	covariates without the certificate of _wide_basis -- slow, and the reference's answer."""
	dt, c64 = np.asarray(dt, dtype=np.float64), np.asarray(dc, dtype=np.float64)
	w, wt = np.asarray(w, dtype=np.float64), np.asarray(wt, dtype=np.float64)
	out = np.empty_like(dt)
	for g in range(dt.shape[0]):
		e = w**wt[g] if wt[g] != 0 else np.ones_like(w)
		y, c = dt[g] * e, c64 * e
		mi, r = inv_rank(np.matmul(c, c.T), tol)
		if r <= 0:
			raise RuntimeError('Zero-rank covariates found.')
		res = y - np.matmul(np.matmul(mi, np.matmul(c, y)), c)
		if keepvar:
			with np.errstate(divide='ignore', invalid='ignore'):
				res = res * (np.sqrt(((y - y.mean())**2).mean()) / np.sqrt((res**2).mean()))**wt[g]
		out[g] = res
	return out


def _wide_blocks(nt, ns, r):
	"""(genes per block, pair rows per panel) of the wide normvar path from a byte budget: a gene holds its packed M_g (r (r + 1) / 2 doubles) and its rows of U and
	V; a panel row is one row of P.  NRM_DEBUG nv_gene_block / nv_panel_rows set them (tests: several blocks and panels at small sizes)."""
	npair = r * (r + 1) // 2
	kp = _engine.round_up(ns, K_TILE)
	per_gene = 8 * (_engine.round_up(npair, ROW_TILE) + ROW_TILE + 2 * kp + _engine.round_up(r, ROW_TILE))
	gb = max(ROW_TILE, (3 << 29) // per_gene // ROW_TILE * ROW_TILE)  # 1.5 GiB
	pr = max(ROW_TILE, (1 << 28) // (8 * kp) // ROW_TILE * ROW_TILE)  # 256 MiB
	gb = int(_opts.debug('nv_gene_block', gb))
	pr = int(_opts.debug('nv_panel_rows', pr))
	if gb <= 0 or pr <= 0:
		raise ValueError('nv_gene_block and nv_panel_rows must be positive.')
	return min(gb, nt), min(pr, npair)


def _normvar_wide(eng, y, ycode, nt, ns, d_lnw, d_wt, basis, r, keepvar, out, ocode):
	"""normvar's result for many covariates, on the device (csrc/nrm_normvar_wide.hip): per block of genes, U = e^2 and V = e^2 y (nrm_normvar_weights), the
	packed M_g as rows of U P^T with P built a panel at a time (nrm_normvar_pairs) and a_g = V B^T, both on the fp64 matrix cores with whole tiles (the same bits
	for every block and panel size), a Cholesky solve per gene (nrm_normvar_chol); then one result pass with B as the covariates (nrm_normvar_apply).
	Returns the counters of nrm_normvar_chol (int32[4] on the device)."""
	torch, lib = eng.torch, eng.lib
	npair = r * (r + 1) // 2
	kp = _engine.round_up(ns, K_TILE)
	gb, pr = _wide_blocks(nt, ns, r)
	gbp, prp, rp = _engine.round_up(gb, ROW_TILE), _engine.round_up(pr, ROW_TILE), _engine.round_up(r, ROW_TILE)
	ldm = _engine.round_up(npair, ROW_TILE) + ROW_TILE  # (a panel's launch writes whole 16-column groups: up to 15 columns past its last pair, zeros, before the next panel's)
	f64 = dict(dtype=torch.float64, device=eng.device)
	st = eng._stream()
	bp = torch.zeros((rp, kp), **f64)
	bp[:r, :ns] = eng.upload(np.ascontiguousarray(basis))
	u, v = torch.empty((gbp, kp), **f64), torch.empty((gbp, kp), **f64)
	s1, s2 = torch.empty((gbp, ), **f64), torch.empty((gbp, ), **f64)
	pan = torch.empty((prp, kp), **f64)
	m, a = torch.empty((gbp, ldm), **f64), torch.empty((gbp, rp), **f64)
	d_b, d_scale = torch.empty((nt, r), **f64), torch.empty((nt, ), **f64)
	status = torch.empty((nt, ), dtype=torch.int32, device=eng.device)
	cflags = eng.zeros((4, ), torch.int32)
	ysize = y.element_size()
	with _engine._Span(eng, 'normvar_wide'):
		for g0 in range(0, nt, gb):
			g = min(gb, nt - g0)
			_lib.check(lib.nrm_normvar_weights(y.data_ptr() + g0 * y.stride(0) * ysize, ycode, g, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr() + 8 * g0, u.data_ptr(),
											   v.data_ptr(), kp, gbp, s1.data_ptr(), s2.data_ptr(), st))
			for p0 in range(0, npair, pr):
				cnt = min(pr, npair - p0)
				cp = _engine.round_up(cnt, ROW_TILE)
				_lib.check(lib.nrm_normvar_pairs(bp.data_ptr(), r, ns, kp, p0, cnt, pan.data_ptr(), cp, kp, st))
				_lib.check(lib.nrm_gram_f64_whole(u.data_ptr(), pan.data_ptr(), gbp, cp, kp, kp, kp, m.data_ptr() + 8 * p0, ldm, g, cnt, st))
			_lib.check(lib.nrm_gram_f64_whole(v.data_ptr(), bp.data_ptr(), gbp, rp, kp, kp, kp, a.data_ptr(), rp, g, r, st))
			_lib.check(lib.nrm_normvar_chol(m.data_ptr(), ldm, a.data_ptr(), rp, g, r, s1.data_ptr(), s2.data_ptr(), d_wt.data_ptr() + 8 * g0, ns, 1 if keepvar else 0,
											d_b.data_ptr() + 8 * g0 * r, d_scale.data_ptr() + 8 * g0, status.data_ptr() + 4 * g0, cflags.data_ptr(), st))
		_lib.check(lib.nrm_normvar_apply(y.data_ptr(), ycode, nt, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr(), bp.data_ptr(), r, kp, d_b.data_ptr(), d_scale.data_ptr(),
										 out.data_ptr(), ocode, ns, cflags.data_ptr(), st))
	eng._normvar_wide_last = dict(rank=r, gene_block=gb, panel_rows=pr, status=status)  # (tests)
	return cflags


NV_TAU, NV_MARK = 2.0**-20, -1.0  # NRM_NV_TAU, NRM_NV_MARK of csrc/nrm_nv_scale.h: when the one-pass variance sums count as cancelled, and what then stands for the scale


def _rescale(eng, y, ycode, nt, ns, d_lnw, d_wt, d_c, nc, d_b, d_scale):
	"""Between the solve and the result pass, on every route: the scale of the genes marked NV_MARK from the row itself (nrm_normvar_rescale; nothing read back)."""
	_lib.check(eng.lib.nrm_normvar_rescale(y.data_ptr(), ycode, nt, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr(), d_c.data_ptr(), nc, d_c.stride(0), d_b.data_ptr(),
										   d_scale.data_ptr(), eng._stream()))


def normvar(dt, dc, w, wt, dextra=None, cat=1, nth=1, bs=500, keepvar=True, normmean=False, tol=1E-8, device_out=False):
	"""Mean and variance normalisation, same contract as reference norm.py:166-289: returns [dtn, dcn] (+ [dextran]).
	nth and bs are accepted for compatibility and ignored.
	dt may be a torch CUDA tensor already in HBM; device_out=True leaves dtn there (a torch tensor) -- what coex / de / binnet take next
	(examples/GSE123139/code/cmd_coex.sh:38-46 chains the three through files): nothing of the expression matrix crosses PCIe.  With up to 8
	covariates the whole computation stays on the device (csrc/nrm_normvar.hip: per-gene moments in one pass, pseudo-inverses by a thread per
	gene with the host's Jacobi code, one more pass writes the result); 9 to 63 covariates take the Gram-launch form with the host's batched
	pseudo-inverses; 64 to nrm_wide_covariates() (1024), with more cells than covariates, the basis form of csrc/nrm_normvar_wide.hip: one orthonormal
	basis of the covariates' row space for every gene and a Cholesky solve per gene on the device, when _wide_basis certifies that every gene's reference
	rank is the basis rank -- otherwise (nearly collinear covariates, extreme weights) the reference's per-gene algorithm on the host, under a warning."""
	if not _engine.is_dev(dt):
		dt = np.asarray(dt)
	dc, w, wt = np.asarray(dc), np.asarray(w), np.asarray(wt)
	if any(x.ndim != 2 for x in (dt, dc)):
		raise ValueError('dt and dc should have 2 dimensions.')
	if any(x.ndim != 1 for x in (w, wt)):
		raise ValueError('w and wt should have 1 dimension.')
	nt, ns = dt.shape
	nc = dc.shape[0]
	if nc == 0:
		raise ValueError('No covariates.')
	if dc.shape[1] != ns or w.shape[0] != ns or wt.shape[0] != nt:
		raise ValueError('Unmatched gene or cell counts.')
	if dextra is not None:
		dextra = np.asarray(dextra)
		if dextra.ndim != 2 or dextra.shape[0] == 0 or dextra.shape[1] != ns:
			raise ValueError('Unmatched shape or size for dextra.')
	if w.min() <= 0:
		raise ValueError('w must be positive.')
	if wt.min() < 0:
		raise ValueError('wt must be non-negative.')
	if cat not in (0, 1, 2):
		raise ValueError('Invalid cat value.')
	wide = nc > 63
	if wide:
		_check_wide('normvar', nc, ns)
	dt_dtype = np.dtype(str(dt.dtype).replace('torch.', '')) if _engine.is_dev(dt) else dt.dtype
	out_dtype = np.result_type(dt_dtype, dc.dtype, w.dtype, wt.dtype, np.float32)
	out_dtype = np.dtype(np.float32) if out_dtype == np.float32 else np.dtype(np.float64)
	from .association import _use_host_entry
	if not wide and not _engine.is_dev(dt) and not device_out and not normmean and _use_host_entry():
		# no torch in this process (or the command line / NRM_HOST_ENTRY=1): the library's whole-problem entry, numpy buffers in and out
		try:
			return _normvar_host_entry(dt, dc, w, wt, dextra, cat, keepvar, tol, out_dtype)
		except NotImplementedError:
			from .association import _have_torch
			if not _have_torch():
				raise
	basis = None
	if wide:
		basis, rank, certified, gaps = _wide_basis(dc, w, wt, tol)
		if not certified:
			logging.warning('normvar: {} covariates of rank {} without a rank certificate for every gene (lambda_r / lambda_1 = {:.3g}, lambda_r+1 / lambda_1 = {:.3g}, '
							'weight spread kappa = {:.3g}): taking the reference\'s per-gene pseudo-inverses on the host.  Expect a slow call.'.format(nc, rank, *gaps))
	eng = _engine.get_engine()
	with eng.lock:  # one call at a time per device (engine scratch, streams and guard state are shared)
		torch = eng.torch
		c64 = np.asarray(dc, dtype=np.float64)
		npair = nc * (nc + 1) // 2
		iu = np.triu_indices(nc) if not wide else None
		with torch.cuda.device(eng.device):
			y = dt if _engine.is_dev(dt) else eng.upload(_engine.as_input(dt))
			if y.dtype not in (torch.float32, torch.float64):
				y = y.to(torch.float64)
			if y.stride(1) != 1:
				y = y.contiguous()
			ycode = _engine.dtype_code(y)
			d_lnw = eng.upload(np.log(np.asarray(w, dtype=np.float64)))
			d_wt = eng.upload(np.asarray(wt, dtype=np.float64))
			d_c = eng.upload(c64)
			tdt = torch.float64 if out_dtype == np.float64 else torch.float32
			flags = eng.zeros((4, ), torch.int32)
			on_device = nc <= int(eng.lib.nrm_normvar_device_covariates()) and _opts.debug('normvar', 'device') != 'host'
			if wide:
				out = torch.empty((nt, ns), dtype=tdt, device=eng.device)
				if certified:
					wflags = _normvar_wide(eng, y, ycode, nt, ns, d_lnw, d_wt, basis, rank, keepvar, out, _engine.dtype_code(out_dtype))
					wf = wflags.cpu().numpy()
					assert not wf[0] and not wf[1]  # a pivot that is not positive or a value that is not finite (csrc/nrm_normvar_wide.hip): np.isfinite(dtn).all() (norm.py:286)
				else:
					ref = _normvar_wide_reference(y.cpu().numpy(), c64, w, wt, keepvar, tol)
					assert _finite_within(ref)
					out.copy_(eng.upload(ref))
			elif on_device:
				# everything on the device: one pass sums the per-gene moments, a thread per gene solves its small OLS, one pass writes the result
				mom = torch.empty((nt, npair + nc + 2), dtype=torch.float64, device=eng.device)
				d_b = torch.empty((nt, nc), dtype=torch.float64, device=eng.device)
				d_scale = torch.empty((nt, ), dtype=torch.float64, device=eng.device)
				d_rank = torch.empty((nt, ), dtype=torch.int64, device=eng.device)
				with _engine._Span(eng, 'normvar_solve'):
					_lib.check(eng.lib.nrm_normvar_solve(y.data_ptr(), ycode, nt, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr(), d_c.data_ptr(), nc, d_c.stride(0), float(tol),
														 1 if keepvar else 0, mom.data_ptr(), d_b.data_ptr(), d_scale.data_ptr(), d_rank.data_ptr(), flags.data_ptr(), eng._stream()))
					_rescale(eng, y, ycode, nt, ns, d_lnw, d_wt, d_c, nc, d_b, d_scale)
				out = torch.empty((nt, ns), dtype=tdt, device=eng.device)
				with _engine._Span(eng, 'normvar_apply'):
					_lib.check(eng.lib.nrm_normvar_apply(y.data_ptr(), ycode, nt, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr(), d_c.data_ptr(), nc, d_c.stride(0),
														 d_b.data_ptr(), d_scale.data_ptr(), out.data_ptr(), _engine.dtype_code(out_dtype), ns,
														 flags.data_ptr(), eng._stream()))
				eng._normvar_ranks = d_rank  # (tests: the integer ranks of the last call)
			if not on_device and not wide:
				rp, kp = _engine.round_up(nt, ROW_TILE), _engine.round_up(ns, K_TILE)
				u = torch.empty((rp, kp), dtype=torch.float64, device=eng.device)
				v = torch.empty((rp, kp), dtype=torch.float64, device=eng.device)
				s1 = torch.empty((rp, ), dtype=torch.float64, device=eng.device)
				s2 = torch.empty((rp, ), dtype=torch.float64, device=eng.device)
				_lib.check(eng.lib.nrm_normvar_weights(y.data_ptr(), ycode, nt, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr(), u.data_ptr(),
													   v.data_ptr(), kp, rp, s1.data_ptr(), s2.data_ptr(), eng._stream()))
				# operands of the two Gram contractions: P = pairwise products of covariate rows, C itself
				pr = torch.zeros((_engine.round_up(npair, ROW_TILE), kp), dtype=torch.float64, device=eng.device)
				pr[:npair, :ns] = d_c[torch.as_tensor(iu[0], device=eng.device)] * d_c[torch.as_tensor(iu[1], device=eng.device)]
				cp = torch.zeros((_engine.round_up(nc, ROW_TILE), kp), dtype=torch.float64, device=eng.device)
				cp[:nc, :ns] = d_c
				R = _engine.Residualized
				gm = eng.gram(R(nt, ns, u, None, None), R(npair, ns, pr, None, None), False)[:nt, :npair].cpu().numpy()
				ga = eng.gram(R(nt, ns, v, None, None), R(nc, ns, cp, None, None), False)[:nt, :nc].cpu().numpy()
				# per-gene pseudo-inverse on the host: batched SVD, rank rule of inv_rank (association.py:77)
				m = np.zeros((nt, nc, nc))
				m[:, iu[0], iu[1]] = gm
				m[:, iu[1], iu[0]] = gm
				from .association import small_pinv
				mi, rk = small_pinv(m, tol)  # per-gene pseudo-inverse by the rank rule of inv_rank (association.py:77), threaded in the library
				if (np.asarray(rk) <= 0).any():
					raise RuntimeError('Zero-rank covariates found.')
				b = np.einsum('gcd,gd->gc', mi, ga)  # b_g = M_g^+ a_g
				scale = np.ones(nt)
				if keepvar:
					mean = s1[:nt].cpu().numpy() / ns
					h2 = s2[:nt].cpu().numpy()
					d1, d2 = h2 / ns - mean * mean, h2 - np.einsum('gc,gc->g', ga, b)
					dv = np.sqrt(np.maximum(d1, 0.0))  # norm.py:248-249
					dv2 = np.sqrt(np.maximum(d2, 0.0) / ns)  # |y' - P y'|^2 = |y'|^2 - a.b
					wt64 = np.asarray(wt, dtype=np.float64)
					with np.errstate(divide='ignore', invalid='ignore'):
						scale = (dv / dv2)**wt64  # norm.py:259
					# the rule of csrc/nrm_nv_scale.h: a difference that has cancelled marks its gene, nrm_normvar_rescale takes that scale from the row itself
					scale[(wt64 != 0) & ((d1 < NV_TAU * (h2 / ns)) | (d2 < NV_TAU * h2))] = NV_MARK
				out = torch.empty((nt, ns), dtype=tdt, device=eng.device)
				d_b, d_scale = eng.upload(b), eng.upload(scale)
				_rescale(eng, y, ycode, nt, ns, d_lnw, d_wt, d_c, nc, d_b, d_scale)
				_lib.check(eng.lib.nrm_normvar_apply(y.data_ptr(), ycode, nt, ns, y.stride(0), d_lnw.data_ptr(), d_wt.data_ptr(), d_c.data_ptr(), nc,
													 d_c.stride(0), d_b.data_ptr(), d_scale.data_ptr(), out.data_ptr(),
													 _engine.dtype_code(out_dtype), ns, flags.data_ptr(), eng._stream()))
			# covariates: continuous rows (and the intercept for cat=1) are scaled by w (norm.py:261-273)
			dcn = _scaled_covariates(dc, w, cat)
			if normmean:
				dcn64 = np.asarray(dcn, dtype=np.float64)
				mi, r = inv_rank(np.matmul(dcn64, dcn64.T))
				if r <= 0:
					raise RuntimeError('Zero-rank covariates found.')
				cov = eng.covariates(dcn64, mi)
				res = eng.residualize(out, cov[0], cov[1], r)
				out = res.data[:nt, :ns].to(tdt).contiguous()
			f = flags.cpu().numpy()
			if f[0]:
				raise RuntimeError('Zero-rank covariates found.')
			assert not f[1]  # np.isfinite(dtn).all() (norm.py:286): counted by the kernel that wrote the values
			dtn = out if device_out else eng.download(out)
		assert (device_out or _finite_within(dtn)) and _finite_within(dcn)
		ans = [dtn, dcn]
		if dextra is not None:
			dextran = dextra * w
			assert _finite_within(dextran)
			ans.append(dextran)
		return ans


def normcov(dc, c=True):
	"""Standardise every continuous covariate to zero mean and unit variance and (c=True) append the constant-1 row, same contract as reference norm.py:4-53.
	Rows holding only 0 and 1 (one-hot categories) are left as they are.  Host numpy: the matrix is (n_cov, n_cell)."""
	import warnings
	assert dc is not None
	dc = dc.cpu().numpy() if _engine.is_dev(dc) else np.asarray(dc)
	if dc.ndim != 2:
		raise ValueError('Covariates must have 2 dimensions.')
	ns = dc.shape[1]
	if dc.shape[0] == 0:
		return np.ones((1, ns)) if c else dc
	if ns == 0 or (dc == dc[:, :1]).all(axis=1).any():
		raise ValueError('Detected constant covariate. Please only provide full-rank covariate without constant covariate.')
	cont = ((dc != 0) & (dc != 1)).any(axis=1)
	out = dc.copy()
	if cont.any():
		mean = dc[cont].mean(axis=1)
		dev = dc[cont].T - mean
		sd = np.sqrt((dev**2).mean(axis=0))
		with np.errstate(divide='ignore', invalid='ignore'):
			near = sd.min() < 1E-50 or np.abs(sd / mean).min() < 1E-6
		if near:
			warnings.warn('Detected near constant covariate. Results may be error-prone.', RuntimeWarning)
		out[cont] = (dev / sd).T
	if c:
		out = np.concatenate([out, np.ones((1, ns))], axis=0)
	return out


def _pinv_gram_unit_rows(x):
	"""(x x^T)^+ for x (rows, cells) by inv_rank on the Gram matrix of the rows scaled to unit length, D inv_rank(D x x^T D) D with D = diag(1 / |row|): the rank
	rule, relative to the largest eigenvalue, then does not depend on the units of the rows.  The reference fits with a least-squares solver on the design
	matrix, centred, beside a separate intercept (norm.py:92,109), so covariates in units of 1e-6 or 1e6 beside the constant-1 row lose nothing there; on the
	Gram matrix as it stands their eigenvalues fall below 1e-8 of the intercept's (or the intercept's below theirs) and the fit drops them."""
	d = np.sqrt(np.einsum('ij,ij->i', x, x))
	d = 1 / np.where(d > 0, d, 1.0)
	xs = x * d[:, None]
	mi, r = inv_rank(np.matmul(xs, xs.T))
	return mi * d[:, None] * d[None, :]


def _projector(x):
	"""x^T (x x^T)^+ x for x (rows, cells): the fitted values of a least-squares regression on the rows of x, whatever their rank and their units."""
	mi = _pinv_gram_unit_rows(x)
	return lambda z: np.matmul(np.matmul(mi, np.matmul(x, z)), x)


def _compute_var_host_entry(dt, c64, stepmax, eps):
	"""compute_var through nrm_compute_var_host (include/normalisr_hip.h): host buffers in and out, no torch, the pseudo-inverse of [dc;1][dc;1]^T from the
	library's Jacobi routine -- what `normalisr fitvar` needs in a process that has numpy and the library only.  Returns (weights, best change, steps taken).
	NotImplementedError beyond 63 covariates (a pseudo-inverse larger than that routine takes; the caller then takes the torch engine if there is one);
	AssertionError for what compute_var asserts (norm.py:125-127)."""
	import ctypes
	lib = _lib.load()
	y = _engine.as_input(dt)
	nt, ns = y.shape
	nc = c64.shape[0]
	if nc > 63:
		raise NotImplementedError('compute_var without torch takes 1 to 63 covariates ({} given): the pseudo-inverse of [dc;1][dc;1]^T comes from the library\'s Jacobi '
								  'routine of at most 64 rows.'.format(nc))
	w, state = np.empty(ns, dtype=np.float64), np.zeros(2, dtype=np.float64)
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	_lib.check(lib.nrm_compute_var_host(vp(y), _engine.dtype_code(y), nt, ns, vp(c64), nc, int(stepmax), float(eps), vp(w), vp(state)))
	logging.debug('Step {}, best maximum relative difference: {}'.format(int(state[1]), state[0]))
	return w, float(state[0]), int(state[1])


def compute_var(dt, dc, stepmax=1, eps=1E-6):
	"""Variance-normalisation multiplier of every cell, same contract as reference norm.py:56-128 (`normalisr fitvar`): returns (n_cell,) weights >= 1.
	dt: (n_gene, n_cell) logCPM, fp32 or fp64, a numpy array or a torch CUDA tensor already in HBM (lcpm(..., device_out=True)); dc (n_cov, n_cell), 1 to 63
	rows, or up to nrm_wide_covariates() (1024) with more cells than covariates (csrc/nrm_fitvar.hip: the coefficient table in dynamic LDS), rank-deficient sets included (both projections take the pseudo-inverse of inv_rank).  AssertionError for a gene whose residual is constant (the
	reference divides by its zero spread, norm.py:108, and fails norm.py:125).
	Host input in a process without torch (or with NRM_HOST_ENTRY=1, or from the command line) goes through the library's whole-problem entry
	nrm_compute_var_host, 1 to 63 covariates: numpy and the library suffice; beyond 63 it needs the torch engine."""
	if eps <= 0 or stepmax <= 0:
		raise ValueError('eps and stepmax must be positive.')
	if not _engine.is_dev(dt):
		dt = np.asarray(dt)
	dc = dc.cpu().numpy() if _engine.is_dev(dc) else np.asarray(dc)
	if dt.ndim != 2 or dc.ndim != 2:
		raise ValueError('dt and dc must both have 2 dimensions.')
	if dt.shape[1] != dc.shape[1]:
		raise ValueError('dt and dc must have the same cell count.')
	nt, ns = dt.shape
	nc = dc.shape[0]
	if nc == 0:
		raise NotImplementedError('compute_var on the device takes at least one covariate.')
	if nc > 63:
		_check_wide('compute_var', nc, ns)
	if nt == 0 or ns == 0:
		raise ValueError('dt must not be empty.')
	c64 = np.ascontiguousarray(dc, dtype=np.float64)
	if not _engine.is_dev(dt):
		from .association import _use_host_entry
		if _use_host_entry():
			# no torch in this process (or the command line / NRM_HOST_ENTRY=1): the library's whole-problem entry, numpy buffers in and out
			try:
				return _compute_var_host_entry(dt, c64, stepmax, eps)[0]
			except NotImplementedError:
				from .association import _have_torch
				if not _have_torch():
					raise
	fit_log = _projector(np.concatenate([c64, np.ones((1, ns))], axis=0))  # the second regression has an intercept (norm.py:92,109-110)
	eng = _engine.get_engine(dt.device.index if _engine.is_dev(dt) else None)
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			y = dt if _engine.is_dev(dt) else eng.upload(_engine.as_input(dt))
			if y.dtype not in (torch.float32, torch.float64):
				y = y.to(torch.float64)
			if y.stride(1) != 1:
				y = y.contiguous()
			ycode = _engine.dtype_code(y)
			d_c = eng.upload(c64)
			f64 = dict(dtype=torch.float64, device=eng.device)
			d_a, d_b = torch.empty((nt, nc), **f64), torch.empty((nt, nc), **f64)
			d_mean, d_sc, d_v = torch.empty((nt, ), **f64), torch.empty((nt, ), **f64), torch.empty((ns, ), **f64)
			part = torch.empty((-(-nt // int(eng.lib.nrm_fitvar_row_tile())), ns), **f64)
			flags = eng.zeros((4, ), torch.int32)
			scale = np.ones(ns)
			best, bestv, n = None, 1E300, 0
			while n < stepmax and bestv > eps:
				u = 1 / scale
				cu = c64 * u
				mi, r = inv_rank(np.matmul(cu, cu.T))
				d_u, d_cw, d_mi = eng.upload(u), eng.upload(cu * u), eng.upload(np.ascontiguousarray(mi, dtype=np.float64))
				with _engine._Span(eng, 'fitvar'):
					_lib.check(eng.lib.nrm_fitvar_moments(y.data_ptr(), ycode, nt, ns, y.stride(0), d_cw.data_ptr(), nc, d_cw.stride(0), d_a.data_ptr(), eng._stream()))
					_lib.check(eng.lib.nrm_fitvar_genes(y.data_ptr(), ycode, nt, ns, y.stride(0), d_u.data_ptr(), d_c.data_ptr(), nc, d_c.stride(0), d_a.data_ptr(),
														d_mi.data_ptr(), d_b.data_ptr(), d_mean.data_ptr(), d_sc.data_ptr(), flags.data_ptr(), eng._stream()))
					_lib.check(eng.lib.nrm_fitvar_cells(y.data_ptr(), ycode, nt, ns, y.stride(0), d_u.data_ptr(), d_c.data_ptr(), nc, d_c.stride(0), d_b.data_ptr(),
														d_mean.data_ptr(), d_sc.data_ptr(), part.data_ptr(), d_v.data_ptr(), eng._stream()))
				v = d_v.cpu().numpy()
				assert not flags.cpu().numpy()[0]  # a gene whose residual is constant: its spread divides (norm.py:108), the result is not finite (norm.py:125)
				with np.errstate(divide='ignore', invalid='ignore'):
					new = np.exp(fit_log(np.log(np.sqrt(v)))) * scale
					new /= new.min()
					t1 = np.abs((new - scale) / scale).max()
				scale = new
				n += 1
				if t1 < bestv:
					bestv, best = t1, scale
				logging.debug('Step {}, maximum relative difference: {}'.format(n, t1))
	assert best is not None
	w = 1 / best.astype(float, copy=False)
	w /= w.min()
	assert w.shape == (ns, )
	assert np.isfinite(w).all()
	assert (w > 0).all()
	return w



class NormvarPlan:
	"""normvar on an expression matrix RESIDENT in HBM, step after step (the matrix rewritten in place between steps: the pipeline normvar -> coex -> binnet of
	examples/GSE123139/code/cmd_coex.sh:38-46 over batches of one shape).  What a call of normvar does on the host for such a step -- log w, three uploads, five
	allocations, the scaled covariates, the flags read back -- is done ONCE here; a step is the three kernels of csrc/nrm_normvar.hip (moments, a lane per gene
	for its small system, the result pass) on the same buffers, one HIP graph from the second step on.  Same results as normvar(dt, ..., device_out=True), bit for bit
	(the same kernels on the same inputs).  check() reads the counters of the last step and raises what normvar raises (norm.py:160,286).
	Up to nrm_normvar_device_covariates() covariates and normmean=False; otherwise every step is the public call."""

	def __init__(self, dt, dc, w, wt, cat=1, keepvar=True, tol=1E-8, eng=None):
		from .distributed import StepGraph
		if not _engine.is_dev(dt):
			raise ValueError('NormvarPlan takes an expression matrix resident in HBM (a torch CUDA tensor); normvar() is the call for host arrays.')
		self.eng = eng = eng or _engine.get_engine(dt.device.index)
		torch = eng.torch
		self.dt, self.dc, self.w, self.wt = dt, np.asarray(dc), np.asarray(w), np.asarray(wt)
		self.cat, self.keepvar, self.tol = cat, keepvar, tol
		nt, ns = dt.shape
		nc = self.dc.shape[0]
		first = normvar(dt, self.dc, self.w, self.wt, cat=cat, keepvar=keepvar, tol=tol, device_out=True)  # (every argument check and error of the public call, once)
		self.dcn = first[1]
		self.lean = nc <= int(eng.lib.nrm_normvar_device_covariates()) and _opts.debug('normvar', 'device') != 'host' and dt.dtype in (torch.float32, torch.float64) and dt.stride(1) == 1
		self.out = first[0]
		self._graph = StepGraph(torch)
		if self.lean:
			with eng.lock, torch.cuda.device(eng.device):
				npair = nc * (nc + 1) // 2
				self._lnw = eng.upload(np.log(np.asarray(self.w, dtype=np.float64)))
				self._wt = eng.upload(np.asarray(self.wt, dtype=np.float64))
				self._c = eng.upload(np.asarray(self.dc, dtype=np.float64))
				self._mom = torch.empty((nt, npair + nc + 2), dtype=torch.float64, device=eng.device)
				self._b = torch.empty((nt, nc), dtype=torch.float64, device=eng.device)
				self._scale = torch.empty((nt, ), dtype=torch.float64, device=eng.device)
				self._rank = torch.empty((nt, ), dtype=torch.int64, device=eng.device)
				self._flags = eng.zeros((4, ), torch.int32)

	def _launch(self):
		# (the C library's twin on its own buffers: NrmNormvarStep, csrc/nrm_normvar_step.h)
		eng, y, out = self.eng, self.dt, self.out
		nt, ns = y.shape
		nc = self.dc.shape[0]
		ycode = _engine.dtype_code(y)
		ocode = _engine.dtype_code(out)
		_lib.check(eng.lib.nrm_normvar_solve(y.data_ptr(), ycode, nt, ns, y.stride(0), self._lnw.data_ptr(), self._wt.data_ptr(), self._c.data_ptr(), nc, self._c.stride(0), float(self.tol),
											 1 if self.keepvar else 0, self._mom.data_ptr(), self._b.data_ptr(), self._scale.data_ptr(), self._rank.data_ptr(), self._flags.data_ptr(), eng._stream()))
		_rescale(eng, y, ycode, nt, ns, self._lnw, self._wt, self._c, nc, self._b, self._scale)
		_lib.check(eng.lib.nrm_normvar_apply(y.data_ptr(), ycode, nt, ns, y.stride(0), self._lnw.data_ptr(), self._wt.data_ptr(), self._c.data_ptr(), nc, self._c.stride(0),
											 self._b.data_ptr(), self._scale.data_ptr(), out.data_ptr(), ocode, ns, self._flags.data_ptr(), eng._stream()))

	def step(self, timed=False):
		"""One pass over the matrix as it stands in HBM now; the result in self.out (the same tensor every step), the scaled covariates in self.dcn."""
		eng = self.eng
		with eng.lock, eng.torch.cuda.device(eng.device):
			if not self.lean:
				self.out, self.dcn = normvar(self.dt, self.dc, self.w, self.wt, cat=self.cat, keepvar=self.keepvar, tol=self.tol, device_out=True)[:2]
			else:
				self._graph.run(self._launch)
		return self.out

	def check(self):
		"""The counters of the steps since the last check (one small read-back): RuntimeError / AssertionError as normvar raises them."""
		if not self.lean:
			return True
		eng = self.eng
		with eng.lock, eng.torch.cuda.device(eng.device):
			f = self._flags.cpu().numpy()
			self._flags.zero_()
		if f[0]:
			raise RuntimeError('Zero-rank covariates found.')
		assert not f[1]  # np.isfinite(dtn).all() (norm.py:286): counted by the kernel that wrote the values
		return True

	def results(self):
		"""[dtn, dcn] as normvar returns them (dtn downloaded)."""
		self.check()
		return [self.eng.download(self.out), self.dcn]


class ComputeVarPlan:
	"""compute_var on a logCPM matrix RESIDENT in HBM, step after step (the matrix rewritten in place between steps), with nothing on the host: what a call of
	compute_var does in numpy between its three streaming passes -- the weighted covariates and the pseudo-inverse of their Gram matrix, the log, the fit on
	span(dc, 1), exp, the minimum, the best-step rule of norm.py:116-120 and the loop test of norm.py:98 -- are the kernels of csrc/nrm_fitvar_plan.hip on a
	small state record in HBM.  A step enqueues all stepmax iterations and the weights; no kernel waits for the host and the host decides nothing, so a step is ONE
	HIP graph from the second on and that graph stays valid when dt is rewritten in place.  Iterations enqueued past the stop condition leave the state as it is.
	The covariates' upload, the pseudo-inverse of [dc;1][dc;1]^T (host inv_rank: it does not depend on dt) and every buffer are made once, here.
	64 to nrm_wide_covariates() covariates (with more cells than covariates): orthonormal bases of the covariates' row space and of span(dc, 1) are made once on
	the host (_fitvar_bases) and stand in for the covariates; an iteration's matrix (B u)(B u)^T is then positive definite, formed on the fp64 matrix cores
	(nrm_gram_f64_whole) and inverted by a blocked Cholesky inverse spread over the chip (csrc/nrm_chol_inverse.hip) -- no eigen-decomposition on the device, one
	stream, one graph.  That the basis keeps the directions the reference's rank rule keeps is certified as in _wide_basis: at creation for equal weights
	(NotImplementedError otherwise), per iteration on the device for the weights as they are (check() raises NotImplementedError: compute_var() is then the call).
	check() reads the counters of the steps since the last check and raises what compute_var raises (norm.py:125-127); results() returns the weights as compute_var
	does and sets steps_taken (iterations that ran) and best_change (the smallest maximum relative change of the scale, the reference's bestv)."""

	def __init__(self, dt, dc, stepmax=1, eps=1E-6, eng=None):
		from .distributed import StepGraph
		if eps <= 0 or stepmax <= 0:
			raise ValueError('eps and stepmax must be positive.')
		dc = dc.cpu().numpy() if _engine.is_dev(dc) else np.asarray(dc)
		shape = tuple(dt.shape) if _engine.is_dev(dt) else np.asarray(dt).shape
		if len(shape) != 2 or dc.ndim != 2:
			raise ValueError('dt and dc must both have 2 dimensions.')
		if shape[1] != dc.shape[1]:
			raise ValueError('dt and dc must have the same cell count.')
		nt, ns = shape
		nc = dc.shape[0]
		if nc == 0:
			raise NotImplementedError('compute_var on the device takes at least one covariate.')
		self.wide = nc > 63
		if self.wide:
			_check_wide('compute_var', nc, ns)
		if nt == 0 or ns == 0:
			raise ValueError('dt must not be empty.')
		if self.wide:
			# the bases of _fitvar_bases in the place of the covariates; refused when the rank certificate fails already for equal weights (nearly collinear
			# covariates: an eigenvalue of dc dc^T inside the band around the rank rule's tolerance) -- host numpy, before any device call
			b, r, hi, lo, b1 = self._bases = _fitvar_bases(dc)
			self.rank, self._cert = r, (hi, lo, 1E-8, WIDE_SAFETY, 1 if r == nc else 0)
			if not _fitvar_certified(hi, lo, r == nc, 1.0):
				raise NotImplementedError('ComputeVarPlan beyond 63 covariates needs covariates whose rank is certain: eigenvalue {} of dc dc^T is {:.3g} of the largest, the '
										  'next {:.3g}, around the rank rule\'s 1e-8.  compute_var() is the call for these covariates.'.format(r, hi, lo))
		if not _engine.is_dev(dt):
			raise ValueError('ComputeVarPlan takes a logCPM matrix resident in HBM (a torch CUDA tensor); compute_var() is the call for host arrays.')
		self.eng = eng = eng or _engine.get_engine(dt.device.index)
		torch = eng.torch
		if dt.dtype not in (torch.float32, torch.float64) or dt.stride(1) != 1:
			raise ValueError('ComputeVarPlan takes an fp32 or fp64 matrix with unit column stride.')
		self.dt, self.stepmax, self.eps = dt, int(stepmax), float(eps)
		self.dc = c64 = np.array(dc, dtype=np.float64, order='C')
		self.steps_taken = self.best_change = None
		self._graph = StepGraph(torch)
		if self.wide:
			self._init_wide(nt, ns)
			return
		c1 = np.concatenate([c64, np.ones((1, ns))], axis=0)  # the second regression has an intercept (norm.py:92,109-110)
		m2i = _pinv_gram_unit_rows(c1)
		with eng.lock, torch.cuda.device(eng.device):
			f64 = dict(dtype=torch.float64, device=eng.device)
			self._c, self._m2i = eng.upload(c64), eng.upload(np.ascontiguousarray(m2i, dtype=np.float64))
			self._a, self._b = torch.empty((nt, nc), **f64), torch.empty((nt, nc), **f64)
			self._mean, self._sc, self._v = torch.empty((nt, ), **f64), torch.empty((nt, ), **f64), torch.empty((ns, ), **f64)
			self._part = torch.empty((-(-nt // int(eng.lib.nrm_fitvar_row_tile())), ns), **f64)
			self._s, self._best, self._u = torch.empty((ns, ), **f64), torch.empty((ns, ), **f64), torch.empty((ns, ), **f64)
			self._cw, self._mi = torch.empty((nc, ns), **f64), torch.empty((nc, nc), **f64)
			self._rank = torch.empty((1, ), dtype=torch.int64, device=eng.device)
			self._ws = torch.empty((int(eng.lib.nrm_fitvar_plan_workspace(ns, nc)), ), **f64)
			# the state records (one per iteration and the first) and, right after the last, the weights: results() reads both in one copy
			self._out = torch.empty((4 * (self.stepmax + 1) + ns, ), **f64)
			self._state = self._out[:4 * (self.stepmax + 1)].view(self.stepmax + 1, 4)
			self.w = self._out[4 * (self.stepmax + 1):]
			self._flags = eng.zeros((4, ), torch.int32)

	def _init_wide(self, nt, ns):
		"""64 .. nrm_wide_covariates() covariates: the bases uploaded once, and every buffer of a step."""
		eng, torch, lib = self.eng, self.eng.torch, self.eng.lib
		b, r, hi, lo, b1 = self._bases
		del self._bases
		r1 = b1.shape[0]
		rp, kp = _engine.round_up(r, ROW_TILE), _engine.round_up(ns, K_TILE)
		with eng.lock, torch.cuda.device(eng.device):
			f64 = dict(dtype=torch.float64, device=eng.device)
			self._c, self._b1 = eng.upload(np.ascontiguousarray(b)), eng.upload(np.ascontiguousarray(b1))
			self._a, self._b = torch.empty((nt, r), **f64), torch.empty((nt, r), **f64)
			self._mean, self._sc, self._v = torch.empty((nt, ), **f64), torch.empty((nt, ), **f64), torch.empty((ns, ), **f64)
			self._part = torch.empty((-(-nt // int(lib.nrm_fitvar_row_tile())), ns), **f64)
			self._s, self._best, self._u = torch.empty((ns, ), **f64), torch.empty((ns, ), **f64), torch.empty((ns, ), **f64)
			self._cw, self._mi = torch.empty((r, ns), **f64), torch.empty((r, r), **f64)
			self._bu, self._m = torch.empty((rp, kp), **f64), torch.empty((rp, rp), **f64)
			self._ws = torch.empty((int(lib.nrm_fitvar_wide_workspace(ns, r, r1)), ), **f64)
			self._ciws = torch.empty((int(lib.nrm_chol_inverse_workspace(r)), ), **f64)
			self._out = torch.empty((4 * (self.stepmax + 1) + ns, ), **f64)
			self._state = self._out[:4 * (self.stepmax + 1)].view(self.stepmax + 1, 4)
			self.w = self._out[4 * (self.stepmax + 1):]
			self._flags = eng.zeros((8, ), torch.int32)  # [0], [1] as below; [2] iterations without the rank certificate; [3], [4] nrm_chol_inverse's status

	def _launch_wide(self):
		eng, y, lib = self.eng, self.dt, self.eng.lib
		nt, ns = y.shape
		r, r1 = self._c.shape[0], self._b1.shape[0]
		rp, kp = self._bu.shape
		ycode = _engine.dtype_code(y)
		st, p = eng._stream(), lambda t: t.data_ptr()
		hi, lo, tol, safety, full = self._cert
		_lib.check(lib.nrm_fitvar_plan_start(ns, p(self._s), p(self._best), p(self._state[0]), st))
		for i in range(self.stepmax):
			now, nxt = p(self._state[i]), p(self._state[i + 1])
			_lib.check(lib.nrm_fitvar_wide_design(p(self._c), r, self._c.stride(0), ns, p(self._s), now, self.eps, hi, lo, tol, safety, full, p(self._u), p(self._bu), rp, kp,
												  p(self._cw), p(self._ws), p(self._flags), st))
			_lib.check(lib.nrm_gram_f64_whole(p(self._bu), p(self._bu), rp, rp, kp, kp, kp, p(self._m), rp, r, r, st))
			_lib.check(lib.nrm_chol_inverse(p(self._m), rp, r, p(self._mi), r, p(self._ciws), p(self._flags) + 12, st))
			_lib.check(lib.nrm_fitvar_moments(p(y), ycode, nt, ns, y.stride(0), p(self._cw), r, self._cw.stride(0), p(self._a), st))
			_lib.check(lib.nrm_fitvar_genes(p(y), ycode, nt, ns, y.stride(0), p(self._u), p(self._c), r, self._c.stride(0), p(self._a), p(self._mi), p(self._b), p(self._mean),
											p(self._sc), p(self._flags), st))
			_lib.check(lib.nrm_fitvar_cells(p(y), ycode, nt, ns, y.stride(0), p(self._u), p(self._c), r, self._c.stride(0), p(self._b), p(self._mean), p(self._sc), p(self._part),
											p(self._v), st))
			_lib.check(lib.nrm_fitvar_wide_update(p(self._v), p(self._b1), r1, self._b1.stride(0), ns, p(self._s), p(self._best), now, nxt, self.eps, p(self._ws), st))
		_lib.check(lib.nrm_fitvar_weights(p(self._best), ns, p(self._ws), p(self.w), p(self._flags), st))

	def _launch(self):
		# (the C library's twin on its own buffers: NrmFitvarStep::enqueue, csrc/nrm_fitvar_step.h)
		if self.wide:
			return self._launch_wide()
		eng, y, lib = self.eng, self.dt, self.eng.lib
		nt, ns = y.shape
		nc = self.dc.shape[0]
		ycode = _engine.dtype_code(y)
		st, p = eng._stream(), lambda t: t.data_ptr()
		_lib.check(lib.nrm_fitvar_plan_start(ns, p(self._s), p(self._best), p(self._state[0]), st))
		for i in range(self.stepmax):
			now, nxt = p(self._state[i]), p(self._state[i + 1])
			_lib.check(lib.nrm_fitvar_design(p(self._c), nc, self._c.stride(0), ns, p(self._s), now, self.eps, p(self._u), p(self._cw), p(self._ws), st))
			_lib.check(lib.nrm_fitvar_pinv(ns, nc, 1E-8, now, self.eps, p(self._ws), p(self._mi), p(self._rank), st))
			_lib.check(lib.nrm_fitvar_moments(p(y), ycode, nt, ns, y.stride(0), p(self._cw), nc, self._cw.stride(0), p(self._a), st))
			_lib.check(lib.nrm_fitvar_genes(p(y), ycode, nt, ns, y.stride(0), p(self._u), p(self._c), nc, self._c.stride(0), p(self._a), p(self._mi), p(self._b), p(self._mean),
											p(self._sc), p(self._flags), st))
			_lib.check(lib.nrm_fitvar_cells(p(y), ycode, nt, ns, y.stride(0), p(self._u), p(self._c), nc, self._c.stride(0), p(self._b), p(self._mean), p(self._sc), p(self._part),
											p(self._v), st))
			_lib.check(lib.nrm_fitvar_update(p(self._v), p(self._c), nc, self._c.stride(0), ns, p(self._m2i), p(self._s), p(self._best), now, nxt, self.eps, p(self._ws), st))
		_lib.check(lib.nrm_fitvar_weights(p(self._best), ns, p(self._ws), p(self.w), p(self._flags), st))

	def step(self):
		"""All stepmax iterations and the weights on the matrix as it stands in HBM now; the weights in self.w (device fp64, the same tensor every step)."""
		eng = self.eng
		with eng.lock, eng.torch.cuda.device(eng.device):
			self._graph.run(self._launch)
		return self.w

	def check(self):
		"""The counters of the steps since the last check (one small read-back): AssertionError as compute_var raises it."""
		eng = self.eng
		with eng.lock, eng.torch.cuda.device(eng.device):
			f = self._flags.cpu().numpy()
			self._flags.zero_()
		assert not f[0]  # a gene whose residual is constant: its spread divides (norm.py:108), the result is not finite (norm.py:125)
		if self.wide and f[2]:
			raise NotImplementedError('ComputeVarPlan: {} iteration(s) ran with cell weights too far apart for the rank certificate of the covariates\' basis; compute_var() is '
									  'the call for these weights.'.format(int(f[2])))
		assert not (self.wide and (f[3] or f[4]))  # nrm_chol_inverse: a pivot that is not positive, a value that is not finite
		assert not f[1]  # weights finite and positive (norm.py:126-127), `best is not None` (norm.py:122)
		return True

	def results(self):
		"""The weights as compute_var returns them; steps_taken and best_change from the last state record, read in the same copy."""
		self.check()
		eng = self.eng
		with eng.lock, eng.torch.cuda.device(eng.device):
			o = self._out[4 * self.stepmax:].cpu().numpy()
		self.best_change, self.steps_taken = float(o[0]), int(o[1])
		return o[4:].copy()


assert __name__ != "__main__"
