"""Plain-numpy restatement of the principal-gene selection and of pccovt (normalisr_amd/gocovt.py), written for this project: the independent check of the
GPU tests, in a float type given as argument (np.float64, or np.longdouble as the yardstick the device is held to).  Nothing here calls LAPACK, so every step
runs in the type asked for: the projection is a twice-applied modified Gram-Schmidt, the component a power iteration carried to the rounding of that type.

  project_off   rows minus their orthogonal projection onto span(design rows), whatever the rank of the design
  pccovt        projection (off [dc; 1], or off the constant row alone), scaling to mean square 1 (+ 1e-200), correlation matrix, power iteration, sign
                rule (the loading of largest magnitude positive, the first of equals), score Z^T v
  principal     the genes whose degree reaches that of the gene ranked n
  g21_case, rel the cases of golden G21 as the tests take them, and the distance they measure
"""
import numpy as np


def principal(net, n):
	"""Indices of the principal genes of a binary network: degree >= the degree of the gene ranked n (0-based, descending)."""
	deg = (np.asarray(net) != 0).sum(axis=1)
	thr = np.sort(deg)[::-1][n]
	if thr == 0:
		raise RuntimeError('Not enough principal genes that have co-expression')
	return np.flatnonzero(deg >= thr).astype(np.int64)


def _basis(design, ft, tol=1e-8):
	"""Orthonormal rows spanning the rows of design (Gram-Schmidt applied twice; a row that keeps less than tol of its length is dependent and dropped)."""
	q = []
	for row in np.asarray(design, dtype=ft):
		norm0 = np.sqrt((row * row).sum())
		if norm0 == 0:
			continue
		r = row / norm0
		for _ in range(2):
			for b in q:
				r = r - (r * b).sum() * b
		norm = np.sqrt((r * r).sum())
		if norm > tol:
			q.append(r / norm)
	return q


def project_off(rows, design, ft=np.float64):
	rows = np.array(rows, dtype=ft)
	q = _basis(design, ft)
	for _ in range(2):
		for b in q:
			rows = rows - np.outer((rows * b).sum(axis=1), b)
	return rows


def start(m, ft):
	"""The start of the power iteration: positive and not constant, free of any seed (the package's own start, restated)."""
	g = np.arange(m, dtype=np.uint64)
	v = (1.0 + ((g * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / 2.0**32).astype(ft)
	return v / np.sqrt((v * v).sum())


def power(r, ft, max_iter=200000):
	"""Top eigenvector of the symmetric non-negative definite r by power iteration in ft, to that type's rounding: (v, lambda, iterations, converged).  The
	start is positive and not constant."""
	m = r.shape[0]
	u = np.finfo(ft).eps / 2
	v = start(m, ft)
	lam, mark = ft(0), None
	for it in range(1, max_iter + 1):
		w = (r * v[None, :]).sum(axis=1)
		lam = (v * w).sum()
		d = w - lam * v
		res = np.sqrt((d * d).sum())
		nw = np.sqrt((w * w).sum())
		if nw == 0:
			return v, lam, it, True
		v = w / nw
		if res <= 2 * np.sqrt(ft(m)) * u * lam:
			return v, lam, it, True
		# (the floor of the computed residual is not known in advance: also stop once 50 steps no longer halve it -- the floor, for sigma_2 / sigma_1 < 0.993)
		if it % 50 == 0:
			if mark is not None and res > 0.5 * mark and res <= 64 * m * u * lam:
				return v, lam, it, True
			mark = res
	return v, lam, max_iter, False


def pccovt(dt, dc, idx, condcov=True, ft=np.float64, return_all=False):
	"""The score row (n_cell,) in ft of the top principal component of rows idx of dt; return_all: (score, loadings v, lambda = sigma_1^2 / n, the scaled rows Z)."""
	dt = np.asarray(dt)
	dc = np.asarray(dc)
	idx = np.asarray(idx, dtype=np.int64)
	n = dt.shape[1]
	rows = dt[idx].astype(ft)
	one = np.ones((1, n), dtype=ft)
	design = np.concatenate([dc.astype(ft), one], axis=0) if condcov and dc.shape[0] > 0 else one
	res = project_off(rows, design, ft)
	a = 1 / (np.sqrt((res * res).sum(axis=1) / ft(n)) + ft(1e-200))
	z = res * a[:, None]
	r = np.empty((len(idx), len(idx)), dtype=ft)
	for g in range(len(idx)):  # (row by row: no BLAS, so the type asked for is the type used)
		r[g] = (z * z[g][None, :]).sum(axis=1) / ft(n)
	r = (r + r.T) / 2
	v, lam, _, ok = power(r, ft)
	assert ok, 'power iteration did not converge'
	top = int(np.argmax(np.abs(v)))
	if v[top] < 0:
		v = -v
	score = (z * v[:, None]).sum(axis=0)
	return (score, v, lam, z) if return_all else score


def singular_ratio(z):
	"""sigma_2 / sigma_1 of the scaled rows (float64 LAPACK: a description of the case, not a yardstick)."""
	s = np.linalg.svd(np.asarray(z, dtype=np.float64), compute_uv=False)
	return float(s[1] / s[0]) if len(s) > 1 and s[0] > 0 else 0.0


def g21_case(g, name):
	"""(dt, dc, namet, genes, idx, condcov, what the reference returned) of a case of G21."""
	src = 'c1' if name in ('c4', 'c5') else name
	if src == 'c3':
		dt = 200.0 + g['c3_code'].astype(np.float64) / 8
	else:
		dt = g[src + '_dt'].astype(np.float32 if name == 'c5' else np.float64)
	dc = g[src + '_dc']
	if name == 'c5':
		dc = dc.astype(np.float32)
	return dt, dc, [str(v) for v in g[name + '_namet']], [str(v) for v in g[name + '_genes']], g[name + '_idx'], name not in ('c4', 'c5'), g[name + '_out']


def rel(a, b):
	b = np.asarray(b, dtype=np.float64)
	return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())
