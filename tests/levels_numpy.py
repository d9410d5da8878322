"""Plain-numpy restatement of normalisr_amd/levels.py, written for this project: the independent check of the GPU tests, in a float type given as argument
(np.float64, or np.longdouble as the yardstick the device is held to).

  span_basis    orthonormal rows spanning what coex removes for covariates dc: the eigenvectors of dc dc^T whose eigenvalue reaches tol x the largest (the rule of
                inv_rank, reference association.py:77-80; the one LAPACK call, in fp64, since the rank is defined by it), then Gram-Schmidt twice in the type asked for
  gram          the from-scratch residual Gram matrix G = X (I - P) X^T and its diagonal, the sums of squares
  update        G - a a^T, ss - a^2 with a = X q on the raw rows
  decide        the rank / rho decision of an append: a pure function of (basis, dc, rows)
  guard         the two counters of the downdate
  outputs       (p, dot, var) of coex from (G, ss): R^2 = G^2 / (ss_i ss_j), p = I_{1 - R^2}(dof / 2, 1 / 2) (association.py:230-249), zero diagonals
  Levels        the class, restated on the above
  g23_case, p_errors, of_largest   the problems of golden G23 as the tests take them, and the distances they measure
"""
import numpy as np

RHO_MIN, RHO_SPAN, GUARD = 1e-6, 1e-12, 2.0**-10


def _gs(rows, ft, against=()):
	"""rows made orthonormal in type ft by modified Gram-Schmidt, every projection applied twice, first against the orthonormal rows `against`."""
	out = []
	for v in np.asarray(rows, dtype=ft):
		for _ in range(2):
			for b in list(against) + out:
				v = v - (v * b).sum() * b
		out.append(v / np.sqrt((v * v).sum()))
	return out


def span_basis(dc, ft=np.float64, tol=1E-8):
	dc64 = np.asarray(dc, dtype=np.float64)
	nc, n = dc64.shape
	if nc == 0 or not (dc64 != 0).any():
		return np.zeros((0, n), dtype=ft), 0
	_, s, vh = np.linalg.svd(dc64 @ dc64.T)
	r = int((s >= tol * s[0]).sum())
	b0 = (vh[:r] @ dc64) / np.sqrt(s[:r])[:, None]
	return np.array(_gs(b0, ft), dtype=ft).reshape(r, n), r


def off_span(b, v):
	for _ in range(2):
		for row in b:
			v = v - (v * row).sum() * row
	return v


def gram(dt, dc, ft=np.float64):
	b, r = span_basis(dc, ft)
	x = np.array(dt, dtype=ft)
	for _ in range(2):
		if r:
			x = x - (x @ b.T) @ b
	return x @ x.T, (x * x).sum(axis=1), b, r


def update(g, ss, dt, q, ft=np.float64):
	"""One direction q (n_cell, ), unit length and orthogonal to the covariates removed so far."""
	a = np.asarray(dt, dtype=ft) @ np.asarray(q, dtype=ft)
	return g - np.outer(a, a), ss - a * a, a


def decide(b, dc, rows, ft=np.float64):
	"""dict(rank, rho, update, q): rank of the enlarged covariates by the eigenvalue rule; rho = |v - B^T B v|^2 / |v|^2 per row, B the basis and the rows accepted before it; update: the rank grows by exactly
	the rows with rho >= RHO_MIN and every other row has rho <= RHO_SPAN; q: those rows made orthonormal to b and to each other, in order."""
	rows = np.asarray(rows, dtype=ft).reshape(-1, np.shape(dc)[1])
	rank = span_basis(np.concatenate([np.asarray(dc, dtype=np.float64), rows.astype(np.float64)]))[1]
	rho = np.zeros(len(rows))
	qs, ok = [], True
	for i, v in enumerate(rows):
		vv = (v * v).sum()
		if vv == 0:
			continue
		q = off_span(qs, off_span(b, v))
		left = (q * q).sum()
		rho[i] = float(left / vv)
		if rho[i] >= RHO_MIN:
			qs.append(q / np.sqrt(left))
		elif rho[i] > RHO_SPAN:
			ok = False
	ok = bool(ok and rank - len(b) == len(qs))
	return dict(rank=rank, rho=rho, update=ok, q=qs if ok else [])


def guard(ss_new, ss_ref):
	ss_new, ss_ref = np.asarray(ss_new, dtype=np.float64), np.asarray(ss_ref, dtype=np.float64)
	return int((~(np.isfinite(ss_new) & (ss_new > 0))).sum()), int((ss_new < GUARD * ss_ref).sum())


def outputs(g, ss, n, dof, out_dtype=np.float64):
	from scipy.special import betainc
	g, ss = np.asarray(g), np.asarray(ss)
	var = np.asarray(ss / n, dtype=np.float64)
	var[var == 0] = 1
	s = np.where(ss == 0, np.asarray(n, dtype=ss.dtype), ss)
	r2 = np.asarray((g * g) / np.outer(s, s), dtype=np.float64)
	p = betainc(dof / 2.0, 0.5, 1 - np.minimum(r2, 1.0))
	dot = np.asarray(g / n, dtype=np.float64)
	np.fill_diagonal(p, 0)
	np.fill_diagonal(dot, 0)
	return p.astype(out_dtype), dot.astype(out_dtype), var.astype(out_dtype)


class Levels:
	def __init__(self, dt, dc, dimreduce=0, ft=np.float64):
		self.dt, self.dc, self.dimreduce, self.ft = np.asarray(dt), np.asarray(dc, dtype=np.float64), dimreduce, ft
		self.rebuilt, self.info = [], None
		self._build()

	def _build(self):
		self.g, self.ss, self.b, self.rank = gram(self.dt, self.dc, self.ft)
		self.ss_ref = self.ss.copy()

	@property
	def dof(self):
		return self.dt.shape[1] - 1 - self.rank - self.dimreduce

	def results(self, out_dtype=np.float64):
		return outputs(self.g, self.ss, self.dt.shape[1], self.dof, out_dtype)

	def append(self, rows):
		rows = np.asarray(rows, dtype=np.float64).reshape(-1, self.dt.shape[1])
		plan = decide(self.b, self.dc, rows, self.ft)
		self.dc = np.concatenate([self.dc, rows])
		counters, rebuilt = (0, 0), not plan['update']
		if plan['update'] and plan['q']:
			g, ss = self.g, self.ss
			for q in plan['q']:
				g, ss, _ = update(g, ss, self.dt, q, self.ft)
			counters = guard(ss, self.ss_ref)
			rebuilt = counters[0] > 0 or counters[1] > 0
			if not rebuilt:
				self.g, self.ss, self.rank = g, ss, plan['rank']
				self.b = np.concatenate([self.b, np.array(plan['q'], dtype=self.ft)])
		if rebuilt:
			self._build()
		self.info = dict(rho=plan['rho'], counters=counters)
		self.rebuilt.append(bool(rebuilt))
		return self


def g23_case(g, name):
	"""(dt fp32, dc, rows) of a G23 problem: A as stored, B rebuilt from its seed (tests/golden/g23_inputs.py); both held to the stored check sums."""
	import os
	import sys
	here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
	if here not in sys.path:
		sys.path.insert(0, here)
	from g23_inputs import checksum, g23_inputs
	dt, dc, rows, _ = g23_inputs(name)
	if name == 'A':
		assert np.array_equal(dt, g['A_dt']) and np.array_equal(dc, g['A_dc']) and np.array_equal(rows, g['A_rows'])
	for key, v in (('dt', dt), ('dc', dc), ('rows', rows)):
		want = g['{}_sum_{}'.format(name, key)]
		assert np.allclose(checksum(v), want, rtol=1e-12, atol=1e-9 * np.abs(want).max()), (name, key)
	return dt, dc, rows


def p_errors(p, want):
	"""(largest relative error where the reference's P >= 1e-290, largest P elsewhere), off the diagonal."""
	p, want = np.asarray(p, dtype=np.float64), np.asarray(want, dtype=np.float64)
	off = ~np.eye(len(p), dtype=bool)
	big, small = off & (want >= 1e-290), off & (want < 1e-290)
	return (float((np.abs(p[big] - want[big]) / want[big]).max()) if big.any() else 0.0, float(p[small].max()) if small.any() else 0.0)


def of_largest(a, want):
	return float(np.abs(np.asarray(a, dtype=np.float64) - want).max() / np.abs(want).max())
