#!/usr/bin/env python3
"""G25: ln P of the single=0 sweeps (logp=True) against exact arithmetic -- two fixtures.

G25_logp_grid.npz: (r2, dof, lnp), lnp = ln I_x(dof/2, 1/2) with x = fl(1 - r2), correct to far more than a double holds.  The dofs of G12 and its
alpha u grid, extended to 1e3, 1e4, 1e5 and 1e6 wherever R^2 stays below 1 in double precision; both sides of R^2 = 1/4 (where the device's logarithm
changes form) and of u = 1.5 (series / continued fraction); R^2 in {0.5, 0.9, 0.99, 0.999999, 1 - 2^-52} (ln P down to -9e6), 1e-300 and 5e-324 (x = 1).

G25_logp_case.npz: one small problem with its inputs stored -- dt (70, 2100) fp32 (two ragged tile columns; above the 2048 cells from which the integer
engine runs), dc (4, 2100) three covariates and the intercept, dg (5, 2100) a sparse binary design -- and the expected ln P of coex (70, 70) and de (5, 70),
from a residualisation of exactly those inputs in longdouble (in the manner of tests/k1_longdouble.py) and the same exact function.  The genes hold null
pairs, moderate pairs, pairs with R^2 near 0.6 and 0.9 whose P is exactly 0 in double precision (asserted below), one pair with 1 - R^2 near 1e-4, one
constant gene (variance 0 -> 1; constant at 0: any other constant leaves rounding noise for a residual, in the reference's arithmetic as in the
device's, its variance is then not 0 and its R^2 is that noise's) and one exact duplicate of another gene (R^2 = 1 up to rounding: named in `dup`, left
out of value comparisons).

The function: mpmath's betainc does not converge for a in the tens of thousands, so I_x(a, 1/2) is summed here from its two hypergeometric series with
positive terms -- I_x(a, b) = x^a (1-x)^b / (a B(a,b)) sum_n (a+b)_n / (a+1)_n x^n, or 1 - the same with (a, x) and (b, 1-x) exchanged where P is not
small -- in 400-bit fixed point (every ratio is rational: 2a = dof is an integer), the prefactor in mpmath at 80 digits.  Checked against mpmath's betainc
where that converges.  Needs mpmath; a few minutes.

    python3 tests/golden/make_g25.py
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 80
HERE = os.path.dirname(os.path.abspath(__file__))
PREC = 400  # bits of the fixed-point sums
LD = np.longdouble


def _series(dof2, lower, x, tol_bits=300):
	"""sum_n t_n, t_0 = 1, t_{n+1} = t_n (dof2 + 1 + 2n) / (lower + 2n) x for the double x, as an mpf: dof2 = 2a an integer, b = 1/2."""
	xm, xe = np.frexp(x)
	xi, sh = int(xm * 2**53), 53 - int(xe)  # x = xi 2^-sh exactly
	one = 1 << PREC
	t, s, n = one, one, 0
	while True:
		num, den = dof2 + 1 + 2 * n, lower + 2 * n
		t = (t * num * xi) // (den << sh)
		s += t
		n += 1
		rho = max(num * x / den, x)  # the ratios of the later terms lie between this one's and x: the tail is below t / (1 - rho)
		if rho < 1.0 and t < (s >> tol_bits) * (1.0 - rho):
			break
	return mp.mpf(s) / mp.mpf(one)


def lnp_exact(r2, dof):
	"""ln I_x(dof/2, 1/2), x = fl(1 - r2): 0 for x >= 1, -inf for x <= 0."""
	x = float(np.float64(1.0) - np.float64(r2))
	if x <= 0:
		return -mp.inf
	if x >= 1:
		return mp.mpf(0)
	w = 1.0 - x  # exact in double (Sterbenz, or x < 1/2: no bits lost either way for x = fl(1 - r2))
	assert mp.mpf(x) + mp.mpf(w) == 1
	dof2 = int(dof)
	assert dof2 == dof
	a = mp.mpf(dof2) / 2
	lnB = mp.loggamma(a) + mp.loggamma(mp.mpf(1) / 2) - mp.loggamma(a + mp.mpf(1) / 2)
	if float(a) * w < 30 and w <= 0.5:  # P above e^-30 or so: 1 - I_w(1/2, a), at most 14 of the 80 digits cancel (its series falls as w^n: not for w near 1)
		s = _series(dof2, 3, w)
		t = mp.sqrt(mp.mpf(w)) * mp.exp(a * mp.log(mp.mpf(x)) - lnB) * 2 * s
		return mp.log1p(-t)
	s = _series(dof2, dof2 + 2, x)
	return a * mp.log(mp.mpf(x)) + mp.log(mp.mpf(w)) / 2 - lnB - mp.log(a) + mp.log(s)


def self_check():
	for r2, dof in ((0.0012, 99980.0), (0.3, 100.0), (1e-5, 996.0), (0.05, 996.0), (0.5, 30.0), (0.028, 996.0), (0.031, 996.0)):
		x = float(np.float64(1.0) - np.float64(r2))
		ref = mp.log(mp.betainc(mp.mpf(dof) / 2, mp.mpf(1) / 2, 0, mp.mpf(x), regularized=True))
		got = lnp_exact(r2, dof)
		assert abs(got - ref) < mp.mpf(10)**-40 * (1 + abs(ref)), (r2, dof, got, ref)
	assert abs(lnp_exact(0.0012, 99980.0) + mp.mpf('62.65')) < 0.01  # (the figure quoted when this mode was asked for)


def make_grid():
	dofs = [16.0, 17.0, 30.0, 100.0, 996.0, 9996.0, 49990.0, 99980.0, 499996.0]
	r2s, ds, lps = [], [], []
	for dof in dofs:
		alpha = dof / 2 - 0.25
		zs = np.concatenate([np.logspace(-12, 0, 13), np.linspace(1.5, 30, 20), np.linspace(35, 740, 25), [1e3, 1e4, 1e5, 1e6]])
		grid = [float(-mp.expm1(-mp.mpf(z) / alpha)) for z in zs]  # R^2 with alpha u = z
		grid += [0.2, 0.2499999, 0.25, 0.2500001, 0.3, 0.5, 0.77, 0.7768, 0.78, 0.9, 0.99, 0.999999, 1.0 - 2.0**-52, 1e-300, 5e-324]
		for r2 in grid:
			if not 0 < r2 < 1:
				continue
			lp = lnp_exact(r2, dof)
			assert mp.isfinite(lp) and lp <= 0
			r2s.append(r2)
			ds.append(dof)
			lps.append(float(lp))
		print('grid: dof', dof, 'done', flush=True)
	out = os.path.join(HERE, 'G25_logp_grid.npz')
	np.savez_compressed(out, r2=np.array(r2s), dof=np.array(ds), lnp=np.array(lps))
	print(out, len(r2s), 'points; ln P from', min(lps), 'to', max(lps))


# ---- the case ---------------------------------------------------------------------------------------------------------------------------------------------
NG, NCELL, DUP = 70, 2100, (5, 69)
PLANTED = dict(r2_06=(0, 50), r2_09=(1, 51), near_one=(2, 52), constant=53)


def case_inputs():
	rng = np.random.default_rng(25)
	n = NCELL
	dc = np.ones((4, n))
	dc[0] = np.round(rng.normal(size=n), 3)
	dc[1] = np.round(rng.normal(size=n) * 2 + 1, 3)
	dc[2] = (rng.random(n) < 0.4).astype(np.float64)  # a batch
	dg = np.zeros((5, n), dtype=np.uint8)
	for i, k in enumerate((60, 90, 110, 120, 130)):  # 4.9 % of the entries set: a design the sparse-design kernels take
		dg[i, rng.choice(n, k, replace=False)] = 1
	z = rng.normal(size=(NG, n))
	dt = z.copy()
	for k in range(10):  # moderate pairs: gene 40 + k with gene k, R^2 from 0.002 to 0.09
		rho = 0.045 + 0.028 * k
		dt[40 + k] = rho * z[k] + np.sqrt(1 - rho * rho) * z[40 + k]
	dt[50] = np.sqrt(0.6) * z[0] + np.sqrt(0.4) * z[50]
	dt[51] = np.sqrt(0.9) * z[1] + np.sqrt(0.1) * z[51]
	dt[52] = z[2] + 0.01 * z[52]
	dt[54] += 0.5 * dg[0]  # de effects: moderate, strong, very strong
	dt[55] += 3.0 * dg[1]
	dt[56] += 8.0 * dg[2]
	dt += rng.uniform(1, 5, size=(NG, 1)) + rng.normal(size=(NG, 3)) @ dc[:3] * 0.3  # means and covariate effects
	dt[PLANTED['constant']] = 0.0
	dt = dt.astype(np.float32)
	dt[DUP[1]] = dt[DUP[0]]
	return dt, dc, dg


def residualize_ld(x, dc):
	"""x - (x C^T)(C C^T)^+ C in longdouble from the fp64 pseudo-inverse the library's host side computes, applied twice (the second pass removes what the
	rounding of that inverse left)."""
	import sys
	sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
	from normalisr_amd.association import _prepare_covariates
	c64, dci, rank = _prepare_covariates(dc)
	C, D = c64.astype(LD), np.asarray(dci).astype(LD)
	x = np.asarray(x).astype(LD)
	res = x
	for _ in range(2):
		res = res - (res @ C.T) @ D.T @ C
	return res, (res * res).sum(axis=1), int(rank)


CUT = 300  # the same problem on its first 300 cells: below the 2048 cells from which the integer engine runs


def expected(dt, dc, dg):
	"""ln P of coex (genes x genes, -inf on the diagonal) and de (design rows x genes) of one problem, with the R^2 they come from, dof and |y~|^2."""
	ng, n = dt.shape
	ry, ssy, rank = residualize_ld(dt, dc)
	rx, ssx, _ = residualize_ld(dg, dc)
	dof = n - 1 - rank
	assert rank == 4
	vy = np.where(ssy == 0, LD(n), ssy)  # variance 0 -> 1
	vx = np.where(ssx == 0, LD(n), ssx)
	r2c = ((ry @ ry.T)**2 / np.outer(vy, vy)).astype(np.float64)
	r2d = ((rx @ ry.T)**2 / np.outer(vx, vy)).astype(np.float64)
	coex = np.full((ng, ng), -np.inf)
	for i in range(ng):
		for j in range(i + 1, ng):
			coex[i, j] = coex[j, i] = float(lnp_exact(r2c[i, j], dof))
	de = np.array([[float(lnp_exact(r2d[i, j], dof)) for j in range(ng)] for i in range(dg.shape[0])])
	return coex, de, r2c, r2d, dof, ssy


def make_case():
	dt, dc, dg = case_inputs()
	coex, de, r2c, r2d, dof, ssy = expected(dt, dc, dg)
	coex_cut, de_cut, r2c_cut, _, dof_cut, _ = expected(dt[:, :CUT], dc[:, :CUT], dg[:, :CUT])
	assert dof_cut == CUT - 5 and (dg[:, :CUT].sum(axis=1) >= 5).all() and r2c_cut[DUP] > 1 - 1e-12
	# what the genes hold by construction
	for key, lo, hi in (('r2_06', 0.5, 0.7), ('r2_09', 0.85, 0.95)):
		i, j = PLANTED[key]
		assert lo < r2c[i, j] < hi, (key, r2c[i, j])
		assert np.exp(coex[i, j]) == 0.0 and coex[i, j] < -745.2 and np.isfinite(coex[i, j])  # the linear P-value is exactly 0 in double precision
	i, j = PLANTED['near_one']
	assert 0.5e-4 < 1 - r2c[i, j] < 2e-4, 1 - r2c[i, j]
	c = PLANTED['constant']
	assert ssy[c] == 0 and (np.delete(coex[c], c) == 0).all() and (de[:, c] == 0).all()
	assert r2c[DUP] > 1 - 1e-12
	off = ~np.eye(NG, dtype=bool)
	null = (coex > -3) & off
	moderate = (coex < -5) & (coex > -200)
	assert null.sum() > 1000 and moderate.sum() >= 10
	assert (np.exp(de) == 0).any() and ((de < -5) & (de > -200)).any()
	out = os.path.join(HERE, 'G25_logp_case.npz')
	np.savez_compressed(out, dt=dt, dc=dc, dg=dg, lnp_coex=coex, lnp_de=de, dof=np.int64(dof), dup=np.array(DUP),
						planted_pairs=np.array([PLANTED['r2_06'], PLANTED['r2_09'], PLANTED['near_one']]), constant=np.int64(c),
						r2_coex=r2c, r2_de=r2d, cut=np.int64(CUT), lnp_coex_cut=coex_cut, lnp_de_cut=de_cut,
						# ln P at 1 - R^2 = 1e-6 for the two dofs: what the duplicate pair, whose R^2 rounding decides, has to stay below
						lnp_dup_bound=np.array([float(lnp_exact(1 - 1e-6, dof)), float(lnp_exact(1 - 1e-6, dof_cut))]))
	print(out, os.path.getsize(out), 'bytes; finite ln P from', coex[np.isfinite(coex)].min())


if __name__ == '__main__':
	self_check()
	make_grid()
	make_case()
