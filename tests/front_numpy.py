"""numpy restatements of lcpm, scaling_factor and compute_var -- TEST INFRASTRUCTURE ONLY.

Written from the mathematics (the header of include/normalisr_hip.h names the reference lines), in fp64 numpy with scipy's digamma: the independent
check for random shapes on the GPU, itself pinned against what the reference returned (tests/golden/G18_front*.npz, tests/test_front_cpu.py).
"""
import numpy as np


def lcpm(reads, normalize=True, ntot=None, nocov=False):
	"""(lcpm, cov): lcpm[g,k] = T[x_gk] - ln sum_g exp(T[x_gk]) + ln 1e6 with T[x] = psi(1 + x) - psi(sum(x) + 2)."""
	from scipy.special import digamma
	x = np.asarray(reads).astype(np.int64)
	t0 = float(x.sum() + 2) if ntot is None else ntot + 2
	tab = digamma(1.0 + np.arange(int(x.max()) + 1)) - digamma(t0)
	out = tab[x]
	if normalize:
		out = out - (np.log(np.exp(out).sum(axis=0)) - np.log(1E6))
	cov = None
	if not nocov:
		tot = np.log(x.sum(axis=0))
		cov = np.array([tot, x.shape[0] - (x != 0).sum(axis=0), tot**2])
	return out, cov


def scaling_factor(reads):
	d = (np.asarray(reads) == 0).mean(axis=1)
	return d / d.max()


def _project(x, z):
	"""The orthogonal projection of the rows of z onto the row space of x (pseudo-inverse: any rank)."""
	return z @ np.linalg.pinv(x, rcond=1E-10) @ x


def compute_var(dt, dc, stepmax=1, eps=1E-6):
	"""The per-cell weights: two orthogonal projections per step (the gene rows onto the weighted covariates, the per-cell log-RMS onto span(dc, 1))."""
	dt, dc = np.asarray(dt, dtype=np.float64), np.asarray(dc, dtype=np.float64)
	ns = dt.shape[1]
	c1 = np.vstack([dc, np.ones((1, ns))])
	s = np.ones(ns)
	best, bestv, n = None, 1E300, 0
	while n < stepmax and bestv > eps:
		y, c = dt / s, dc / s
		r = y - _project(c, y)
		r = (r.T - r.mean(axis=1)).T
		r = (r.T / np.sqrt((r**2).mean(axis=1))).T
		z = np.log(np.sqrt((r**2).mean(axis=0)))
		new = np.exp(_project(c1, z[None, :])[0]) * s
		new /= new.min()
		t1 = np.abs((new - s) / s).max()
		s = new
		n += 1
		if t1 < bestv:
			bestv, best = t1, s
	w = 1 / best
	return w / w.min()
