"""Inputs of golden G23, rebuilt from a seed on either side (as g14_inputs.py): two co-expression problems whose covariates grow row by row.
  A  48 genes x 700 cells        B  24 genes x 30 000 cells
Each: covariates as the reference's normcov returns them for a three-level factor (one-hot) and four continuous columns -- 8 rows with the intercept, of rank 7 --
and four rows to append in order: latent factor 0, latent factor 1, a combination of covariates and the two rows before it (in the span), latent factor 2.  The
ranks of the cumulative sets are 7, 8, 9, 9, 10.  The expression, rounded to fp32, is loadings x factors + covariate effects + noise + 3; gene 1 keeps 1 % of its
variance once factor 1 is removed, gene 2 has a mean 1000 times its spread.  G23 keeps the reference's coex on every cumulative set and check sums of these inputs."""
import numpy as np

CASES = dict(A=(2301, 48, 700), B=(2302, 24, 30000))
RANKS = (7, 8, 9, 9, 10)


def raw_covariates(rng, n):
	f = rng.integers(0, 3, n)
	f[:3] = np.arange(3)
	onehot = (f[None, :] == np.arange(3)[:, None]).astype(np.float64)
	cont = np.array([rng.standard_normal(n), 100 + 30 * rng.standard_normal(n), 0.05 + 0.01 * rng.standard_normal(n), rng.standard_normal(n)**2])
	return np.concatenate([onehot, cont])


def normcov(raw):
	"""What the reference's normcov does to these rows (norm.py:39-54): continuous rows to zero mean and unit mean square, binary rows as they are, an intercept."""
	out = np.array(raw, dtype=np.float64)
	cont = ((out != 0) & (out != 1)).any(axis=1)
	c = out[cont].T - out[cont].mean(axis=1)
	out[cont] = (c / np.sqrt((c**2).mean(axis=0))).T
	return np.concatenate([out, np.ones((1, out.shape[1]))])


def g23_inputs(name):
	"""(dt fp32 (genes, cells), dc (8, cells), rows (4, cells), raw covariates (7, cells))."""
	seed, ng, n = CASES[name]
	rng = np.random.default_rng(seed)
	raw = raw_covariates(rng, n)
	dc = normcov(raw)
	fac = rng.standard_normal((3, n))
	rows = np.array([fac[0] + 0.1 * rng.standard_normal(n), fac[1], np.zeros(n), fac[2] + 0.3 * rng.standard_normal(n)])
	rows[2] = 0.5 * dc[4] - 2.0 * rows[0] + 3.0 * dc[7] + 0.25 * rows[1]
	load = rng.standard_normal((ng, 3)) * (rng.random((ng, 3)) < 0.5)
	beta = 0.3 * rng.standard_normal((ng, 8))
	dt = load @ fac + beta @ dc + rng.standard_normal((ng, n)) + 3.0
	dt[1] = 10.0 * fac[1] + rng.standard_normal(n) + 3.0
	dt[2] = 1000.0 + rng.standard_normal(n) + 0.5 * fac[0]
	return dt.astype(np.float32), dc, rows, raw


def checksum(a):
	a = np.asarray(a, dtype=np.float64)
	return np.array([a.sum(), np.abs(a).sum(), (a * np.cos(np.arange(a.size).reshape(a.shape) % 1000)).sum()])
