#!/usr/bin/env python3
"""Generate tests/golden/G22_wide_covariates.npz by IMPORTING the reference (dev container only, like make_g21.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g22.py

compute_var and normvar with more than 63 covariates, built as the reference's co-expression example builds them (examples/GSE123139/code/prepare_raw.py:78-93:
every categorical column one-hot encoded, every level a row) and passed through the reference's normcov:
  A  24 genes x 700 cells, factor levels (40, 9, 40, 2, 4, 12, 2) + three continuous rows in units of 1, 30 and 0.01 + the intercept: 113 rows of rank 106
  B  8 genes x 1500 cells, the level counts of the example's `dysfunctional` subset (164, 164, 19, 25, 4, 2, 2) + the same: 384 rows of rank 377
  C  16 genes x 300 cells, 70 continuous covariates of full rank (69 + the intercept)
Per case: the expression (fp32-representable, stored as fp32), the covariates, wt with one 0 and one 1, the reference's compute_var for stepmax 1 and 3, and the
reference's normvar (w of stepmax 3) with its dcn and every gene's rank by the reference's inv_rank.  Gene 2 of every case has covariate effects that explain
99 % of its variance.  The script asserts that every gene's reference rank is the rank of the one basis and prints the two spectral gaps.  Arrays only; one
file, below 1 MB (the one-hot rows compress).
"""
import os
import sys
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')
sys.path.insert(0, os.path.dirname(HERE))

import normalisr.norm as refnorm  # noqa: E402
from normalisr.association import inv_rank as ref_inv_rank  # noqa: E402
import normvar_wide_numpy as wide  # noqa: E402


def one_hot_covariates(rng, n, levels):
	rows = []
	for lv in levels:
		f = rng.integers(0, lv, n)
		f[:lv] = np.arange(lv)  # every level present
		f = f[rng.permutation(n)]
		rows.append((f[None, :] == np.arange(lv)[:, None]).astype(float))
	cont = np.array([rng.normal(0, 1, n), rng.normal(100, 30, n), rng.normal(0.05, 0.01, n)])
	raw = np.concatenate(rows + [cont])
	dc = refnorm.normcov(raw)
	assert dc.shape == (sum(levels) + 4, n) and (dc[-1] == 1).all()
	return dc


def expression(rng, ng, dc, spread):
	"""noise whose spread varies from cell to cell (what compute_var fits) + covariate effects + 3, rounded to fp32; gene 2: effects explain 99 % of the variance."""
	n = dc.shape[1]
	cell = np.exp(spread * (0.6 * dc[-2] + 0.4 * rng.normal(0, 1, n)))
	beta = rng.normal(0, 0.5, (ng, dc.shape[0])) / np.sqrt(dc.shape[0] / 8)
	fit = beta @ dc
	noise = rng.normal(0, 1, (ng, n)) * cell
	noise[2] *= 0.1 * fit[2].std() / noise[2].std()
	return (fit + noise + 3.0).astype(np.float32)


def case(name, rng, ng, dc, out, rank):
	dt32 = expression(rng, ng, dc, 0.25)
	dt = dt32.astype(np.float64)
	wt = rng.uniform(0.05, 0.95, ng)
	wt[0], wt[1] = 0.0, 1.0
	w1 = refnorm.compute_var(dt, dc, stepmax=1)
	w3 = refnorm.compute_var(dt, dc, stepmax=3)
	nv, dcn = refnorm.normvar(dt, dc, w3, wt)
	b, r, lam = wide.basis(dc)
	assert r == rank, (name, r)
	ranks = np.empty(ng, dtype=np.int64)
	for g in range(ng):
		e = w3**wt[g] if wt[g] != 0 else np.ones_like(w3)
		ranks[g] = ref_inv_rank(np.matmul(dc * e, (dc * e).T))[1]
	assert (ranks == r).all(), (name, ranks)
	mine = wide.normvar(dt, dc, w3, wt)
	err = float(np.abs(mine - nv).max() / np.abs(nv).max())
	explained = 1 - np.var(dt[2] - (np.linalg.lstsq(dc.T, dt[2], rcond=None)[0] @ dc)) / np.var(dt[2])
	print('{}: {} genes x {} cells, {} covariates of rank {}; lambda_r/lambda_1 = {:.3g}, lambda_r+1/lambda_1 = {:.3g}; w3 in [1, {:.3g}]; basis form against the '
		  'reference {:.3g} of the scale; gene 2 explained {:.4f}'.format(name, ng, dc.shape[1], dc.shape[0], r, lam[r - 1] / lam[0], (lam[r] / lam[0]) if r < len(lam) else 0.0,
																		  w3.max(), err, explained))
	assert err < 1e-11 and explained > 0.985
	for k, v in (('dt', dt32), ('dc', dc), ('wt', wt), ('w1', w1), ('w3', w3), ('nv', nv), ('dcn', dcn), ('ranks', ranks)):
		out[name + '_' + k] = v


def main():
	import logging
	logging.disable(logging.WARNING)
	out = {}
	rng = np.random.default_rng(2201)
	case('A', rng, 24, one_hot_covariates(rng, 700, (40, 9, 40, 2, 4, 12, 2)), out, 106)
	case('B', rng, 8, one_hot_covariates(rng, 1500, (164, 164, 19, 25, 4, 2, 2)), out, 377)
	n = 300
	units = 10.0**rng.integers(-2, 3, 69)
	dcc = refnorm.normcov(rng.normal(0, 1, (69, n)) * units[:, None] + units[:, None])
	assert dcc.shape == (70, n)
	case('C', rng, 16, dcc, out, 70)
	path = os.path.join(HERE, 'G22_wide_covariates.npz')
	np.savez_compressed(path, **out)
	print(os.path.basename(path), os.path.getsize(path), 'bytes')
	assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
	main()
