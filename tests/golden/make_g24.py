#!/usr/bin/env python3
"""Generate tests/golden/g24.npz by IMPORTING the reference (dev container only, like make_g23.py), whose package is found through PYTHONPATH:

    PYTHONPATH=<reference>/src python3 tests/golden/make_g24.py

single=1 with more than 8 covariates: the reference's own association_tests(dx, dy, dc, single=1, lowmem=False, return_dot=False) on 7 groupings x 11 genes x
600 cells (a 0/1 design at low MOI: two cells in five carry one grouping, one in twenty carries two and is used by nobody) for two covariate sets --

    c12   6 one-hot batches + 5 continuous covariates + the intercept: rank 11 wherever a grouping's cells meet every batch
    c32   31 continuous covariates + the intercept: full rank

The script prints the ranks by the reference's inv_rank per grouping.  Arrays only (inputs and results), one file, below 1 MB.
"""
import os
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))

from normalisr.association import association_tests as ref_tests  # noqa: E402
from normalisr.association import inv_rank as ref_inv_rank  # noqa: E402

NX, NY, N = 7, 11, 600


def inputs():
	rng = np.random.default_rng(24)
	dx = np.zeros((NX, N))
	kind = rng.random(N)
	for k in range(N):
		if kind[k] < 0.4:
			dx[rng.integers(NX), k] = 1
		elif kind[k] < 0.45:
			dx[rng.choice(NX, 2, replace=False), k] = 1
	batch = rng.integers(6, size=N)
	onehot = (batch[None] == np.arange(6)[:, None]).astype(float)
	c12 = np.concatenate([onehot, rng.normal(size=(5, N)), np.ones((1, N))])
	c32 = np.concatenate([rng.normal(size=(31, N)), np.ones((1, N))])
	dy = rng.normal(size=(NY, N)) + 0.3 * c12[6:8].sum(axis=0) + 0.5 * dx[:NY % NX + 1].sum(axis=0)
	dy[3] += 2.0 * dx[2]  # a planted pair
	return dx, dy, dict(c12=c12, c32=c32)


def main():
	import logging
	logging.disable(logging.WARNING)
	dx, dy, covs = inputs()
	out = dict(dx=dx, dy=dy)
	sel = dx == dx.sum(axis=0)
	for name, dc in covs.items():
		ranks = [int(ref_inv_rank(dc[:, s] @ dc[:, s].T)[1]) for s in sel]
		print(name, 'cells per grouping', sel.sum(axis=1).tolist(), 'ranks', ranks)
		p, gamma, alpha, varx, vary = ref_tests(dx, dy, dc, single=1, lowmem=False, return_dot=False)
		out[name + '_dc'] = dc
		out[name + '_rank'] = np.array(ranks)
		for key, v in (('p', p), ('gamma', gamma), ('alpha', alpha), ('varx', varx), ('vary', vary)):
			out['{}_{}'.format(name, key)] = np.asarray(v)
	path = os.path.join(HERE, 'g24.npz')
	np.savez_compressed(path, **out)
	print(os.path.basename(path), os.path.getsize(path), 'bytes')
	assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
	main()
