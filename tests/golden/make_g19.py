#!/usr/bin/env python3
"""Generate tests/golden/G19_lcpm_sparse.npz by IMPORTING the reference (dev container only, like make_g18.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g19.py

lcpm called WITH A scipy.sparse MATRIX, and scaling_factor of the dense array, on two seeded count matrices: `lo` below 1 % stored entries, so that the
reference takes its own sparse branch (lcpm.py:118), and `hi` around 10 % with one gene whose counts do not fit a byte; every cell has a read.  Arrays
only: the counts and what the reference returned for them (default, normalize=False, ntot=1E9, nocov=True, lowmem=False).  One file, below 1 MB.
"""
import os
import sys
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')

import normalisr.normalisr as norm  # noqa: E402
import scipy.sparse  # noqa: E402


def counts(rng, ng, n, mean, sd, big):
	mu = np.exp(rng.normal(mean, sd, ng))
	if big:
		mu[3] = 400.0  # one gene whose counts do not fit a byte
	x = rng.poisson(mu[:, None] * np.exp(rng.normal(0.0, 0.5, n))[None, :])
	empty = x.sum(axis=0) == 0
	x[rng.integers(0, ng, n)[empty], np.nonzero(empty)[0]] = 1  # every cell has a read
	return x.astype(np.int64)


def main():
	import logging
	logging.disable(logging.WARNING)
	rng = np.random.default_rng(19)
	out = {}
	for name, x in (('lo', counts(rng, 300, 400, -7.2, 1.5, False)), ('hi', counts(rng, 160, 260, -3.2, 1.3, True))):
		dens = (x != 0).mean()
		s = scipy.sparse.csr_matrix(x)
		lc, mean, var, cov = norm.lcpm(s)
		assert mean is None and var is None and lc.shape == x.shape
		out.update({name + '_reads': x.astype(np.int32), name + '_density': dens, name + '_lcpm': lc, name + '_cov': cov})
		lc2, mean2, var2, _ = norm.lcpm(s, lowmem=False)
		out.update({name + '_lowmem_lcpm_equal': np.array_equal(lc2, lc), name + '_lowmem_mean_equal': np.array_equal(mean2, lc),
					name + '_lowmem_var_zero': bool((var2 == 0).all() and var2.shape == x.shape)})
		lc3, _, _, cov3 = norm.lcpm(s, normalize=False)
		out.update({name + '_nonorm_lcpm': lc3, name + '_nonorm_cov': cov3})
		lc4, _, _, cov4 = norm.lcpm(s, ntot=1E9)
		out.update({name + '_ntot_lcpm': lc4, name + '_ntot_cov': cov4})
		lc5, _, _, cov5 = norm.lcpm(s, nocov=True)
		assert cov5 is None
		out[name + '_nocov_lcpm'] = lc5
		out[name + '_sf'] = norm.scaling_factor(x)
		# the reference's own agreement between its sparse and dense inputs, for the record
		print(name, x.shape, 'density %.4f' % dens, 'max', x.max(), 'sparse vs dense input: %.3g' % np.abs(lc - norm.lcpm(x)[0]).max())
	assert out['lo_density'] < 0.01 and 0.05 < out['hi_density'] < 0.2 and out['hi_reads'].max() > 255
	f = os.path.join(HERE, 'G19_lcpm_sparse.npz')
	np.savez_compressed(f, **out)
	print(os.path.basename(f), os.path.getsize(f), 'bytes')


if __name__ == '__main__':
	main()
