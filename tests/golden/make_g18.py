#!/usr/bin/env python3
"""Generate tests/golden/G18_front.npz and G18_front_chain.npz by IMPORTING the reference (dev container only, like make_g17.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g18.py

The front half of the pipeline -- lcpm, scaling_factor, normcov, compute_var -- and the chain's end (normvar, coex) on one seeded count matrix:
Poisson counts with log-normal gene means and cell depths (about 60 % zeros, one gene far above 255 reads), four one-hot batches.  Arrays only:
the inputs and what the reference returned for them; scipy's digamma / trigamma at the arguments of lcpm's table.  Two files, each below 1 MB.
"""
import os
import sys
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')

import normalisr.normalisr as norm  # noqa: E402
from scipy.special import digamma, polygamma  # noqa: E402


def counts(rng, ng, n):
	mu = np.exp(rng.normal(-1.2, 1.3, ng))
	mu[3] = 400.0  # one gene whose counts do not fit a byte
	depth = np.exp(rng.normal(0.0, 0.5, n))
	x = rng.poisson(mu[:, None] * depth[None, :])
	x = x[(x != 0).sum(axis=1) >= 5]
	assert (x.sum(axis=0) > 0).all() and x.max() > 255
	return x.astype(np.int64)


def main():
	import logging
	logging.disable(logging.WARNING)
	rng = np.random.default_rng(18)
	n = 240
	reads = counts(rng, 112, n)
	ng = reads.shape[0]
	batch = rng.integers(0, 4, n)
	onehot = (batch[None, :] == np.arange(4)[:, None]).astype(np.float64)
	a = dict(reads=reads.astype(np.int32), batch=batch, zero_fraction=(reads == 0).mean())
	b = {}
	lc, mean, var, cov = norm.lcpm(reads)
	assert mean is None and var is None
	a.update(lcpm=lc, cov=cov)
	lc2, mean2, var2, cov2 = norm.lcpm(reads, lowmem=False)
	b.update(lowmem_lcpm_equal=np.array_equal(lc2, lc), lowmem_mean=mean2, lowmem_var=var2)
	lc3, _, _, cov3 = norm.lcpm(reads, normalize=False)
	a.update(nonorm_lcpm=lc3, nonorm_cov=cov3)
	lc4, _, _, cov4 = norm.lcpm(reads, ntot=1E9)
	a.update(ntot_lcpm=lc4, ntot_cov=cov4)
	lc5, _, _, cov5 = norm.lcpm(reads, nocov=True)
	assert cov5 is None
	b.update(nocov_lcpm=lc5)
	a.update(sf=norm.scaling_factor(reads), sf_logtpropmean_min=norm.scaling_factor(reads, varname='logtpropmean', v0='min'),
			 sf_log1m_min=norm.scaling_factor(reads, varname='log1-nt0mean', v0='min'))
	raw = np.vstack([onehot, cov])
	dc = norm.normcov(raw)
	b.update(cov_raw=raw, normcov_c=dc, normcov_noc=norm.normcov(raw, c=False))
	b.update(w1=norm.compute_var(lc, dc), w3=norm.compute_var(lc, dc, stepmax=3))
	nv = norm.normvar(lc, dc, b['w1'], a['sf'])
	b.update(nv_exp=nv[0], nv_cov=nv[1])
	p, dot, v = norm.coex(nv[0], nv[1])
	b.update(coex_p=p, coex_dot=dot, coex_var=v)
	# scipy at the table's arguments and at several t0
	xs = np.concatenate([np.arange(0, 2000), np.unique(np.round(np.geomspace(2000, 2**24 - 1, 400)).astype(np.int64))])
	t0 = np.array([3.0, 7.0, 11.5, 12.0, 1E3, 12345.0, 1E5, 1E6 + 2, 1E7, 1E8, 1E9 + 2, 1E10, 1E11, 1E12, float(reads.sum() + 2)])
	a.update(psi_x=xs, psi_digamma=digamma(1.0 + xs), psi_trigamma=polygamma(1, 1.0 + xs), psi_t0=t0, psi_t0_digamma=digamma(t0), psi_t0_trigamma=polygamma(1, t0))
	np.savez_compressed(os.path.join(HERE, 'G18_front.npz'), **a)
	np.savez_compressed(os.path.join(HERE, 'G18_front_chain.npz'), **b)
	for f in ('G18_front.npz', 'G18_front_chain.npz'):
		print(f, os.path.getsize(os.path.join(HERE, f)), 'bytes')
	print('genes', ng, 'cells', n, 'zeros', a['zero_fraction'], 'max', reads.max())


if __name__ == '__main__':
	main()
