#!/usr/bin/env python3
"""Generate tests/golden/G17_single4_onehot.npz by IMPORTING the reference (dev container only, like make_golden.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g17.py

single=4 (`normalisr de -m covariate`) with the covariates a high-MOI screen passes: one-hot batches and continuous covariates through the
reference's normcov, which appends the intercept -- the batch columns sum to it, so C C^T is rank deficient by one (nc = 8, rank 7).  Arrays
only: seeded inputs and what the reference returned for them.
"""
import os
import sys
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')

import normalisr.normalisr as norm  # noqa: E402
from normalisr.association import association_tests, inv_rank  # noqa: E402


def onehot_covariates(rng, n, nbatch=4, ncont=3):
	"""normcov([nbatch one-hot batch rows; ncont continuous rows]): the intercept appended by the reference."""
	batch = rng.integers(0, nbatch, n)
	oh = (batch[None, :] == np.arange(nbatch)[:, None]).astype(np.float64)
	cont = rng.normal(size=(ncont, n)) * np.array([[1.0], [3.0], [0.5]])[:ncont] + 2.0
	return norm.normcov(np.vstack([oh, cont])), batch


def main():
	rng = np.random.default_rng(17)
	nx, ny, n = 40, 60, 600
	dc, batch = onehot_covariates(rng, n)
	nc = dc.shape[0]
	dg = (rng.random((nx, n)) < 0.1).astype(np.float64)
	dt = rng.normal(size=(ny, n)) + 0.6 * (rng.normal(size=(ny, 4)) @ dg[:4]) + 0.4 * (rng.normal(size=(ny, nc)) @ dc)
	_, rc = inv_rank(dc @ dc.T)
	assert rc == nc - 1, rc
	out = dict(dg=dg, dt=dt, dc=dc, batch=batch, rc=rc)
	# norm.de: lowmem=False (alpha), return_dot=False inside de (de.py:99-105)
	p, g, a, vg, vt = norm.de(dg, dt, dc, single=4, lowmem=False)
	out.update(de_p=p, de_gamma=g, de_alpha=a, de_varg=vg, de_vart=vt)
	# association_tests with return_dot True and False
	for rd in (1, 0):
		p, d, a, vx, vy = association_tests(dg, dt, dc, single=4, lowmem=False, return_dot=bool(rd))
		out.update({'at%d_p' % rd: p, 'at%d_stat' % rd: d, 'at%d_vx' % rd: vx, 'at%d_vy' % rd: vy})
		if rd:  # (alpha does not depend on return_dot)
			out['at_alpha'] = a
	# one dimreduce per gene
	dr = rng.integers(0, 3, ny)
	p, g, a, vg, vt = norm.de(dg, dt, dc, single=4, dimreduce=dr)
	out.update(dr=dr, dr_p=p, dr_gamma=g, dr_varg=vg, dr_vart=vt)
	# dy=None: every pair of 14 rows given all the others and the covariates
	for rd in (1, 0):
		p, d, a, vx, vy = association_tests(dt[:14], None, dc, single=4, return_dot=bool(rd))
		out.update({'sx_p_rd%d' % rd: p, 'sx_dot_rd%d' % rd: d, 'sx_vy_rd%d' % rd: vy})
	# a grouping equal to a batch indicator: rank-deficient given C (the per-grouping algorithm)
	dgb = dg.copy()
	dgb[5] = dc[1]
	p, g, a, vg, vt = norm.de(dgb, dt, dc, single=4, lowmem=False)
	out.update(bi_dg=dgb, bi_p=p, bi_gamma=g, bi_alpha=a, bi_varg=vg, bi_vart=vt)
	# covariates whose smallest kept eigenvalue of C C^T sits within 4x of tol x the largest (one more covariate, nearly a copy of a continuous one)
	mcc = dc @ dc.T
	lam1 = np.linalg.eigvalsh(mcc)[-1]
	z = rng.normal(size=n)
	z -= dc.T @ np.linalg.lstsq(dc.T, z, rcond=None)[0]
	z /= np.linalg.norm(z)
	dcn = np.vstack([dc, dc[4] + np.sqrt(8e-8 * lam1) * z])
	ev = np.linalg.eigvalsh(dcn @ dcn.T)
	_, rcn = inv_rank(dcn @ dcn.T)
	assert rcn == nc and 1e-8 * ev[-1] <= ev[1] <= 4e-8 * ev[-1], (rcn, ev[:3] / ev[-1])
	p, g, a, vg, vt = norm.de(dg, dt, dcn, single=4)
	out.update(near_dc=dcn, near_p=p, near_gamma=g, near_varg=vg, near_vart=vt)
	path = os.path.join(HERE, 'G17_single4_onehot.npz')
	np.savez_compressed(path, **out)
	print('G17_single4_onehot.npz {:9.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
	main()
