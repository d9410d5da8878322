"""CPU: the rank certificate that lets single=4 take its closed form for rank-deficient covariates (single4.pinv_rank_certificate and its
spectrum form) against the reference's own per-grouping ranks -- oracle.inv_rank on every T_i, A A^T without row and column i
(association.py:521-530) -- on seeded designs, near the threshold included.  The certificate may refuse a design whose ranks are all
nx - 1 + rc; it must never accept one where any grouping's rank differs."""
import numpy as np
import pytest

import oracle
from normalisr_amd.single4 import _pinv_rank_spectrum, pinv_rank_certificate

TOL = 1E-8


def cert_inputs(x, c, tol=TOL):
	"""What the device's closed form hands the certificate, in numpy: ||M~||_1, ||N~||_1, b_x, |x~_i|^2 (rows residualised with inv_rank's
	pseudo-inverse of C C^T)."""
	mcc = c @ c.T
	dci, rc = oracle.inv_rank(mcc, tol=tol)
	b = (x @ c.T) @ dci
	xt = x - b @ c
	mt = xt @ xt.T
	try:
		ninv = np.linalg.inv(mt)
		norm_ninv = float(np.abs(ninv).sum(axis=0).max())
	except np.linalg.LinAlgError:
		norm_ninv = np.inf
	return (float(np.abs(mt).sum(axis=0).max()), norm_ninv, b, (xt * xt).sum(axis=1)), mcc, rc


def reference_ranks(x, c, tol=TOL):
	a = np.vstack([x, c])
	m = a @ a.T
	k = a.shape[0]
	return np.array([oracle.inv_rank(m[np.ix_([j for j in range(k) if j != i], [j for j in range(k) if j != i])], tol=tol)[1] for i in range(x.shape[0])])


def decide(x, c, tol=TOL):
	"""(norm certificate, spectrum certificate, reference ranks, rc)."""
	cert, mcc, rc = cert_inputs(x, c, tol)
	a = np.vstack([x, c])
	ev = np.linalg.eigvalsh(a @ a.T)
	return pinv_rank_certificate(*cert, mcc, tol), _pinv_rank_spectrum(ev, mcc, tol), reference_ranks(x, c, tol), rc


def onehot(rng, n, nbatch=4, ncont=3):
	batch = rng.integers(0, nbatch, n)
	oh = (batch[None, :] == np.arange(nbatch)[:, None]).astype(np.float64)
	cont = rng.normal(size=(ncont, n))
	return np.vstack([oh, cont, np.ones((1, n))])


def test_g17_onehot_design_is_certified(golden):
	g = golden('G17_single4_onehot')
	by_norms, by_spectrum, ranks, rc = decide(g['dg'], g['dc'])
	nx = g['dg'].shape[0]
	assert rc == int(g['rc']) == g['dc'].shape[0] - 1
	assert (ranks == nx - 1 + rc).all()
	assert by_norms and by_spectrum


def test_g17_batch_indicator_grouping_is_refused(golden):
	g = golden('G17_single4_onehot')
	by_norms, by_spectrum, ranks, rc = decide(g['bi_dg'], g['dc'])
	assert not (ranks == g['bi_dg'].shape[0] - 1 + rc).all()
	assert not by_norms and not by_spectrum


def _designs():
	"""Seeded designs: sparse groupings against one-hot covariates, groupings and covariates brought towards the threshold at several scales."""
	out = []
	for seed in range(6):
		rng = np.random.default_rng(900 + seed)
		n, nx = int(rng.integers(150, 400)), int(rng.integers(4, 20))
		c = onehot(rng, n, nbatch=int(rng.integers(2, 5)), ncont=int(rng.integers(0, 3)))
		x = (rng.random((nx, n)) < 0.15).astype(np.float64)
		out.append(('plain%d' % seed, x, c))
		# a grouping moved towards a batch indicator: from clearly independent to inside the covariates' span
		for eps in (1e-1, 1e-3, 1e-4, 3e-5, 1e-5, 1e-6, 0.0):
			xe = x.copy()
			xe[0] = c[0] + eps * rng.normal(size=n)
			out.append(('near_span%d_%g' % (seed, eps), xe, c))
		# two groupings nearly equal
		for eps in (1e-3, 3e-5, 1e-6):
			xe = x.copy()
			xe[1] = x[2] + eps * rng.normal(size=n)
			out.append(('near_pair%d_%g' % (seed, eps), xe, c))
		# a covariate nearly a copy of another: its kept eigenvalue of C C^T from 100x down to below tol x the largest
		lam1 = np.linalg.eigvalsh(c @ c.T)[-1]
		z = rng.normal(size=n)
		z -= c.T @ np.linalg.lstsq(c.T, z, rcond=None)[0]
		z /= np.linalg.norm(z)
		for f in (1e2, 8.0, 4.0, 2.5, 1.5, 1.0, 0.6, 0.3, 0.1):
			cn = np.vstack([c, c[-2] + np.sqrt(2.0 * f * TOL * lam1) * z])
			out.append(('near_cov%d_%g' % (seed, f), x, cn))
	return out


@pytest.mark.parametrize('name,x,c', _designs(), ids=lambda v: v if isinstance(v, str) else '')
def test_certificate_never_accepts_a_wrong_rank(name, x, c):
	by_norms, by_spectrum, ranks, rc = decide(x, c)
	nx = x.shape[0]
	if by_norms or by_spectrum:
		assert (ranks == nx - 1 + rc).all(), (name, ranks, nx - 1 + rc, by_norms, by_spectrum)
	if by_norms:
		assert by_spectrum, name  # (the norms bound what the spectrum states)
	if name.startswith('plain'):
		assert by_norms, name


def test_certificate_count():
	"""The seeded designs reach both sides: accepted, refused with the reference's ranks off, refused although they hold."""
	acc = wrong = 0
	for name, x, c in _designs():
		by_norms, by_spectrum, ranks, rc = decide(x, c)
		acc += bool(by_spectrum)
		wrong += not (ranks == x.shape[0] - 1 + rc).all()
	assert acc >= 30 and wrong >= 6, (acc, wrong)
