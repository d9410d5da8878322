"""CPU: compute_var and normvar with more than 63 covariates -- the fixture G22 (tests/golden/make_g22.py: what the reference returned for one-hot
covariates built like its co-expression example's) against the oracle and the numpy restatements the GPU tests lean on, the basis and rank certificate of
normalisr_amd.norm._wide_basis, and the argument checks that come before any device call.  Bound: close(1e-9, floor=1), the project's bound for the front half."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, relerr

import front_numpy
import normvar_wide_numpy as wide

CASES = {'A': (113, 106), 'B': (384, 377), 'C': (70, 70)}


def close(a, b, rtol=1e-9, floor=1.0):
	return relerr(a, b, floor) < rtol


@pytest.fixture(scope='module')
def g22(golden):
	g = golden('G22_wide_covariates')
	return {c: {k: g['%s_%s' % (c, k)] for k in ('dt', 'dc', 'wt', 'w1', 'w3', 'nv', 'dcn', 'ranks')} for c in CASES}


@pytest.mark.parametrize('case', sorted(CASES))
def test_oracle_and_restatements_against_the_reference(g22, case):
	import oracle
	d = g22[case]
	dt, dc = d['dt'].astype(np.float64), d['dc']
	assert d['dt'].dtype == np.float32 and dc.shape[0] == CASES[case][0] and (d['ranks'] == CASES[case][1]).all()
	assert (d['wt'] == 0).sum() == 1 and (d['wt'] == 1).sum() == 1
	for steps, key in ((1, 'w1'), (3, 'w3')):
		w = front_numpy.compute_var(dt, dc, stepmax=steps)
		print(case, 'compute_var stepmax', steps, relerr(w, d[key], 1.0))
		assert close(w, d[key])
	got = oracle.normvar(dt, dc, d['w3'], d['wt'])
	print(case, 'oracle.normvar', relerr(got[0], d['nv'], 1.0))
	assert close(got[0], d['nv']) and close(got[1], d['dcn'])
	mine = wide.normvar(dt, dc, d['w3'], d['wt'])
	print(case, 'basis form', relerr(mine, d['nv'], 1.0), np.abs(mine - d['nv']).max() / np.abs(d['nv']).max())
	assert close(mine, d['nv'])


def test_basis_and_certificate(g22):
	"""_wide_basis: the rank of inv_rank's rule, orthonormal rows that span the covariates, and a certificate that holds for the fixture's covariates and is
	refused for a nearly duplicated row (an eigenvalue inside the forbidden band) and for weights that span four decades."""
	from normalisr_amd import norm
	rng = np.random.default_rng(2210)
	for case, (nc, rank) in CASES.items():
		d = g22[case]
		b, r, ok, gaps = norm._wide_basis(d['dc'], d['w3'], d['wt'])
		assert r == rank and ok and b.shape == (rank, d['dc'].shape[1])
		assert np.abs(b @ b.T - np.eye(r)).max() < 1e-10
		proj = b.T @ (b @ d['dc'].T)  # the rows of dc lie in the span of B
		assert np.abs(proj.T - d['dc']).max() < 1e-8 * np.abs(d['dc']).max()
		bn, rn, _ = wide.basis(d['dc'])
		assert rn == r
		hi, lo, kappa = gaps
		assert hi >= norm.WIDE_SAFETY * 1e-8 * kappa and lo < 1e-8 / (norm.WIDE_SAFETY * kappa)
		# a nearly duplicated row, row + eps noise: the new direction has the eigenvalue |eps noise_perp|^2 / 2, about eps^2 n / 2, against lambda_1 of a few n.
		# eps = 1e-4 puts it at 1e-9 .. 1e-8 of lambda_1, inside the forbidden band (tol / (c kappa), c tol kappa): neither kept for sure nor dropped for
		# sure, no certificate.  eps = 1e-6 puts it near 1e-13, below the band: dropped for sure in every gene, the certificate stands and the rank is unchanged.
		noise = rng.normal(size=d['dc'].shape[1])
		_, rd, okd, gd = norm._wide_basis(np.vstack([d['dc'], d['dc'][-2] + 1e-4 * noise]), d['w3'], d['wt'])
		assert not okd and 1e-8 / (norm.WIDE_SAFETY * kappa) <= (gd[0] if rd == r + 1 else gd[1]) < norm.WIDE_SAFETY * 1e-8 * kappa
		_, rd, okd, gd = norm._wide_basis(np.vstack([d['dc'], d['dc'][-2] + 1e-6 * noise]), d['w3'], d['wt'])
		assert okd and rd == r and 0 < gd[1] < 1e-8 / (norm.WIDE_SAFETY * kappa)
		# weights over four decades: kappa = 1e8 for the gene with wt = 1
		wbig = np.exp(rng.uniform(0, np.log(1e4), d['w3'].shape[0]))
		wbig[0], wbig[1] = 1.0, 1e4
		assert not norm._wide_basis(d['dc'], wbig, d['wt'])[2]
		assert norm._wide_basis(d['dc'], wbig, np.zeros_like(d['wt']))[2]  # (wt = 0 everywhere: e = 1, kappa = 1)


def test_reference_fallback_in_numpy(g22):
	"""The per-gene algorithm normvar falls back to without a certificate is the reference's (host numpy: no device)."""
	from normalisr_amd import norm
	d = g22['A']
	got = norm._normvar_wide_reference(d['dt'][:5], d['dc'], d['w3'], d['wt'][:5], True)
	assert close(got, d['nv'][:5])


def test_symbols_and_argument_checks():
	from normalisr_amd import _lib, norm
	header = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	for name in ('nrm_wide_covariates', 'nrm_normvar_pairs', 'nrm_normvar_chol', 'nrm_gram_f64_whole'):
		assert re.search(r'\b%s\(' % name, header) and name in _lib.exported_symbols()
	assert 'norm.py:154-163' in header
	lim = norm.wide_covariates()
	assert lim == 1024 and not re.search(r'\b1024\b', open(os.path.join(ROOT, 'normalisr_amd', 'norm.py')).read().split('def _check_wide')[1].split('def ')[0])
	y = np.ones((5, 20))
	for call in (lambda c: norm.compute_var(np.ones((5, c.shape[1])), c), lambda c: norm.normvar(np.ones((5, c.shape[1])), c, np.ones(c.shape[1]), np.ones(5))):
		with pytest.raises(NotImplementedError, match='more cells than covariates'):
			call(np.ones((64, 20)))
		with pytest.raises(NotImplementedError, match='more cells than covariates'):
			call(np.ones((64, 64)))
		with pytest.raises(NotImplementedError, match=str(lim)):
			call(np.ones((lim + 1, lim + 50)))
	for key in ('nv_panel_rows', 'nv_gene_block'):
		from normalisr_amd import _opts
		assert key in _opts.DEBUG_KEYS
