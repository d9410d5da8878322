"""GPU: the pipeline's front half on the device -- lcpm (+ scaling_factor), compute_var -- against what the reference returned for golden G18
(tests/golden/make_g18.py) and, for seeded random shapes, against the numpy restatements of tests/front_numpy.py (themselves pinned to G18 in
tests/test_front_cpu.py).  Tolerances: integers exact; lcpm, covariates, weights and normvar's output close(1e-9, floor=1) -- the project's bound for
fp64 quantities that are not P-values, absolute near zero because logCPM and standardised covariates are O(1) and pass through zero; scaling factors
1e-12 absolute; P-values p_close (1e-6); fp32 output equal to the fp64 result rounded once."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

import front_numpy
from test_gpu_parity import close, p_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ok(a, b):
	return close(a, b, 1e-9, floor=1.0)


@pytest.fixture(scope='module')
def norm():
	import normalisr_amd.normalisr as norm
	return norm


@pytest.fixture(scope='module')
def torch():
	import torch
	return torch


def _inputs(torch, reads):
	"""The same counts as every input form lcpm takes."""
	return {
		'int64': reads.astype(np.int64), 'int32': reads.astype(np.int32), 'uint16': reads.astype(np.uint16), 'float64': reads.astype(np.float64),
		'dev_int32': torch.as_tensor(reads.astype(np.int32)).cuda(), 'dev_int64': torch.as_tensor(reads.astype(np.int64)).cuda(),
		'dev_int16': torch.as_tensor(reads.astype(np.int16)).cuda(),
		'sparse_csr': scipy.sparse.csr_matrix(reads), 'sparse_coo_float': scipy.sparse.coo_matrix(reads.astype(np.float64)),
	}


def _host(a):
	return a.cpu().numpy() if hasattr(a, 'is_cuda') else a


def test_g18_lcpm_every_variant(golden, norm, torch):
	g, h = golden('G18_front'), golden('G18_front_chain')
	reads = g['reads']
	for name, x in _inputs(torch, reads).items():
		for device_out in (False, True):
			lc, mean, var, cov = norm.lcpm(x, device_out=device_out)
			assert mean is None and var is None and isinstance(cov, np.ndarray) and cov.shape == (3, reads.shape[1])
			assert (hasattr(lc, 'is_cuda') and lc.is_cuda) == device_out, name
			lc = _host(lc)
			assert lc.dtype == np.float64 and lc.shape == reads.shape
			print(name, device_out, 'lcpm max abs error %.3g' % np.abs(lc - g['lcpm']).max())
			assert ok(lc, g['lcpm']) and ok(cov[[0, 2]], g['cov'][[0, 2]]) and (cov[1] == g['cov'][1]).all(), name
		lc, mean, var, cov = norm.lcpm(x, lowmem=False)
		assert bool(h['lowmem_lcpm_equal']) and ok(lc, g['lcpm']) and ok(mean, h['lowmem_mean']) and (var == 0).all() and var.shape == reads.shape
		lc, _, _, cov = norm.lcpm(x, normalize=False)
		assert ok(lc, g['nonorm_lcpm']) and ok(cov[[0, 2]], g['nonorm_cov'][[0, 2]]) and (cov[1] == g['nonorm_cov'][1]).all()
		lc, _, _, cov = norm.lcpm(x, ntot=1E9)
		assert ok(lc, g['ntot_lcpm']) and (cov[1] == g['ntot_cov'][1]).all()
		lc, _, _, cov = norm.lcpm(x, nocov=True, nth=3, seed=5)
		assert cov is None and ok(lc, h['nocov_lcpm'])
		lc64 = norm.lcpm(x)[0]
		lc32, m32, v32, _ = norm.lcpm(x, out_dtype=np.float32, lowmem=False, device_out=True)
		assert lc32.dtype == torch.float32 and m32.is_cuda and v32.is_cuda and (lc32.cpu().numpy() == lc64.astype(np.float32)).all()
		assert (m32.cpu().numpy() == lc64.astype(np.float32)).all() and not v32.any().item()


def test_g18_scaling_factor_and_compute_var(golden, norm, torch):
	g, h = golden('G18_front'), golden('G18_front_chain')
	reads, dc = g['reads'], h['normcov_c']
	for x in (reads, reads.astype(np.float64), torch.as_tensor(reads).cuda()):
		assert np.abs(norm.scaling_factor(x) - g['sf']).max() <= 1e-12
	assert np.abs(norm.scaling_factor(reads, varname='logtpropmean', v0='min') - g['sf_logtpropmean_min']).max() <= 1e-12
	assert np.abs(norm.scaling_factor(torch.as_tensor(reads).cuda(), varname='log1-nt0mean', v0='min') - g['sf_log1m_min']).max() <= 1e-12
	lc = g['lcpm']
	for steps, key in ((1, 'w1'), (3, 'w3')):
		for name, dt in (('host64', lc), ('dev64', torch.as_tensor(lc).cuda())):
			w = norm.compute_var(dt, dc, stepmax=steps)
			print(name, steps, 'weights max relative error %.3g' % np.abs(w / h[key] - 1).max())
			assert w.shape == (lc.shape[1], ) and w.dtype == np.float64 and w.min() == 1 and ok(w, h[key]), (name, steps)
		lc32 = lc.astype(np.float32)
		ref32 = front_numpy.compute_var(lc32.astype(np.float64), dc, stepmax=steps)  # (fp32 logCPM is another input: its own restatement)
		for dt in (lc32, torch.as_tensor(lc32).cuda()):
			assert ok(norm.compute_var(dt, dc, stepmax=steps), ref32)


def _counts(rng, ng, n, big=None):
	mu = np.exp(rng.normal(-0.8, 1.2, ng))
	x = rng.poisson(mu[:, None] * np.exp(rng.normal(0, 0.4, n))[None, :]).astype(np.int64)
	empty = x.sum(axis=0) == 0
	x[rng.integers(0, ng, n)[empty], np.nonzero(empty)[0]] = 1  # every cell has a read
	if big is not None:
		x[ng // 2, n // 3] = big
	return x


SHAPES = [  # genes, cells, covariates (the last is the intercept), largest count forced, one-hot batches among the covariates
	(1, 64, 1, None, 0), (7, 13, 2, None, 0), (33, 65, 3, None, 0), (100, 1023, 8, None, 4), (129, 1025, 9, None, 0), (64, 257, 21, None, 4),
	(40, 4099, 5, None, 0), (300, 130, 4, None, 3), (50, 200, 1, None, 0), (20, 300, 63, None, 0), (30, 100, 3, 10**6, 0), (16, 1024, 2, None, 0),
	(45, 250, 26, 70000, 5),
]


@pytest.mark.parametrize('ng,n,nc,big,nb', SHAPES)
def test_front_random_shapes_against_numpy(norm, torch, ng, n, nc, big, nb):
	rng = np.random.default_rng(1000 * ng + n + nc)
	x = _counts(rng, ng, n, big)
	ref, rcov = front_numpy.lcpm(x)
	batch = rng.integers(0, max(nb, 1), n)
	rows = [(batch[None, :] == np.arange(nb)[:, None]).astype(np.float64)] if nb else []
	dc = np.vstack(rows + [rng.normal(size=(nc - 1 - nb, n)), np.ones((1, n))])
	assert dc.shape[0] == nc
	wide = torch.zeros((ng, n + 3), dtype=torch.int32, device='cuda')
	wide[:, 1:n + 1] = torch.as_tensor(x.astype(np.int32)).cuda()
	for src in (x, x.astype(np.int32), wide[:, 1:n + 1]):  # (the last: rows that start on no 16-byte boundary)
		lc, _, _, cov = norm.lcpm(src)
		assert ok(lc, ref) and ok(cov[[0, 2]], rcov[[0, 2]]) and (cov[1] == rcov[1]).all()
		if ng > 1:
			assert np.abs(norm.scaling_factor(src) - front_numpy.scaling_factor(x)).max() <= 1e-12
		else:  # (one gene without a zero count: the largest zero share is 0 = v0, and the reference asserts v1 != v0, lcpm.py:277)
			with pytest.raises(AssertionError):
				norm.scaling_factor(src)
	lc32 = norm.lcpm(x, out_dtype=np.float32)[0]
	assert lc32.dtype == np.float32 and (lc32 == lc.astype(np.float32)).all()
	if ng > 1:  # (a single gene has no spread across genes to fit: its standardised residual is +-1 everywhere)
		for steps in (1, 2):
			w = norm.compute_var(lc, dc, stepmax=steps)
			wr = front_numpy.compute_var(ref, dc, stepmax=steps)
			print(ng, n, nc, steps, 'weights max relative error %.3g' % np.abs(w / wr - 1).max())
			assert ok(w, wr)
	else:
		w = norm.compute_var(lc + 0.3 * rng.normal(size=lc.shape), dc)
		assert w.shape == (n, ) and np.isfinite(w).all()


def test_front_run_to_run_bit_identical(golden, norm, torch):
	rng = np.random.default_rng(7)
	x = _counts(rng, 700, 3001)
	dc = np.vstack([rng.normal(size=(6, 3001)), np.ones((1, 3001))])
	dx = torch.as_tensor(x).cuda()
	a, b = norm.lcpm(dx), norm.lcpm(dx)
	assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
	for steps in (1, 3):
		assert np.array_equal(norm.compute_var(a[0], dc, stepmax=steps), norm.compute_var(b[0], dc, stepmax=steps))
	g = golden('G18_front')
	assert np.array_equal(norm.lcpm(g['reads'])[0], norm.lcpm(g['reads'])[0])


def test_front_errors_from_the_device_flags(norm, torch):
	rng = np.random.default_rng(3)
	x = _counts(rng, 40, 90)
	bad = torch.as_tensor(x).cuda()
	bad[5, 7] = -1
	with pytest.raises(ValueError):
		norm.lcpm(bad)
	empty = x.copy()
	empty[:, 11] = 0
	for src in (empty, torch.as_tensor(empty).cuda()):
		with pytest.raises(ValueError):
			norm.lcpm(src)
		assert norm.lcpm(src, nocov=True)[3] is None  # (no covariates, no test for empty cells: lcpm.py:190-196)
	with pytest.raises(NotImplementedError):
		norm.lcpm(torch.as_tensor(x).cuda(), varscale=1)
	with pytest.raises(NotImplementedError):
		huge = x.copy()
		huge[0, 0] = 1 << 24
		norm.lcpm(huge)
	lc = norm.lcpm(x)[0]
	dc = np.vstack([rng.normal(size=(2, 90)), np.ones((1, 90))])
	lc[9] = 0.0  # the covariates explain a constant row exactly: its residual is constant, its spread zero
	for dt in (lc, torch.as_tensor(lc).cuda()):
		with pytest.raises(AssertionError):
			norm.compute_var(dt, dc)


def test_g18_resident_chain(golden, norm, torch):
	"""reads uploaded once -> lcpm -> normcov -> compute_var -> normvar -> coex; only cov, the weights and the scaling factor visit the host."""
	g, h = golden('G18_front'), golden('G18_front_chain')
	reads = torch.as_tensor(g['reads']).cuda()
	lc, _, _, cov = norm.lcpm(reads, device_out=True)
	assert lc.is_cuda and isinstance(cov, np.ndarray)
	sf = norm.scaling_factor(reads)
	dc = norm.normcov(np.vstack([h['cov_raw'][:4], cov]))
	assert ok(dc, h['normcov_c'])
	w = norm.compute_var(lc, dc)
	assert isinstance(w, np.ndarray) and ok(w, h['w1'])
	nv = norm.normvar(lc, dc, w, sf, device_out=True)
	assert nv[0].is_cuda and ok(nv[0].cpu().numpy(), h['nv_exp']) and ok(nv[1], h['nv_cov'])
	p, dot, var = norm.coex(nv[0], nv[1])
	assert p_close(_host(p), h['coex_p']) and close(_host(var), h['coex_var'], 1e-9)


def test_cli_front_round_trip(golden, tmp_path):
	"""`normalisr lcpm | normcov | fitvar | normvar` through files, each its own process, against G18's reference chain ('%.8G' keeps 8 digits)."""
	g, h = golden('G18_front'), golden('G18_front_chain')
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('reads.tsv'), g['reads'], fmt='%i', delimiter='\t')
	np.savetxt(f('batch.tsv'), h['cov_raw'][:4], fmt='%.8G', delimiter='\t')
	env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))

	def run(*args):
		r = subprocess.run([sys.executable, '-m', 'normalisr_amd'] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
		assert r.returncode == 0, r.stderr[-3000:]
	run('lcpm', '-c', f('batch.tsv'), '--var_out', f('var.tsv'), f('reads.tsv'), f('lcpm.tsv'), f('scale.tsv'), f('cov.tsv'))
	run('normcov', f('cov.tsv'), f('ncov.tsv'))
	run('fitvar', f('lcpm.tsv'), f('ncov.tsv'), f('w.tsv'))
	run('normvar', f('lcpm.tsv'), f('w.tsv'), f('ncov.tsv'), f('scale.tsv'), f('exp.tsv'), f('ecov.tsv'))
	load = lambda name: np.loadtxt(f(name), delimiter='\t', ndmin=2)
	near = lambda a, b: close(a, b, 1e-6, floor=1.0)  # (every file in the chain is rounded to 8 significant digits)
	assert near(load('lcpm.tsv'), g['lcpm']) and near(load('scale.tsv').ravel(), g['sf']) and near(load('cov.tsv'), h['cov_raw'])
	assert (load('var.tsv') == 0).all() and load('var.tsv').shape == g['lcpm'].shape
	assert near(load('ncov.tsv'), h['normcov_c']) and near(load('w.tsv').ravel(), h['w1'])
	assert near(load('ecov.tsv'), h['nv_cov'])
	# normvar's output is linear in the logCPM it reads.  lcpm.tsv holds 8 significant digits of values between 10 and 100: an absolute error up to 5e-7.
	# normvar multiplies a row by w**wt <= max(w) and by the variance-keeping scale (bounded here by the growth of the largest magnitude from input to
	# output), and the fit it removes carries an error of the size of the row's own: a factor 2.  All from the reference's arrays, none from the result.
	tol = 5e-7 * h['w1'].max() * max(1.0, np.abs(h['nv_exp']).max() / np.abs(g['lcpm']).max()) * 2
	err = np.abs(load('exp.tsv') - h['nv_exp']).max()
	print('exp.tsv max abs error %.3g, bound %.3g' % (err, tol))
	assert err <= tol
