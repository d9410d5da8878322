"""GPU: the public front-half calls on inputs chosen to expose errors, against the extended-precision references of tests/front_longdouble.py.

compute_var / ComputeVarPlan.  The existing tests give every covariate set an intercept; the residual's row mean is then zero to rounding and the mean path of
k_fv_genes / k_fv_cells computes dead values.  Here: NO intercept in dc; covariate rows with norms 30 x and 1/30 x the others and one with mean 3; gene rows
with offsets in 0 .. 14 and scales exp(N(0, 1)); a per-cell scale exp(0.9 c_last + 0.2 N(0, 1)), so that the weights spread (a scale independent of the
covariates leaves w near 1); fp64 and fp32, contiguous and a padded row stride; stepmax 1 and 3 with eps = 1e-300.  The same with one-hot batches plus an
intercept (the longdouble reference is given a full-rank basis: one batch row dropped).
The tolerance is not fixed in advance: per case, the error of an fp64 numpy restatement of what the device does (both projections through inv_rank on the Gram
matrix; front_longdouble.compute_var_fp64) against longdouble -- two references, no code under test -- times 10 (the same precision, another summation order
and contraction, one sample of a distribution), floored at 64 * 2^-53 and asserted never to exceed 1e-10.  The inputs are asserted to keep every Gram
eigenvalue a factor 100 from inv_rank's threshold.
Relations that need no reference, to the same allowance: common and single-row rescaling of the covariates, scaling gene rows, adding combinations of dc rows
to gene rows, permuting genes, permuting cells.

lcpm, dense and CSR: the all-non-zero tile at the dtype's maximum, ntot non-integer and near zero, the table's last entry (2^24 - 1), a padded-stride device
input.  Bound: the digamma bound (1e-14 |psi| + 1e-15) on the two table values, u |T| for their difference; for t1 the largest such bound, 2 u for the host's
exp and the stage bound of tests/test_gpu_front_stages.py; u |lcpm| for the last subtraction.  Dense and CSR within the sum of their bounds of each other."""
import functools

import numpy as np
import pytest

import front_longdouble as fl
from test_gpu_front_stages import LOG_ULP, U
from test_gpu_compute_var_plan import SHAPES, _problem

pytestmark = pytest.mark.gpu

FLOOR, CEILING = 64 * U, 1e-10
CV_SHAPES = [(129, 1025, 5), (33, 4099, 9), (300, 130, 4), (64, 257, 21)]


@pytest.fixture(scope='module')
def norm():
	import normalisr_amd.normalisr as norm
	return norm


@pytest.fixture(scope='module')
def torch():
	import torch
	return torch


@pytest.fixture(scope='module')
def Plan():
	from normalisr_amd.norm import ComputeVarPlan
	return ComputeVarPlan


def rel(a, b):
	return float(np.max(np.abs(fl.ld(a) - fl.ld(b)) / np.abs(fl.ld(b))))


# ---- compute_var ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(ng, n, nc, onehot):
	"""(dt fp64, dc, full-rank basis of span(dc), full-rank basis of span(dc, 1))."""
	rng = np.random.default_rng(1000 * ng + n + nc + 7 * onehot)
	if onehot:
		nb = 3 if nc >= 6 else 2
		batch = np.arange(n) % nb
		rng.shuffle(batch)
		cont = rng.normal(size=(nc - nb - 1, n))
	else:
		cont = rng.normal(size=(nc, n))
	cont[0] *= 30.0
	if cont.shape[0] > 2:
		cont[1] /= 30.0
		cont[2] += 3.0
	last = cont[-1] if cont.shape[0] > 1 else cont[-1] / 30.0
	if onehot:
		hot = (batch[None, :] == np.arange(nb)[:, None]).astype(np.float64)
		dc = np.vstack([hot, cont, np.ones((1, n))])
		basis = basis1 = dc[1:]
	else:
		dc = cont
		basis, basis1 = dc, np.vstack([dc, np.ones((1, n))])
	assert dc.shape == (nc, n)
	load = rng.normal(size=(ng, dc.shape[0])) / np.sqrt((dc**2).mean(axis=1))  # every covariate moves every gene by O(1)
	scale = np.exp(0.9 * last + 0.2 * rng.normal(size=n))
	dt = rng.uniform(0, 14, ng)[:, None] + load @ dc + np.exp(rng.normal(size=ng))[:, None] * rng.normal(size=(ng, n)) * scale
	for a in (dt, dc):
		a.setflags(write=False)
	return dt, dc, basis, basis1


def _eigen_guard(dc):
	"""Every eigenvalue of dc dc^T is either above 1e-6 of the largest or below 1e-10 of it: a factor 100 from inv_rank's relative threshold 1e-8."""
	ev = np.linalg.eigvalsh(dc @ dc.T)
	ratio = ev / ev.max()
	return bool(((ratio >= 1e-6) | (np.abs(ratio) <= 1e-10)).all()), float(ratio[ratio > 1e-10].min())


@functools.lru_cache(maxsize=None)
def _references(ng, n, nc, onehot, dtype, steps):
	"""(the longdouble weights, the per-case allowance) on the values the device reads."""
	dt, dc, basis, basis1 = _inputs(ng, n, nc, onehot)
	x = dt.astype(dtype)
	w, t1s = fl.compute_var(x, basis, basis1, stepmax=steps, eps=1e-300)
	err = rel(fl.compute_var_fp64(x, dc, stepmax=steps, eps=1e-300), w)
	tol = max(10 * err, FLOOR)
	assert len(t1s) == steps and tol <= CEILING, (err, tol)
	return w, tol, err


def _device(torch, a, padded):
	t = torch.tensor(np.ascontiguousarray(a)).cuda()
	if not padded:
		return t
	n = a.shape[1]
	wide = torch.full((a.shape[0], n + 4 - n % 4), 1e3, dtype=t.dtype, device='cuda')  # (a stride of a multiple of four elements on the allocation's base)
	wide[:, :n] = t
	return wide[:, :n]


@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('onehot', [False, True])
@pytest.mark.parametrize('ng,n,nc', CV_SHAPES)
def test_compute_var_and_plan_against_longdouble(norm, torch, Plan, ng, n, nc, onehot, dtype, padded, steps):
	dt, dc, _, _ = _inputs(ng, n, nc, onehot)
	good, ratio = _eigen_guard(dc)
	assert good, ratio
	if not onehot:
		r1 = dt - dt @ np.linalg.pinv(dc) @ dc
		assert np.abs(r1.mean(axis=1) / r1.std(axis=1)).max() > 1e-3  # without an intercept the residual's mean is a live value
	w_ref, tol, err = _references(ng, n, nc, onehot, dtype, steps)
	assert w_ref.max() > 3  # the weights spread
	d = _device(torch, dt.astype(dtype), padded)
	assert d.stride(1) == 1 and (not padded or (d.stride(0) % 4 == 0 and d.stride(0) > n))
	w = norm.compute_var(d, dc, stepmax=steps, eps=1e-300)
	plan = Plan(d, dc, stepmax=steps, eps=1e-300)
	plan.step()
	wp = plan.results()
	e, ep = rel(w, w_ref), rel(wp, w_ref)
	print('(%d, %d, %d) onehot %s %s padded %s steps %d: eigenvalue ratio %.3g, weights up to %.3g, restatement error %.3g, allowance %.3g, compute_var %.3g, plan %.3g' % (
		ng, n, nc, onehot, dtype, padded, steps, ratio, float(w_ref.max()), err, tol, e, ep))
	assert w.shape == (n, ) and w.min() == 1 and e <= tol
	assert wp.shape == (n, ) and wp.min() == 1 and ep <= tol and plan.steps_taken == steps


def _relation_cases():
	"""name -> (dt, dc) -> (dt', dc', the cells' permutation or None)."""
	def common(f):
		return lambda dt, dc, rng: (dt, dc * f, None)

	def single(dt, dc, rng):
		f = np.ones(dc.shape[0])
		f[0], f[1] = 1 / 3.0, 3.0  # (towards the others: the eigenvalue guard holds)
		f[-1] = 2.5
		return dt, dc * f[:, None], None

	def gene_scale(dt, dc, rng):
		return dt * np.exp(rng.normal(size=dt.shape[0]))[:, None], dc, None

	def add_rows(dt, dc, rng):
		return dt + (rng.normal(size=(dt.shape[0], dc.shape[0])) / np.sqrt((dc**2).mean(axis=1))) @ dc, dc, None

	def perm_genes(dt, dc, rng):
		return dt[rng.permutation(dt.shape[0])], dc, None

	def perm_cells(dt, dc, rng):
		p = rng.permutation(dt.shape[1])
		return dt[:, p], dc[:, p], p
	return {'covariates x 1e-6': common(1e-6), 'covariates x 1e6': common(1e6), 'single covariate rows': single, 'gene rows scaled': gene_scale,
			'dc rows added to gene rows': add_rows, 'genes permuted': perm_genes, 'cells permuted': perm_cells}


RELATIONS = _relation_cases()


@pytest.fixture(scope='module')
def base_weights(norm, torch):
	out = {}

	def get(ng, n, nc):
		if (ng, n, nc) not in out:
			dt, dc, _, _ = _inputs(ng, n, nc, False)
			out[(ng, n, nc)] = norm.compute_var(_device(torch, dt, False), dc, stepmax=3, eps=1e-300)
		return out[(ng, n, nc)]
	return get


@pytest.mark.parametrize('name', list(RELATIONS))
@pytest.mark.parametrize('ng,n,nc', [(129, 1025, 5), (300, 130, 4)])
def test_compute_var_relations_without_a_reference(norm, torch, base_weights, ng, n, nc, name):
	dt, dc, _, _ = _inputs(ng, n, nc, False)
	tol = _references(ng, n, nc, False, 'float64', 3)[1]
	w0 = base_weights(ng, n, nc)
	dt2, dc2, perm = RELATIONS[name](dt, dc, np.random.default_rng(len(name)))
	assert _eigen_guard(dc2)[0]
	w = norm.compute_var(_device(torch, dt2, False), dc2, stepmax=3, eps=1e-300)
	want = w0 if perm is None else w0[perm]
	e = rel(w, want)
	print('(%d, %d, %d) %s: max relative change of the weights %.3g, allowance %.3g' % (ng, n, nc, name, e, tol))
	assert e <= tol


@pytest.mark.parametrize('ng,n,nc,big,nb', [s for s in SHAPES if s[0] > 1])
def test_plan_fp32_and_padded_over_the_existing_shapes(norm, torch, Plan, ng, n, nc, big, nb):
	"""ComputeVarPlan on fp32 and on padded-stride inputs over the shapes of tests/test_gpu_compute_var_plan.py (which runs them in contiguous fp64): against
	the public call, against longdouble, and the rank k_fvp_pinv writes in the first iteration against inv_rank's."""
	from normalisr_amd.association import inv_rank
	lc, dc = _problem(ng, n, nc, big, nb)
	basis = dc[1:] if nb else dc  # (one-hot batches plus the intercept: one batch row dropped)
	assert np.linalg.matrix_rank(basis) == basis.shape[0] == inv_rank(dc @ dc.T)[1]
	for dtype, padded in (('float32', False), ('float32', True), ('float64', True)):
		x = lc.astype(dtype)
		d = _device(torch, x, padded)
		for steps in (1, 2):
			w_ref, t1s = fl.compute_var(x, basis, basis, stepmax=steps, eps=1e-300)
			err = rel(fl.compute_var_fp64(x, dc, stepmax=steps, eps=1e-300), w_ref)
			tol = max(10 * err, FLOOR)
			assert tol <= CEILING
			plan = Plan(d, dc, stepmax=steps, eps=1e-300)
			plan.step()
			w = plan.results()
			pub = norm.compute_var(d, dc, stepmax=steps, eps=1e-300)
			print(ng, n, nc, dtype, 'padded' if padded else 'contiguous', steps, 'allowance %.3g; plan against longdouble %.3g, against the public call %.3g' % (
				tol, rel(w, w_ref), rel(w, pub)))
			assert w.min() == 1 and rel(w, w_ref) <= tol and rel(pub, w_ref) <= tol
			assert plan.steps_taken == len(t1s)  # (an intercept alone changes nothing: t1 = 0 ends the loop after one iteration, here as in the reference)
			if steps == 1:
				assert int(plan._rank.cpu().numpy()[0]) == inv_rank(dc @ dc.T)[1]


# ---- lcpm ----------------------------------------------------------------------------------------------------------------------------------------------------
def _tile_matrix(ng, n, top, seed):
	"""Sparse Poisson counts; in four cells every gene of the first and of the last 32-gene tile is non-zero, at and just below the dtype's maximum; a cell whose
	only read sits in the last gene."""
	rng = np.random.default_rng(seed)
	x = rng.poisson(0.3, (ng, n)).astype(np.int64)
	for k in (0, n // 2, n - 2, n - 1):
		for g0 in (0, 32 * ((ng - 1) // 32)):
			x[g0:g0 + 32, k] = top - rng.integers(0, 3, x[g0:g0 + 32, k].shape)
	x[:, 1] = 0
	x[ng - 1, 1] = 1
	empty = x.sum(axis=0) == 0
	x[0, empty] = 1
	return x


LCPM_CASES = {  # name: (genes, cells, count dtype, the largest count, ntot, padded-stride input)
	'uint8 tile at 255': (70, 301, 'uint8', 255, None, False),
	'int16 tile at 32767': (33, 1027, 'int16', 32767, None, False),
	'ntot near zero': (40, 130, 'int32', 300, 2.0**-20, False),
	'ntot non-integer': (40, 130, 'int32', 300, 12345.678, False),
	'table end': (35, 70, 'int32', 2**24 - 1, None, False),
	'padded stride': (65, 4099, 'int32', 5000, None, True),
	'padded stride uint8': (64, 259, 'uint8', 255, None, True),
}


@pytest.mark.parametrize('name', list(LCPM_CASES))
def test_lcpm_dense_and_csr_against_longdouble(norm, torch, name):
	import scipy.sparse
	from normalisr_amd.lcpm import DeviceCSR
	ng, n, dtype, top, ntot, padded = LCPM_CASES[name]
	x = _tile_matrix(ng, n, top, len(name))
	if name == 'table end':
		x[x > 2] = 2  # (one count at the table's end among small ones: the table's last entry is the point here)
		x[ng // 2, n // 3] = top
	ref, t1, info = fl.lcpm(x, ntot=ntot)
	dpsi = (1e-14 * np.abs(info['psi_x']) + 1e-15) + (1e-14 * np.abs(info['psi_t0']) + 1e-15)
	dtab = dpsi + U * np.abs(info['psi_x'] - info['psi_t0'])
	nnz = (x != 0).sum(axis=0)
	stage = lambda terms: terms + U * np.abs(t1) + 16 * U + LOG_ULP * fl.ulp(t1)
	bounds = {}
	for route, terms in (('dense', ng * U), ('csr', nnz * 2.0**-62 + 3 * U)):
		dt1 = dtab.max() + 2 * U + stage(terms)
		bounds[route] = dtab + dt1[None, :] + U * np.abs(ref)
	d = _device_counts(torch, x.astype(dtype), padded)
	kw = {} if ntot is None else dict(ntot=ntot)
	dense = norm.lcpm(d, **kw)[0]
	m = scipy.sparse.csr_matrix(x.astype(dtype))
	sparse = norm.lcpm(DeviceCSR.from_scipy(m), **kw)[0]
	ed, es = np.abs(fl.ld(dense) - ref), np.abs(fl.ld(sparse) - ref)
	print('%s: error/bound dense %.3g, csr %.3g; dense against csr %.3g' % (name, float((ed / bounds['dense']).max()), float((es / bounds['csr']).max()),
																		   float((np.abs(fl.ld(dense) - fl.ld(sparse)) / (bounds['dense'] + bounds['csr'])).max())))
	assert dense.shape == sparse.shape == (ng, n) and dense.dtype == sparse.dtype == np.float64
	assert (ed <= bounds['dense']).all() and (es <= bounds['csr']).all()
	assert (np.abs(fl.ld(dense) - fl.ld(sparse)) <= bounds['dense'] + bounds['csr']).all()
	cov = norm.lcpm(d, **kw)[3]
	assert np.array_equal(cov[1], ng - nnz) and np.abs(fl.ld(cov[0]) - np.log(fl.ld(x.sum(axis=0)))).max() <= 4 * U * np.log(float(x.sum(axis=0).max()))


def _device_counts(torch, x, padded):
	t = torch.tensor(np.ascontiguousarray(x)).cuda()
	if not padded:
		return t
	n = x.shape[1]
	wide = torch.full((x.shape[0], n + 4 - n % 4), 9, dtype=t.dtype, device='cuda')
	wide[:, :n] = t
	return wide[:, :n]
