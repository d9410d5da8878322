"""GPU: lcpm and scaling_factor from SPARSE count matrices through the CSR kernels (csrc/nrm_lcpm_sparse.hip) -- scipy.sparse input of every format, a
DeviceCSR, a torch.sparse_csr tensor -- against what the reference returned for scipy.sparse input (golden G19, tests/golden/make_g19.py), and against the
dense route of this project on the same matrix (NRM_DEBUG lcpm_sparse=force | 0 runs both).  Tolerances as tests/test_gpu_front.py: integers exact; lcpm
and covariates close(1e-9, floor=1); the table looked up without normalisation bit for bit the dense route's; fp32 output the fp64 result rounded once.
No test here relies on a fault: a malformed matrix is an ordinary input to a checked entry and must come back as a ValueError."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

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


@contextlib.contextmanager
def route(mode):
	"""NRM_DEBUG lcpm_sparse=<mode> ('force': the CSR kernels, '0': densified on the host) for scipy.sparse input; None: the default by density."""
	old = os.environ.get('NRM_DEBUG')
	keep = [p for p in (old or '').split(',') if p.strip() and not p.strip().lower().startswith('lcpm_sparse=')]
	os.environ['NRM_DEBUG'] = ','.join(keep + (['lcpm_sparse=' + mode] if mode else []))
	try:
		yield
	finally:
		if old is None:
			del os.environ['NRM_DEBUG']
		else:
			os.environ['NRM_DEBUG'] = old


def _host(a):
	return a.cpu().numpy() if hasattr(a, 'is_cuda') else a


def dev_csr(torch, x, vdtype=np.int32, idtype=np.int32, pdtype=np.int64):
	"""A canonical DeviceCSR of a dense (or scipy.sparse) count matrix."""
	from normalisr_amd.lcpm import DeviceCSR
	m = scipy.sparse.csr_matrix(x)
	m.sum_duplicates()
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
	return DeviceCSR(up(m.indptr.astype(pdtype)), up(m.indices.astype(idtype)), up(m.data.astype(vdtype)), m.shape)


def torch_csr(torch, x):
	"""A torch.sparse_csr tensor in HBM: torch's default widths, int64 for both index tensors and the values."""
	m = scipy.sparse.csr_matrix(x)
	m.sum_duplicates()
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a.astype(np.int64))).cuda()
	return torch.sparse_csr_tensor(up(m.indptr), up(m.indices), up(m.data), size=m.shape)


def sf_or_none(norm, d):
	try:
		return norm.scaling_factor(d)
	except AssertionError:  # (every gene with the same share of zeros: the reference asserts v1 != v0, lcpm.py:277)
		return None


def _forms(torch, reads):
	"""The same counts as every sparse input form lcpm takes."""
	return {
		'csr': scipy.sparse.csr_matrix(reads), 'csc': scipy.sparse.csc_matrix(reads), 'coo': scipy.sparse.coo_matrix(reads),
		'coo_float': scipy.sparse.coo_matrix(reads.astype(np.float64)),
		'dev_int32': dev_csr(torch, reads, np.int32), 'dev_int16': dev_csr(torch, reads, np.int16), 'dev_int64': dev_csr(torch, reads, np.int64, np.int64),
		'torch_sparse_csr': torch_csr(torch, reads),
	}


def test_g19_lcpm_every_sparse_form_and_variant(golden, norm, torch):
	g = golden('G19_lcpm_sparse')
	with route('force'):
		for name in ('lo', 'hi'):
			reads = g[name + '_reads']
			k = lambda key: g[name + '_' + key]
			for form, x in _forms(torch, reads).items():
				tag = (name, form)
				for device_out in (False, True):
					lc, mean, var, cov = norm.lcpm(x, device_out=device_out)
					assert mean is None and var is None and isinstance(cov, np.ndarray) and cov.shape == (3, reads.shape[1]), tag
					assert (hasattr(lc, 'is_cuda') and lc.is_cuda) == device_out, tag
					lc = _host(lc)
					assert lc.dtype == np.float64 and lc.shape == reads.shape, tag
					print(name, form, device_out, 'lcpm max abs error %.3g' % np.abs(lc - k('lcpm')).max())
					assert ok(lc, k('lcpm')) and ok(cov[[0, 2]], k('cov')[[0, 2]]) and (cov[1] == k('cov')[1]).all(), tag
					lc, _, _, cov = norm.lcpm(x, normalize=False, device_out=device_out)
					assert ok(_host(lc), k('nonorm_lcpm')) and ok(cov[[0, 2]], k('nonorm_cov')[[0, 2]]) and (cov[1] == k('nonorm_cov')[1]).all(), tag
					lc, _, _, cov = norm.lcpm(x, ntot=1E9, device_out=device_out)
					assert ok(_host(lc), k('ntot_lcpm')) and ok(cov[[0, 2]], k('ntot_cov')[[0, 2]]) and (cov[1] == k('ntot_cov')[1]).all(), tag
					lc, _, _, cov = norm.lcpm(x, nocov=True, nth=3, seed=5, device_out=device_out)
					assert cov is None and ok(_host(lc), k('nocov_lcpm')), tag
					lc, mean, var, _ = norm.lcpm(x, lowmem=False, device_out=device_out)
					assert bool(k('lowmem_lcpm_equal')) and bool(k('lowmem_mean_equal')) and bool(k('lowmem_var_zero'))
					assert ok(_host(lc), k('lcpm')) and np.array_equal(_host(mean), _host(lc)) and var.shape == reads.shape and not _host(var).any(), tag
				lc64 = norm.lcpm(x)[0]
				lc32 = norm.lcpm(x, out_dtype=np.float32, device_out=True)[0]
				assert lc32.dtype == torch.float32 and (lc32.cpu().numpy() == lc64.astype(np.float32)).all(), tag
				assert np.abs(norm.scaling_factor(x) - k('sf')).max() <= 1e-12, tag
	# the default route, whatever the threshold is: the same answers
	for name in ('lo', 'hi'):
		lc, _, _, cov = norm.lcpm(scipy.sparse.csr_matrix(g[name + '_reads']))
		assert ok(lc, g[name + '_lcpm']) and (cov[1] == g[name + '_cov'][1]).all()


def test_g18_resident_chain_from_a_device_csr(golden, norm, torch):
	"""tests/test_gpu_front.py::test_g18_resident_chain with the counts resident as CSR: the stored entries uploaded once -> lcpm -> ... -> coex."""
	g, h = golden('G18_front'), golden('G18_front_chain')
	reads = dev_csr(torch, g['reads'])
	lc, _, _, cov = norm.lcpm(reads, device_out=True)
	assert lc.is_cuda and isinstance(cov, np.ndarray) and ok(lc.cpu().numpy(), g['lcpm'])
	sf = norm.scaling_factor(reads)
	assert np.abs(sf - g['sf']).max() <= 1e-12
	for varname, key in (('logtpropmean', 'sf_logtpropmean_min'), ('log1-nt0mean', 'sf_log1m_min')):  # (whole-matrix numpy expressions: dense on the host)
		assert np.abs(norm.scaling_factor(reads, varname=varname, v0='min') - g[key]).max() <= 1e-12
	dc = norm.normcov(np.vstack([h['cov_raw'][:4], cov]))
	assert ok(dc, h['normcov_c'])
	w = norm.compute_var(lc, dc)
	assert isinstance(w, np.ndarray) and ok(w, h['w1'])
	nv = norm.normvar(lc, dc, w, sf, device_out=True)
	assert nv[0].is_cuda and ok(nv[0].cpu().numpy(), h['nv_exp']) and ok(nv[1], h['nv_cov'])
	p, dot, var = norm.coex(nv[0], nv[1])
	assert p_close(_host(p), h['coex_p']) and close(_host(var), h['coex_var'], 1e-9)


def _counts(rng, ng, n, mean=-2.2, big=None, empty_row=None, full_row=None):
	mu = np.exp(rng.normal(mean, 1.2, ng))
	x = rng.poisson(mu[:, None] * np.exp(rng.normal(0, 0.4, n))[None, :]).astype(np.int64)
	if empty_row is not None:
		x[empty_row] = 0
	if full_row is not None:
		x[full_row] = 1 + rng.integers(0, 5, n)
	empty = x.sum(axis=0) == 0
	rows = rng.integers(0, ng, n)
	if empty_row is not None and ng > 1:
		rows[rows == empty_row] = (empty_row + 1) % ng
	x[rows[empty], np.nonzero(empty)[0]] = 1  # every cell has a read
	if big is not None:
		x[ng // 2, n // 3] = big
	return x


SHAPES = [  # genes, cells, largest count forced, a gene without reads, a gene with a read in every cell
	(1, 64, None, None, None), (7, 13, None, None, None), (33, 65, None, 5, None), (100, 1023, None, None, 9), (129, 1025, None, 128, 0), (40, 4099, None, None, None),
	(30, 101, 10**6, None, None), (50, 4097, 70000, 49, 3), (300, 130, None, None, None), (16, 1024, None, 0, 15), (45, 8193, None, None, None), (3, 4096, None, 1, 2),
]


@pytest.mark.parametrize('ng,n,big,empty_row,full_row', SHAPES)
def test_sparse_route_equals_the_dense_route(norm, torch, ng, n, big, empty_row, full_row):
	rng = np.random.default_rng(1000 * ng + n)
	x = _counts(rng, ng, n, big=big, empty_row=empty_row, full_row=full_row)
	m = scipy.sparse.csr_matrix(x)
	res = {}
	for mode in ('force', '0'):
		with route(mode):
			r = dict(raw=norm.lcpm(m, normalize=False), raw32=norm.lcpm(m, normalize=False, out_dtype=np.float32), full=norm.lcpm(m), ntot=norm.lcpm(m, ntot=1E9))
			r['sf'] = sf_or_none(norm, m)
			res[mode] = r
	a, b = res['force'], res['0']
	assert np.array_equal(a['raw'][0], b['raw'][0]) and np.array_equal(a['raw32'][0], b['raw32'][0])  # the same table looked up: bit for bit
	assert a['raw32'][0].dtype == np.float32 and np.array_equal(a['raw32'][0], a['raw'][0].astype(np.float32))
	for key in ('raw', 'full', 'ntot'):
		assert np.array_equal(a[key][3], b[key][3]), key  # the covariates come from the same integers
	print(ng, n, 'normalised: max abs difference %.3g' % np.abs(a['full'][0] - b['full'][0]).max())
	assert ok(a['full'][0], b['full'][0]) and ok(a['ntot'][0], b['ntot'][0])  # (only the order of the per-cell sum differs)
	assert (a['sf'] is None) == (b['sf'] is None) and (a['sf'] is None or np.array_equal(a['sf'], b['sf']))
	# the device forms on the same matrix, index tensors of torch's default width among them
	for d in (dev_csr(torch, x, np.int64, np.int64), torch_csr(torch, x)):
		lc, _, _, cov = norm.lcpm(d)
		assert np.array_equal(lc, a['full'][0]) and np.array_equal(cov, a['full'][3])
	# stored zeros are legal and count as zeros
	z = scipy.sparse.csr_matrix(x)
	z.data[::3] = 0
	dz = dev_csr(torch, z.toarray())
	from normalisr_amd.lcpm import DeviceCSR
	up = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
	withz = DeviceCSR(up(z.indptr.astype(np.int64)), up(z.indices.astype(np.int32)), up(z.data.astype(np.int32)), z.shape)
	assert withz.data.numel() > dz.data.numel() or z.nnz < 3
	ra, rb = norm.lcpm(withz, nocov=True), norm.lcpm(dz, nocov=True)
	assert np.array_equal(ra[0], rb[0])
	sa, sb = sf_or_none(norm, withz), sf_or_none(norm, dz)
	assert (sa is None) == (sb is None) and (sa is None or np.array_equal(sa, sb))


def test_sparse_route_run_to_run_bit_identical(norm, torch):
	rng = np.random.default_rng(7)
	x = _counts(rng, 700, 3001)
	d = dev_csr(torch, x)
	a, b = norm.lcpm(d), norm.lcpm(d)
	assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
	with route('force'):
		m = scipy.sparse.coo_matrix(x)
		c, e = norm.lcpm(m), norm.lcpm(m)
	assert np.array_equal(c[0], e[0]) and np.array_equal(c[0], a[0])
	assert np.array_equal(norm.scaling_factor(d), norm.scaling_factor(d))


def test_sparse_errors_from_the_device_flags(norm, torch):
	from normalisr_amd.lcpm import DeviceCSR
	rng = np.random.default_rng(3)
	x = _counts(rng, 40, 90, mean=-1.0)
	good = dev_csr(torch, x)
	assert norm.lcpm(good)[0].shape == x.shape

	def variant(indptr=None, indices=None, data=None):
		t = [good.indptr.clone(), good.indices.clone(), good.data.clone()]
		for i, f in enumerate((indptr, indices, data)):
			if f is not None:
				f(t[i])
		return DeviceCSR(t[0], t[1], t[2], good.shape)

	def at(i, v):
		def f(t):
			t[i] = v
		return f
	nnz = int(good.data.numel())
	p = good.indptr.cpu().numpy()
	row = int(np.nonzero(np.diff(p) >= 2)[0][0])  # a row with two stored entries at least
	a = int(p[row])
	with pytest.raises(ValueError, match='Negative'):
		norm.lcpm(variant(data=at(5, -1)))
	malformed = {
		'column beyond the last cell': variant(indices=at(nnz - 1, x.shape[1])), 'negative column': variant(indices=at(0, -1)),
		'far column': variant(indices=at(nnz // 2, 2**31 - 1)),
		'unsorted row': variant(indices=lambda t: t.__setitem__(slice(a, a + 2), t[a:a + 2].flip(0))),
		'duplicate column': variant(indices=lambda t: t.__setitem__(a + 1, t[a])),
		'indptr decreasing': variant(indptr=at(row + 1, a - 1 if a > 0 else int(p[row + 2]) + 1)), 'indptr short of nnz': variant(indptr=at(-1, nnz - 1)),
		'indptr beyond nnz': variant(indptr=at(-1, nnz + 1000)), 'indptr far beyond': variant(indptr=at(3, 2**40)), 'indptr negative': variant(indptr=at(2, -7)),
		'indptr not from 0': variant(indptr=at(0, 1)),
	}
	for name, d in malformed.items():
		for call in (lambda: norm.lcpm(d), lambda: norm.lcpm(d, normalize=False, nocov=True), lambda: norm.scaling_factor(d)):
			with pytest.raises(ValueError, match='Malformed'):
				call()
	# and the device is as it was: the well-formed matrix still gives the same answer
	assert np.array_equal(norm.lcpm(good)[0], norm.lcpm(dev_csr(torch, x))[0])
	empty = x.copy()
	empty[:, 11] = 0
	for src in (dev_csr(torch, empty), scipy.sparse.csr_matrix(empty)):
		with route('force'):
			with pytest.raises(ValueError, match='no read'):
				norm.lcpm(src)
			assert norm.lcpm(src, nocov=True)[3] is None  # (no covariates, no test for empty cells: lcpm.py:190-196)
	with pytest.raises(NotImplementedError):
		norm.lcpm(good, varscale=1)
	huge = x.copy()
	huge[0, 0] = 1 << 24
	for src in (dev_csr(torch, huge), scipy.sparse.csr_matrix(huge)):
		with route('force'):
			with pytest.raises(NotImplementedError):
				norm.lcpm(src)


def test_sparse_route_forms_no_dense_counts(norm, torch):
	"""4096 genes x 65 536 cells at 2 % stored entries, fp32 result left in HBM: the call's peak device memory above what was allocated before it stays below
	the result plus a quarter of the dense int32 counts (both 1.07 GB) -- a condition from the shapes, which a dense upload of the counts exceeds."""
	nt, ns = 4096, 65536
	rng = np.random.default_rng(41)
	m = scipy.sparse.random(nt, ns, density=0.02, format='csr', random_state=rng, data_rvs=lambda k: rng.integers(1, 40, k)).astype(np.int32)
	m.sum_duplicates()
	assert 5.2e6 < m.nnz < 5.6e6
	d = dev_csr(torch, m)
	out_bytes, dense_bytes = nt * ns * 4, nt * ns * 4
	torch.cuda.synchronize()
	torch.cuda.empty_cache()
	torch.cuda.reset_peak_memory_stats()
	before = torch.cuda.memory_allocated()
	lc, _, _, cov = norm.lcpm(d, nocov=True, out_dtype=np.float32, device_out=True)
	torch.cuda.synchronize()
	peak = torch.cuda.max_memory_allocated() - before
	print('peak above the start: %.1f MB; result %.1f MB; bound %.1f MB' % (peak / 1e6, out_bytes / 1e6, (out_bytes + dense_bytes / 4) / 1e6))
	assert cov is None and lc.is_cuda and lc.dtype == torch.float32 and tuple(lc.shape) == (nt, ns)
	assert peak < out_bytes + dense_bytes / 4
	# the values: the sparse form of the per-cell sum in numpy, and a few whole rows of the result
	from scipy.special import digamma
	x = m.data.astype(np.int64)
	tab = digamma(1.0 + np.arange(int(x.max()) + 1)) - digamma(float(x.sum() + 2))
	e = np.exp(tab)
	t1 = np.log(nt * e[0] + np.bincount(m.indices, weights=e[x] - e[0], minlength=ns)) - np.log(1E6)
	for g in (0, 1, 2047, 4095):
		want = np.full(ns, tab[0])
		want[m.indices[m.indptr[g]:m.indptr[g + 1]]] = tab[x[m.indptr[g]:m.indptr[g + 1]]]
		got = lc[g].cpu().numpy()
		assert np.array_equal(got, (want - t1).astype(np.float32)) or close(got, want - t1, 1e-6, floor=1.0), g  # (fp32 output: 24 bits of values up to 20)
		assert np.abs(got.astype(np.float64) - (want - t1)).max() <= 2e-6


def test_cli_lcpm_sparse_matrix_market(golden, tmp_path):
	"""`normalisr lcpm -s` on a Matrix Market file of G19's denser matrix, as a child process, against what the reference returned ('%.8G' keeps 8 digits)."""
	import scipy.io
	g = golden('G19_lcpm_sparse')
	f = lambda name: str(tmp_path / name)
	scipy.io.mmwrite(f('reads.mtx'), scipy.sparse.coo_matrix(g['hi_reads']))
	env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
	env['NRM_DEBUG'] = ','.join([p for p in env.get('NRM_DEBUG', '').split(',') if p.strip()] + ['lcpm_sparse=force'])
	r = subprocess.run([sys.executable, '-m', 'normalisr_amd', 'lcpm', '-s', f('reads.mtx'), f('lcpm.tsv'), f('scale.tsv'), f('cov.tsv')], env=env, stdout=subprocess.PIPE,
					   stderr=subprocess.PIPE, text=True, timeout=600)
	assert r.returncode == 0, r.stderr[-3000:]
	load = lambda name: np.loadtxt(f(name), delimiter='\t', ndmin=2)
	near = lambda a, b: close(a, b, 1e-6, floor=1.0)  # (every file is rounded to 8 significant digits)
	assert near(load('lcpm.tsv'), g['hi_lcpm']) and near(load('scale.tsv').ravel(), g['hi_sf']) and near(load('cov.tsv'), g['hi_cov'])
