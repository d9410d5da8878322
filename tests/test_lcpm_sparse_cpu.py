"""CPU-only checks of the sparse route of lcpm / scaling_factor: the numpy restatement of the SPARSE form of the per-cell sum,
    sum_g E[x_gk] = rows * E[0] + sum over the stored entries of cell k of (E[x] - E[0]),
against what the reference returned for scipy.sparse input (golden G19, tests/golden/make_g19.py); the host's canonicalisation of scipy.sparse input; the
argument checks of DeviceCSR that need no device; the parser.  Tolerance: the project's bound for fp64 quantities that are O(1) and pass through zero,
close(1e-9, floor=1); integers and scaling factors as tests/test_front_cpu.py has them."""
import numpy as np
import pytest
import scipy.sparse

from test_gpu_parity import close

VARIANTS = (('lcpm', {}), ('nonorm_lcpm', dict(normalize=False)), ('ntot_lcpm', dict(ntot=1E9)), ('nocov_lcpm', dict(nocov=True)))


def lcpm_sparse_numpy(m, normalize=True, ntot=None, nocov=False):
	"""(lcpm, cov, scaling factor) from a canonical scipy CSR matrix, touching its stored entries only until the dense result is written."""
	from scipy.special import digamma
	m = scipy.sparse.csr_matrix(m)
	nt, ns = m.shape
	x = m.data.astype(np.int64)
	t0 = float(x.sum() + 2) if ntot is None else ntot + 2
	tab = digamma(1.0 + np.arange(int(x.max()) + 1)) - digamma(t0)
	out = np.full((nt, ns), tab[0])
	rows = np.repeat(np.arange(nt), np.diff(m.indptr))
	out[rows, m.indices] = tab[x]
	if normalize:
		e = np.exp(tab)
		s = nt * e[0] + np.bincount(m.indices, weights=e[x] - e[0], minlength=ns)
		out = out - (np.log(s) - np.log(1E6))
	cov = None
	if not nocov:
		tot = np.log(np.bincount(m.indices, weights=x, minlength=ns))
		cov = np.array([tot, nt - np.bincount(m.indices, weights=x != 0, minlength=ns), tot**2])
	zero = (ns - np.bincount(rows, weights=x != 0, minlength=nt)) / float(ns)
	return out, cov, zero / zero.max()


def test_sparse_form_restatement_matches_the_reference(golden):
	g = golden('G19_lcpm_sparse')
	assert float(g['lo_density']) < 0.01 < 0.05 < float(g['hi_density']) and g['hi_reads'].max() > 255 and (g['lo_reads'].sum(axis=0) > 0).all()
	for name in ('lo', 'hi'):
		m = scipy.sparse.csr_matrix(g[name + '_reads'])
		for key, ka in VARIANTS:
			lc, cov, sf = lcpm_sparse_numpy(m, **ka)
			print(name, key, 'max abs error %.3g' % np.abs(lc - g[name + '_' + key]).max())
			assert close(lc, g[name + '_' + key], 1e-9, floor=1.0), (name, key)
			if key in ('lcpm', 'nonorm_lcpm', 'ntot_lcpm'):
				rc = g[name + '_' + key.replace('lcpm', 'cov')]
				assert close(cov[[0, 2]], rc[[0, 2]], 1e-9, floor=1.0) and (cov[1] == rc[1]).all()
			else:
				assert cov is None
		assert np.abs(sf - g[name + '_sf']).max() <= 1e-12
		assert bool(g[name + '_lowmem_lcpm_equal']) and bool(g[name + '_lowmem_mean_equal']) and bool(g[name + '_lowmem_var_zero'])


def test_host_canonicalisation_of_scipy_input():
	from normalisr_amd.lcpm import canonical_csr
	rng = np.random.default_rng(5)
	x = rng.poisson(0.08, (37, 53)).astype(np.int64)
	x[4, 9] = 300
	ref = scipy.sparse.csr_matrix(x)
	ref.sum_duplicates()
	want = (ref.indptr.astype(np.int64), ref.indices.astype(np.int32), ref.data.astype(np.int16))
	r, c = np.nonzero(x)
	v = x[r, c]
	# COO with duplicate entries: every value above 1 split into two entries, in a shuffled order
	split = v > 1
	rr, cc, vv = np.concatenate([r, r[split]]), np.concatenate([c, c[split]]), np.concatenate([np.where(split, v - 1, v), np.ones(split.sum(), dtype=np.int64)])
	o = rng.permutation(rr.size)
	dup = scipy.sparse.coo_matrix((vv[o], (rr[o], cc[o])), shape=x.shape)
	unsorted = scipy.sparse.csr_matrix(x)
	for g in range(x.shape[0]):  # the columns of every row reversed
		a, b = unsorted.indptr[g], unsorted.indptr[g + 1]
		unsorted.indices[a:b] = unsorted.indices[a:b][::-1].copy()
		unsorted.data[a:b] = unsorted.data[a:b][::-1].copy()
	unsorted.has_sorted_indices = False
	stored0 = scipy.sparse.coo_matrix((np.concatenate([v, [0, 0]]), (np.concatenate([r, [0, 36]]), np.concatenate([c, [0, 52]]))), shape=x.shape)
	assert x[0, 0] == 0 and x[36, 52] == 0
	forms = {'coo_duplicates': dup, 'csc': scipy.sparse.csc_matrix(x), 'unsorted_csr': unsorted, 'explicit_zeros': stored0,
			 'float_coo': scipy.sparse.coo_matrix(x.astype(np.float64)), 'float32_csr': scipy.sparse.csr_matrix(x.astype(np.float32)), 'csr': scipy.sparse.csr_matrix(x)}
	for name, m in forms.items():
		before = m.copy()
		got = canonical_csr(m)
		for a, b in zip(got, want):
			assert a.dtype == b.dtype and np.array_equal(a, b), name
		assert (before != m).nnz == 0 and m.nnz == before.nnz, name  # the caller's matrix is left as it was
	# the narrowest value type that holds the maximum
	for top, dtype in ((1, np.uint8), (255, np.uint8), (256, np.int16), (32767, np.int16), (32768, np.int32), (2**31 - 1, np.int32), (2**31, np.int64)):
		y = x.copy()
		y[y > top] = top
		y[7, 7] = top
		assert canonical_csr(scipy.sparse.csr_matrix(y))[2].dtype == dtype, top
	empty = canonical_csr(scipy.sparse.csr_matrix((3, 4), dtype=np.int64))
	assert np.array_equal(empty[0], np.zeros(4)) and empty[1].size == 0 and empty[2].size == 0
	neg = x.copy()
	neg[2, 2] = -1
	with pytest.raises(ValueError):
		canonical_csr(scipy.sparse.csr_matrix(neg))
	with pytest.raises(TypeError):
		canonical_csr(scipy.sparse.csr_matrix(x.astype(np.complex128)))


def test_sparse_argument_validation_before_any_device_call():
	import normalisr_amd.normalisr as norm
	x = np.ones((3, 5), dtype=np.int64)
	for f in (scipy.sparse.csr_matrix, scipy.sparse.coo_matrix, scipy.sparse.csc_matrix):
		with pytest.raises(ValueError):
			norm.lcpm(f(x - 2))
		with pytest.raises(ValueError):
			norm.lcpm(f(x.astype(np.float64) - 1.5))  # (as the dense route: tests/test_front_cpu.py)
		with pytest.raises(ValueError):
			norm.lcpm(f(x), varscale=-1)
		with pytest.raises(NotImplementedError):
			norm.lcpm(f(x), varscale=1)
		with pytest.raises(ValueError):
			norm.lcpm(f(x), out_dtype=np.float16)
		with pytest.raises(ValueError):
			norm.scaling_factor(f(x), varname='median')


def test_device_csr_argument_validation_without_a_device():
	import torch
	from normalisr_amd.lcpm import DeviceCSR
	indptr, indices, data = torch.tensor([0, 2, 3, 3]), torch.tensor([0, 4, 1], dtype=torch.int32), torch.tensor([1, 2, 3], dtype=torch.int16)
	bad = [
		((indptr, indices, data, (3, )), 'shape'), ((indptr, indices, data, (3, 5, 1)), 'shape'), ((indptr, indices, data, (3, -5)), 'shape'),
		((indptr, indices, data, (4, 5)), 'indptr'), ((indptr[:3], indices, data, (3, 5)), 'indptr'), ((indptr.reshape(2, 2), indices, data, (3, 5)), 'indptr'),
		((indptr, indices[:2], data, (3, 5)), 'length'), ((indptr.double(), indices, data, (3, 5)), 'integer'), ((indptr, indices.float(), data, (3, 5)), 'integer'),
		((indptr, indices, data.to(torch.complex64), (3, 5)), 'counts'), ((indptr.numpy(), indices, data, (3, 5)), 'torch'),
	]
	for args, word in bad:
		with pytest.raises(ValueError, match=word):
			DeviceCSR(*args)
	with pytest.raises(ValueError, match='CUDA'):  # well formed, but on the host: the container is for matrices in HBM
		DeviceCSR(indptr, indices, data, (3, 5))
	import normalisr_amd.lcpm as lc
	assert lc._as_device_csr(np.ones((2, 2))) is None and lc._as_device_csr(torch.ones(2, 2)) is None


def test_route_switch_and_debug_key(monkeypatch):
	from normalisr_amd import _opts
	import normalisr_amd.lcpm as lc
	assert 'lcpm_sparse' in _opts.DEBUG_KEYS and 0 < lc.SPARSE_MAX_DENSITY <= 1
	x = np.zeros((10, 100), dtype=np.int64)
	x[:, :3] = 1
	thin, full = scipy.sparse.csr_matrix(x), scipy.sparse.csr_matrix(np.ones((10, 100), dtype=np.int64))
	monkeypatch.delenv('NRM_DEBUG', raising=False)
	monkeypatch.delenv('NRM_LCPM_SPARSE', raising=False)
	assert lc._takes_csr(thin) and (lc._takes_csr(full) == (lc.SPARSE_MAX_DENSITY >= 1))
	monkeypatch.setenv('NRM_DEBUG', 'lcpm_sparse=0')
	assert not lc._takes_csr(thin) and not lc._takes_csr(full)
	monkeypatch.setenv('NRM_DEBUG', 'lcpm_sparse=force')
	assert lc._takes_csr(thin) and lc._takes_csr(full)


def test_parser_still_accepts_lcpm_sparse_flag():
	from normalisr_amd.__main__ import build_parser
	a = vars(build_parser().parse_args(['lcpm', '-s', 'r.mtx', 'l.tsv', 's.tsv', 'c.tsv']))
	assert a['cmd'] == 'lcpm' and a['sparse'] is True and a['reads_in'] == 'r.mtx'
	from normalisr_amd import run
	assert callable(run.file_read_coo)


def test_library_declares_the_csr_entries():
	import ctypes
	from normalisr_amd import _lib
	lib = ctypes.CDLL(_lib.LIB_PATH)
	for name in ('nrm_lcpm_csr_workspace', 'nrm_lcpm_csr_count', 'nrm_lcpm_csr_colsum', 'nrm_lcpm_csr_write'):
		assert hasattr(lib, name) and name in _lib.exported_symbols(), name
	n = _lib.load().nrm_lcpm_csr_workspace(100, 1000)
	assert n >= 1000 + 4  # at least one slab of n words and one record of four
