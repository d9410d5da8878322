"""Sparse design matrices as far as they go without a GPU: the canonical CSR form of a scipy.sparse design (de_sparse.canonical_design_csr), the row filter
of de.py:93 taken from the entries instead of the dense rows, the constructor checks of de_sparse.DesignCSR, and the three C entries of
csrc/nrm_design_csr.hip declared, bound and exported."""
import os

import numpy as np
import pytest

sp = pytest.importorskip('scipy.sparse')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
	return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _canonical(m):
	from normalisr_amd.de_sparse import canonical_design_csr
	indptr, indices, data = canonical_design_csr(m)
	assert indptr.dtype == np.int64 and indices.dtype == np.int32 and indptr.shape == (m.shape[0] + 1, ) and indices.shape == data.shape
	assert indptr[0] == 0 and indptr[-1] == indices.size and (np.diff(indptr) >= 0).all()
	for i in range(m.shape[0]):  # strictly increasing columns inside a row, no stored zero
		seg = indices[indptr[i]:indptr[i + 1]]
		assert (np.diff(seg) > 0).all() and (seg >= 0).all() and (seg < m.shape[1]).all()
	assert not (data == 0).any()
	return indptr, indices, data, sp.csr_matrix((data, indices, indptr), shape=m.shape)


@pytest.mark.parametrize('dtype', [np.bool_, np.int8, np.int64, np.float32, np.float64])
def test_canonical_design_csr_equals_toarray(dtype):
	"""COO input with duplicates, unsorted CSC, stored zeros, NaN entries, every data kind: the canonical arrays densify to what toarray() gives, in fp32 for
	fp32 input and fp64 for the rest."""
	rng = np.random.default_rng(3)
	nx, n = 9, 57
	rows, cols = rng.integers(0, nx, 150), rng.integers(0, n, 150)  # (150 draws from 513 places: duplicates)
	rows[rows == 4] = 5  # a row without entries
	vals = rng.integers(1, 4, 150)
	vals[::7] = 0  # stored zeros
	want_dtype = np.float32 if dtype == np.float32 else np.float64
	coo = sp.coo_matrix((vals.astype(dtype), (rows, cols)), shape=(nx, n))
	for m in (coo, coo.tocsc(), coo.tocsr(), coo.tolil()):
		_, _, data, back = _canonical(m)
		assert data.dtype == want_dtype
		assert _same(back.toarray(), m.toarray().astype(want_dtype))
	# an unsorted CSC with explicit zeros, as slicing and arithmetic leave them
	csc = coo.tocsc()
	csc.sum_duplicates()
	for j in range(n):
		a, b = csc.indptr[j], csc.indptr[j + 1]
		csc.indices[a:b] = csc.indices[a:b][::-1].copy()
		csc.data[a:b] = csc.data[a:b][::-1].copy()
	csc.has_sorted_indices = False
	_, _, _, back = _canonical(csc)
	assert _same(back.toarray(), coo.toarray().astype(want_dtype))


def test_canonical_design_csr_keeps_nan_and_takes_empty_matrices():
	from normalisr_amd.de_sparse import canonical_design_csr
	d = np.zeros((4, 11))
	d[1, 3], d[1, 7], d[3, 0] = np.nan, 2.0, np.nan
	m = sp.coo_matrix(d)
	m.data[:] = d[m.row, m.col]
	indptr, indices, data, back = _canonical(m)
	assert np.isnan(data).sum() == 2 and _same(back.toarray(), d)
	# NaN + a duplicate stays NaN; a duplicate pair that cancels is dropped
	m = sp.coo_matrix((np.array([np.nan, 1.0, 2.0, -2.0]), (np.array([0, 0, 1, 1]), np.array([5, 5, 2, 2]))), shape=(2, 8))
	indptr, indices, data, back = _canonical(m)
	assert indices.tolist() == [5] and np.isnan(data[0]) and indptr.tolist() == [0, 1, 1]
	for shape in ((3, 5), (1, 1)):
		indptr, indices, data, back = _canonical(sp.csr_matrix(shape, dtype=np.float32))
		assert indices.size == 0 and data.dtype == np.float32 and (indptr == 0).all()
	with pytest.raises(TypeError):
		canonical_design_csr(sp.csr_matrix(np.ones((2, 2), dtype=np.complex128)))


def _filter_design(rng, nx, n, dtype):
	d = (rng.random((nx, n)) < 0.1) * rng.integers(1, 3, (nx, n))
	d = d.astype(dtype)
	d[0] = 0            # an empty row
	d[1] = 1            # a full constant row
	d[2] = 1
	d[2, n // 2] = 2    # a full row with two values
	d[4] = 0
	d[4, n - 1] = 1     # a row with one entry
	if np.dtype(dtype).kind == 'f':
		d[3] = np.nan   # a full all-NaN row
		d[5] = np.nan
		d[5, 0] = 1     # NaN and a number: two values
		d[6] = 0
		d[6, n - 1] = np.nan  # zeros and one NaN (n = 1: the NaN alone)
	return d


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32, np.bool_])
@pytest.mark.parametrize('nx,n', [(12, 40), (9, 1), (8, 2), (30, 700)])
def test_sparse_row_filter_equals_the_dense_one(dtype, nx, n):
	"""de.py:93 from the entries: k = 0 constant, 0 < k < n varying, k = n by the values (NaN equal to NaN) -- against de._varying_rows of the densified matrix."""
	from normalisr_amd import de
	for seed in range(3):
		rng = np.random.default_rng(100 * seed + nx + n)
		d = _filter_design(rng, nx, n, dtype)
		_, _, _, m = _canonical(sp.coo_matrix(d))
		want = de._varying_rows(d)
		assert np.array_equal(de._varying_rows_scipy(m), want)
		if n > 2:
			assert want[4] and not want[0] and not want[1] and want[2] == (np.dtype(dtype).kind != 'b')  # (a bool row holds one value where it is full)
			if np.dtype(dtype).kind == 'f':
				assert not want[3] and want[5] and want[6]


def test_design_csr_constructor_errors():
	"""Shape and dtype errors first, the 'must be CUDA tensors' error after them (the checks can be met with CPU tensors up to that one)."""
	torch = pytest.importorskip('torch')
	from normalisr_amd.de_sparse import DesignCSR
	ip, ix, da = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.ones(5)
	with pytest.raises(ValueError, match='shape must be'):
		DesignCSR(ip, ix, da, (3, ))
	with pytest.raises(ValueError, match='1-D torch tensor'):
		DesignCSR(ip.reshape(2, 2), ix, da, (3, 9))
	with pytest.raises(ValueError, match='1-D torch tensor'):
		DesignCSR(np.zeros(4, dtype=np.int64), ix, da, (3, 9))
	with pytest.raises(ValueError, match='integer dtype'):
		DesignCSR(ip.to(torch.float32), ix, da, (3, 9))
	with pytest.raises(ValueError, match='integer dtype'):
		DesignCSR(ip, ix.to(torch.bool), da, (3, 9))
	with pytest.raises(ValueError, match='real numbers'):
		DesignCSR(ip, ix, da.to(torch.complex64), (3, 9))
	with pytest.raises(ValueError, match=r'n_grouping \+ 1 = 4'):
		DesignCSR(ip[:3], ix, da, (3, 9))
	with pytest.raises(ValueError, match='same length'):
		DesignCSR(ip, ix, da[:4], (3, 9))
	with pytest.raises(NotImplementedError, match='2\\*\\*31 - 1 cells'):
		DesignCSR(ip, ix, da, (3, 2**31))
	for data in (da, da.to(torch.int8), da.to(torch.bool), None):
		with pytest.raises(ValueError, match='must be CUDA tensors on one device'):
			DesignCSR(ip, ix, data, (3, 9))


def test_sparse_inputs_other_than_the_design_are_refused():
	"""A sparse dt / dc, and a sparse design where only a dense one is taken, raise TypeError that names the way through -- before anything touches a GPU."""
	from normalisr_amd import de, de_sparse
	from normalisr_amd.association import association_tests
	from normalisr_amd.single5 import association_tests_single5
	from normalisr_amd import distributed
	rng = np.random.default_rng(0)
	dg, dt, dc = sp.csr_matrix((rng.random((4, 50)) < 0.2).astype(float)), rng.normal(size=(6, 50)), np.ones((1, 50))
	assert de_sparse.is_sparse_design(dg) and not de_sparse.is_sparse_design(dt) and not de_sparse.is_sparse_design(None)
	for call in (lambda: de.de(dg, sp.csr_matrix(dt), dc), lambda: de.de(dg, dt, sp.csr_matrix(dc)), lambda: association_tests(dg.toarray(), sp.csr_matrix(dt), dc),
				 lambda: association_tests(dg.toarray(), dt, sp.csr_matrix(dc))):
		with pytest.raises(TypeError, match='dense'):
			call()
	for call in (lambda: association_tests(dg, None, dc, single=5, mask=np.ones((4, 4), dtype=bool)), lambda: association_tests_single5(dg, None, dc, np.ones((4, 4), dtype=bool)),
				 lambda: distributed.de(dg, dt, dc)):
		with pytest.raises(TypeError, match=r'DesignCSR\.dense\(\)'):
			call()


def test_design_csr_entries_are_declared_bound_and_exported():
	from normalisr_amd import _lib
	lib = _lib.load()
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	for name in ('nrm_design_csr_count', 'nrm_design_csr_fill', 'nrm_design_csr_dense'):
		assert name in _lib.exported_symbols() and hasattr(lib, name) and name + '(' in hdr
	assert '#define NRM_DESIGN_CSR_BAD %d' % _lib.DESIGN_CSR_BAD in hdr
	# the entries cite the reference lines the dense entries cite
	block = hdr[hdr.index('csrc/nrm_design_csr.hip'):hdr.index('int nrm_design_csr_count(')]
	assert 'association.py:224-235' in block and 'association.py:914-918' in block
	# argument errors are answered on the host, before any launch
	assert lib.nrm_design_csr_count(0, 0, 0, 0, 4, 100, 0, 0, 64, 0, 0) == _lib.NRM_E_ARG
	assert lib.nrm_design_csr_fill(0, 0, 0, 0, 4, 100, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) == _lib.NRM_E_ARG
	assert lib.nrm_design_csr_dense(0, 0, 0, 0, 4, 100, 0, 0, 100, 0) == _lib.NRM_E_ARG
