"""Sparse design matrices on the GPU (csrc/nrm_design_csr.hip, de_sparse.DesignCSR / Lists.from_csr, the routes of de and association_tests).

The contract under test: for a canonical CSR design every array the CSR kernels produce is byte for byte what the dense kernels produce from the densified
matrix -- so everything downstream of the lists computes the same bits -- and a malformed matrix ends in a ValueError, never in an access out of range.
Integer work: torch.equal / np.array_equal throughout, tolerances only against the oracle's arithmetic."""
import os
import sys

import numpy as np
import pytest

import oracle
from test_gpu_parity import close, p_close  # noqa: F401

pytestmark = pytest.mark.gpu

sp = pytest.importorskip('scipy.sparse')
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

SHAPES = [(1, 1), (5, 2047), (64, 2048), (70, 2049), (130, 4100), (1030, 6145)]
KINDS = [('binary', np.float32), ('binary', np.float64), ('valued', np.float32), ('valued', np.float64), ('none', None)]


@pytest.fixture(scope='module')
def norm():
	import normalisr_amd.normalisr as norm
	return norm


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd.engine import get_engine
	return get_engine()


def _dense_design(rng, nx, n, kind, dtype):
	"""The smallest designs the kernels can go wrong at: a row without entries, a row with every cell set (nx >= 64: it keeps the density under 1/16), entries
	at cells 0, 2047, 2048 and n - 1 where they exist, a list of more than 64 x 8 entries in one chunk."""
	d = (rng.random((nx, n)) < 0.01).astype(np.float64)
	r = lambda i: min(i, nx - 1)
	for k in (0, 2047, 2048, n - 1):
		if k < n:
			d[r(2), k] = 1
	if n >= 600:
		d[r(4), 5:5 + 560] = 1       # 560 > 64 * 8 entries of one row in chunk 0
	if n >= 4100:
		d[r(5), 2048:2048 + 530] = 1  # and in a later chunk
	if nx >= 64:
		d[7] = 1                      # every cell set
	if nx > 1:
		d[r(3)] = 0                   # no entry
	if kind == 'valued':
		d *= rng.uniform(0.5, 2.0, d.shape)
		d[r(2), 0] = 1.0
		if nx > 1:
			d[0, n // 2] = -1.25
	return d.astype(dtype or np.float64)


def _csr_arrays(d, rng, stored_zeros):
	"""Canonical CSR of a dense design; stored_zeros: some cells that hold 0 are stored too (legal, and not entries)."""
	stored = d != 0
	if stored_zeros:
		stored |= (rng.random(d.shape) < 0.005)
		stored[min(3, d.shape[0] - 1)] |= (rng.random(d.shape[1]) < 0.01) if d.shape[0] > 1 else False  # the row without entries stores zeros only
	ii, kk = np.nonzero(stored)
	indptr = np.zeros(d.shape[0] + 1, dtype=np.int64)
	np.add.at(indptr, ii + 1, 1)
	return np.cumsum(indptr), kk.astype(np.int32), d[ii, kk]


def _design_csr(d, rng, kind):
	import torch
	from normalisr_amd.de_sparse import DesignCSR
	indptr, indices, data = _csr_arrays(d, rng, stored_zeros=kind != 'none')
	t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
	return DesignCSR(t(indptr), t(indices), None if kind == 'none' else t(data), d.shape)


_FIELDS = ('row_ptr', 'slot2x')
_ELL_FIELDS = ('sig', 'w', 'base')


def _same_lists(a, b, ell):
	import torch
	assert (a.ok, a.nnz, a.padded, a.bits, a.binary, a.ngroups) == (b.ok, b.nnz, b.padded, b.bits, b.binary, b.ngroups)
	for f in _FIELDS:
		assert torch.equal(getattr(a, f), getattr(b, f)), f
	if not a.ok:
		return
	assert torch.equal(a.cells[:a.nnz], b.cells[:a.nnz])
	assert (a.row_vals is None) == (b.row_vals is None) == a.binary
	if not a.binary:
		assert torch.equal(a.row_vals[:a.nnz].view(torch.int64), b.row_vals[:a.nnz].view(torch.int64))  # (bits: a NaN equals itself)
	if ell:
		for f in _ELL_FIELDS:
			assert torch.equal(getattr(a, f), getattr(b, f)), f
		assert torch.equal(a.ell[:a.padded], b.ell[:a.padded])
		assert (a.vals is None) == (b.vals is None) == a.binary
		if not a.binary:
			assert torch.equal(a.vals[:a.padded].view(torch.int64), b.vals[:a.padded].view(torch.int64))
	else:
		assert a.ell is None and b.ell is None


@pytest.mark.parametrize('kind,dtype', KINDS)
@pytest.mark.parametrize('nx,n', SHAPES)
def test_lists_from_csr_are_the_bytes_of_the_dense_lists(eng, nx, n, kind, dtype):
	"""Lists.from_csr against Lists(eng, dense) on the same design, ELL and CSR-only, built twice; the reader of tests/tools gives the dense matrix back."""
	import torch
	import lists_reference as lr
	from normalisr_amd import de_sparse
	rng = np.random.default_rng(1000 * nx + n)
	d = _dense_design(rng, nx, n, 'binary' if kind == 'none' else kind, dtype)
	csr = _design_csr(d, rng, kind)
	d_x = torch.from_numpy(d).cuda()
	nnz = np.count_nonzero(d)
	md = de_sparse.MAX_DENSITY if nnz <= de_sparse.MAX_DENSITY * nx * n else 1.0  # (the two smallest shapes cannot hold these rows under 1/16)
	assert md == de_sparse.MAX_DENSITY or nx < 64
	want = de_sparse.Lists(eng, d_x, max_density=md)
	got = de_sparse.Lists.from_csr(eng, csr, max_density=md)
	assert want.ok and want.nnz == nnz and want.binary == (not ((d != 0) & (d != 1)).any())
	_same_lists(got, want, True)
	_same_lists(de_sparse.Lists.from_csr(eng, csr, max_density=md), got, True)  # the same bits run to run
	md1 = max(md, 0.25)
	_same_lists(de_sparse.Lists.from_csr(eng, csr, ell=False, max_density=md1), de_sparse.Lists(eng, d_x, ell=False, max_density=md1), False)
	if nx * n <= 6_000_000:  # (the reader is a Python loop)
		back, padded = lr.decode(nx, n, got.binary, got.ell.cpu().numpy(), None if got.binary else got.vals.cpu().numpy(), got.base.cpu().numpy(), got.w.cpu().numpy(),
								 got.slot2x.cpu().numpy(), got.sig.cpu().numpy(), got.ngroups)
		assert np.array_equal(back, d.astype(np.float64)) and padded == got.padded
	# above the limit: refused with the right count, on both sides alike
	low = de_sparse.Lists.from_csr(eng, csr, max_density=0.5 * nnz / (nx * n))
	assert not low.ok and low.nnz == nnz and not hasattr(low, 'cells')


def test_entry_description_empty_and_dense_designs_and_the_cache(eng):
	import torch
	from normalisr_amd import de_sparse, _lib
	from normalisr_amd.de_sparse import DesignCSR, Lists
	t = lambda a, dt: torch.tensor(a, dtype=dt, device='cuda')
	# the three entries of the dense test: 1, -2, NaN, then inf
	mk = lambda v: DesignCSR(t([0, 0, 1, 2, 2, 3], torch.int64), t([7, 4099, 2048], torch.int32), t([1.0, v, float('nan')], torch.float32), (5, 4100))
	x = torch.zeros((5, 4100), device='cuda')
	x[1, 7], x[2, 4099], x[4, 2048] = 1.0, -2.0, float('nan')
	lst = Lists.from_csr(eng, mk(-2.0), max_density=1.0)
	assert lst.ok and lst.nnz == 3 and lst.bits == (_lib.DESIGN_HAS1 | _lib.DESIGN_NOTONE | _lib.DESIGN_NEG | _lib.DESIGN_NAN) and not lst.binary
	_same_lists(lst, Lists(eng, x, max_density=1.0), True)
	assert Lists.from_csr(eng, mk(float('inf')), max_density=1.0).bits & _lib.DESIGN_GT1
	# nothing stored, and zeros stored only: an empty design
	for ix, da in (([], []), ([3, 9], [0.0, 0.0])):
		ip = [0, 0, len(ix), len(ix), len(ix), len(ix)]
		lst = Lists.from_csr(eng, DesignCSR(t(ip, torch.int64), t(ix, torch.int32), t(da, torch.float64), (5, 4100)))
		assert not lst.ok and lst.nnz == 0 and lst.bits == 0
	# every cell set, no data at all: above the limit, counted right
	full = DesignCSR(torch.arange(0, 41 * 3000, 3000, device='cuda'), torch.arange(3000, dtype=torch.int32, device='cuda').repeat(40), None, (40, 3000))
	lst = Lists.from_csr(eng, full)
	assert not lst.ok and lst.nnz == 40 * 3000 and not hasattr(lst, 'ell') and lst.bits == _lib.DESIGN_HAS1
	# integer and bool data, int32 indptr, int64 indices: cast on the device
	rng = np.random.default_rng(5)
	d = (rng.random((40, 5000)) < 0.02).astype(np.float32)
	indptr, indices, data = _csr_arrays(d, rng, True)
	want = Lists(eng, torch.from_numpy(d).cuda())
	for dt in (torch.int8, torch.bool, torch.int64, torch.float16):
		c = DesignCSR(torch.from_numpy(indptr).cuda().to(torch.int32), torch.from_numpy(indices).cuda().to(torch.int64), torch.from_numpy(data).cuda().to(dt), d.shape)
		_same_lists(Lists.from_csr(eng, c), want, True)
	# the caches: the same object in the same state pays once; an in-place write, or another object with the same content: listed again
	c = DesignCSR(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(data).cuda(), d.shape)
	a = de_sparse.lists_for(eng, c)
	assert de_sparse.lists_for(eng, c) is a
	_same_lists(a, want, True)
	c.data[0] = 2.0
	b = de_sparse.lists_for(eng, c)
	assert b is not a and not b.binary and b.nnz in (a.nnz, a.nnz + 1)
	from normalisr_amd.single1 import _lists_for
	s = _lists_for(eng, c)
	assert _lists_for(eng, c) is s and s.ell is None and s.nnz == b.nnz
	# a torch.sparse_csr tensor is taken wherever a DesignCSR is
	ts = torch.sparse_csr_tensor(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda().to(torch.int64), torch.from_numpy(data).cuda(), size=d.shape)
	_same_lists(Lists.from_csr(eng, ts), want, True)
	assert de_sparse.lists_for(eng, ts) is de_sparse.lists_for(eng, ts)


def _malformed(name, indptr, indices, n):
	indptr, indices = indptr.copy(), indices.copy()
	nnz = indices.size
	row = int(np.argmax(np.diff(indptr) >= 3))  # a row with at least three stored entries
	a = int(indptr[row])
	if name == 'indptr[0] != 0':
		indptr[0] = 1
	elif name == 'decreasing indptr':
		indptr[row + 1], indptr[row + 2] = indptr[row + 2], indptr[row + 1] - 1
	elif name == 'indptr[-1] < nnz':
		indptr[-1] = nnz - 1
	elif name == 'indptr[-1] > nnz':
		indptr[-1] = nnz + 100000
	elif name == 'indptr far out of range':
		indptr[row + 1:] += 1 << 40
	elif name == 'negative indptr':
		indptr[1] = -5
	elif name == 'column == n':
		indices[int(indptr[row + 1]) - 1] = n
	elif name == 'column far beyond n':
		indices[int(indptr[row + 1]) - 1] = 2**31 - 1
	elif name == 'column < 0':
		indices[a] = -1
	elif name == 'repeated column':
		indices[a + 1] = indices[a]
	elif name == 'descending columns':
		indices[a], indices[a + 1] = indices[a + 1], indices[a]
	else:
		raise KeyError(name)
	return indptr, indices


MALFORMED = ['indptr[0] != 0', 'decreasing indptr', 'indptr[-1] < nnz', 'indptr[-1] > nnz', 'indptr far out of range', 'negative indptr', 'column == n',
			 'column far beyond n', 'column < 0', 'repeated column', 'descending columns']


@pytest.mark.parametrize('name', MALFORMED)
def test_malformed_csr_is_a_value_error(eng, norm, name):
	"""The count kernel rejects without addressing anything through an unchecked value: a ValueError with the module's message from the list builder, from
	dense() and from the public call; the process goes on and a valid design passes afterwards."""
	import torch
	from normalisr_amd import de_sparse
	from normalisr_amd.de_sparse import DesignCSR, Lists
	rng = np.random.default_rng(11)
	nx, n = 70, 2049
	d = _dense_design(rng, nx, n, 'valued', np.float32)
	indptr, indices, data = _csr_arrays(d, rng, True)
	bad_ip, bad_ix = _malformed(name, indptr, indices, n)
	t = lambda a: torch.from_numpy(a).cuda()
	bad = DesignCSR(t(bad_ip), t(bad_ix), t(data), d.shape)
	msg = 'Malformed CSR design matrix'
	assert de_sparse.MALFORMED_DESIGN_CSR.startswith(msg)
	for data_none in (False, True):
		with pytest.raises(ValueError, match=msg):
			Lists.from_csr(eng, DesignCSR(bad.indptr, bad.indices, None, d.shape) if data_none else bad)
	with pytest.raises(ValueError, match=msg):
		Lists.from_csr(eng, bad, ell=False, max_density=0.25)
	with pytest.raises(ValueError, match=msg):
		bad.dense()
	dt, dc = rng.normal(size=(8, n)), np.ones((1, n))
	for single in (0, 1, 4):
		with pytest.raises(ValueError, match=msg):
			norm.de(bad, dt, dc, single=single)
	torch.cuda.synchronize()
	good = DesignCSR(t(indptr), t(indices), t(data), d.shape)
	_same_lists(Lists.from_csr(eng, good), Lists(eng, torch.from_numpy(d).cuda()), True)
	assert np.array_equal(good.dense().cpu().numpy(), d)


@pytest.mark.parametrize('kind,dtype', KINDS)
@pytest.mark.parametrize('out', ['float32', 'float64'])
def test_design_csr_dense_equals_toarray(eng, kind, dtype, out):
	"""nrm_design_csr_dense into fp32 and fp64 outputs with a padded leading dimension: toarray(), zeros in the padding; DesignCSR.dense() runs it once per state."""
	import torch
	from normalisr_amd import _lib, engine as _engine
	rng = np.random.default_rng(21)
	nx, n, ldo = 70, 2049, 2049 + 13
	d = _dense_design(rng, nx, n, 'binary' if kind == 'none' else kind, dtype)
	csr = _design_csr(d, rng, kind)
	odt = getattr(torch, out)
	buf = torch.full((nx, ldo), 7.0, dtype=odt, device='cuda')
	indptr, indices, data, code, _ = csr._ready(eng)
	_lib.check(eng.lib.nrm_design_csr_dense(indptr.data_ptr(), indices.data_ptr(), _engine.ptr(data), code, nx, n, buf.data_ptr(), _engine.dtype_code(buf), ldo, eng._stream()))
	h = buf.cpu().numpy()
	assert np.array_equal(h[:, :n], d.astype(out)) and not h[:, n:].any()
	a = csr.dense(odt)
	assert a.shape == (nx, n) and a.dtype == odt and np.array_equal(a.cpu().numpy(), d.astype(out)) and csr.dense(odt) is a
	assert csr.dense().dtype == (torch.float32 if dtype == np.float32 else torch.float64)
	if csr.data is not None:
		csr.data[0] += 1.0  # written to in place: scattered again
		assert csr.dense(odt) is not a


def _same_results(got, want):
	assert len(got) == len(want) == 5
	for g, w in zip(got, want):
		assert (g is None) == (w is None)
		if g is not None:
			assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True)


def _screen(rng, ydtype, nc, low_moi=False):
	nx, ny, n = 70, 64, 4100
	dg = (rng.random((nx, n)) < (1.0 / nx if low_moi else 0.01)).astype(np.float64)
	dg[9] = 0  # a constant design row: de drops and re-inflates it
	dt = (rng.normal(size=(ny, n)) + 0.5 * dg[0] + 0.4 * dg[1]).astype(ydtype)
	dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	return dg, dt, dc


def _no_dense_design(monkeypatch, m):
	"""From here on neither the device nor the host may densify a design."""
	from normalisr_amd.de_sparse import DesignCSR

	def boom(*a, **ka):
		raise AssertionError('a dense design was formed')
	monkeypatch.setattr(DesignCSR, 'dense', boom)
	for name in ('toarray', 'todense'):
		monkeypatch.setattr(m, name, boom)
		monkeypatch.setattr(type(m), name, boom)


@pytest.mark.parametrize('ydtype', [np.float32, np.float64])
def test_de_from_a_sparse_design_without_a_dense_one(norm, eng, monkeypatch, ydtype):
	"""single=0 on the sparse-design kernel and the two list routes of single=1 from a scipy matrix and from a DesignCSR: no dense design on either side, and
	the results of the dense-input call -- equal arrays: identical lists go into identical kernels (the dense call itself is first checked to repeat its bits)."""
	from normalisr_amd.de_sparse import DesignCSR
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	rng = np.random.default_rng(7)
	dg, dt, dc = _screen(rng, ydtype, 3)
	dg1, _, dc12 = _screen(rng, ydtype, 12, low_moi=True)
	dc2 = dc12[-2:]
	calls = [(dg, dc, dict()), (dg, dc, dict(lowmem=False)), (dg1, dc2, dict(single=1)), (dg1, dc12, dict(single=1)), (dg1, dc2, dict(single=1, lowmem=False)),
			 (dg1, dc12, dict(single=1, lowmem=False))]
	want = []
	for d, c, ka in calls:
		want.append(norm.de(d, dt, c, **ka))
		_same_results(norm.de(d, dt, c, **ka), want[-1])  # the parent's route repeats its bits
		if not ka.get('single'):
			assert 'the sparse-design kernel' in eng._tls.path
	ms = [sp.csr_matrix(d) for d, _, _ in calls]
	cs = [DesignCSR.from_scipy(sp.coo_matrix(d)) for d, _, _ in calls]
	_no_dense_design(monkeypatch, ms[0])
	for (d, c, ka), m, csr, w in zip(calls, ms, cs, want):
		for design in (m, csr):
			eng._tls.path = None
			got = norm.de(design, dt, c, **ka)
			_same_results(got, w)
			if not ka.get('single'):
				assert 'the sparse-design kernel' in eng._tls.path
		assert (got[0][9] == 1).all() and (got[1][9] == 0).all()


def test_routes_that_densify_do_it_once_on_the_device(norm, eng, monkeypatch):
	"""single=4, single=0 off the sparse-design kernel (switched off; a 20 %-dense design; dy=None), single=1 with a negative entry: the results of the
	dense-input call, from ONE DesignCSR.dense() per call and no toarray() on the host."""
	import torch
	from normalisr_amd.association import association_tests
	from normalisr_amd.de_sparse import DesignCSR
	rng = np.random.default_rng(8)
	dg, dt, dc = _screen(rng, np.float64, 3)
	dg20 = (rng.random(dg.shape) < 0.2).astype(np.float64)
	dg1, _, _ = _screen(rng, np.float64, 3, low_moi=True)
	k = int(np.nonzero((dg1 != 0).sum(axis=0) == 0)[0][0])
	dg1[4, k] = -1.0  # a negative entry in a cell of its own: the masked-Gram fallback
	ran = []
	real = DesignCSR.dense
	monkeypatch.setattr(DesignCSR, 'dense', lambda self, *a, **ka: (ran.append(1), real(self, *a, **ka))[1])

	def both(call, d):
		want = call(d)
		for design in (sp.csr_matrix(d), DesignCSR.from_scipy(sp.csr_matrix(d)), torch.from_numpy(d).cuda().to_sparse_csr()):
			if hasattr(design, 'toarray'):
				monkeypatch.setattr(design, 'toarray', None)
			del ran[:]
			got = call(design)
			assert len(ran) == 1
			assert len(got) == len(want)
			for g, w in zip(got, want):
				assert (g is None) == (w is None) and (g is None or np.array_equal(g, w, equal_nan=True))
	both(lambda d: norm.de(d, dt, dc, single=4), dg)
	both(lambda d: norm.de(d, dt, dc, single=4, lowmem=False), dg)
	both(lambda d: norm.de(d, dt, dc, single=1), dg1)
	both(lambda d: association_tests(d, None, dc), dg)
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	both(lambda d: norm.de(d, dt, dc), dg20)
	monkeypatch.setenv('NRM_DE_SPARSE', '0')
	both(lambda d: norm.de(d, dt, dc), dg)
	both(lambda d: norm.de(d, dt, dc, lowmem=False), dg)


def test_whole_problem_entries_take_the_design_densified_on_the_host(norm, monkeypatch, caplog):
	"""NRM_HOST_ENTRY=1 (what a process without torch does too): the library's whole-problem C entries take dense host buffers, so a scipy design is densified
	on the host -- a debug-level log line says so -- and the results are the dense-input call's."""
	import logging
	rng = np.random.default_rng(12)
	dg, dt, dc = _screen(rng, np.float64, 3)
	dg1, _, _ = _screen(rng, np.float64, 3, low_moi=True)
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	for d, ka in ((dg, dict()), (dg1, dict(single=1)), (dg, dict(single=4))):
		want = norm.de(d, dt, dc, **ka)
		caplog.clear()
		with caplog.at_level(logging.DEBUG):
			got = norm.de(sp.csr_matrix(d), dt, dc, **ka)
		assert 'sparse design densified on the host' in caplog.text
		_same_results(got, want)


def test_sparse_design_against_the_reference_arithmetic(norm, monkeypatch):
	"""single=0 (sparse-design kernel) and single=1 from a scipy design against the oracle on the densified design, with the tolerances the dense-input tests of
	the same paths hold (tests/test_gpu_round5.py)."""
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	rng = np.random.default_rng(9)
	dg, dt, dc = _screen(rng, np.float64, 3)
	got = norm.de(sp.csc_matrix(dg), dt, dc, lowmem=False)
	ref = oracle.de(dg, dt, dc, lowmem=False)
	assert p_close(got[0], ref[0]) and close(got[1], ref[1], 1e-6, 1e-12) and close(got[2], ref[2], 1e-6, 1e-9) and close(got[3], ref[3], 1e-9, 1e-15) and close(got[4], ref[4], 1e-7, 1e-15)  # (the constant row: variance 0 on both sides)
	dg1, dt1, dc1 = _screen(rng, np.float64, 5, low_moi=True)
	got = norm.de(sp.coo_matrix(dg1), dt1, dc1, single=1)
	ref = oracle.de(dg1, dt1, dc1, single=1)
	assert p_close(got[0], ref[0]) and close(got[1], ref[1], 1e-9, 1e-12) and close(got[3], ref[3], floor=1e-15) and close(got[4], ref[4], floor=1e-15)


def test_rejections_and_torch_sparse_csr(norm, monkeypatch):
	"""Plans, single=5 and a sparse dy take no sparse matrix: TypeError naming the way through.  A torch.sparse_csr design gives the results of the DesignCSR built
	from its parts."""
	import torch
	from normalisr_amd.association import association_tests
	from normalisr_amd.de_sparse import DesignCSR
	from normalisr_amd.single1 import Single1Plan
	from normalisr_amd.single4 import Single4Plan
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	rng = np.random.default_rng(10)
	dg, dt, dc = _screen(rng, np.float32, 3)
	csr = DesignCSR.from_scipy(sp.csr_matrix(dg))
	d_t = torch.from_numpy(dt).cuda()
	for plan in (Single1Plan, Single4Plan):
		for design in (csr, sp.csr_matrix(dg)):
			with pytest.raises(TypeError, match=r'DesignCSR\.dense\(\)'):
				plan(design, d_t, dc)
	with pytest.raises(TypeError, match=r'DesignCSR\.dense\(\)'):
		association_tests(csr, None, dc, single=5, mask=np.ones((70, 70), dtype=bool))
	for dy in (sp.csr_matrix(dt), d_t.to_sparse_csr()):
		with pytest.raises(TypeError, match='dense'):
			norm.de(csr, dy, dc)
	dg1, _, _ = _screen(rng, np.float32, 3, low_moi=True)
	for d, ka in ((dg, dict()), (dg1, dict(single=1)), (dg, dict(single=4))):
		c = DesignCSR.from_scipy(sp.csr_matrix(d))
		ts = torch.sparse_csr_tensor(c.indptr, c.indices.to(torch.int64), c.data, size=c.shape)
		_same_results(norm.de(ts, dt, dc, **ka), norm.de(c, dt, dc, **ka))
