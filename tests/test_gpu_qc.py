"""GPU: quality control on the device (normalisr_amd/qc.py, csrc/nrm_qc.hip) -- qc_reads in every input form against what the reference returned (golden
G20, tests/golden/make_g20.py), the statistics, decision and subset kernels alone against numpy (tests/qc_numpy.py), the resident chain reads -> qc_reads ->
subset -> lcpm, and the three sub-commands as child processes.  Every result here is an integer, a boolean, a name or a copy: all comparisons are exact.
No test here relies on a fault: a malformed matrix is an ordinary input to a checked entry and must come back as a ValueError."""
import os
import subprocess
import sys

import numpy as np
import pytest

import qc_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('a', 'b', 'c')
NP_OF = {'int64': np.int64, 'int32': np.int32, 'int16': np.int16, 'uint8': np.uint8}


@pytest.fixture(scope='module')
def torch():
	import torch
	return torch


@pytest.fixture(scope='module')
def qc():
	import normalisr_amd.qc as qc
	return qc


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd import engine
	return engine.get_engine()


def up(torch, a):
	return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def dev_csr(torch, m, vdtype=np.int32):
	"""A DeviceCSR of a scipy CSR matrix exactly as stored (stored zeros stay)."""
	from normalisr_amd.lcpm import DeviceCSR
	return DeviceCSR(up(torch, m.indptr.astype(np.int64)), up(torch, m.indices.astype(np.int32)), up(torch, m.data.astype(vdtype)), m.shape)


def host_csr(d):
	import scipy.sparse
	return scipy.sparse.csr_matrix((d.data.cpu().numpy(), d.indices.cpu().numpy(), d.indptr.cpu().numpy()), shape=d.shape)


# ---- qc_reads against the reference ---------------------------------------------------------------------------------------------------------------------------

def test_golden_qc_reads_every_input_form(golden, qc, torch):
	scipy_sparse = pytest.importorskip('scipy.sparse')
	g = golden('G20_qc')
	for name in CASES:
		reads, params = g[name + '_reads'], tuple(float(v) for v in g[name + '_params'])
		assert reads.max() < 256
		m = scipy_sparse.csr_matrix(reads)
		forms = {
			'numpy int64': reads.astype(np.int64), 'torch int32': up(torch, reads.astype(np.int32)), 'torch uint8': up(torch, reads.astype(np.uint8)),
			'scipy csr': m, 'scipy coo': scipy_sparse.coo_matrix(reads), 'DeviceCSR': dev_csr(torch, m), 'DeviceCSR uint8': dev_csr(torch, m, np.uint8),
			'torch.sparse_csr': torch.sparse_csr_tensor(up(torch, m.indptr.astype(np.int64)), up(torch, m.indices.astype(np.int64)), up(torch, m.data.astype(np.int64)),
														size=m.shape),
		}
		for form, x in forms.items():
			tag = (name, form)
			genes, cells, info = qc.qc_reads(x, *params, return_info=True)
			assert isinstance(genes, np.ndarray) and genes.dtype == np.int64 and cells.dtype == np.int64, tag
			assert np.array_equal(genes, g[name + '_genes']) and np.array_equal(cells, g[name + '_cells']), tag
			assert info['iterations'] == int(g[name + '_iterations']), tag
			assert info['gene_mask'].dtype == np.bool_ and np.array_equal(np.flatnonzero(info['gene_mask']), genes), tag
			assert np.array_equal(np.flatnonzero(info['cell_mask']), cells), tag
			dg, dc = qc.qc_reads(x, *params, device_out=True)
			assert dg.is_cuda and dc.is_cuda and dg.dtype == torch.int64 and dc.dtype == torch.int64, tag
			assert np.array_equal(dg.cpu().numpy(), genes) and np.array_equal(dc.cpu().numpy(), cells), tag
			again = qc.qc_reads(x, *params)
			assert len(again) == 2 and np.array_equal(again[0], genes) and np.array_equal(again[1], cells), tag


def test_golden_qc_reads_errors_and_negative_entries(golden, qc, torch):
	import scipy.sparse
	reads = golden('G20_qc')['b_reads']
	for x in (reads, up(torch, reads), dev_csr(torch, scipy.sparse.csr_matrix(reads))):
		with pytest.raises(RuntimeError, match='All genes removed'):  # everything goes in one decision: the gene error comes first
			qc.qc_reads(x, 10**9, 0, 0, 10**9, 0, 0)
		with pytest.raises(RuntimeError, match='All cells removed'):
			qc.qc_reads(x, 0, 0, 0, 10**9, 0, 0)
		with pytest.raises(RuntimeError, match='All genes removed'):
			qc.qc_reads(x, 0, 0, 1.0, 0, 0, 0)  # no gene is seen in every cell
	bad = reads.astype(np.int64)
	bad[5, 7] = -3
	m = scipy.sparse.csr_matrix(reads).astype(np.int32)
	m.data[11] = -1
	for x in (up(torch, bad), up(torch, bad.astype(np.int16)), dev_csr(torch, m)):
		with pytest.raises(ValueError, match='Negative'):
			qc.qc_reads(x, 0, 0, 0, 0, 0, 0)


# ---- the statistics kernels alone ---------------------------------------------------------------------------------------------------------------------------------

def mask_sets(rng, rows, n):
	yield 'all alive', np.ones(rows, dtype=bool), np.ones(n, dtype=bool)
	yield 'random', rng.random(rows) < 0.7, rng.random(n) < 0.7
	if rows > 32:
		g = rng.random(rows) < 0.7
		g[:32] = False
		yield 'a whole row tile dead', g, rng.random(n) < 0.7
	if n > 1024:
		c = rng.random(n) < 0.7
		c[:1024] = False
		yield 'every cell of a chunk dead', rng.random(rows) < 0.7, c
	yield 'one of each', np.arange(rows) == rows - 1, np.arange(n) == n // 2


class Stats:
	"""The raw entries on buffers of their own."""

	def __init__(self, torch, eng, rows, n):
		self.torch, self.eng, self.rows, self.n = torch, eng, rows, n
		self.buf = torch.full((2 * rows + 2 * n + 2, ), -7, dtype=torch.int64, device='cuda')
		self.work = torch.empty((int(eng.lib.nrm_qc_stats_workspace(rows, n)), ), dtype=torch.int64, device='cuda')

	def _out(self, g, c):
		rows, n, b = self.rows, self.n, self.buf
		self.g, self.c = up(self.torch, g.astype(np.uint8)), up(self.torch, c.astype(np.uint8))
		parts = (b[:rows], b[rows:2 * rows], b[2 * rows:2 * rows + n], b[2 * rows + n:2 * rows + 2 * n], b[2 * rows + 2 * n:])
		return (self.g.data_ptr(), self.c.data_ptr()) + tuple(p.data_ptr() for p in parts) + (self.work.data_ptr(), self.eng._stream())

	def _read(self):
		rows, n = self.rows, self.n
		h = self.buf.cpu().numpy()
		return (h[:rows], h[rows:2 * rows], h[2 * rows:2 * rows + n], h[2 * rows + n:2 * rows + 2 * n]), h[2 * rows + 2 * n:]

	def dense(self, x, code, g, c):
		from normalisr_amd import _lib
		_lib.check(self.eng.lib.nrm_qc_stats(x.data_ptr(), code, self.rows, self.n, x.stride(0), *self._out(g, c)))
		return self._read()

	def csr(self, d, code, g, c):
		from normalisr_amd import _lib
		_lib.check(self.eng.lib.nrm_qc_csr_stats(d.indptr.data_ptr(), d.indices.data_ptr(), d.data.data_ptr(), code, self.rows, self.n, int(d.data.numel()), *self._out(g, c)))
		return self._read()


def same_where_alive(got, want, g, c):
	return all(np.array_equal(a[m], b[m]) for a, b, m in zip(got, want, (g, g, c, c)))


@pytest.mark.parametrize('dtype', ['int64', 'int32', 'int16', 'uint8'])
def test_stats_kernel_dense_against_numpy(torch, eng, dtype):
	from normalisr_amd import _lib
	from normalisr_amd.lcpm import _CODES
	code = _CODES['torch.' + dtype]
	rng = np.random.default_rng(100 + sorted(NP_OF).index(dtype))
	for rows in (1, 31, 33, 97):
		for n in (1, 255, 257, 1025):
			x = (rng.poisson(0.6, (rows, n)) * rng.integers(1, 60, (rows, n))).astype(NP_OF[dtype])
			layouts = {'contiguous': up(torch, x)}
			ld = n + 3 if (n + 3) % 4 else n + 2
			pitched = torch.zeros((rows, ld), dtype=getattr(torch, dtype), device='cuda')  # a pitch that is no multiple of 4 elements, rows off the 16-byte grid
			pitched[:, 1:n + 1] = layouts['contiguous']
			layouts['pitched'] = pitched[:, 1:n + 1]
			if n % 4 == 1:
				wide = torch.zeros((rows, n + 3), dtype=getattr(torch, dtype), device='cuda')  # aligned rows and a ragged last chunk
				wide[:, :n] = layouts['contiguous']
				layouts['aligned pitch'] = wide[:, :n]
			st = Stats(torch, eng, rows, n)
			for what, g, c in mask_sets(rng, rows, n):
				want = qc_numpy.stats(x, g, c)
				for layout, t in layouts.items():
					got, info = st.dense(t, code, g, c)
					assert same_where_alive(got, want, g, c), (rows, n, what, layout)
					assert info[0] == 0 and info[1] == 0, (rows, n, what, layout)
	# totals beyond 2^31 and 2^32, and the negative flag: only an ALIVE negative entry counts
	if dtype == 'int64':
		x = (rng.random((33, 257)) < 0.5).astype(np.int64) * 3000000000
		g, c = rng.random(33) < 0.8, rng.random(257) < 0.8
		want = qc_numpy.stats(x, g, c)
		assert want[0].max() > 2**32 and want[2].max() > 2**32
		got, info = Stats(torch, eng, 33, 257).dense(up(torch, x), code, g, c)
		assert same_where_alive(got, want, g, c) and info[0] == 0
	if dtype != 'uint8':
		x = rng.integers(0, 5, (40, 300)).astype(NP_OF[dtype])
		x[7, 123] = -2
		g, c = np.ones(40, dtype=bool), np.ones(300, dtype=bool)
		st = Stats(torch, eng, 40, 300)
		assert st.dense(up(torch, x), code, g, c)[1][0] == 1
		g[7] = False
		got, info = st.dense(up(torch, x), code, g, c)
		assert info[0] == 0 and same_where_alive(got, qc_numpy.stats(x, g, c), g, c)
		g[7], c[123] = True, False
		assert st.dense(up(torch, x), code, g, c)[1][0] == 0


@pytest.mark.parametrize('dtype', ['int64', 'int32', 'int16', 'uint8'])
def test_stats_kernel_csr_against_numpy(torch, eng, dtype):
	import scipy.sparse
	from normalisr_amd.lcpm import _CODES
	code = _CODES['torch.' + dtype]
	rng = np.random.default_rng(200 + sorted(NP_OF).index(dtype))
	for rows in (1, 31, 33, 97):
		for n in (1, 255, 257, 1025, 4097):
			x = np.minimum(rng.poisson(0.5, (rows, n)) * rng.integers(1, 60, (rows, n)), 255).astype(np.int64)  # (every dtype holds them)
			if rows > 2:
				x[1] = 0  # an empty row
				x[2] = 1 + rng.integers(0, 5, n)  # a full row
			m = scipy.sparse.csr_matrix(x)
			keep = m.data.copy()
			m.data[::3] = 0  # stored zeros: legal, and they count as zeros
			x0 = m.toarray()
			d, d0 = dev_csr(torch, scipy.sparse.csr_matrix((keep, m.indices, m.indptr), shape=m.shape), NP_OF[dtype]), dev_csr(torch, m, NP_OF[dtype])
			assert d0.data.numel() == d.data.numel()
			st = Stats(torch, eng, rows, n)
			for what, g, c in mask_sets(rng, rows, n):
				for mat, dense in ((d, x), (d0, x0)):
					got, info = st.csr(mat, code, g, c)
					assert same_where_alive(got, qc_numpy.stats(dense, g, c), g, c), (rows, n, what)
					assert info[0] == 0 and info[1] == 0, (rows, n, what)
	if dtype == 'int64':
		x = (rng.random((33, 257)) < 0.3).astype(np.int64) * 3000000000
		g, c = rng.random(33) < 0.8, rng.random(257) < 0.8
		want = qc_numpy.stats(x, g, c)
		assert want[0].max() > 2**32 and want[2].max() > 2**32
		got, info = Stats(torch, eng, 33, 257).csr(dev_csr(torch, scipy.sparse.csr_matrix(x), np.int64), code, g, c)
		assert same_where_alive(got, want, g, c) and info[0] == 0
	if dtype != 'uint8':
		x = rng.integers(0, 3, (40, 300)).astype(np.int64)
		x[7, 123] = 4
		m = scipy.sparse.csr_matrix(x)
		m.data[np.flatnonzero(m.data == 4)[0]] = -2
		d = dev_csr(torch, m, NP_OF[dtype])
		g, c = np.ones(40, dtype=bool), np.ones(300, dtype=bool)
		st = Stats(torch, eng, 40, 300)
		assert st.csr(d, code, g, c)[1][0] == 1
		g[7] = False
		assert st.csr(d, code, g, c)[1][0] == 0
		g[7], c[123] = True, False
		assert st.csr(d, code, g, c)[1][0] == 0


def test_malformed_csr_is_flagged_and_the_process_survives(golden, qc, torch):
	"""The malformed matrices of tests/test_gpu_lcpm_sparse.py::test_sparse_errors_from_the_device_flags, through qc_reads and subset."""
	import scipy.sparse
	from normalisr_amd.lcpm import DeviceCSR
	g = golden('G20_qc')
	x, params = g['b_reads'], tuple(float(v) for v in g['b_params'])
	good = dev_csr(torch, scipy.sparse.csr_matrix(x))
	want = qc.qc_reads(good, *params)

	def variant(indptr=None, indices=None):
		t = [good.indptr.clone(), good.indices.clone(), good.data.clone()]
		for i, f in enumerate((indptr, indices)):
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
		with pytest.raises(ValueError, match='Malformed'):
			qc.qc_reads(d, *params)
		with pytest.raises(ValueError, match='Malformed'):
			qc.subset(d, genes=want[0], cells=want[1])
	# and the device is as it was: the well-formed matrix still gives the same answer
	again = qc.qc_reads(good, *params)
	assert np.array_equal(again[0], g['b_genes']) and np.array_equal(again[1], g['b_cells'])


# ---- the decision kernel ----------------------------------------------------------------------------------------------------------------------------------------------

def test_decide_kernel_against_numpy(torch, eng):
	from normalisr_amd import _lib
	rng = np.random.default_rng(11)
	rows, n = 301, 1030
	x = rng.poisson(np.exp(rng.normal(-1.5, 1.4, rows))[:, None] * np.exp(rng.normal(0, 0.9, n))[None, :])
	g0, c0 = rng.random(rows) < 0.8, rng.random(n) < 0.8
	st = qc_numpy.stats(x, g0, c0)
	d_st = [up(torch, v) for v in st]
	cases = [(0, 0, 0, 0, 0, 0), (30, 0, 0, 0, 0, 0), (0, 25, 0, 0, 0, 0), (0, 0, 60, 0, 0, 0), (0, 0, 0, 40, 0, 0), (0, 0, 0, 0, 12, 0), (0, 0, 0, 0, 0, 35),
			 (30, 25, 60, 40, 12, 35), (10**12, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 10**12), (10**12, 10**12, 10**12, 10**12, 10**12, 10**12)]
	for thr in cases:
		g, c = up(torch, g0.astype(np.uint8)), up(torch, c0.astype(np.uint8))
		out = torch.full((2, ), -1, dtype=torch.int64, device='cuda')
		h = np.array(thr, dtype=np.int64)
		_lib.check(eng.lib.nrm_qc_decide(*[v.data_ptr() for v in d_st], rows, n, h.ctypes.data, g.data_ptr(), c.data_ptr(), out.data_ptr(), eng._stream()))
		wg, wc = qc_numpy.decide(st, thr, g0, c0)
		assert np.array_equal(g.cpu().numpy().astype(bool), wg) and np.array_equal(c.cpu().numpy().astype(bool), wc), thr
		assert out.cpu().numpy().tolist() == [int(wg.sum()), int(wc.sum())], thr
	assert not wg.any() and not wc.any()  # the last case removes everything
	thr = (30, 25, 60, 40, 12, 35)
	wg, wc = qc_numpy.decide(st, thr, g0, c0)
	assert 0 < wg.sum() < g0.sum() and 0 < wc.sum() < c0.sum()  # (the combined case decides something on both axes)
	for i in range(6):  # every criterion alone removes something, and not everything
		one = tuple(v if j == i else 0 for j, v in enumerate(thr))
		wg, wc = qc_numpy.decide(st, one, g0, c0)
		left, all_ = (wg.sum(), g0.sum()) if i < 3 else (wc.sum(), c0.sum())
		assert 0 < left < all_, i


# ---- subset ---------------------------------------------------------------------------------------------------------------------------------------------------------

def bits(a):
	a = np.ascontiguousarray(a)
	return a.view('u{}'.format(a.dtype.itemsize))


@pytest.mark.parametrize('dtype', [np.int64, np.int32, np.int16, np.uint8, np.float32, np.float64])
def test_subset_dense_against_numpy_indexing(qc, torch, dtype):
	rng = np.random.default_rng(np.dtype(dtype).itemsize)
	for rows, n in ((1, 1), (37, 301), (70, 1027)):
		if np.dtype(dtype).kind == 'f':
			x = rng.normal(size=(rows, n)).astype(dtype)
			x.flat[::7] = np.nan
			x.flat[1::11] = -0.0
		else:
			x = rng.integers(0, np.iinfo(dtype).max, (rows, n), dtype=dtype)
		r = rng.integers(0, rows, 2 * rows + 3)  # any order, with repeats
		c = rng.integers(0, n, n + 5)
		gm, cm = rng.random(rows) < 0.6, rng.random(n) < 0.6
		gm[0] = cm[0] = True
		for gsel, csel, want in ((r, c, x[np.ix_(r, c)]), (r, None, x[r]), (None, c, x[:, c]), (None, None, x), (gm, cm, x[gm][:, cm]), (r - rows, c - n, x[np.ix_(r, c)]),
								 (list(range(rows - 1, -1, -1)), None, x[::-1])):
			got = qc.subset(x, gsel, csel)
			assert isinstance(got, np.ndarray) and got.dtype == x.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want)), (rows, n)
		xt = up(torch, x)
		got = qc.subset(xt, up(torch, r), up(torch, c))
		assert got.is_cuda and np.array_equal(bits(got.cpu().numpy()), bits(x[np.ix_(r, c)]))
		got = qc.subset(x, r, c, device_out=True)
		assert got.is_cuda and got.dtype == xt.dtype and np.array_equal(bits(got.cpu().numpy()), bits(x[np.ix_(r, c)]))
		base = torch.zeros((rows, n + 3), dtype=xt.dtype, device='cuda')  # pitched input, rows off the element grid of wider loads
		base[:, 1:n + 1] = xt
		got = qc.subset(base[:, 1:n + 1], r, up(torch, cm))
		assert np.array_equal(bits(got.cpu().numpy()), bits(x[r][:, cm]))
		got = qc.subset(xt.t().contiguous().t(), r, c)  # (a column-major view is made row-major first)
		assert np.array_equal(bits(got.cpu().numpy()), bits(x[np.ix_(r, c)]))
		assert qc.subset(x, np.zeros(0, dtype=np.int64), None).shape == (0, n)


def test_subset_csr_on_the_golden_matrices(golden, qc, torch):
	import scipy.sparse
	from normalisr_amd.lcpm import DeviceCSR
	g = golden('G20_qc')
	rng = np.random.default_rng(3)
	for name in CASES:
		x = g[name + '_reads']
		m = scipy.sparse.csr_matrix(x)
		m.data[::3] = 0  # stored zeros stay stored
		ones = scipy.sparse.csr_matrix((np.ones_like(m.data), m.indices, m.indptr), shape=m.shape)
		d = dev_csr(torch, m)
		nt, ns = x.shape
		sels = [(rng.random(nt) < 0.6, rng.random(ns) < 0.6), (g[name + '_genes'], g[name + '_cells']), (None, rng.random(ns) < 0.3), (np.arange(nt) % 7 == 0, None),
				(np.array([nt - 1]), np.array([0, ns - 1])), (None, None)]
		for gsel, csel in sels:
			out = qc.subset(d, gsel, csel)
			assert isinstance(out, DeviceCSR) and out.indptr.dtype == torch.int64 and out.indices.dtype == torch.int32 and out.data.dtype == d.data.dtype
			gi = np.arange(nt) if gsel is None else np.flatnonzero(gsel) if gsel.dtype == bool else gsel
			ci = np.arange(ns) if csel is None else np.flatnonzero(csel) if csel.dtype == bool else csel
			want = m.toarray()[np.ix_(gi, ci)]
			h = host_csr(out)
			p, idx = h.indptr, h.indices
			assert out.shape == want.shape and p[0] == 0 and p[-1] == idx.size == h.data.size and (np.diff(p) >= 0).all()
			for r in range(len(p) - 1):  # canonical: the columns of every row inside the matrix and strictly increasing
				cols = idx[p[r]:p[r + 1]]
				assert cols.size == 0 or (cols[0] >= 0 and cols[-1] < want.shape[1] and (np.diff(cols) > 0).all())
			assert np.array_equal(h.toarray(), want)
			assert idx.size == int(ones[gi][:, ci].sum())  # every stored entry of the selection, zeros included
			if gsel is not None and csel is not None:  # device selections: the index tensors qc_reads returns with device_out=True
				again = qc.subset(d, up(torch, gi), up(torch, ci))
				assert all(torch.equal(u, v) for u, v in ((again.indptr, out.indptr), (again.indices, out.indices), (again.data, out.data)))
		# the other sparse forms come back as their own kind
		gsel, csel = sels[0]
		want = x[gsel][:, csel]
		s = qc.subset(scipy.sparse.coo_matrix(x), gsel, csel)
		assert scipy.sparse.issparse(s) and s.format == 'csr' and s.dtype == x.dtype and np.array_equal(s.toarray(), want)
		assert isinstance(qc.subset(scipy.sparse.csr_matrix(x), gsel, csel, device_out=True), DeviceCSR)
		mm = scipy.sparse.csr_matrix(x)
		t = torch.sparse_csr_tensor(up(torch, mm.indptr.astype(np.int64)), up(torch, mm.indices.astype(np.int64)), up(torch, mm.data.astype(np.int64)), size=mm.shape)
		s = qc.subset(t, gsel, csel)
		assert str(s.layout) == 'torch.sparse_csr' and s.is_cuda and s.values().dtype == torch.int64 and tuple(s.shape) == want.shape
		back = scipy.sparse.csr_matrix((s.values().cpu().numpy(), s.col_indices().cpu().numpy(), s.crow_indices().cpu().numpy()), shape=want.shape)
		assert np.array_equal(back.toarray(), want)
		for bad in (dict(genes=np.array([3, 2])), dict(cells=np.array([0, 5, 5])), dict(genes=up(torch, np.array([1, 0]))), dict(cells=up(torch, np.array([4, 4])))):
			with pytest.raises(ValueError, match='increase strictly'):
				qc.subset(d, **bad)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_resident_chain_reads_qc_subset_lcpm(golden, qc, torch):
	"""DeviceCSR reads -> qc_reads -> subset -> lcpm against lcpm of the CSR built from the numpy-subset matrix: the CSR passes are order-independent (integer
	sums, fixed-order folds), so the bar is equality of bits.  The dense counts never exist: qc_reads and subset together stay below the bytes of the dense
	int32 matrix -- statistics, masks, slabs of one word per row tile and cell, and a result no larger than the input's stored entries."""
	import scipy.sparse
	from normalisr_amd.lcpm import DeviceCSR, lcpm
	g = golden('G20_qc')
	x, params = g['a_reads'], tuple(float(v) for v in g['a_params'])
	d = dev_csr(torch, scipy.sparse.csr_matrix(x))
	qc.qc_reads(d, *params)  # (the engine and the library's pools exist before the measurement)
	torch.cuda.synchronize()
	torch.cuda.reset_peak_memory_stats()
	before = torch.cuda.memory_allocated()
	genes, cells = qc.qc_reads(d, *params, device_out=True)
	sub = qc.subset(d, genes, cells)
	torch.cuda.synchronize()
	peak = torch.cuda.max_memory_allocated() - before
	print('peak above the start: %d bytes; the dense int32 counts: %d bytes' % (peak, x.size * 4))
	assert peak < x.size * 4
	assert isinstance(sub, DeviceCSR) and sub.shape == (len(g['a_genes']), len(g['a_cells']))
	want = x[g['a_genes']][:, g['a_cells']]
	assert np.array_equal(host_csr(sub).toarray(), want)
	ref = dev_csr(torch, scipy.sparse.csr_matrix(want))
	a, b = lcpm(sub, device_out=True), lcpm(ref, device_out=True)
	assert a[0].is_cuda and torch.equal(a[0], b[0]) and np.array_equal(a[3], b[3])
	# the dense route of the same chain: the gather, then lcpm of the dense counts
	xt = up(torch, x)
	dg, dc = qc.qc_reads(xt, *params, device_out=True)
	dsub = qc.subset(xt, dg, dc)
	assert dsub.is_cuda and np.array_equal(dsub.cpu().numpy(), want)
	assert torch.equal(lcpm(dsub, device_out=True)[0], lcpm(up(torch, want), device_out=True)[0])


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_qc_reads_subset_qc_outlier(golden, tmp_path):
	"""`normalisr qc_reads`, `subset` and `qc_outlier` as child processes on files written from case b, against the files the reference's command line wrote; once
	more with -s from a Matrix Market file, names in their order (the CSR subset) and reversed (indexed on the host)."""
	g = golden('G20_qc')
	f = lambda name: str(tmp_path / name)
	x, p = g['b_reads'], g['b_params']
	np.savetxt(f('reads.tsv'), x, delimiter='\t', fmt='%i')
	np.savetxt(f('w.tsv'), g['w'], delimiter='\t', fmt='%.8G')
	for name, key in (('genes.txt', 'cli_genes_in'), ('cells.txt', 'cli_cells_in'), ('wcells.txt', 'cli_wcells_in')):
		with open(f(name), 'w') as fh:
			fh.write('\n'.join(g[key]))
	env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))

	def run(*args):
		r = subprocess.run([sys.executable, '-m', 'normalisr_amd'] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
		assert r.returncode == 0, r.stderr[-3000:]

	names = lambda name: [v.strip() for v in open(f(name)) if v.strip()]
	flags = ['--gene_read_count', str(int(p[0])), '--gene_cell_count', str(int(p[1])), '--gene_cell_prop', repr(float(p[2])), '--cell_read_count', str(int(p[3])),
			 '--cell_gene_count', str(int(p[4])), '--cell_gene_prop', repr(float(p[5]))]
	run('qc_reads', f('reads.tsv'), f('genes.txt'), f('cells.txt'), f('genes_out.txt'), f('cells_out.txt'), *flags)
	assert names('genes_out.txt') == list(g['cli_genes_out']) and names('cells_out.txt') == list(g['cli_cells_out'])
	run('subset', f('reads.tsv'), f('sub.tsv'), '-r', f('genes.txt'), f('genes_out.txt'), '-c', f('cells.txt'), f('cells_out.txt'))
	assert np.array_equal(np.loadtxt(f('sub.tsv'), delimiter='\t', ndmin=2), g['cli_subset'])
	run('qc_outlier', f('w.tsv'), f('wcells.txt'), f('wcells_out.txt'))
	assert names('wcells_out.txt') == list(g['cli_wcells_out'])
	try:
		import scipy.io
		import scipy.sparse
	except ImportError:
		return
	scipy.io.mmwrite(f('reads.mtx'), scipy.sparse.coo_matrix(x))
	run('qc_reads', '-s', f('reads.mtx'), f('genes.txt'), f('cells.txt'), f('genes_s.txt'), f('cells_s.txt'), *flags)
	assert names('genes_s.txt') == list(g['cli_genes_out']) and names('cells_s.txt') == list(g['cli_cells_out'])
	run('subset', '-s', f('reads.mtx'), f('sub_s.tsv'), '-r', f('genes.txt'), f('genes_out.txt'), '-c', f('cells.txt'), f('cells_out.txt'))
	text = open(f('sub_s.tsv')).read()
	assert '.' not in text and 'E' not in text  # (integer data is written with '%i')
	assert np.array_equal(np.loadtxt(f('sub_s.tsv'), delimiter='\t', ndmin=2), g['cli_subset'])
	with open(f('genes_rev.txt'), 'w') as fh:
		fh.write('\n'.join(g['cli_genes_out'][::-1]))
	run('subset', '-s', f('reads.mtx'), f('sub_r.tsv'), '-r', f('genes.txt'), f('genes_rev.txt'), '--nodummy')
	want = x[g['b_genes'][::-1]]
	want = want[:, [len(np.unique(v)) > 1 for v in want.T]]
	assert np.array_equal(np.loadtxt(f('sub_r.tsv'), delimiter='\t', ndmin=2), want)
