"""GPU: every C entry of the front half on its own, against the extended-precision reference of ITS stage (tests/front_longdouble.py).

The inputs of a stage are the reference's outputs of the stage before it, rounded to fp64 -- never the device's --, so a wrong number names its kernel.
Parametrised over the layout matrix (count dtype x storage x output dtype x table length; logCPM dtype x storage), not only over shapes.  Storage:
contiguous | a pointer one element past an aligned base (rows on no 16-byte boundary) | a padded row stride on an aligned base with a RAGGED last group of
four cells (the 16-byte paths of lc_ld4 / fv_ld4 / k_lc_write together with their scalar tail).  The padding holds a sentinel: a read past the row's end
changes the result, a write past it is seen.

Bounds.  u = 2^-53.  Integer outputs are exact.  fp32 stores and single IEEE operations (T[x] - t1, 1 / s, (1 / best) / min) are bit-equal to numpy's.  A sum
of m terms is held to m u sum|terms| with sum|terms| from the reference, plus the first-order propagation of the same bounds through what feeds it:
  lcpm colsum  partial[tile][k]: rows(tile) u sum E              t1: rows u + u |t1| + 16 u (the constant ln 1e6) + LOG ulp(t1)
  csr colsum   t1: entries_k 2^-62 (the fixed-point claim) + 3 u (rows E[0], the conversion, the addition) + u |t1| + 16 u + LOG ulp(t1)
  moments      a: n u sum_k |y| |cw|
  genes        b: nc u sum |mi| |a| =: Db
               r = u_k (y - b C): Dr = |u_k| (nc u |b||C| + Db |C|) + 2 u |r|
               m: (sum_k Dr + n u sum_k |r|) / n + u |m| =: Dm
               sc: d = r - m, Dd = Dr + Dm + u |d|, S = sum d^2, DS = 2 sum |d| Dd + (n + 1) u S; sc (DS / 2S + u) + SQRT ulp(sc)
  cells        (b, m, sc given) Dr = |u_k| nc u |b||C| + 2 u |r|; d = (r - m) / sc, Dd = Dr / sc + 2 u |d|; v: (2 sum_g |d| Dd + (G + 1) u sum d^2) / G + u v
  design       u: bit-equal to 1 / s; cw: 4 u |cw| (1 / s counts twice); Gram (the chunks added here in longdouble): (256 + 4) u sum_k |u C_i| |u C_j|
  update       l = ln sqrt v: Dl = u (the square root's rounding through the log) + L ulp(l)
               g = [C;1] l: n u sum |C| |l| + |C| Dl =: Dg;  coef: (nc + 1) u |m2i| |g| + |m2i| Dg =: Dc;  f: (nc + 1) u |coef| |[C;1]| + Dc |[C;1]| =: Df
               new = exp(f) s / min: relative Df_k + max Df over the cells at the minimum + 4 u + 2 EXP ulp
               t1 = max |(new - s) / s|: max_k (Dnew_k / s_k + 2 u t_k)
  weights      bit-equal to numpy's (1 / best) / min.
LOG, L, EXP, SQRT are the device library's errors in ulps of the output; they are not derivable here, so each test PRINTS the worst excess over the propagated
part in ulps and the allowance below is four times the largest value measured on an MI355X (DESIGN.md section 6f has the table, the date and the commit).
Measured: t1 0, sc 0, new 0 (the propagated parts alone cover the library functions there: the allowance is none) and l 0.38 ulp over 756 values."""
import functools

import numpy as np
import pytest

import front_longdouble as fl
from test_gpu_parity import close
from test_compute_var_plan_cpu import _covariates, _pinv_host, TOL, CELLS

pytestmark = pytest.mark.gpu

U = fl.U
# ulps allowed to the device's log, exp and sqrt on top of the propagated bounds: 4 x the worst measured (see the docstring); more than 8 measured is a finding
LOG_ULP = 0.0  # t1 = ln(sum) - ln 1e6: measured excess 0 over 36 cases, dense and CSR
L_ULP = 4 * 0.38  # l = ln sqrt v
EXP_ULP = 0.0  # new = exp(f) s / min: measured excess 0
SQRT_ULP = 0.0  # sc: measured excess 0

GENES = [1, 3, 4, 5, 31, 32, 33, 64, 129]
CELLS_ALL = [1, 3, 63, 65, 255, 257, 1023, 1025, 4097, 8193, 64, 256, 1024, 4096]  # the first ten leave a ragged group of four
COVS = [1, 7, 8, 9, 16, 17, 62, 63]
STORAGES = ['contiguous', 'offset', 'padded']
COUNT_DTYPES = ['int64', 'int32', 'int16', 'uint8']
SENTINEL = 7


@functools.lru_cache(maxsize=None)
def _env():
	import torch
	from normalisr_amd import _lib
	from normalisr_amd import engine
	eng = engine.get_engine()
	return torch, _lib, eng


def _place(h, storage, fill=SENTINEL):
	"""The host matrix h (rows, n) in HBM in one of the three storages: (the (rows, n) view, the whole allocation)."""
	torch, _, _ = _env()
	h = np.ascontiguousarray(h)
	rows, n = h.shape
	t = torch.as_tensor(h).cuda()
	if storage == 'contiguous':
		return t, t
	if storage == 'offset':
		whole = torch.full((rows, n + 3), fill, dtype=t.dtype, device='cuda')
		view = whole[:, 1:n + 1]
	else:
		pad = 4 - n % 4  # 1 .. 4: the stride is a multiple of four elements, the base is the allocation's
		whole = torch.full((rows, n + pad), fill, dtype=t.dtype, device='cuda')
		view = whole[:, :n]
	view.copy_(t)
	return view, whole


def _padding_untouched(view, whole, storage, fill=SENTINEL):
	if storage == 'contiguous':
		return True
	n = view.shape[1]
	w = whole.cpu().numpy()
	rest = np.concatenate([w[:, :1], w[:, n + 1:]], axis=1) if storage == 'offset' else w[:, n:]
	return bool((rest == fill).all())


def _ratio(got, ref, bound):
	"""max |got - ref| / bound, with 0 / 0 = 0."""
	e = np.abs(fl.ld(got) - ref)
	b = fl.ld(bound)
	with np.errstate(invalid='ignore', divide='ignore'):
		r = np.where(e == 0, 0, e / b)
	return float(np.max(r))


def _excess_ulps(got, ref, propagated):
	"""The worst excess of |got - ref| over the propagated bound, in ulps of the output."""
	e = np.abs(fl.ld(got) - ref) - fl.ld(propagated)
	return float(np.max(np.maximum(e, 0) / fl.ulp(ref)))


# ---- lcpm ---------------------------------------------------------------------------------------------------------------------------------------------------
def _count_matrix(ng, n, top, seed):
	"""Poisson counts near 0.45 per entry, then: in several cells EVERY gene of a 32-gene tile is non-zero (the top value of the packed word's count field)
	with counts at and just below top; a cell whose only read sits in the last gene; the largest count in the middle."""
	rng = np.random.default_rng(seed)
	x = rng.poisson(0.45, (ng, n)).astype(np.int64)
	for k in sorted({0, n // 2, n - 1, min(n - 1, 1023), min(n - 1, 4096)}):
		for g0 in {0, 32 * ((ng - 1) // 32)}:  # the first tile and the last (ragged) one
			x[g0:g0 + 32, k] = top - rng.integers(0, 3, x[g0:g0 + 32, k].shape)
	if n > 2:
		x[:, 1] = 0
		x[ng - 1, 1] = 1
	x[ng // 2, n // 3 if n >= 6 else 0] = top
	return x


def _lcpm_cases():
	tops = {'uint8': [255], 'int16': [32767, 4095], 'int32': [4096, 10**6, 4095], 'int64': [10**6, 4096, 4095]}  # table lengths 256 | 32768, 4096 | 4097, 10^6 + 1, 4096
	out, i = [], 0
	for si, storage in enumerate(STORAGES):
		for di, dtype in enumerate(COUNT_DTYPES):
			out.append((GENES[i % len(GENES)], CELLS_ALL[i % 10], dtype, storage, tops[dtype][si % len(tops[dtype])]))
			i += 1
	for j, n in enumerate(CELLS_ALL[10:] + [4097, 8193]):  # the four cell counts without a ragged tail, and the two largest once more on other dtypes
		dtype = COUNT_DTYPES[j % 4]
		out.append((GENES[i % len(GENES)], n, dtype, STORAGES[(j + 2) % 3], tops[dtype][j % len(tops[dtype])]))
		i += 1
	assert {c[0] for c in out} == set(GENES) and {c[1] for c in out} == set(CELLS_ALL)
	assert {(c[2], c[3]) for c in out if c[1] % 4} == {(d, s) for d in COUNT_DTYPES for s in STORAGES}
	return out


LCPM_CASES = _lcpm_cases()


@functools.lru_cache(maxsize=4)
def _lcpm_problem(ng, n, top):
	"""The counts, the exact integers, the library's fp64 tables T and E = exp(T), the reference per-cell sums and t1."""
	from normalisr_amd.lcpm import digamma_table
	x = _count_matrix(ng, n, top, 7 * ng + n)
	c = fl.counts(x)
	psi, psi_t0 = digamma_table(c['max'], c['total'] + 2)
	tab = psi - psi_t0
	etab = np.exp(tab)
	s, t1 = fl.colsum(x, etab)
	for a in (x, tab, etab):
		a.setflags(write=False)
	return x, c, tab, etab, s, t1


def _t1_bounds(t1, terms_rel):
	"""(propagated bound, the same plus the log's allowance) of t1 = ln(sum) - ln 1e6 for a sum with relative error terms_rel."""
	prop = fl.ld(terms_rel) + U * np.abs(t1) + 16 * U
	return prop, prop + LOG_ULP * fl.ulp(t1)


def _write_checks(name, lib_call, view_shape, storage, x, tab, t1_64):
	"""nrm_lcpm_write / nrm_lcpm_csr_write into fp64 and fp32 outputs of the storage given, with and without t1: bit equality with numpy's one subtraction (and
	one rounding to fp32), the padding of the output untouched."""
	torch, _lib, eng = _env()
	ng, n = view_shape
	d_t1 = torch.as_tensor(t1_64).cuda()
	want = tab[x] - t1_64[None, :]
	assert np.abs(fl.ld(want) - fl.write(x, tab, t1_64)).max() <= U * np.abs(want).max()  # (numpy's subtraction against longdouble: half an ulp)
	for odt, code in ((np.float64, _lib.NRM_F64), (np.float32, _lib.NRM_F32)):
		for sub in (d_t1, None):
			out, whole = _place(np.full((ng, n), -1.0, dtype=odt), storage, fill=float(SENTINEL))
			lib_call(0 if sub is None else sub.data_ptr(), out.data_ptr(), code, out.stride(0))
			torch.cuda.synchronize()
			ref = (want if sub is not None else tab[x]).astype(odt)
			got = out.cpu().numpy()
			assert got.dtype == odt and np.array_equal(got, ref), (name, odt, sub is None, np.argwhere(got != ref)[:5])
			assert _padding_untouched(out, whole, storage, float(SENTINEL)), (name, odt)


@pytest.mark.parametrize('ng,n,dtype,storage,top', LCPM_CASES)
def test_lcpm_dense_stages(ng, n, dtype, storage, top):
	torch, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	x, c, tab, etab, s_ref, t1_ref = _lcpm_problem(ng, n, top)
	code = {'int64': _lib.NRM_I64, 'int32': _lib.NRM_I32, 'int16': _lib.NRM_I16, 'uint8': _lib.NRM_U8}[dtype]
	d, whole = _place(x.astype(dtype), storage)
	assert d.stride(1) == 1 and (storage != 'padded' or (d.stride(0) % 4 == 0 and d.data_ptr() % 32 == 0))
	# count
	buf = eng.zeros((2 * n + ng + 4, ), torch.int64)
	part = torch.empty((int(lib.nrm_lcpm_count_workspace(ng, n)), ), dtype=torch.int64, device='cuda')
	_lib.check(lib.nrm_lcpm_count(d.data_ptr(), code, ng, n, d.stride(0), buf[:n].data_ptr(), buf[n:2 * n].data_ptr(), buf[2 * n:2 * n + ng].data_ptr(),
								  buf[2 * n + ng:].data_ptr(), part.data_ptr(), st))
	h = buf.cpu().numpy()
	assert np.array_equal(h[:n], c['cell_total']), np.argwhere(h[:n] != c['cell_total'])[:5]
	assert np.array_equal(h[n:2 * n], c['cell_nnz']), np.argwhere(h[n:2 * n] != c['cell_nnz'])[:5]
	assert np.array_equal(h[2 * n:2 * n + ng], c['gene_zero'])
	assert (int(h[-4]), int(h[-3]), int(h[-2])) == (c['total'], c['max'], 0)
	assert (x[:32, 0] != 0).all() and (x[:32, 0] >= top - 2).all() and (n <= 2 or (c['cell_total'][1] == 1 and x[ng - 1, 1] == 1))  # the content this case is about
	# colsum
	tiles = -(-ng // int(lib.nrm_lcpm_row_tile()))
	d_exp, d_t1 = torch.tensor(etab).cuda(), torch.empty((n, ), dtype=torch.float64, device='cuda')
	fpart = torch.empty((tiles, n), dtype=torch.float64, device='cuda')
	_lib.check(lib.nrm_lcpm_colsum(d.data_ptr(), code, ng, n, d.stride(0), d_exp.data_ptr(), etab.size, fpart.data_ptr(), d_t1.data_ptr(), st))
	tr = int(lib.nrm_lcpm_row_tile())
	pref = np.array([fl.ld(etab)[x[t * tr:(t + 1) * tr]].sum(axis=0) for t in range(tiles)])
	rp = _ratio(fpart.cpu().numpy(), pref, min(ng, tr) * U * pref)
	t1 = d_t1.cpu().numpy()
	prop, bound = _t1_bounds(t1_ref, ng * U)
	print('dense %s %s (%d, %d) table %d: partial sums error/bound %.3g, t1 error/bound %.3g, log excess %.3g ulp' % (
		dtype, storage, ng, n, etab.size, rp, _ratio(t1, t1_ref, bound), _excess_ulps(t1, t1_ref, prop)))
	assert rp <= 1 and _ratio(t1, t1_ref, bound) <= 1
	# write
	d_tab = torch.tensor(tab).cuda()
	t1_64 = t1_ref.astype(np.float64)
	_write_checks('dense', lambda p_t1, p_out, ocode, ldo: _lib.check(lib.nrm_lcpm_write(d.data_ptr(), code, ng, n, d.stride(0), d_tab.data_ptr(), tab.size, p_t1,
																							 p_out, ocode, ldo, st)), (ng, n), storage, x, tab, t1_64)
	assert _padding_untouched(d, whole, storage)


@pytest.mark.parametrize('ng,n,dtype,storage,top', LCPM_CASES)
def test_lcpm_csr_stages(ng, n, dtype, storage, top):
	"""The CSR entries on the same matrices (the storage is the OUTPUT's: the stored entries have one layout)."""
	import scipy.sparse
	torch, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	x, c, tab, etab, s_ref, t1_ref = _lcpm_problem(ng, n, top)
	code = {'int64': _lib.NRM_I64, 'int32': _lib.NRM_I32, 'int16': _lib.NRM_I16, 'uint8': _lib.NRM_U8}[dtype]
	m = scipy.sparse.csr_matrix(x)
	m.sort_indices()
	indptr, indices, data = torch.as_tensor(m.indptr.astype(np.int64)).cuda(), torch.as_tensor(m.indices.astype(np.int32)).cuda(), torch.as_tensor(m.data.astype(dtype)).cuda()
	nnz = int(m.nnz)
	head = (indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), code, ng, n, nnz)
	buf = eng.zeros((2 * n + ng + 4, ), torch.int64)
	part = torch.empty((int(lib.nrm_lcpm_csr_workspace(ng, n)), ), dtype=torch.int64, device='cuda')
	_lib.check(lib.nrm_lcpm_csr_count(*head, buf[:n].data_ptr(), buf[n:2 * n].data_ptr(), buf[2 * n:2 * n + ng].data_ptr(), buf[2 * n + ng:].data_ptr(), part.data_ptr(), st))
	h = buf.cpu().numpy()
	assert np.array_equal(h[:n], c['cell_total']) and np.array_equal(h[n:2 * n], c['cell_nnz']) and np.array_equal(h[2 * n:2 * n + ng], c['gene_zero'])
	assert (int(h[-4]), int(h[-3]), int(h[-2]), int(h[-1])) == (c['total'], c['max'], 0, 0)
	# colsum: the fixed-point claim
	unit = float(((etab[1:] - etab[0]) / np.arange(1, etab.size)).max())
	d_exp, d_t1 = torch.tensor(etab).cuda(), torch.empty((n, ), dtype=torch.float64, device='cuda')
	_lib.check(lib.nrm_lcpm_csr_colsum(*head, d_exp.data_ptr(), etab.size, unit, buf[:n].data_ptr(), part.data_ptr(), d_t1.data_ptr(), st))
	t1 = d_t1.cpu().numpy()
	prop, bound = _t1_bounds(t1_ref, c['cell_nnz'] * 2.0**-62 + 3 * U)
	print('csr %s out %s (%d, %d) table %d: t1 error/bound %.3g, log excess %.3g ulp' % (dtype, storage, ng, n, etab.size, _ratio(t1, t1_ref, bound),
																					  _excess_ulps(t1, t1_ref, prop)))
	assert _ratio(t1, t1_ref, bound) <= 1
	d_tab = torch.tensor(tab).cuda()
	_write_checks('csr', lambda p_t1, p_out, ocode, ldo: _lib.check(lib.nrm_lcpm_csr_write(*head, d_tab.data_ptr(), tab.size, p_t1, p_out, ocode, ldo, st)), (ng, n), storage, x,
				  tab, t1_ref.astype(np.float64))


# ---- the three streaming passes of compute_var ---------------------------------------------------------------------------------------------------------------------
def _fitvar_cases():
	out = []
	for i, n in enumerate(CELLS_ALL):
		out.append((GENES[(2 * i + 1) % len(GENES)], n, COVS[i % len(COVS)], ['float64', 'float32'][i % 2], STORAGES[(i // 2) % 3]))
	out += [(300, 4099, 63, 'float32', 'padded'), (33, 130, 4, 'float64', 'contiguous'), (4, 1025, 9, 'float32', 'contiguous'), (31, 65, 8, 'float64', 'offset')]
	assert {c[0] for c in out} >= set(GENES) and {c[1] for c in out} >= set(CELLS_ALL) and {c[2] for c in out} >= set(COVS)
	assert {(c[3], c[4]) for c in out if c[1] % 4} == {(d, s) for d in ('float64', 'float32') for s in STORAGES}
	return out


FITVAR_CASES = _fitvar_cases()


@functools.lru_cache(maxsize=2)
def _fitvar_problem(ng, n, nc, dtype):
	"""logCPM-like rows (offsets 0 .. 14, scales exp(N(0, 1))), covariates WITHOUT an intercept (so the residual's mean is not zero), cell scales s over two
	decades, and every stage's reference from the stage before it rounded to fp64."""
	from normalisr_amd.association import inv_rank
	rng = np.random.default_rng(31 * ng + 7 * n + nc)
	ncu = min(nc, max(n - 1, 1))  # (more covariates than cells: the surplus rows repeat, the pseudo-inverse takes them)
	c = rng.normal(size=(nc, n))
	c[ncu:] = c[np.arange(nc - ncu) % ncu]
	c[0] += 3.0
	s = 10.0**rng.uniform(-1, 1, n)
	y = (rng.uniform(0, 14, ng)[:, None] + np.exp(rng.normal(size=ng))[:, None] * rng.normal(size=(ng, n)) * s).astype(dtype)
	u, cw, m, _ = fl.design(c, s)
	u64, cw64 = u.astype(np.float64), cw.astype(np.float64)
	mi = np.ascontiguousarray(inv_rank(m.astype(np.float64))[0])
	a, a_abs = fl.moments(y, cw64)
	a64 = a.astype(np.float64)
	b, b_abs = fl.coef(a64, mi)
	r, r_abs = fl.resid(y, u64, c, b)  # (k_fv_genes computes b itself and keeps it in fp64 registers: the reference's b is compared with it, not fed to it)
	mean, sc = fl.gene_stats(r)
	b64, mean64, sc64 = b.astype(np.float64), mean.astype(np.float64), sc.astype(np.float64)
	r2, r2_abs = fl.resid(y, u64, c, b64)
	with np.errstate(invalid='ignore', divide='ignore'):
		v = fl.cell_var(r2, mean64, sc64)  # (one cell: the residual is its own mean, the spread zero)
	return dict(y=y, c=c, s=s, u=u64, cw=cw64, mi=mi, a=a, a_abs=a_abs, a64=a64, b=b, b_abs=b_abs, r=r, mean=mean, sc=sc, b64=b64, mean64=mean64, sc64=sc64, r2=r2, v=v)


@pytest.mark.parametrize('ng,n,nc,dtype,storage', FITVAR_CASES)
def test_fitvar_stages(ng, n, nc, dtype, storage):
	torch, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	p = _fitvar_problem(ng, n, nc, dtype)
	y, whole = _place(p['y'], storage, fill=1e3)
	ycode = _lib.NRM_F64 if dtype == 'float64' else _lib.NRM_F32
	# the covariates take the storage of the matrix, so that a padded stride leaves the 16-byte path its ragged tail whatever n is
	c, _ = _place(p['c'], storage if storage == 'padded' else 'contiguous', fill=1e3)
	cw, _ = _place(p['cw'], storage if storage == 'padded' else 'contiguous', fill=1e3)
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
	u, mi = up(p['u']), up(p['mi'])
	f64 = dict(dtype=torch.float64, device='cuda')
	absc, absb = np.abs(fl.ld(p['c'])), np.abs(p['b'])
	# moments
	d_a = torch.full((ng, nc), np.nan, **f64)
	_lib.check(lib.nrm_fitvar_moments(y.data_ptr(), ycode, ng, n, y.stride(0), cw.data_ptr(), nc, cw.stride(0), d_a.data_ptr(), st))
	ra = _ratio(d_a.cpu().numpy(), p['a'], n * U * p['a_abs'])
	# genes
	d_a64 = up(p['a64'])
	d_b, d_mean, d_sc = torch.full((ng, nc), np.nan, **f64), torch.full((ng, ), np.nan, **f64), torch.full((ng, ), np.nan, **f64)
	flags = eng.zeros((4, ), torch.int32)
	_lib.check(lib.nrm_fitvar_genes(y.data_ptr(), ycode, ng, n, y.stride(0), u.data_ptr(), c.data_ptr(), nc, c.stride(0), d_a64.data_ptr(), mi.data_ptr(), d_b.data_ptr(),
									d_mean.data_ptr(), d_sc.data_ptr(), flags.data_ptr(), st))
	db = nc * U * p['b_abs']
	r, mean, sc = p['r'], p['mean'], p['sc']
	absu = np.abs(fl.ld(p['u']))[None, :]
	dr = absu * (nc * U * (absb @ absc) + db @ absc) + 2 * U * np.abs(r)
	dm = (dr.sum(axis=1) + n * U * np.abs(r).sum(axis=1)) / n + U * np.abs(mean)
	d = r - mean[:, None]
	dd = dr + dm[:, None] + U * np.abs(d)
	ss = (d**2).sum(axis=1)
	ds = 2 * (np.abs(d) * dd).sum(axis=1) + (n + 1) * U * ss
	with np.errstate(invalid='ignore', divide='ignore'):
		sc_prop = sc * (ds / (2 * ss) + U)
	rb, rm = _ratio(d_b.cpu().numpy(), p['b'], db), _ratio(d_mean.cpu().numpy(), mean, dm)
	with np.errstate(invalid='ignore', divide='ignore'):
		rs = _ratio(d_sc.cpu().numpy(), sc, sc_prop + SQRT_ULP * fl.ulp(sc))
	if n == 1:  # one cell: the residual IS its mean and the spread is exactly zero whatever the data; every gene is counted
		print('fitvar %s %s (%d, %d, %d): error/bound a %.3g, b %.3g, mean %.3g' % (dtype, storage, ng, n, nc, ra, rb, rm))
		assert ra <= 1 and rb <= 1 and rm <= 1 and (d_sc.cpu().numpy() == 0).all() and int(flags.cpu().numpy()[0]) == ng
		return
	snr = float(np.max(np.abs(mean) / sc))
	# cells
	d_b64, d_m64, d_s64 = up(p['b64']), up(p['mean64']), up(p['sc64'])
	tiles = -(-ng // int(lib.nrm_fitvar_row_tile()))
	part, d_v = torch.full((tiles, n), np.nan, **f64), torch.full((n, ), np.nan, **f64)
	_lib.check(lib.nrm_fitvar_cells(y.data_ptr(), ycode, ng, n, y.stride(0), u.data_ptr(), c.data_ptr(), nc, c.stride(0), d_b64.data_ptr(), d_m64.data_ptr(), d_s64.data_ptr(),
									part.data_ptr(), d_v.data_ptr(), st))
	r2, v = p['r2'], p['v']
	dr2 = absu * (nc * U * (np.abs(fl.ld(p['b64'])) @ absc)) + 2 * U * np.abs(r2)
	scl = fl.ld(p['sc64'])[:, None]
	d2 = (r2 - fl.ld(p['mean64'])[:, None]) / scl
	dd2 = dr2 / scl + 2 * U * np.abs(d2)
	dv = (2 * (np.abs(d2) * dd2).sum(axis=0) + (ng + 1) * U * (d2**2).sum(axis=0)) / ng + U * v
	rv = _ratio(d_v.cpu().numpy(), v, dv)
	assert _ratio(fl.ld(part.cpu().numpy()).sum(axis=0) / ng, v, dv) <= 1  # (the tiles' partial sums, added here: the fold of k_fv_finish apart)
	print('fitvar %s %s (%d, %d, %d): error/bound a %.3g, b %.3g, mean %.3g, sc %.3g, v %.3g; sqrt excess %.3g ulp; max |mean|/sc %.3g' % (
		dtype, storage, ng, n, nc, ra, rb, rm, rs, rv, _excess_ulps(d_sc.cpu().numpy(), sc, sc_prop), snr))
	assert ra <= 1 and rb <= 1 and rm <= 1 and rs <= 1 and rv <= 1
	assert int(flags.cpu().numpy()[0]) == 0
	assert n < 63 or snr > 1e-3  # the mean is a live value here (with an intercept among the covariates it is zero to rounding)
	assert _padding_untouched(y, whole, storage, 1e3)


def test_fitvar_genes_counts_constant_residuals():
	"""flags[0] += genes whose spread is zero: two rows the covariates explain exactly among five."""
	torch, _lib, eng = _env()
	rng = np.random.default_rng(8)
	n, nc, ng = 70, 2, 5
	c = rng.normal(size=(nc, n))
	y = rng.normal(size=(ng, n))
	y[1], y[4] = 0.0, 0.0
	mi = np.linalg.inv(c @ c.T)
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
	d_y, d_c, d_u, d_a, d_mi = up(y), up(c), up(np.ones(n)), up(y @ c.T), up(mi)
	f64 = dict(dtype=torch.float64, device='cuda')
	d_b, d_mean, d_sc = torch.empty((ng, nc), **f64), torch.empty((ng, ), **f64), torch.empty((ng, ), **f64)
	flags = eng.zeros((4, ), torch.int32)
	_lib.check(eng.lib.nrm_fitvar_genes(d_y.data_ptr(), _lib.NRM_F64, ng, n, n, d_u.data_ptr(), d_c.data_ptr(), nc, n, d_a.data_ptr(), d_mi.data_ptr(), d_b.data_ptr(),
										d_mean.data_ptr(), d_sc.data_ptr(), flags.data_ptr(), eng._stream()))
	assert flags.cpu().numpy().tolist() == [2, 0, 0, 0] and (d_sc.cpu().numpy()[[1, 4]] == 0).all() and (d_sc.cpu().numpy()[[0, 2, 3]] > 0).all()


# ---- the plan's kernels ----------------------------------------------------------------------------------------------------------------------------------------
def _state(bestv=1e300, steps=0.0, last=np.nan):
	torch, _, _ = _env()
	return torch.as_tensor(np.array([bestv, steps, last, 0.0])).cuda()


def test_plan_start():
	torch, _lib, eng = _env()
	for n in (1, 3, 257):
		s, best, state = (torch.full((k, ), 5.0, dtype=torch.float64, device='cuda') for k in (n, n, 4))
		_lib.check(eng.lib.nrm_fitvar_plan_start(n, s.data_ptr(), best.data_ptr(), state.data_ptr(), eng._stream()))
		h = state.cpu().numpy()
		assert (s.cpu().numpy() == 1).all() and np.isnan(best.cpu().numpy()).all() and h[0] == 1e300 and h[1] == 0 and np.isnan(h[2]) and h[3] == 0


DESIGN_CASES = [(1, 1), (3, 7), (63, 8), (64, 9), (65, 16), (255, 17), (256, 62), (257, 63), (1023, 1), (1024, 7), (1025, 8), (4096, 9), (4097, 63), (8193, 16)]


@pytest.mark.parametrize('n,nc', DESIGN_CASES)
@pytest.mark.parametrize('padded', [False, True])
def test_plan_design(n, nc, padded):
	torch, _lib, eng = _env()
	rng = np.random.default_rng(n + nc)
	c = rng.normal(size=(nc, n)) * 10.0**rng.uniform(-1.5, 1.5, nc)[:, None]
	s = 10.0**rng.uniform(-1, 1, n)
	d_c, _ = _place(c, 'padded' if padded else 'contiguous', fill=1e3)
	d_s, state = torch.as_tensor(s).cuda(), _state()
	f64 = dict(dtype=torch.float64, device='cuda')
	d_u, d_cw = torch.full((n, ), np.nan, **f64), torch.full((nc, n), np.nan, **f64)
	ws = torch.full((int(eng.lib.nrm_fitvar_plan_workspace(n, nc)), ), np.nan, **f64)
	_lib.check(eng.lib.nrm_fitvar_design(d_c.data_ptr(), nc, d_c.stride(0), n, d_s.data_ptr(), state.data_ptr(), 1e-6, d_u.data_ptr(), d_cw.data_ptr(), ws.data_ptr(), eng._stream()))
	u, cw, m, m_abs = fl.design(c, s)
	assert np.array_equal(d_u.cpu().numpy(), 1 / s)
	rc = _ratio(d_cw.cpu().numpy(), cw, 4 * U * np.abs(cw))
	npair, chunks = nc * (nc + 1) // 2, -(-n // 256)
	tri = fl.ld(ws[:chunks * npair].cpu().numpy().reshape(chunks, npair)).sum(axis=0)
	iu = np.triu_indices(nc)
	rg = _ratio(tri, m[iu], (256 + 4) * U * m_abs[iu])
	print('design (%d, %d) padded %s: error/bound cw %.3g, Gram %.3g' % (n, nc, padded, rc, rg))
	assert rc <= 1 and rg <= 1
	# stopped (bestv <= eps): nothing is written
	d_u.fill_(-1.0)
	stopped = _state(bestv=1e-7)
	_lib.check(eng.lib.nrm_fitvar_design(d_c.data_ptr(), nc, d_c.stride(0), n, d_s.data_ptr(), stopped.data_ptr(), 1e-6, d_u.data_ptr(), d_cw.data_ptr(), ws.data_ptr(), eng._stream()))
	assert (d_u.cpu().numpy() == -1).all()


def _device_pinv(m, tol=TOL):
	"""nrm_fitvar_pinv on a one-chunk workspace that holds the upper triangle of m, row by row."""
	torch, _lib, eng = _env()
	nc = m.shape[0]
	f64 = dict(dtype=torch.float64, device='cuda')
	ws = torch.as_tensor(np.ascontiguousarray(m[np.triu_indices(nc)])).cuda()
	assert int(eng.lib.nrm_fitvar_plan_workspace(1, nc)) >= ws.numel()
	full = torch.full((int(eng.lib.nrm_fitvar_plan_workspace(1, nc)), ), np.nan, **f64)
	full[:ws.numel()] = ws
	mi, rank, state = torch.full((nc, nc), np.nan, **f64), torch.full((1, ), -1, dtype=torch.int64, device='cuda'), _state()
	_lib.check(eng.lib.nrm_fitvar_pinv(1, nc, float(tol), state.data_ptr(), 1e-6, full.data_ptr(), mi.data_ptr(), rank.data_ptr(), eng._stream()))
	return mi.cpu().numpy(), int(rank.cpu().numpy()[0])


@pytest.mark.parametrize('n', [1, 2, 8, 9, 26, 63])
@pytest.mark.parametrize('kind', ['full', 'onehot', 'duplicate'])
@pytest.mark.parametrize('spread', [False, True])
def test_device_pinv_against_inv_rank_and_its_host_twin(n, kind, spread):
	"""The Gram matrices of tests/test_compute_var_plan_cpu.py through the 64-lane kernel: its rank against the host twin's, inv_rank's and the constructed one;
	its matrix symmetric and within that file's bound of both; and the same with every covariate times 1e-6 and 1e6 -- the rank rule is relative to the
	largest eigenvalue, so the ranks stay and the pseudo-inverse scales by the inverse square."""
	from normalisr_amd.association import inv_rank
	rng = np.random.default_rng(100 * n + 10 * len(kind) + spread)
	c, rank = _covariates(kind, n, rng)
	u = 10.0**rng.uniform(-1, 1, CELLS) if spread else np.ones(CELLS)
	cu = c * u
	base = None
	for scale in (1.0, 1e-6, 1e6):
		m = np.matmul(cu * scale, (cu * scale).T)
		sv = np.linalg.svd(m, compute_uv=False)
		assert not ((sv > TOL * sv[0] / 100) & (sv < TOL * sv[0] * 100)).any()  # no singular value near the threshold: the rule alone decides the rank
		ref, rref = inv_rank(m, tol=TOL)
		twin, rtwin = _pinv_host(m)
		got, r = _device_pinv(m)
		print(n, kind, spread, scale, 'rank', r, 'max scaled error: inv_rank %.3g, host twin %.3g' % (np.abs((got - ref) * sv[0]).max(), np.abs((got - twin) * sv[0]).max()))
		assert r == rtwin == rref == rank, (r, rtwin, rref, rank, scale)
		assert np.array_equal(got, got.T)
		assert close(got * sv[0], ref * sv[0], 1e-9, floor=1.0) and close(got * sv[0], twin * sv[0], 1e-9, floor=1.0)
		if base is None:
			base, s0 = got, sv[0]
		else:
			assert close(got * scale**2 * s0, base * s0, 1e-9, floor=1.0), scale


def test_device_pinv_leaves_everything_when_stopped():
	torch, _lib, eng = _env()
	f64 = dict(dtype=torch.float64, device='cuda')
	ws = torch.ones((int(eng.lib.nrm_fitvar_plan_workspace(1, 3)), ), **f64)
	mi, rank, state = torch.full((3, 3), 5.0, **f64), torch.full((1, ), -1, dtype=torch.int64, device='cuda'), _state(bestv=1e-7)
	_lib.check(eng.lib.nrm_fitvar_pinv(1, 3, 1e-8, state.data_ptr(), 1e-6, ws.data_ptr(), mi.data_ptr(), rank.data_ptr(), eng._stream()))
	assert (mi.cpu().numpy() == 5).all() and int(rank.cpu().numpy()[0]) == -1


def _update(v, c, m2i, s, best, state, eps, padded=False):
	"""nrm_fitvar_update on host arrays: (s, best, the next record, the chunks' [C;1] l added in longdouble)."""
	torch, _lib, eng = _env()
	nc, n = c.shape
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()
	d_c, _ = _place(np.asarray(c, dtype=np.float64), 'padded' if padded else 'contiguous', fill=1e3)
	d_v, d_m2i, d_s, d_best, d_state = up(v), up(m2i), up(s), up(best), up(state)
	nxt = torch.full((4, ), -7.0, dtype=torch.float64, device='cuda')
	ws = torch.full((int(eng.lib.nrm_fitvar_plan_workspace(n, nc)), ), np.nan, dtype=torch.float64, device='cuda')
	_lib.check(eng.lib.nrm_fitvar_update(d_v.data_ptr(), d_c.data_ptr(), nc, d_c.stride(0), n, d_m2i.data_ptr(), d_s.data_ptr(), d_best.data_ptr(), d_state.data_ptr(),
										 nxt.data_ptr(), float(eps), ws.data_ptr(), eng._stream()))
	dch, lch = -(-n // 256), -(-n // 1024)
	g0 = dch * (nc * (nc + 1) // 2)
	gp = fl.ld(ws[g0:g0 + lch * (nc + 1)].cpu().numpy().reshape(lch, nc + 1)).sum(axis=0)
	return d_s.cpu().numpy(), d_best.cpu().numpy(), nxt.cpu().numpy(), gp


def test_update_log_of_v_in_ulps():
	"""l = ln sqrt v seen directly: with one-hot covariate rows the partial sums of [C;1] l ARE the l of single cells (products with 1 and sums with 0 are exact)."""
	from normalisr_amd.association import inv_rank
	rng = np.random.default_rng(11)
	nc = n = 63
	c = np.eye(nc)
	c1 = np.vstack([c, np.ones((1, n))])
	m2i = inv_rank(c1 @ c1.T)[0]
	worst = ratio = 0.0
	for rep in range(12):
		v = np.exp(rng.normal(0, [0.01, 0.3, 3.0][rep % 3], n))
		v[:3] = [1.0, 1.0 + 2.0**-30, 4.0]
		_, _, _, g = _update(v, c, m2i, np.ones(n), np.ones(n), [1e300, 0, np.nan, 0], 1e-6)
		l = fl.logsum(v, c)[0]
		prop = U * np.ones(n)
		worst = max(worst, _excess_ulps(g[:nc].astype(np.float64), l, prop))
		ratio = max(ratio, _ratio(g[:nc], l, prop + L_ULP * fl.ulp(l)))
		assert g[0] == 0  # ln sqrt 1
	print('l = ln sqrt v, %d values: excess over the square root\'s rounding %.3g ulp; error/bound %.3g' % (12 * n, worst, ratio))
	assert ratio <= 1


UPDATE_CASES = [(1, 1), (3, 2), (63, 7), (64, 8), (65, 9), (255, 16), (256, 17), (257, 62), (1023, 63), (1024, 1), (1025, 7), (4096, 8), (4097, 9), (8193, 16)]


@pytest.mark.parametrize('n,nc', UPDATE_CASES)
def test_plan_update_against_the_reference(n, nc):
	from normalisr_amd.association import inv_rank
	rng = np.random.default_rng(3 * n + nc)
	nc_eff = min(nc, n)
	c = rng.normal(size=(nc, n))
	c[nc_eff:] = c[np.arange(nc - nc_eff) % nc_eff]
	c[0] += 3.0
	c1 = np.vstack([c, np.ones((1, n))])
	m2i = np.ascontiguousarray(inv_rank(c1 @ c1.T)[0])
	s = 10.0**rng.uniform(-1, 1, n)
	v = np.exp(0.8 * c[-1] + rng.normal(0, 0.3, n))
	bestv = 1e300 if n % 2 else 0.5
	state = np.array([bestv, 2.0, 0.25, 0.0])
	best = rng.uniform(1, 2, n)
	s_dev, best_dev, nxt, g_dev = _update(v, c, m2i, s, best, state, 1e-6, padded=bool(n % 3 == 0))
	l, g, g_abs = fl.logsum(v, c)
	dl = U + L_ULP * fl.ulp(l)
	ac1 = np.abs(fl.ld(c1))
	dg = n * U * g_abs + ac1 @ dl
	co, f, new = fl.new_scale(g.astype(np.float64), m2i, c, s)  # (the kernel keeps g in fp64)
	am = np.abs(fl.ld(m2i))
	dco = (nc + 1) * U * (am @ np.abs(g)) + am @ dg
	df = (nc + 1) * U * (np.abs(co) @ ac1) + dco @ ac1
	atmin = new <= new.min() * (1 + 1e-9)
	rel = df + df[atmin].max() + 4 * U
	ref_s = new / new.min()
	ds = ref_s * (rel + 2 * EXP_ULP * 2 * U)
	rg, rs = _ratio(g_dev, g, dg), _ratio(s_dev, ref_s, ds)
	t = np.abs((ref_s - fl.ld(s)) / fl.ld(s))
	t1 = t.max()
	dt1 = (ds / fl.ld(s) + 2 * U * t).max()
	better = t1 < bestv
	print('update (%d, %d): error/bound [C;1]l %.3g, new scale %.3g, t1 %.3g; exp excess %.3g ulp (two exps); t1 = %.6g' % (
		n, nc, rg, rs, _ratio(nxt[2], t1, dt1), _excess_ulps(s_dev, ref_s, ref_s * rel), float(t1)))
	assert rg <= 1 and rs <= 1 and _ratio(nxt[2], t1, dt1) <= 1
	assert abs(float(t1) - bestv) > 1e3 * float(dt1)  # (the comparison below is decided by the data, not by rounding)
	assert s_dev.min() == 1.0
	assert nxt[0] == (nxt[2] if better else bestv) and nxt[1] == 3.0 and nxt[3] == 0.0
	assert np.array_equal(best_dev, s_dev if better else best)


@pytest.mark.parametrize('name,bestv,eps,nan', [('below', 2.0, 1e-6, False), ('equal', 1.0, 1e-6, False), ('above', 0.5, 1e-6, False), ('stopped', 0.5, 0.5, False),
											   ('stopped below', 1e-7, 1e-6, False), ('nan', 2.0, 1e-6, True), ('first', 1e300, 1e-300, False)])
def test_plan_state_machine_exactly(name, bestv, eps, nan):
	"""Hand-made transitions.  v = 1 makes l, the coefficients and the fit exactly 0 and exp(0) exactly 1, so new = s / min(s) is one IEEE division and
	t1 = max |(new - s) / s| is numpy's to the bit: with min(s) = 1/2 the change is exactly 1.  s, best and the next record are compared EXACTLY with the reference
	transition: t1 below, equal to and above bestv, the stop test true, a NaN in v (a NaN t1 is never the best step, and every cell of the scale is NaN)."""
	from normalisr_amd.association import inv_rank
	rng = np.random.default_rng(1)
	n, nc = 300, 2
	c = rng.normal(size=(nc, n))
	c1 = np.vstack([c, np.ones((1, n))])
	m2i = inv_rank(c1 @ c1.T)[0]
	s = 2.0**rng.integers(-1, 4, n).astype(np.float64)
	s[n - 1] = 0.5
	best = rng.uniform(1, 2, n)
	v = np.ones(n)
	if nan:
		v[n - 2] = np.nan
	state = np.array([bestv, 4.0, 0.125, 0.0])
	new = np.full(n, np.nan) if nan else s / s.min()
	want_s, want_best, want_next = fl.transition(new, s, best, state, eps)
	got_s, got_best, got_next, _ = _update(v, c, m2i, s, best, state, eps)
	assert np.array_equal(got_s, want_s, equal_nan=True), name
	assert np.array_equal(got_best, want_best, equal_nan=True), name
	assert np.array_equal(got_next, want_next, equal_nan=True), (name, got_next, want_next)
	if name in ('below', 'first'):
		assert got_next[0] == 1.0 and np.array_equal(got_best, 2 * s)
	if name in ('equal', 'above', 'nan'):
		assert got_next[0] == bestv and got_next[1] == 5.0 and np.array_equal(got_best, best)


@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 1025, 8193])
def test_plan_weights(n):
	torch, _lib, eng = _env()
	rng = np.random.default_rng(n)
	best = 10.0**rng.uniform(-1, 1, n)

	def run(b):
		d_b, d_w = torch.as_tensor(b).cuda(), torch.full((n, ), np.nan, dtype=torch.float64, device='cuda')
		ws = torch.full((int(eng.lib.nrm_fitvar_plan_workspace(n, 1)), ), np.nan, dtype=torch.float64, device='cuda')
		flags = eng.zeros((4, ), torch.int32)
		_lib.check(eng.lib.nrm_fitvar_weights(d_b.data_ptr(), n, ws.data_ptr(), d_w.data_ptr(), flags.data_ptr(), eng._stream()))
		return d_w.cpu().numpy(), flags.cpu().numpy()
	w, f = run(best)
	want = 1 / best
	want = want / want.min()
	assert np.array_equal(w, want) and w.min() == 1.0 and f.tolist() == [0, 0, 0, 0]
	assert _ratio(w, fl.weights(best), 3 * U * fl.weights(best)) <= 1
	bad = best.copy()
	bad[n // 2] = np.nan  # the reference's `best is None`: weights that are not finite are counted
	w, f = run(bad)
	assert f[1] == n and np.isnan(w).all() and f[0] == 0
	if n > 1:
		bad = best.copy()
		bad[0] = 0.0  # 1 / 0: one infinite weight
		w, f = run(bad)
		assert f[1] == 1 and np.isinf(w[0]) and np.array_equal(w[1:], (1 / best[1:]) / (1 / best[1:]).min())
