"""GPU: the sparse-design de kernels (csrc/nrm_de_sparse.hip) at kernel level -- nrm_design_stats and nrm_de_sparse (and through it k_ds_ct) called directly through
the C ABI at every case of tests/ds_reference.py, every output against the longdouble reference of the same entry.

What is checked: placement (every output pre-filled with NaN, integers with -7, at a pitch above the minimum where the entry takes one, followed by a 1024-byte tail
that must stay untouched: dot only at nx x ny in the requested layout, ssy at ny, common at (nc + 1) x ny and only when d_ct is given, coefy at ny x nc, flags only
[2]); ct whole, bit for bit; the exact-data twin of every case bit for bit on every entry of common, ssy, coefy, dot, ss and coef; real data within the termwise
running-error bounds; the flags[2] count; the inputs unchanged; the lists (built by de_sparse.Lists) taken apart by lists_reference.decode before use, which adds
the tiny shapes (n < 2048, nx = 1025) to what nrm_design_count / _plan / _fill are held to; every call made twice with identical bits; one chain against
de_sparse.run bit for bit; the refusals.  tests/test_ds_reference_cpu.py shows that the comparators accept an fp64 emulation of every kernel at every case used
here and reject mutations of it, and that these cases launch all 32 instantiations of k_de_sparse.

Every test prints its worst error-to-bound ratio per output before it asserts (pytest -rP shows them); the last test prints the table of the run.
Measured on an MI355X: see DESIGN.md section 4b, "Sparse-design de at kernel level"."""
import functools

import numpy as np
import pytest

import ds_reference as ds
import stage_helpers
from stage_helpers import Buf, same, twice

pytestmark = pytest.mark.gpu

WORST = {}
F64, F32 = np.float64, np.float32
I32, I64 = np.int32, np.int64


@functools.lru_cache(maxsize=None)
def _env():
	import torch
	from normalisr_amd import _lib
	from normalisr_amd import engine
	return torch, _lib, engine.get_engine()


note = functools.partial(stage_helpers.note, WORST)


def _sync():
	_env()[0].cuda.synchronize()


def _p(b):
	return 0 if b is None else b.ptr


@functools.lru_cache(maxsize=None)
def problem(i, exact):
	return ds.problem(ds.CASES[i], exact)


LIST_FIELDS = ('ell', 'vals', 'base', 'w', 'sig', 'slot2x')


@functools.lru_cache(maxsize=None)
def _lists(n, nx, valued, exact):
	"""The lists of a design as the library builds them (de_sparse.Lists), held to the reader of tests/tools/lists_reference.py before they are used."""
	import lists_reference as lr
	torch, _, eng = _env()
	from normalisr_amd import de_sparse
	X = ds.design(n, nx, valued, exact)
	L = de_sparse.Lists(eng, torch.from_numpy(X).to(eng.device), max_density=1.0)
	assert L.ok and L.ngroups == ds.round_up(nx, 64) // 64
	h = {k: (None if getattr(L, k) is None else getattr(L, k).cpu().numpy()) for k in LIST_FIELDS}
	back, padded = lr.decode(nx, n, L.binary, h['ell'], h['vals'], h['base'], h['w'], h['slot2x'], h['sig'], L.ngroups)
	assert same(back, X) and padded == L.padded and L.nnz == int((X != 0).sum())
	row_ptr, cells, vals = ds.csr(X)
	assert np.array_equal(L.row_ptr.cpu().numpy(), row_ptr) and np.array_equal(L.cells.cpu().numpy()[:L.nnz], cells) and L.binary == (vals is None)
	assert vals is None or same(L.row_vals.cpu().numpy()[:L.nnz], vals)
	return L, h


def lists_of(pb):
	L, h = _lists(pb['n'], pb['nx'], pb['valued'], pb['exact'])
	assert L.binary == pb['binary']
	return L, h


# ---- nrm_de_sparse ---------------------------------------------------------------------------------------------------------------------------------------------------
def run_de(pb):
	torch, _lib, eng = _env()
	L, h = lists_of(pb)
	n, ny, nx, nc, cidx, by_gene = (pb[k] for k in ('n', 'ny', 'nx', 'nc', 'cidx', 'by_gene'))
	dtype = np.dtype(pb['dtype'])
	ldy, skip = ds.pitches(pb)
	ldc, ldb = ds.round_up(n, 2) + 2, nc + 3
	rows, cols = (ny, nx) if by_gene else (nx, ny)
	ldd = cols + 5
	nct = int(eng.lib.nrm_de_sparse_ct_doubles(n, nc, cidx))
	assert nct == ds.ct_doubles(n, nc, cidx) and int(eng.lib.nrm_de_sparse_chunk()) == ds.CH
	want_ct = ds.ct(pb['C'], nc, cidx, n)
	code = _lib.NRM_F64 if dtype == F64 else _lib.NRM_F32

	def run():
		d_y = Buf((ny, n), dtype, pitch=ldy, data=pb['Y'], skip=skip)
		assert ds.de_aligned(d_y.ptr, ldy, dtype.itemsize, n) == ds.case_aligned(pb), 'the case does not reach the instantiation it is for'
		d_c = Buf((nc, n), F64, pitch=ldc, data=pb['C']) if nc else None
		d_dci = Buf((nc, nc), F64, data=pb['dci']) if nc else None
		d_bx = Buf((nx, nc), F64, pitch=ldb, data=pb['bx']) if nc else None
		common = Buf((nc + 1, ny), F64, data=pb['common_in'])
		dot, ssy = Buf((rows, cols), F64, pitch=ldd), Buf(ny, F64)
		coefy = Buf((ny, nc), F64) if (pb['coefy'] and nc) else None
		flags = Buf(4, I32, data=[-7, -7, 0, -7]) if pb['flags'] else None
		ctb = Buf(nct, F64) if pb['fused'] else None
		_lib.check(eng.lib.nrm_de_sparse(d_y.ptr, code, ny, n, ldy, common.ptr, nc, _p(d_dci), L.ell.data_ptr(), 0 if L.vals is None else L.vals.data_ptr(), L.base.data_ptr(),
										 L.w.data_ptr(), L.sig.data_ptr(), L.ngroups, L.slot2x.data_ptr(), _p(d_bx), ldb, dot.ptr, ldd, by_gene, ssy.ptr, _p(coefy), _p(flags),
										 _p(d_c), ldc, cidx, float(pb['cval']), _p(ctb), eng._stream()))
		_sync()
		# the inputs are as they were
		assert same(d_y.get(), pb['Y']) and (not nc or (same(d_c.get(), pb['C']) and same(d_dci.get(), pb['dci']) and same(d_bx.get(), pb['bx'])))
		for k in LIST_FIELDS:
			assert h[k] is None or same(getattr(L, k).cpu().numpy(), h[k]), k
		res = dict(dot=dot.get(), ssy=ssy.get(), coefy=None if coefy is None else coefy.get(), flag=None, common=None)
		if flags is not None:
			f = flags.get()
			assert (f[[0, 1, 3]] == -7).all(), 'flags: only [2] is this entry\'s'
			res['flag'] = int(f[2])
		if pb['fused']:
			res['common'] = common.get()
			if want_ct is None:
				assert ctb.clean(), 'ct written though there is no group of covariates'
			else:
				res['ct'] = ctb.get()
		else:
			assert same(common.get(), pb['common_in']), 'common written though d_ct is NULL'
		return res
	got = twice(run)
	if want_ct is not None and pb['fused']:
		assert same(got['ct'], want_ct), 'ct differs from the rearranged covariates'
	return got


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('i', range(len(ds.CASES)), ids=lambda i: ds.case_id(ds.CASES[i]))
def test_ds_de_sparse(i, exact):
	"""k_ds_ct and every instantiation of k_de_sparse (float | double x ALIGNED x BINARY x NG -1, 0, 1, 2; one and two passes): common, ssy, coefy, dot bit for bit on
	the exact twin, inside their bounds on real data; the flags[2] count; the single=4 plan's use (Y is the design) also dot[i, j] against dot[j, i]."""
	pb = problem(i, exact)
	got = run_de(pb)
	ws = ds.judge_de_sparse(got, pb['ref'], exact)
	if pb['kind'] == 'self' and not exact:
		ws['symmetry'] = ds.judge_symmetry(got['dot'], pb['ref'])
	if pb['kind'] == 'cond' and not exact:
		ds.print_cancel_table(np.dtype(pb['dtype']).name, got, pb['ref'])
	for name in sorted(ds.de_instantiations(pb, pb['binary'])):
		note(name, ws, '%s %s' % (ds.case_id(pb), 'exact' if exact else 'real'))


# ---- nrm_design_stats ------------------------------------------------------------------------------------------------------------------------------------------------
def run_stats(row_ptr, cells, vals, C, dci, nc, n, with_flags=True):
	torch, _lib, eng = _env()
	nx, nnz = len(row_ptr) - 1, len(cells)
	ldc = n + 3

	def run():
		d_rp, d_cells = Buf(nx + 1, I64, data=row_ptr), Buf(max(nnz, 1), I32, data=cells if nnz else [0])
		d_vals = Buf(max(nnz, 1), F64, data=vals if nnz else [0.0]) if vals is not None else None
		d_c = Buf((nc, n), F64, pitch=ldc, data=C) if nc else None
		d_dci = Buf((nc, nc), F64, data=dci) if nc else None
		ss, coef = Buf(nx, F64), (Buf((nx, nc), F64) if nc else None)
		flags = Buf(4, I32, data=[-7, -7, 0, -7]) if with_flags else None
		_lib.check(eng.lib.nrm_design_stats(d_rp.ptr, d_cells.ptr, _p(d_vals), _p(d_c), ldc, nc, _p(d_dci), nx, ss.ptr, _p(coef), _p(flags), eng._stream()))
		_sync()
		assert same(d_rp.get(), np.asarray(row_ptr, I64)) and (not nnz or same(d_cells.get(), np.asarray(cells, I32))) and (not nc or same(d_c.get(), C))
		res = dict(ss=ss.get(), coef=None if coef is None else coef.get(), flag=None)
		if flags is not None:
			f = flags.get()
			assert (f[[0, 1, 3]] == -7).all(), 'flags: only [2] is this entry\'s'
			res['flag'] = int(f[2])
		return res
	return twice(run)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('case', ds.STATS, ids=lambda c: 'nx%d-nc%d-%s' % (c[0], c[1], 'valued' if c[2] else 'ones'))
def test_ds_design_stats(case, exact):
	"""k_design_stats: rows of 0, 1, 63, 64, 65 and 200 entries; ss against the residual-first value (exact twin: the difference form, bit for bit), coef, the count of
	rows inside the covariates' span (a row equal to an indicator covariate is counted, a row at ratio 2e-4 is not)."""
	nx, nc, valued = case
	C = ds.covariates(nc, ds.STATS_N, nc - 1, 1.0, exact, indicator=True)
	dci = ds.inverse(C, exact)
	row_ptr, cells, vals = ds.csr(ds.stats_design(nx, valued, exact, C))
	ref = ds.design_stats(row_ptr, cells, vals, C, dci, nc, exact)
	got = run_stats(row_ptr, cells, vals, C, dci, nc, ds.STATS_N, with_flags=not (nx == 1 and valued))
	note('k_design_stats', ds.judge_design_stats(got, ref, exact), '%s %s' % (case, 'exact' if exact else 'real'))


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ds_chain_is_what_the_module_runs():
	"""65 design rows x 9 genes x 4100 cells x 5 covariates, fp32: nrm_design_stats -> nrm_de_sparse called here, bit for bit against the buffers de_sparse.run
	produces for the same inputs."""
	torch, _lib, eng = _env()
	from normalisr_amd import de_sparse
	nx, ny, n, nc = (ds.CHAIN[k] for k in ('nx', 'ny', 'n', 'nc'))
	c = ds._case('chain', n, ny, nx, nc, nc - 1, 1.0, F32, False)
	pb = ds.problem(c, False, seed=11)
	d_x, d_y = torch.from_numpy(pb['X']).to(eng.device), torch.from_numpy(pb['Y']).to(eng.device)
	d_c, d_dci = torch.from_numpy(pb['C']).to(eng.device), torch.from_numpy(pb['dci']).to(eng.device)
	L = de_sparse.Lists(eng, d_x, max_density=1.0)
	flags = eng.new_flags()
	dot, rx, ssy, coefy = de_sparse.run(eng, d_x, L, d_y, d_c, d_dci, nc, nx, ny, n, nc, True, flags)
	_sync()
	ci, cval = eng.constant_row(d_c)
	# the same two entries, called here
	ss, coef, fl = Buf(nx, F64), Buf((nx, nc), F64), Buf(4, I32, data=[0, 0, 0, 0])
	_lib.check(eng.lib.nrm_design_stats(L.row_ptr.data_ptr(), L.cells.data_ptr(), 0, d_c.data_ptr(), n, nc, d_dci.data_ptr(), nx, ss.ptr, coef.ptr, fl.ptr, eng._stream()))
	common, mydot, myssy, mycoefy = Buf((nc + 1, ny), F64), Buf((nx, ny), F64), Buf(ny, F64), Buf((ny, nc), F64)
	ctb = Buf(int(eng.lib.nrm_de_sparse_ct_doubles(n, nc, ci)), F64)
	_lib.check(eng.lib.nrm_de_sparse(d_y.data_ptr(), _lib.NRM_F32, ny, n, n, common.ptr, nc, d_dci.data_ptr(), L.ell.data_ptr(), 0, L.base.data_ptr(), L.w.data_ptr(),
									 L.sig.data_ptr(), L.ngroups, L.slot2x.data_ptr(), coef.ptr, nc, mydot.ptr, ny, 0, myssy.ptr, mycoefy.ptr, fl.ptr, d_c.data_ptr(), n, ci, float(cval),
									 ctb.ptr, eng._stream()))
	_sync()
	assert same(ss.get(), rx.ss[:nx].cpu().numpy()) and same(coef.get(), rx.coef.cpu().numpy())
	assert same(mydot.get(), dot[:nx, :ny].cpu().numpy()) and same(myssy.get(), ssy[:ny].cpu().numpy()) and same(mycoefy.get(), coefy.cpu().numpy())
	assert same(common.get()[nc], rx.yraw.cpu().numpy())
	assert fl.get().tolist() == flags.cpu().numpy().tolist()
	# and the chain is right: each entry against its reference
	row_ptr, cells, vals = ds.csr(pb['X'])
	st = ds.design_stats(row_ptr, cells, vals, pb['C'], pb['dci'], nc)
	note('chain: k_design_stats', ds.judge_design_stats(dict(ss=ss.get(), coef=coef.get()), st, False), 'chain')
	ref = ds.de_sparse(pb['Y'], None, pb['C'], pb['dci'], pb['X'], coef.get(), ci, cval)
	note('chain: k_de_sparse', ds.judge_de_sparse(dict(dot=mydot.get(), ssy=myssy.get(), coefy=mycoefy.get(), common=common.get()), ref, False), 'chain')


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
DE_ARGS = ('d_y', 'y_dtype', 'ny', 'n', 'ldy', 'd_common', 'nc', 'd_dci', 'd_ell', 'd_ellv', 'd_base', 'd_w', 'd_sig', 'ngroups', 'd_slot2x', 'd_bx', 'ldb', 'd_dot', 'ldd', 'by_gene',
		   'd_ssy', 'd_coefy', 'd_flags', 'd_c', 'ldc', 'const_idx', 'const_val', 'd_ct', 'stream')


def test_ds_refusals_write_nothing():
	"""Every NRM_REQUIRE of nrm_de_sparse and nrm_design_stats: an error code, and no output touched."""
	torch, _lib, eng = _env()
	n, ny, nx, nc = 2048, 5, 65, 5
	pb = ds.problem(ds._case('refusal', n, ny, nx, nc, 4, 1.0, F32, True), True)
	L, _ = lists_of(pb)
	d_y, d_c = Buf((ny, n), F32, data=pb['Y']), Buf((33, n), F64, data=np.ones((33, n)))
	d_dci, d_bx = Buf((33, 33), F64, data=np.ones((33, 33))), Buf((nx, 33), F64, data=np.ones((nx, 33)))
	out = dict(common=Buf((34, ny), F64), dot=Buf((nx, ny), F64), ssy=Buf(ny, F64), coefy=Buf((ny, 33), F64), flags=Buf(4, I32), ct=Buf(3 * 4 * n, F64))
	base = dict(d_y=d_y.ptr, y_dtype=_lib.NRM_F32, ny=ny, n=n, ldy=n, d_common=out['common'].ptr, nc=nc, d_dci=d_dci.ptr, d_ell=L.ell.data_ptr(), d_ellv=L.vals.data_ptr(),
				d_base=L.base.data_ptr(), d_w=L.w.data_ptr(), d_sig=L.sig.data_ptr(), ngroups=L.ngroups, d_slot2x=L.slot2x.data_ptr(), d_bx=d_bx.ptr, ldb=nc, d_dot=out['dot'].ptr,
				ldd=ny, by_gene=0, d_ssy=out['ssy'].ptr, d_coefy=out['coefy'].ptr, d_flags=out['flags'].ptr, d_c=d_c.ptr, ldc=n, const_idx=4, const_val=1.0, d_ct=out['ct'].ptr,
				stream=eng._stream())
	bad = [dict(nc=33), dict(nc=-1), dict(ny=0), dict(n=0), dict(ngroups=0), dict(ngroups=1 << 24), dict(y_dtype=99), dict(ldy=n - 1), dict(ldb=nc - 1), dict(ldd=ny - 1),
		   dict(nc=9, const_idx=-1), dict(nc=10, const_idx=9, ldb=10), dict(d_c=0), dict(ldc=n - 1)]
	bad += [{k: 0} for k in ('d_y', 'd_common', 'd_ell', 'd_base', 'd_w', 'd_sig', 'd_slot2x', 'd_dot', 'd_ssy', 'd_dci', 'd_bx')]
	for change in bad:
		args = dict(base, **change)
		if 'ldb' not in change:
			args['ldb'] = max(args['nc'], 1)
		rc = eng.lib.nrm_de_sparse(*[args[k] for k in DE_ARGS])
		_sync()
		assert rc != 0, ('nrm_de_sparse accepted', change)
		assert all(b.clean() for b in out.values()), ('nrm_de_sparse wrote something', change)
	assert 'nrm_de_sparse' in eng.lib.nrm_last_error().decode()
	# the same arguments unchanged are accepted (the refusals above are the changes' doing)
	_lib.check(eng.lib.nrm_de_sparse(*[base[k] for k in DE_ARGS]))
	_sync()
	assert not np.isnan(out['dot'].get()).any()
	row_ptr, cells, vals = ds.csr(pb['X'])
	d_rp, d_cells, d_vals = Buf(nx + 1, I64, data=row_ptr), Buf(len(cells), I32, data=cells), Buf(len(cells), F64, data=vals)
	ss, coef, flags = Buf(nx, F64), Buf((nx, 33), F64), Buf(4, I32)
	sbase = [d_rp.ptr, d_cells.ptr, d_vals.ptr, d_c.ptr, n, nc, d_dci.ptr, nx, ss.ptr, coef.ptr, flags.ptr, eng._stream()]
	for at, v in ((7, 0), (5, 33), (5, -1), (0, 0), (1, 0), (8, 0), (3, 0), (6, 0), (9, 0)):
		args = list(sbase)
		args[at] = v
		rc = eng.lib.nrm_design_stats(*args)
		_sync()
		assert rc != 0, ('nrm_design_stats accepted', at, v)
		assert ss.clean() and coef.clean() and flags.clean(), ('nrm_design_stats wrote something', at, v)
	_lib.check(eng.lib.nrm_design_stats(*sbase))
	_sync()
	assert not np.isnan(ss.get()).any()


def test_zz_table_of_the_run():
	"""The worst error-to-bound ratio per kernel and output over the tests above (pytest -rP); alone it prints nothing."""
	for (kernel, name), (ratio, case) in sorted(WORST.items()):
		print('%-40s %-10s %.3g  (%s)' % (kernel, name, ratio, case))
	assert all(r <= 1 for r, _ in WORST.values())
