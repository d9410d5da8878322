"""GPU: the single=4 kernels (csrc/nrm_single4.hip) and K2', the fp64 matrix-core Gram kernel (csrc/nrm_gram.hip), at kernel level -- nrm_gram_f64, _band, _whole,
nrm_gram_i8_fix_dot, nrm_spd_prepare, _start, _transpose_residual, _update, _finish, nrm_single4_design_scalars, nrm_single4_sweep and nrm_single4_sweep_guarded
called directly through the C ABI, every output against the stage reference of tests/s4_reference.py.

What is checked: placement (every output pre-filled with NaN, integers with -7, at a pitch above the minimum where the entry has one, followed by a 1024-byte tail
that must stay untouched; for the Gram kernel: nothing outside the `need` sub-blocks of a tile its workgroup stores, nothing outside the launch's tiles); copies,
integers and exact-data sums bit for bit; real-data sums and every pair's stat and vary within the running-error bounds of the longdouble values (no pair
skipped; the Gram kernel's largest launches on the first, the last and five rows of every tile row -- their exact-data run compares every entry); P of the
planted pairs and a spread of ln P against mpmath at 60 digits; the counters by count; the guard pair by pair; the Newton-Schulz chain bit for bit against
single4._spd_inverse_fixed and its residual against the longdouble residual; every call made twice with identical bits; the refusals.
tests/test_s4_reference_cpu.py shows that the comparators accept an fp64 emulation of every kernel at every shape used here and reject mutations of it.

The Gram kernel contracts all of k_pad: the padded K columns are the caller's to keep zero (K1 writes them as zeros); operand rows at and beyond ceil16(rows) are
NaN here, so a row that leaked into another would show.

Every test prints its worst error-to-bound ratio per output before it asserts (pytest -rP shows them); the last test prints the table of the run.
Measured on an MI355X: see DESIGN.md section 6, "single=4 at kernel level"."""
import functools

import numpy as np
import pytest

import s4_reference as s4
import stage_helpers
from stage_helpers import Buf, same, twice

pytestmark = pytest.mark.gpu

WORST = {}
F64, F32 = np.float64, np.float32
I32, I64 = np.int32, np.int64
note = functools.partial(stage_helpers.note, WORST)


@functools.lru_cache(maxsize=None)
def _env():
	import torch
	from normalisr_amd import _lib
	from normalisr_amd import engine
	return torch, _lib, engine.get_engine()


def _sync():
	_env()[0].cuda.synchronize()


def _code(dtype):
	_lib = _env()[1]
	return _lib.NRM_F64 if np.dtype(dtype) == F64 else _lib.NRM_F32


def _slots():
	"""The persistent workgroups of a K2' launch on this device: two per CU, rounded down to a multiple of 8 (nrm_gram_f64_band, gram_plan)."""
	torch = _env()[0]
	n = 2 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
	return n - n % 8


# ---- gram --------------------------------------------------------------------------------------------------------------------------------------------------------
def run_gram(case, exact):
	_, _lib, eng = _env()
	name, m_pad, n_pad, k_pad, sym, m_rows, n_rows, row0, row1, whole = case
	A, B = s4.gram_data(case, exact)
	lda, ldd = k_pad + 2, n_pad + 2
	row1 = m_pad if row1 is None else row1

	def run():
		d_a = Buf((m_pad, k_pad), F64, pitch=lda, data=A)
		d_b = d_a if sym else Buf((n_pad, k_pad), F64, pitch=lda, data=B)
		out = Buf((m_pad, n_pad), F64, pitch=ldd)
		if whole:
			rc = eng.lib.nrm_gram_f64_whole(d_a.ptr, d_b.ptr, m_pad, n_pad, k_pad, lda, lda, out.ptr, ldd, m_rows, n_rows, eng._stream())
		elif row0 or row1 != m_pad:
			rc = eng.lib.nrm_gram_f64_band(d_a.ptr, d_b.ptr, m_pad, n_pad, k_pad, lda, lda, out.ptr, ldd, sym, m_rows, n_rows, row0, row1, eng._gram_ws(), eng._stream())
		else:
			rc = eng.lib.nrm_gram_f64(d_a.ptr, d_b.ptr, m_pad, n_pad, k_pad, lda, lda, out.ptr, ldd, sym, m_rows, n_rows, eng._gram_ws(), eng._stream())
		_lib.check(rc)
		_sync()
		d_a.get(), d_b.get()  # (operands and their padding untouched)
		return dict(dot=out.get())
	return twice(run)['dot']


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('case', s4.GRAM, ids=lambda c: c[0])
def test_s4_gram(case, exact):
	"""k_gram_f64 + k_gram_fixup on the schedule of this device's slot count: integer-valued operands bit for bit against exact sums, every entry; real operands
	inside k_pad + pieces - 1 roundings of the absolute sum; nothing written outside the need sub-blocks (tiles stored whole) or the launch's tiles."""
	s = s4.gram_case(case, _slots())
	print('%s on %d slots: %s' % (case[0], _slots(), sorted(s4.branches(s))))
	got = run_gram(case, exact)
	m_pad = case[1]
	row1 = m_pad if case[8] is None else case[8]
	rows = np.arange(case[7], min(row1, s['m_rows'])) if exact else s4.gram_rows(case)
	ws = s4.judge_gram(got[rows], s4.gram(case, s, exact, rows), exact)
	ws['placement'] = s4.judge_gram_placement(case, s, got, np.arange(m_pad))
	note('nrm_gram_f64' + ('_whole' if case[9] else ('_band' if case[7] else '')), ws, '%s %s' % (case[0], 'exact' if exact else 'real'))


def test_s4_gram_whole_bits_do_not_depend_on_the_launch():
	"""nrm_gram_f64_whole: an entry is one chain over the cells whatever the launch's shape -- the first tile of 'whole:straddle' launched alone has the same bits."""
	_, _lib, eng = _env()
	case = [c for c in s4.GRAM if c[0] == 'whole:straddle'][0]
	full = run_gram(case, False)
	A, B = s4.gram_data(case, False)
	d_a, d_b, out = Buf((128, 6400), F64, pitch=6402, data=A), Buf((128, 6400), F64, pitch=6402, data=B[:128]), Buf((128, 128), F64, pitch=130)
	_lib.check(eng.lib.nrm_gram_f64_whole(d_a.ptr, d_b.ptr, 128, 128, 6400, 6402, 6402, out.ptr, 130, 128, 128, eng._stream()))
	_sync()
	assert same(np.ascontiguousarray(full[:128, :128]), out.get())


def test_s4_gram_refusals_write_nothing():
	_, _lib, eng = _env()
	lib, st, ws = eng.lib, eng._stream(), eng._gram_ws()
	a, out = Buf((2048, 32), F64, pitch=34, data=np.ones((2048, 32))), Buf((2048, 2048), F64, pitch=2050)
	odd = Buf((128, 32), F64, pitch=35, data=np.ones((128, 32)))
	mis = Buf((128, 32), F64, pitch=34, data=np.ones((128, 32)), skip=1)
	calls = [
		('odd pitch', lambda: lib.nrm_gram_f64(odd.ptr, odd.ptr, 128, 128, 32, 35, 35, out.ptr, 2050, 0, 128, 128, ws, st)),
		('odd output pitch', lambda: lib.nrm_gram_f64(a.ptr, a.ptr, 128, 128, 32, 34, 34, out.ptr, 2051, 0, 128, 128, ws, st)),
		('misaligned operand', lambda: lib.nrm_gram_f64(mis.ptr, a.ptr, 128, 128, 32, 34, 34, out.ptr, 2050, 0, 128, 128, ws, st)),
		('unpadded rows', lambda: lib.nrm_gram_f64(a.ptr, a.ptr, 120, 128, 32, 34, 34, out.ptr, 2050, 0, 120, 128, ws, st)),
		('unpadded cells', lambda: lib.nrm_gram_f64(a.ptr, a.ptr, 128, 128, 30, 34, 34, out.ptr, 2050, 0, 128, 128, ws, st)),
		('symmetric rectangle', lambda: lib.nrm_gram_f64(a.ptr, a.ptr, 128, 256, 32, 34, 34, out.ptr, 2050, 1, 128, 256, ws, st)),
		('band not cut at 1024', lambda: lib.nrm_gram_f64_band(a.ptr, a.ptr, 2048, 2048, 32, 34, 34, out.ptr, 2050, 0, 2048, 2048, 512, 2048, ws, st)),
		('band end not cut at 1024', lambda: lib.nrm_gram_f64_band(a.ptr, a.ptr, 2048, 2048, 32, 34, 34, out.ptr, 2050, 0, 2048, 2048, 0, 1000, ws, st)),
		('null workspace', lambda: lib.nrm_gram_f64(a.ptr, a.ptr, 128, 128, 32, 34, 34, out.ptr, 2050, 0, 128, 128, 0, st)),
		('whole: odd pitch', lambda: lib.nrm_gram_f64_whole(odd.ptr, odd.ptr, 128, 128, 32, 35, 35, out.ptr, 2050, 128, 128, st)),
		('whole: misaligned operand', lambda: lib.nrm_gram_f64_whole(a.ptr, mis.ptr, 128, 128, 32, 34, 34, out.ptr, 2050, 128, 128, st)),
	]
	for what, call in calls:
		rc = call()
		_sync()
		print('%-28s -> %d  %s' % (what, rc, lib.nrm_last_error().decode()))
		assert rc != 0, what
		assert out.clean(), what


# ---- fix_dot -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('ns', s4.FIX_NS)
def test_s4_fix_dot(ns, exact):
	"""k_fix_dot over ragged 16-row x 64-column blocks: dot += the mean-product correction, in place; bit for bit on exact records."""
	_, _lib, eng = _env()
	for rows in s4.FIX_ROWS:
		for cols in s4.FIX_COLS:
			dot, fr, fc, n = s4.fix_problem(rows, cols, ns, exact)

			def run():
				d = Buf((rows, cols), F64, pitch=cols + 3, data=dot)
				d_fr, d_fc = Buf((rows, 8), F64, data=fr), Buf((cols, 8), F64, data=fc)
				_lib.check(eng.lib.nrm_gram_i8_fix_dot(d.ptr, cols + 3, d_fr.ptr, d_fc.ptr, rows, cols, ns, n, eng._stream()))
				_sync()
				assert same(d_fr.get(), fr) and same(d_fc.get(), fc)
				return dict(dot=d.get())
			got = twice(run)['dot']
			note('nrm_gram_i8_fix_dot', s4.judge_fix_dot(got, s4.fix_dot(dot, fr, fc, ns, n, exact), exact), '%dx%d ns%d %s' % (rows, cols, ns, 'exact' if exact else 'real'))


# ---- the small steps around the Newton-Schulz inverse --------------------------------------------------------------------------------------------------------------
def _m_device(m, nx, ldm):
	"""d_m as a symmetric Gram launch leaves it, and worse: the strict lower triangle is NaN (it must not be read)."""
	md = np.triu(m).copy()
	md[np.tril_indices(nx, -1)] = np.nan
	return Buf((nx, nx), F64, pitch=ldm, data=md), md


def run_prepare(md, nx, nxp, ldm):
	_, _lib, eng = _env()

	def run():
		d_m = Buf((nx, nx), F64, pitch=ldm, data=md)
		mp, scal, work = Buf((nxp, nxp), F64), Buf(2, F64), Buf(2 * nxp, F64)
		_lib.check(eng.lib.nrm_spd_prepare(d_m.ptr, ldm, nx, nxp, mp.ptr, scal.ptr, work.ptr, eng._stream()))
		_sync()
		w = work.get()
		assert np.isnan(w[nx:nxp]).all() and np.isnan(w[nxp + nx:]).all(), 'd_work: only rows [0, nx) of each half'
		return dict(mp=mp.get(), scal=scal.get())
	return twice(run)


@pytest.mark.parametrize('nx,nxp', s4.SPD)
def test_s4_spd_small_kernels(nx, nxp):
	"""nrm_spd_prepare (k_spd_sym, k_spd_rows, k_spd_scale), both nrm_spd_start, nrm_spd_transpose_residual and nrm_spd_finish on one matrix per shape."""
	_, _lib, eng = _env()
	st = eng._stream()
	m = s4.spd_matrix(nx)
	ldm = nx + 3
	_, md = _m_device(m, nx, ldm)
	got = run_prepare(md, nx, nxp, ldm)
	ref = s4.spd_prepare(md, nx, nxp)
	note('nrm_spd_prepare', s4.judge_spd_prepare(got['mp'], got['scal'], ref, nx, nxp), 'nx %d' % nx)
	if nx >= 2:  # NaN off the diagonal -> scal[0]; on it -> scal[1]
		for (i, j) in ((0, nx - 1), (nx // 2, nx // 2)):
			mn = md.copy()
			mn[i, j] = np.nan
			g = run_prepare(mn, nx, nxp, ldm)
			assert np.isnan(g['scal'][0]) and np.isnan(g['scal'][1]) == (i == j), ('NaN at', i, j, g['scal'])
	mp, scal = got['mp'], got['scal']
	xs = {}
	for diagonal in (1, 0):
		def run():
			d_mp, d_scal, x = Buf((nxp, nxp), F64, data=mp), Buf(2, F64, data=scal), Buf((nxp, nxp), F64)
			_lib.check(eng.lib.nrm_spd_start(d_mp.ptr, nxp, diagonal, d_scal.ptr, x.ptr, st))
			_sync()
			return dict(x=x.get())
		xs[diagonal] = twice(run)['x']
		note('nrm_spd_start', dict(x=s4.bits(xs[diagonal], s4.spd_start(mp, nxp, diagonal, scal[0]), 'diag(1 / M_ii) | I / ||M||_1')), 'nx %d diagonal %d' % (nx, diagonal))
	t = mp @ xs[1]  # (any matrix will do: the stage is judged on what it is given)
	t[nxp - 1, 0] = 0.375

	def run_tr():
		d_t, tt, res, work = Buf((nxp, nxp), F64, data=t), Buf((nxp, nxp), F64), Buf(1, F64), Buf((nxp // 32)**2, F64)
		_lib.check(eng.lib.nrm_spd_transpose_residual(d_t.ptr, nxp, tt.ptr, res.ptr, work.ptr, st))
		_sync()
		return dict(tt=tt.get(), res=res.get(), part=work.get())
	g = twice(run_tr)
	rr = s4.spd_transpose_residual(t, nxp)
	note('nrm_spd_transpose_residual', dict(tt=s4.bits(g['tt'], rr['tt'], 'tt == t^T'), res=s4.worst(np.abs(s4.ld(g['res']) - rr['res']), np.asarray([rr['res_bound']]), '||I - T||_F')),
		 'nx %d' % nx)
	xn = xs[1] @ t.T
	ss = np.diagonal(m).copy()

	def run_fin():
		d_x, d_ss, n_, small = Buf((nxp, nxp), F64, data=xn), Buf(nx, F64, data=ss), Buf((nxp, nxp), F64), Buf((3, nx), F64)
		_lib.check(eng.lib.nrm_spd_finish(d_x.ptr, nx, nxp, d_ss.ptr, n_.ptr, small.ptr, st))
		_sync()
		return dict(n=n_.get(), small=small.get())
	g = twice(run_fin)
	note('nrm_spd_finish', s4.judge_spd_finish(g['n'], g['small'], s4.spd_finish(xn, nx, nxp, ss)), 'nx %d' % nx)


@pytest.mark.parametrize('count', s4.UPDATE_COUNTS)
def test_s4_spd_update(count):
	"""k_spd_update: the double2 body and the scalar tail; 2 x - xt is one rounding."""
	_, _lib, eng = _env()
	rng = np.random.default_rng(count)
	x, xt = rng.normal(size=count), rng.normal(size=count)

	def run():
		d_x, d_xt = Buf(count, F64, data=x), Buf(count, F64, data=xt)
		_lib.check(eng.lib.nrm_spd_update(d_x.ptr, d_xt.ptr, count, eng._stream()))
		_sync()
		assert same(d_xt.get(), xt)
		return dict(x=d_x.get())
	note('nrm_spd_update', dict(x=s4.bits(twice(run)['x'], s4.spd_update(x, xt), 'fl(2 x - xt)')), 'count %d' % count)


def test_s4_spd_refusals_write_nothing():
	"""nrm_spd_update reads and writes double2: a pointer that is not 16-byte aligned is refused before any launch.  And one NRM_REQUIRE of each other entry."""
	_, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	x, xt = Buf(64, F64, data=np.ones(64)), Buf(64, F64, data=np.ones(64))
	x1, xt1 = Buf(64, F64, data=np.ones(64), skip=1), Buf(64, F64, data=np.ones(64), skip=1)
	out = Buf((64, 64), F64)
	calls = [
		('update: d_x misaligned', lambda: lib.nrm_spd_update(x1.ptr, xt.ptr, 64, st)),
		('update: d_xt misaligned', lambda: lib.nrm_spd_update(x.ptr, xt1.ptr, 64, st)),
		('update: count 0', lambda: lib.nrm_spd_update(x.ptr, xt.ptr, 0, st)),
		('prepare: nxp not a multiple of 32', lambda: lib.nrm_spd_prepare(x.ptr, 8, 8, 40, out.ptr, out.ptr, out.ptr, st)),
		('prepare: ldm < nx', lambda: lib.nrm_spd_prepare(x.ptr, 7, 8, 64, out.ptr, out.ptr, out.ptr, st)),
		('transpose_residual: nxp not a multiple of 32', lambda: lib.nrm_spd_transpose_residual(x.ptr, 8, out.ptr, out.ptr, out.ptr, st)),
		('finish: d_n == d_x', lambda: lib.nrm_spd_finish(out.ptr, 8, 64, x.ptr, out.ptr, out.ptr, st)),
		('design_scalars: nx 0', lambda: lib.nrm_single4_design_scalars(x.ptr, 0, 16, out.ptr, out.ptr, out.ptr, st)),
	]
	for what, call in calls:
		rc = call()
		_sync()
		print('%-46s -> %d  %s' % (what, rc, lib.nrm_last_error().decode()))
		assert rc != 0, what
		assert out.clean() and same(x.get(), np.ones(64)) and same(x1.get(), np.ones(64)), what


# ---- design scalars ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nx', s4.SCALARS_NX)
def test_s4_design_scalars(nx):
	"""k_s4_design_scalars: dxx = fl(1 / fl(n d)), varx with 0 -> 1, flags[5] += rows whose d, kappa numerator or row sum is not a positive finite number."""
	_, _lib, eng = _env()
	small, n = s4.scalars_input(nx), 4096
	ref = s4.design_scalars(small, nx, n)

	def run():
		d_small, dxx, varx = Buf((3, nx), F64, data=small), Buf(nx, F64), Buf(nx, F64)
		flags = Buf(8, I32, data=np.array([-7, -7, -7, -7, -7, 11, -7, -7], dtype=I32))
		_lib.check(eng.lib.nrm_single4_design_scalars(d_small.ptr, nx, n, dxx.ptr, varx.ptr, flags.ptr, eng._stream()))
		_sync()
		f = flags.get()
		assert (np.delete(f, 5) == -7).all(), 'only flags[5]'
		return dict(dxx=dxx.get(), varx=varx.get(), count=int(f[5]) - 11)
	g = twice(run)
	note('nrm_single4_design_scalars', dict(dxx=s4.bits(g['dxx'], ref['dxx'], 'fl(1 / fl(n d))'), varx=s4.bits(g['varx'], ref['varx'], '0 -> 1'),
											flags5=s4.Worst(0.0 if g['count'] == ref['count'] else np.inf, None, 'flags[5] += %d == %d' % (g['count'], ref['count']))), 'nx %d' % nx)


# ---- rss and the sweep -----------------------------------------------------------------------------------------------------------------------------------------------
def run_sweep(pb, dtype, return_dot, guard=None, flags0=(3, 5, 0, 0), with_hits=True):
	"""guard: (fy, kappa, cstar, gstar, ns, budget) -> nrm_single4_sweep_guarded."""
	_, _lib, eng = _env()
	nx, ny, m = pb.nx, pb.ny, pb.m
	ldb, ldo = m + 3, ny + 3

	def run():
		bt, pt = Buf((ny, m), F64, pitch=ldb, data=pb.bt), Buf((ny, m), F64, pitch=ldb, data=pb.pt)
		yy, dxx, work = Buf(ny, F64, data=pb.yy), Buf(nx, F64, data=pb.dxx), Buf(ny, F64)
		o = {k: Buf((nx, ny), dtype, pitch=ldo) for k in ('p', 'stat', 'vary')}
		flags = Buf(6, I32, data=np.array(list(flags0) + [-7, -7], dtype=I32))
		args = (bt.ptr, pt.ptr, ldb, yy.ptr, dxx.ptr, nx, ny, m, pb.n, pb.dof, return_dot, o['p'].ptr, o['stat'].ptr, o['vary'].ptr, _code(dtype), ldo, work.ptr, flags.ptr)
		hits = None
		if guard is None:
			_lib.check(eng.lib.nrm_single4_sweep(*args, eng._stream()))
		else:
			fy, kappa, cstar, gstar, ns, budget = guard
			d_fy, d_k = Buf((ny, 8), F64, data=fy), Buf(nx, F64, data=kappa)
			hits = Buf(ny, I32, data=np.zeros(ny, dtype=I32)) if with_hits else None
			_lib.check(eng.lib.nrm_single4_sweep_guarded(*args, d_fy.ptr, d_k.ptr, cstar, gstar, ns, budget, hits.ptr if hits else 0, eng._stream()))
		_sync()
		res = {k: b.get() for k, b in o.items()}
		res.update(rss=work.get(), flags=flags.get())
		if hits is not None:
			res['hits'] = hits.get()
		return res
	return twice(run)


@pytest.mark.parametrize('case', s4.sweep_cases(), ids=lambda c: 'nx%d-ny%d-m+%d-dof%d-%s-dot%d' % (c[0], c[1], c[2], c[3], np.dtype(c[4]).name, c[5]))
def test_s4_rss_and_sweep(case):
	"""k_s4_rss and k_s4_sweep<double | float>: ragged 64-wide tiles on both axes, the edge values of s4_reference.sweep_problem; every pair's stat and vary,
	P on the planted pairs and a spread, flags[0..1] by count on top of a non-zero pre-fill."""
	nx, ny, extra, dof, dtype, rd = case
	pb = s4.sweep_problem(nx, ny, extra, dof)
	g = run_sweep(pb, dtype, rd)
	rr = s4.rss(pb)
	ws = dict(rss=s4.judge_values(g['rss'], rr['rss'], rr['bound'], 'rss'))
	ref = s4.sweep(pb, g['rss'], rd, dtype)
	assert ref['undecided'] == 0
	ws.update(s4.judge_sweep(g, pb, ref, dtype))
	f = g['flags']
	assert (f[2:] == (0, 0, -7, -7)).all(), 'the unguarded entry writes flags[0..1] only'
	got = (int(f[0]) - 3, int(f[1]) - 5)
	ws['flags'] = s4.Worst(0.0 if got == ref['flags'] else np.inf, None, 'flags[0..1] += %r == %r' % (got, ref['flags']))
	note('nrm_single4_sweep', ws, 'nx %d ny %d m %d dof %d %s return_dot %d' % (nx, ny, pb.m, dof, np.dtype(dtype).name, rd))


def test_s4_sweep_refusals_write_nothing():
	_, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	a, out, fl = Buf((4, 8), F64, data=np.ones((4, 8))), Buf((4, 8), F64), Buf(6, I32)
	base = lambda **k: [k.get('bt', a.ptr), a.ptr, k.get('ldb', 8), a.ptr, a.ptr, k.get('nx', 4), 4, k.get('m', 6), 16, 5.0, 0, out.ptr, out.ptr, out.ptr, k.get('dt', 1), k.get('ldo', 8),
						k.get('work', out.ptr), fl.ptr]
	calls = [
		('m < nx', lambda: lib.nrm_single4_sweep(*base(m=3), st)),
		('ldb < m', lambda: lib.nrm_single4_sweep(*base(ldb=5), st)),
		('ldo < ny', lambda: lib.nrm_single4_sweep(*base(ldo=3), st)),
		('bad out_dtype', lambda: lib.nrm_single4_sweep(*base(dt=7), st)),
		('null work', lambda: lib.nrm_single4_sweep(*base(work=0), st)),
		('guarded: 4 slices', lambda: lib.nrm_single4_sweep_guarded(*base(), a.ptr, a.ptr, 1e-6, 1e-6, 4, 0.1, 0, st)),
		('guarded: budget 0', lambda: lib.nrm_single4_sweep_guarded(*base(), a.ptr, a.ptr, 1e-6, 1e-6, 5, 0.0, 0, st)),
		('guarded: no records', lambda: lib.nrm_single4_sweep_guarded(*base(), 0, a.ptr, 1e-6, 1e-6, 5, 0.1, 0, st)),
		('fix_dot: 7 slices', lambda: lib.nrm_gram_i8_fix_dot(out.ptr, 8, a.ptr, a.ptr, 4, 8, 7, 16, st)),
		('fix_dot: ldd < cols', lambda: lib.nrm_gram_i8_fix_dot(out.ptr, 7, a.ptr, a.ptr, 4, 8, 5, 16, st)),
	]
	for what, call in calls:
		rc = call()
		_sync()
		print('%-24s -> %d  %s' % (what, rc, lib.nrm_last_error().decode()))
		assert rc != 0, what
		assert out.clean() and fl.clean(), what


# ---- the guard ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_hits', [True, False], ids=['hits', 'nohits'])
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('name', s4.GUARD_CASES)
def test_s4_guarded_sweep(name, dtype, with_hits):
	"""nrm_single4_sweep_guarded pair by pair: flags[2] and flags[3] inside the reference's intervals, gene_hits holds the must-set and none of the must-not set,
	a saturated flags[2] stays put, and P, stat, vary are the unguarded entry's bits."""
	pb, fy, kappa, cstar, gstar, ns, budget = s4.guard_case(name)
	plain = run_sweep(pb, dtype, 0, flags0=(0, 0, 0, 0))
	g = run_sweep(pb, dtype, 0, guard=(fy, kappa, cstar, gstar, ns, budget), flags0=(0, 0, 0, 0), with_hits=with_hits)
	for k in ('p', 'stat', 'vary', 'rss'):
		assert same(plain[k], g[k]), '%s differs from the unguarded entry' % k
	assert (g['flags'][[0, 1, 4, 5]] == (0, 0, -7, -7)).all()
	ref = s4.guard(pb, g['rss'], fy, kappa, cstar, gstar, ns, budget, dtype)
	assert ref['undecided'] == 0
	print('%s: %d over (%d counted, %d exempt), %d under; budget %.6g' % (name, ref['over'].sum(), ref['counted'].sum(), ref['exempt'].sum(), ref['under'].sum(), budget))
	# the stored P is zero exactly where the reference's class says so
	zero = np.asarray(g['p']) == 0
	assert zero[ref['exempt']].all()
	ws = s4.check_guard(g['flags'], 0, g.get('hits'), ref)
	sat = run_sweep(pb, dtype, 0, guard=(fy, kappa, cstar, gstar, ns, budget), flags0=(0, 0, 1 << 30, 0), with_hits=with_hits)
	ws['saturation'] = s4.Worst(0.0 if int(sat['flags'][2]) == 1 << 30 else np.inf, None, 'flags[2] stays at 1 << 30')
	note('nrm_single4_sweep_guarded', ws, '%s %s %s' % (name, np.dtype(dtype).name, 'gene_hits' if with_hits else 'NULL'))


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _floor(M, X, nxp):
	"""Rounding floor of one step X' = 2 X - X (M X)^T as the device takes it, then N = (X' + X'^T) / 2, in ||M dN||_F, by the running-error rule:
	T = M X on K2' (depth nxp + 7: k_pad and at most eight pieces) |dT| <= u d |M||X|; X T^T the same on |X||T| plus |X||dT|; the update and the finish one
	rounding each of |X'| (<= 2 |X| + |X||T|).  Evaluated in fp64 (1 % added)."""
	u, d = s4.U, nxp + 7
	aM, aX = np.abs(M), np.abs(X)
	aT = aM @ aX
	dT = u * d * aT
	aXT = aX @ aT.T
	dX = u * d * aXT + aX @ dT.T + 2 * u * (2 * aX + aXT)
	return 1.01 * float(np.linalg.norm(aM @ dX))


@pytest.mark.parametrize('nx,nxp,want', [(65, 128, 'diagonal'), (1000, 1024, 'norm')])
def test_s4_newton_schulz_chain(nx, nxp, want):
	"""prepare, start, k x (gram, transpose_residual, gram, update), finish driven here with the start and step count _spd_inverse_device reports: bit for bit
	single4._spd_inverse_fixed on the same M; ||I - M N||_F <= r^2 + floor, r the residual of the iterate that entered the last step, both taken on the host
	(longdouble at nx = 65; at nx = 1000 in fp64 with the evaluation's own gamma(nx) || |M||N| ||_F added to the bound -- two longdouble 1000^3 products take
	a quarter of a minute); the device's res of that iterate inside its stage bound."""
	torch, _lib, eng = _env()
	from normalisr_amd import single4
	lib, st, ws_ = eng.lib, eng._stream(), eng._gram_ws()
	m = s4.spd_matrix(nx, seed=1, weak=want == 'diagonal')  # (one matrix for each start)
	md = np.zeros((nxp, nxp))
	md[:nx, :nx] = np.triu(m)
	m_d = torch.from_numpy(md).cuda()
	ss = torch.from_numpy(np.diagonal(m).copy()).cuda()
	assert single4._spd_inverse_device(eng, m_d, nx, ss) is not None
	start, iters = eng._s4_inverse
	print('start %s, %d steps' % (start, iters))
	assert start == want
	n_fixed, scal_f, small_f, res_f = single4._spd_inverse_fixed(eng, m_d, nx, ss, start, iters)
	torch.cuda.synchronize()
	mk = lambda *shape: Buf(shape, F64)
	mp, t, tt, xt, x, nn = (mk(nxp, nxp) for _ in range(6))
	scal, work, res, small = mk(2), mk(max(2 * nxp, (nxp // 32)**2)), mk(1), mk(3, nx)
	gram = lambda a, b, out: _lib.check(lib.nrm_gram_f64_band(a.ptr, b.ptr, nxp, nxp, nxp, nxp, nxp, out.ptr, nxp, 0, nxp, nxp, 0, nxp, ws_, st))
	_lib.check(lib.nrm_spd_prepare(m_d.data_ptr(), nxp, nx, nxp, mp.ptr, scal.ptr, work.ptr, st))
	_lib.check(lib.nrm_spd_start(mp.ptr, nxp, 1 if start == 'diagonal' else 0, scal.ptr, x.ptr, st))
	x_prev = t_prev = None
	for it in range(iters):
		if it == iters - 1:
			_sync()
			x_prev = x.get()
		gram(mp, x, t)
		_lib.check(lib.nrm_spd_transpose_residual(t.ptr, nxp, tt.ptr, res.ptr, work.ptr, st))
		if it == iters - 1:
			_sync()
			t_prev = t.get()
		gram(x, tt, xt)
		_lib.check(lib.nrm_spd_update(x.ptr, xt.ptr, nxp * nxp, st))
	_lib.check(lib.nrm_spd_finish(x.ptr, nx, nxp, ss.data_ptr(), nn.ptr, small.ptr, st))
	_sync()
	N, MP = nn.get(), mp.get()
	assert same(N, n_fixed.cpu().numpy()) and same(small.get(), small_f.cpu().numpy()) and same(res.get(), res_f.cpu().numpy()) and same(scal.get(), scal_f.cpu().numpy())
	rr = s4.spd_transpose_residual(t_prev, nxp)
	wsd = dict(res=s4.worst(np.abs(s4.ld(res.get()) - rr['res']), np.asarray([rr['res_bound']]), 'res of the iterate that entered the last step'))
	M = MP[:nx, :nx]
	floor = _floor(MP, x_prev, nxp)
	if nx <= 128:
		r_prev = float(np.sqrt(((np.eye(nxp, dtype=s4.LD) - s4.ld(MP) @ s4.ld(x_prev))**2).sum()))
		r_new = float(np.sqrt(((np.eye(nx, dtype=s4.LD) - s4.ld(M) @ s4.ld(N[:nx, :nx]))**2).sum()))
		extra = 0.0
	else:
		r_prev = float(np.linalg.norm(np.eye(nxp) - MP @ x_prev))
		r_new = float(np.linalg.norm(np.eye(nx) - M @ N[:nx, :nx]))
		extra = s4.gamma(nx) * float(np.linalg.norm(np.abs(M) @ np.abs(N[:nx, :nx]))) + s4.gamma(nxp) * float(np.linalg.norm(np.abs(MP) @ np.abs(x_prev))) * 2 * r_prev
	print('||I - M X||_F entering the last step %.3g, ||I - M N||_F %.3g, floor %.3g' % (r_prev, r_new, floor))
	wsd['residual'] = s4.worst(np.asarray([r_new]), np.asarray([r_prev * r_prev + floor + extra]), '||I - M N||_F against r^2 + floor')
	note('Newton-Schulz chain', wsd, 'nx %d' % nx)


def test_s4_zz_worst_ratios_of_this_run():
	"""The table for DESIGN.md: the worst ratio of every output over the tests that ran before this one."""
	for key in sorted(WORST):
		print('%-44s %-14s %.3g   (%s)' % (key + WORST[key]))
	assert all(v[0] <= 1 for v in WORST.values())
