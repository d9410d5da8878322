"""GPU: the single=1 kernels (csrc/nrm_single1.hip, the selection in csrc/nrm_design_lists.hip) at kernel level -- nrm_single1_select, nrm_single1_common_gram,
nrm_single1_group_stats, nrm_single1_group_info, nrm_single1_stream, nrm_single1_cells and nrm_single1_sweep called directly through the C ABI, every output
against the stage reference of tests/s1_reference.py.

What is checked: placement (every output pre-filled with NaN, integers with -7, at a pitch above the minimum where the entry has one, followed by a 1024-byte
tail that must stay untouched); integers, copies and exact-data sums bit for bit; real-data sums and every pair's stat, vary and alpha within the running-error
bounds of the longdouble values (no pair skipped); P of a subset (the planted pairs and a spread of ln P) against mpmath at 60 digits with G12's tolerance; the
counters flags[0..4] by count; the P-value plan of every record bit for bit against nrm_pvalue_plan_fill_many; the masked-Gram sweep bit for bit against
k_s1_cells on the same sums; the five entries in Single1Plan's order bit for bit against Single1Plan.step(); every call made twice with identical bits; the
refusals.  tests/test_s1_reference_cpu.py shows that the comparators accept an fp64 emulation of every kernel at every shape used here and reject mutations of
it, and that these cases launch every instantiation.

Every test prints its worst error-to-bound ratio per output before it asserts (pytest -rP shows them); the last test prints the table of the run.
Measured on an MI355X: see DESIGN.md section 6, "single=1 at kernel level"."""
import ctypes
import functools

import numpy as np
import pytest

import s1_reference as s1
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


def _code(dtype):
	_lib = _env()[1]
	return _lib.NRM_F64 if np.dtype(dtype) == F64 else _lib.NRM_F32


def plans(dof):
	"""nrm_pvalue_plan_fill_many (the host's compilation of csrc/nrm_pvalue_plan.h) for every dof: (len, 24)."""
	_, _lib, eng = _env()
	d = np.ascontiguousarray(dof, dtype=F64)
	out = np.zeros((len(d), s1.HEAD - 2))
	_lib.check(eng.lib.nrm_pvalue_plan_fill_many(d.ctypes.data_as(ctypes.c_void_p), len(d), out.ctypes.data_as(ctypes.c_void_p), s1.HEAD - 2))
	return out


# ---- select ----------------------------------------------------------------------------------------------------------------------------------------------------
def run_select(row_ptr, cells, vals, n, C, gram_inside=True):
	_, _lib, eng = _env()
	nx, nnz = len(row_ptr) - 1, len(cells)
	nc = 0 if C is None else C.shape[0]
	nb = (nc + 7) // 8
	gb = int(eng.lib.nrm_single1_select_gram_blocks())
	assert gb == s1.GB
	ldc = n + 3

	def run():
		d_rp, d_cells = Buf(nx + 1, I64, data=row_ptr), Buf(max(nnz, 1), I32, data=cells if nnz else [0])
		d_vals = Buf(max(nnz, 1), F64, data=vals if nnz else [0.0]) if vals is not None else None
		d_c = Buf((nc, n), F64, pitch=ldc, data=C) if nc else None
		o = dict(cnt=Buf(n, I32), code=Buf(n, I32), seg=Buf(nx + 1, I64), idx=Buf(max(nnz, 1), I64), xe=Buf(max(nnz, 1), F64), ce=Buf((max(nnz, 1), max(nc, 1)), F64),
				 rowinfo=Buf((nx, 3), F64), gpart=Buf((max(nb * (nb + 1) // 2, 1), gb, 64), F64), info=Buf(8, I64))
		p = lambda b: 0 if b is None else b.ptr
		_lib.check(eng.lib.nrm_single1_select(d_rp.ptr, d_cells.ptr, p(d_vals), nx, n, nnz, p(d_c), ldc, nc, o['cnt'].ptr, o['code'].ptr, o['seg'].ptr, o['idx'].ptr, o['xe'].ptr,
											  o['ce'].ptr if nc else 0, o['rowinfo'].ptr, o['gpart'].ptr if (nc and gram_inside) else 0, o['info'].ptr, eng._stream()))
		_sync()
		if nc and not gram_inside:
			assert o['gpart'].clean()
			_lib.check(eng.lib.nrm_single1_common_gram(o['cnt'].ptr, n, d_c.ptr, ldc, nc, o['gpart'].ptr, eng._stream()))
			_sync()
		info = o['info'].get()
		assert (info[[0, 1, 2, 5, 6, 7]] == -7).all(), 'sel_info: only [3] and [4] are the selection\'s'
		nk = int(info[4])
		res = dict(cnt=o['cnt'].get(), code=o['code'].get(), seg=o['seg'].get(), rowinfo=o['rowinfo'].get(), n_common=int(info[3]), n_kept=nk)
		idx, xe, ce = o['idx'].get(), o['xe'].get(), o['ce'].get()
		assert 0 <= nk <= nnz and (idx[nk:] == -7).all() and np.isnan(xe[nk:]).all() and np.isnan(ce[nk:]).all(), 'idx, xe, ce past sel_info[4]'
		if not nc:
			assert o['ce'].clean() and o['gpart'].clean()
		res.update(idx=idx[:nk], xe=xe[:nk], ce=ce[:nk, :nc], gram=s1.gram_from_parts(o['gpart'].get(), nc) if nc else None, gpart=o['gpart'].get() if nc else None)
		return res
	return twice(run)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('case', s1.SELECT, ids=lambda c: 'n%d-nx%d-nc%d-%s' % (c[0], c[1], c[2], 'valued' if c[3] else 'ones'))
def test_s1_select(case, exact):
	"""k_s1_cellcount, k_s1_rows<false / true>, k_s1_scan (per = 2 at nx = 1030), k_s1_codes, k_s1_common_gram (1, 3 and 10 block pairs; inside the entry and by
	nrm_single1_common_gram): integers, xe, ce, rowinfo bit for bit; the Gram matrix bit for bit on exact data, inside its bound on real data."""
	n, nx, nc, valued = case
	row_ptr, cells, vals = s1.design(n, nx, 0, valued, exact)
	C = s1.covariates(nc, n, 0, exact) if nc else None
	ref = s1.select(row_ptr, cells, vals, n, C)
	got = run_select(row_ptr, cells, vals, n, C)
	note('nrm_single1_select', s1.judge_select(got, ref, exact), str(case))
	if nc:
		alone = run_select(row_ptr, cells, vals, n, C, gram_inside=False)
		note('nrm_single1_common_gram', dict(gram=s1.judge_select(alone, ref, exact)['gram']), str(case))
		assert same(alone['gpart'], got['gpart']), 'the Gram blocks inside the entry and by nrm_single1_common_gram differ'


# ---- group_stats -----------------------------------------------------------------------------------------------------------------------------------------------
def run_group_stats(seg, cells, xe, C, nc, n):
	_, _lib, eng = _env()
	nx = len(seg) - 1
	npk = nc * (nc + 1) // 2 + nc + 1

	def run():
		d_seg, d_cells, d_xe = Buf(nx + 1, I64, data=seg), Buf(len(cells), I64, data=cells), Buf(len(xe), F64, data=xe)
		d_c = Buf((nc, n), F64, pitch=n + 3, data=C) if nc else None
		out = Buf((nx, npk), F64)
		_lib.check(eng.lib.nrm_single1_group_stats(d_seg.ptr, d_cells.ptr, d_xe.ptr, d_c.ptr if nc else 0, n + 3, nc, nx, out.ptr, eng._stream()))
		_sync()
		return dict(gs=out.get())
	return twice(run)['gs']


@pytest.mark.parametrize('nc', s1.GS_NC)
def test_s1_group_stats(nc):
	"""k_s1_group_stats: segments of 0, 1, 63, 64, 65, 130 cells; the output packed for nc covariates (the tail behind nx rows of that width stays untouched)."""
	for exact in (True, False):
		pb = s1.gs_problem(nc, 0, exact)
		ref, bound = s1.group_stats(pb['seg'], pb['cells'], pb['xe'], pb['C'], nc)
		got = run_group_stats(pb['seg'], pb['cells'], pb['xe'], pb['C'], nc, pb['n'])
		w = s1.bits(got, np.asarray(ref, F64), 'gs (exact)') if exact else s1.worst(np.abs(s1.ld(got) - ref), bound, 'gs')
		note('nrm_single1_group_stats', dict(gs=w), 'nc%d %s' % (nc, 'exact' if exact else 'real'))


# ---- group_info ------------------------------------------------------------------------------------------------------------------------------------------------
def run_group_info(pb, extra_pitch=5, prefill=(0, 0, 0, 0, 0, -7, -7, -7)):
	_, _lib, eng = _env()
	nx, nc = pb['nx'], pb['nc']
	pitch = s1.HEAD + nc + nc * nc + extra_pitch

	def run():
		d_gs, d_rows = Buf(pb['gs'].shape, F64, data=pb['gs']), Buf((nx, 3), F64, data=pb['rowinfo'])
		d_gp = Buf((s1.GB, 64), F64, data=pb['gpart']) if nc else None
		sel = np.full(8, -7, I64)
		sel[3] = pb['n_common']
		d_sel = Buf(8, I64, data=sel)
		info, varx, flags = Buf((nx, s1.HEAD + nc + nc * nc), F64, pitch=pitch), Buf(nx, F64), Buf(8, I32, data=prefill)
		_lib.check(eng.lib.nrm_single1_group_info(d_gs.ptr, d_gp.ptr if nc else 0, d_rows.ptr, d_sel.ptr, nc, nx, pb['dimreduce'], info.ptr, pitch, varx.ptr, flags.ptr,
												  eng._stream()))
		_sync()
		return dict(info=info.get(), varx=varx.get(), flags=flags.get())
	return twice(run)


@pytest.mark.parametrize('nc', s1.GI_NC)
@pytest.mark.parametrize('nx', s1.GI_NX)
def test_s1_group_info(nx, nc):
	"""k_s1_group_info<nc>: a duplicated covariate (rank nc - 1 through dof), a covariate that is 0, nearly dependent covariates, vx = 0 -> 1, dof <= 0, a
	non-finite Gram entry (the identity instead), a single value with and without shared cells, no shared cells; the plan of every record bit for bit."""
	for variant in s1.GI_VARIANTS:
		pb = s1.gi_problem(nx, nc, variant)
		ref = s1.group_info(pb['gs'], pb['gpart'], pb['rowinfo'], pb['n_common'], nc, pb['dimreduce'])
		got = run_group_info(pb)
		ws = s1.judge_group_info(got['info'], got['varx'], got['flags'], ref, nc)
		want = plans(ref['dof'])
		ws['plan (dof)'] = s1.bits(got['info'][:, 2:s1.HEAD].copy(), want, 'rec[2..25] == nrm_pvalue_plan_fill_many(dof)')
		assert (got['flags'][[0, 1]] == 0).all() and (got['flags'][5:] == -7).all(), got['flags']
		note(s1.group_info_instantiation(nc), ws, 'nx%d %s' % (nx, variant))


# ---- stream ----------------------------------------------------------------------------------------------------------------------------------------------------
def run_stream(pb, ldye, mis=None, C=None, nc=None):
	_, _lib, eng = _env()
	n, ny = pb['n'], pb['ny']
	nc = pb['nc'] if nc is None else nc
	C = pb['C'] if C is None else C
	dtype = pb['Y'].dtype
	V = 16 // dtype.itemsize
	ldy = (n | 1) if mis == 'ldy' else (n + V - 1) // V * V
	ldc = (n | 1) if mis == 'ldc' else (n + 1) // 2 * 2 + 2
	nk = pb['n_kept']

	def run():
		d_y = Buf((ny, n), dtype, pitch=ldy, data=pb['Y'], skip=1 if mis == 'y' else 0)
		d_c = Buf((nc, n), F64, pitch=ldc, data=C) if nc else None
		d_code = Buf(n, I32, data=pb['code'], skip=1 if mis == 'code' else 0)
		aligned = s1.stream_aligned(d_y.ptr, ldy, dtype.itemsize, d_code.ptr, d_c.ptr if nc else 0, ldc, nc)
		assert aligned == (mis is None), 'the case does not reach the instantiation it is for'
		common, ye = Buf((nc + 1, ny), F64), Buf((nk + 2, ldye), dtype)
		assert ye.ptr % 64 == 0
		_lib.check(eng.lib.nrm_single1_stream(d_y.ptr, _code(dtype), ldy, d_c.ptr if nc else 0, ldc, nc, d_code.ptr, n, ny, common.ptr, ye.ptr, ldye, eng._stream()))
		_sync()
		y = ye.get()
		assert np.isnan(y[nk:]).all(), 'YE: rows without a cell written'
		return dict(common=common.get(), ye=y[:nk])
	return twice(run)


@pytest.mark.parametrize('case', s1.stream_cases(), ids=lambda c: 'n%d-ny%d-nc%d-%s-%s-ldye%d' % (c[0], c[1], c[2], c[3].__name__, c[4], c[5]))
def test_s1_stream(case):
	"""k_s1_stream<T, NC, R, ALIGNED, FIRST>: YE bit for bit at the kept cells, NaN in the rows without a cell, NaN or row ny - 1 in the padding columns; common
	written at (nc + 1) x ny only, bit for bit on exact data and inside its bound on real data; a reach-back pass stores what a single pass gives."""
	n, ny, nc, dtype, mis, ldye = case
	for exact in (True, False):
		pb = s1.stream_problem(n, ny, nc, dtype, 0, exact)
		ref = s1.stream(pb['Y'], pb['C'], pb['code'], nc, pb['n_kept'], ldye)
		got = run_stream(pb, ldye, mis)
		for k in s1.stream_instantiations(nc, dtype, mis is None):
			note(k, s1.judge_stream(got['common'], got['ye'], ref, ny, exact), '%s %s' % (case[:3] + case[4:], 'exact' if exact else 'real'))
		if nc > 8 and nc % 8:  # the covariates of the last pass alone, as a first pass: the same sums, bit for bit
			alone = run_stream(pb, ldye, mis, C=pb['C'][nc - 8:], nc=8)
			assert same(alone['common'][:8], got['common'][nc - 8:nc]), 'the reach-back pass stores other sums than a single pass'
			assert same(alone['common'][8], got['common'][nc]) and same(alone['ye'], got['ye'])


# ---- cells and the masked-Gram sweep -----------------------------------------------------------------------------------------------------------------------------
def _info(pb, extra=3):
	nc = pb['nc']
	info = pb['info'].copy()
	info[:, 2:s1.HEAD] = plans(pb['dof'])
	return info, s1.HEAD + nc + nc * nc + extra


def _outs(nx, ny, nc, odt, alpha):
	ldo = ny + 5
	o = {k: Buf((nx, ny), odt, pitch=ldo) for k in ('p', 'stat', 'vary')}
	o['alpha'] = Buf((nx, ny * max(nc, 1)), odt, pitch=ldo * max(nc, 1)) if alpha else None  # alpha[(i ldo + y) nc + c]
	return o, ldo


def _take(o, fl, nx, ny, nc):
	res = {k: o[k].get() for k in ('p', 'stat', 'vary')}
	res['alpha'] = o['alpha'].get().reshape(nx, ny, max(nc, 1))[:, :, :nc] if o['alpha'] is not None and nc else None
	if o['alpha'] is not None and not nc:
		assert o['alpha'].clean()
	res['flags'] = fl.get()
	return res


def run_cells(pb, rd, alpha, odt, common=None, seg=None, with_flags=True):
	_, _lib, eng = _env()
	nx, ny, nc = pb['nx'], pb['ny'], pb['nc']
	info, pitch = _info(pb)
	ydt = pb['ye'].dtype
	sel = pb['sel']
	nk = max(sel['n_kept'], 1)

	def run():
		d_ye = Buf((nk, pb['ldye']), ydt, data=pb['ye'] if sel['n_kept'] else np.zeros((1, pb['ldye'])))
		d_ce = Buf((nk, max(nc, 1)), F64, data=sel['ce'] if (nc and sel['n_kept']) else None)
		d_xe = Buf(nk, F64, data=sel['xe'] if sel['n_kept'] else [0.0])
		d_seg = Buf(nx + 1, I64, data=sel['seg'] if seg is None else seg)
		d_common = Buf((nc + 1, ny), F64, data=pb['common'] if common is None else common)
		d_info = Buf((nx, info.shape[1]), F64, pitch=pitch, data=info)
		o, ldo = _outs(nx, ny, nc, odt, alpha)
		fl = Buf(8, I32, data=(0, 0, -7, -7, -7, -7, -7, -7))
		_lib.check(eng.lib.nrm_single1_cells(d_ye.ptr, _code(ydt), pb['ldye'], d_ce.ptr if nc else 0, d_xe.ptr, d_seg.ptr, d_common.ptr, d_info.ptr, pitch, nc, nx, ny, rd,
											 o['p'].ptr, o['stat'].ptr, o['vary'].ptr, o['alpha'].ptr if alpha else 0, _code(odt), ldo, fl.ptr if with_flags else 0, eng._stream()))
		_sync()
		return _take(o, fl, nx, ny, nc)
	return twice(run)


def run_sweep(G, G2, pb, rd, alpha, odt):
	_, _lib, eng = _env()
	nx, ny, nc = pb['nx'], pb['ny'], pb['nc']
	info, pitch = _info(pb)

	def run():
		d_g, d_g2 = Buf(G.shape, F64, data=G), Buf(G2.shape, F64, data=G2)  # (their own pitch padding holds NaN already)
		d_info = Buf((nx, info.shape[1]), F64, pitch=pitch, data=info)
		o, ldo = _outs(nx, ny, nc, odt, alpha)
		fl = Buf(8, I32, data=(0, 0, -7, -7, -7, -7, -7, -7))
		_lib.check(eng.lib.nrm_single1_sweep(d_g.ptr, G.shape[1], d_g2.ptr, G2.shape[1], d_info.ptr, pitch, nc, nx, ny, rd, o['p'].ptr, o['stat'].ptr, o['vary'].ptr,
											 o['alpha'].ptr if alpha else 0, _code(odt), ldo, fl.ptr, eng._stream()))
		_sync()
		return _take(o, fl, nx, ny, nc)
	return twice(run)


def judge_all(got, ref, pb, odt, limit):
	ws = s1.judge_pairs(got, ref, odt, got['flags'])
	assert (got['flags'][2:] == -7).all(), got['flags']
	picks = s1.p_subset(ref, pb['dof'], pb['plants'].values(), limit=limit)
	assert set(pb['plants'].values()) <= set(picks)
	ws['p mpmath'] = s1.judge_p(got['p'], ref, pb['dof'], picks, odt)
	r2 = np.asarray(ref['r2'], F64)
	over = ref['finite'] & (r2 > 1.0 + 1e-8)
	assert (got['p'][over] == 0).all(), 'R^2 > 1: the P-value nrm_pvalue returns is 0'
	assert np.isnan(got['p'][~ref['finite'] & np.isnan(r2)]).all()
	return ws


@pytest.mark.parametrize('case', s1.cells_cases(), ids=lambda c: 'ny%d-nc%d-%s-%s-dot%d-alpha%d' % (c[0], c[1], c[2].__name__, c[3].__name__, c[4], c[5]))
def test_s1_cells(case):
	"""k_s1_cells<T, NCT>: segments of 0, 1, 7, 8, 9, 17 cells, planted pairs (R^2 near 0, 1/4 from both sides, near 1), a zero gene (flags[0] counts exactly its
	pairs), alpha absent and present at ldo = ny + 5, both statistics.  Every pair's stat, vary, alpha; P on the subset (200 pairs at ny 257, nc 5, fp64 out)."""
	ny, nc, ydt, odt, rd, alpha = case
	pb = s1.cells_problem(ny, nc, ydt)
	ref = s1.cells_reference(pb, rd)
	got = run_cells(pb, rd, alpha, odt)
	big = ny == 257 and nc == 5 and odt == F64
	ws = judge_all(got, ref, pb, odt, 220 if big else 12)
	note(s1.cells_instantiation(nc, ydt), ws, str(case[:2] + case[3:]))
	if ny > 1:
		assert got['flags'][0] == pb['nx'] and got['flags'][1] == 0
	assert same(run_cells(pb, rd, alpha, odt, with_flags=False)['p'], got['p'])  # (flags = NULL: the same results)


def test_s1_cells_r2_above_one():
	"""common[qrow] handed in too small: flags[1] counts exactly the pairs with R^2 > 1 + 1e-8 and their P-value is nrm_pvalue's 0."""
	ny, nc = s1.CANCEL_SHAPE
	pb = s1.cells_problem(ny, nc, F64, zero_gene=False)
	ref0 = s1.cells_reference(pb, 0)
	common = pb['common'].copy()
	common[nc, :4] -= s1.q_cut(ref0, pb['nx'] - 1)[:4]
	ref = s1.cells_reference(pb, 0, common)
	assert ref['flag1'] >= 4 and ref['flag0'] == 0
	got = run_cells(pb, 0, True, F64, common=common)
	ws = judge_all(got, ref, pb, F64, 12)
	print('flags', got['flags'][:2], 'want', ref['flag0'], ref['flag1'])
	note(s1.cells_instantiation(nc, F64), ws, 'R2 above one')


def test_s1_cells_cancellation():
	"""An intercept among the covariates and genes with mean / sd = 1, 30, 1000: the closed form |y~|^2 = q - a.M+a cancels 1 + (mean / sd)^2 of q.  fp64 input:
	stat and vary stay inside bounds that carry that cancellation; the table gives the digits lost against the reference's residual-first form
	(association.py:357-360).  fp32 input at mean / sd = 30 stays far inside the project's parity bar (1e-6 relative, BASELINE.json)."""
	rows = []
	ny, nc = s1.CANCEL_SHAPE
	for ydt in s1.CANCEL_DTYPES:
		pb = s1.cells_problem(ny, nc, ydt, mean_over_sd=s1.CANCEL, zero_gene=False)
		ref = s1.cells_reference(pb, 0)
		rf = np.asarray(s1.residual_first(pb) / s1.ld(pb['info'][:, 0])[:, None], F64)
		got = run_cells(pb, 0, True, ydt)
		note(s1.cells_instantiation(nc, ydt) + ' cancellation', judge_all(got, ref, pb, ydt, 12), ydt.__name__)
		for k, r in enumerate(s1.CANCEL):
			cols = np.arange(k, ny, len(s1.CANCEL))
			rel = np.abs(got['vary'][:, cols].astype(F64) - rf[:, cols]) / rf[:, cols]
			want = np.asarray(ref['stat'], F64)[:, cols]
			rel_s = np.abs(got['stat'][:, cols].astype(F64) - want) / np.where(want == 0, 1.0, np.abs(want))  # (a grouping without cells of its own: 0 = 0)
			u = 2.0**-53 if ydt == F64 else 2.0**-24
			rows.append((ydt.__name__, r, float(np.log10(ref['q_over_yy'][:, cols]).max()), float(rel.max()), float(np.log10(max(rel.max(), u) / u)), float(rel_s.max())))
			if ydt == F32 and r <= 30:
				assert rel.max() < 1e-6 and rel_s.max() < 1e-6  # the parity bar; (what is left of it is the fp32 output's own 6e-8)
	print('in/out   mean/sd  log10(q/yy)  vary rel. error  digits lost (of the output type)  stat rel. error')
	for row in rows:
		print('%-8s %-8g %-12.2f %-16.3g %-33.2f %.3g' % row)
		WORST[('cancellation %s mean/sd %g' % row[:2], 'digits lost')] = (row[4], 'log10(q/yy) %.2f, vary rel. error %.3g' % row[2:4])


@pytest.mark.parametrize('nc', s1.SWEEP_NC)
def test_s1_sweep_masked_gram(nc):
	"""k_s1_sweep<OutT>: on sums both kernels receive identically (empty segments, a and q as `common`, xy = 0) bit for bit k_s1_cells; on a screen's own sums
	(the cells' a, xy, q in longdouble, rounded) inside the bounds with no input error."""
	ny = s1.SWEEP_NY
	for ydt, odt, rd in s1.SWEEP_VARIANTS:
		pb = s1.cells_problem(ny, nc, ydt)
		a, _, xy, _, q, _ = s1.cell_sums(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], pb['common'], nc, ny)
		a64, xy64, q64 = np.asarray(a, F64), np.asarray(xy, F64), np.asarray(q, F64)
		z = np.zeros_like(xy64)
		ref = s1.pairs(s1.ld(a64), np.zeros(a64.shape), s1.ld(xy64), z, s1.ld(q64), z, pb['info'], nc, rd)
		G, G2 = s1.sweep_inputs(a64, xy64, q64, nc)
		got = run_sweep(G, G2, pb, rd, True, odt)
		note('k_s1_sweep<%s>' % ('double' if odt == F64 else 'float'), judge_all(got, ref, pb, odt, 12), 'nc%d' % nc)
		# the same sums to both kernels: grouping-independent a and q, no own cells
		common = pb['common']
		nx = pb['nx']
		G, G2 = s1.sweep_inputs(np.broadcast_to(common[:nc].T, (nx, ny, nc)), np.zeros((nx, ny)), np.broadcast_to(common[nc], (nx, ny)), nc)
		sw = run_sweep(G, G2, pb, rd, True, odt)
		ce = run_cells(pb, rd, True, odt, seg=np.zeros(nx + 1, I64))
		for k in ('p', 'stat', 'vary') + (('alpha', ) if nc else ()):
			assert same(sw[k], ce[k]), 'k_s1_sweep and k_s1_cells differ in %s on the same sums' % k
		assert (sw['flags'] == ce['flags']).all()


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------------------
def test_s1_chain_equals_the_plan():
	"""The five entries in Single1Plan's order on one small screen (65 groupings, 69 genes, 2051 cells, 5 covariates, fp32), each from the previous one's outputs
	as they lie in HBM: every intermediate passes its stage's comparator and equals the plan's own buffer bit for bit, and so do the final outputs."""
	torch, _lib, eng = _env()
	from normalisr_amd import single1
	cp = s1.chain_problem()
	nx, ny, n, nc, row_ptr, cells, C, Y = (cp[k] for k in ('nx', 'ny', 'n', 'nc', 'row_ptr', 'cells', 'C', 'Y'))
	assert cp['ldye'] == (ny + 7) // 8 * 8 and cp['return_dot'] == 1 and cp['out_dtype'] == F32
	dx = torch.from_numpy(s1.dense(row_ptr, cells, None, n)).cuda()
	plan = single1.Single1Plan(dx, torch.from_numpy(Y).cuda(), C, lowmem=False, return_dot=True, eng=eng)
	plan.step()
	_sync()
	host = lambda t: t.cpu().numpy()
	# select
	sel_ref = s1.select(row_ptr, cells, None, n, C)
	sel = run_select(row_ptr, cells, None, n, C, gram_inside=False)
	note('chain: select', s1.judge_select(sel, sel_ref, False), 'chain')
	nk = sel['n_kept']
	assert nk == plan.n_kept and same(sel['seg'], host(plan.seg)) and same(sel['code'], host(plan.code)) and same(sel['idx'], host(plan.idx)[:nk])
	assert same(sel['gpart'][0], host(plan.gpart)[0])
	assert same(sel['cnt'], host(plan.cnt)) and same(sel['rowinfo'], host(plan.rowinfo)) and same(sel['xe'], host(plan.xe)[:nk]) and same(sel['ce'], host(plan.ce)[:nk])
	# group_stats, group_info
	gs = run_group_stats(sel['seg'], sel['idx'], sel['xe'], C, nc, n)
	gs_ref, gs_bound = s1.group_stats(sel['seg'], sel['idx'], sel['xe'], C, nc)
	note('chain: group_stats', dict(gs=s1.worst(np.abs(s1.ld(gs) - gs_ref), gs_bound, 'gs')), 'chain')
	assert same(gs, host(plan.gs))
	gpb = dict(gs=gs, gpart=sel['gpart'][0], rowinfo=sel['rowinfo'], n_common=sel['n_common'], nc=nc, nx=nx, dimreduce=0)
	gi = run_group_info(gpb, extra_pitch=0)
	gi_ref = s1.group_info(gs, sel['gpart'][0], sel['rowinfo'], sel['n_common'], nc, 0)
	note('chain: group_info', s1.judge_group_info(gi['info'], gi['varx'], gi['flags'], gi_ref, nc), 'chain')
	assert same(gi['info'], host(plan.info)) and same(gi['varx'], host(plan.varx))
	# stream
	spb = dict(Y=Y, C=C, code=sel['code'], n_kept=nk, n=n, ny=ny, nc=nc)
	st = run_stream(spb, plan.ldye)
	note('chain: stream', s1.judge_stream(st['common'], st['ye'], s1.stream(Y, C, sel['code'], nc, nk, plan.ldye), ny, False), 'chain')
	assert same(st['common'], host(plan.common))
	assert same(st['ye'][:, :ny], host(plan.ye)[:nk, :ny])
	# cells
	pb = dict(nx=nx, ny=ny, nc=nc, sel=sel, ye=np.where(np.isnan(st['ye']), 0, st['ye']), ldye=plan.ldye, common=st['common'], info=gi['info'], dof=gi_ref['dof'], plants={})
	out = run_cells(pb, 1, True, F32)
	ref = s1.cells_reference(pb, 1)
	note('chain: cells', judge_all(out, ref, pb, F32, 24), 'chain')
	assert same(out['p'], host(plan.p)) and same(out['stat'], host(plan.stat)) and same(out['vary'], host(plan.vary)) and same(out['alpha'], host(plan.alpha))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
def test_s1_refusals_write_nothing():
	"""Each NRM_REQUIRE of the seven entries: an error code, and nothing written."""
	_, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	nx, ny, n, nc = 3, 5, 16, 2
	i64 = lambda k: Buf(k, I64, data=np.zeros(k, I64))
	rp, cl, vals, c = i64(nx + 1), Buf(4, I32, data=np.zeros(4, I32)), Buf(4, F64, data=np.ones(4)), Buf((nc, n), F64, data=np.ones((nc, n)))
	y, code = Buf((ny, n), F32, data=np.ones((ny, n))), Buf(n, I32, data=np.full(n, -2))
	outs = dict(cnt=Buf(n, I32), code=Buf(n, I32), seg=Buf(nx + 1, I64), idx=Buf(4, I64), xe=Buf(4, F64), ce=Buf(4 * nc, F64), rows=Buf(nx * 3, F64), gp=Buf(64 * 64, F64),
				info=Buf(8, I64), gs=Buf(nx * 6, F64), rec=Buf(nx * 40, F64), varx=Buf(nx, F64), flags=Buf(8, I32), common=Buf((nc + 1) * ny, F64), ye=Buf(4 * 8, F32),
				p=Buf(nx * ny, F64), stat=Buf(nx * ny, F64), vary=Buf(nx * ny, F64), alpha=Buf(nx * ny * nc, F64))
	o = {k: b.ptr for k, b in outs.items()}
	big = 40

	def select(nc_=nc, n_=n, ldc=n, cnt=o['cnt'], cp=c.ptr, rowp=rp.ptr):
		return lib.nrm_single1_select(rowp, cl.ptr, vals.ptr, nx, n_, 0, cp, ldc, nc_, cnt, o['code'], o['seg'], o['idx'], o['xe'], o['ce'], o['rows'], o['gp'], o['info'], st)

	def gram(nc_=nc, ldc=n, gp=o['gp']):
		return lib.nrm_single1_common_gram(code.ptr, n, c.ptr, ldc, nc_, gp, st)

	def gstats(nc_=nc, out=o['gs'], seg=rp.ptr):
		return lib.nrm_single1_group_stats(seg, rp.ptr, vals.ptr, c.ptr, n, nc_, nx, out, st)

	def ginfo(nc_=nc, pitch=big, gp=c.ptr, flags=o['flags']):
		return lib.nrm_single1_group_info(vals.ptr, gp, vals.ptr, rp.ptr, nc_, nx, 0, o['rec'], pitch, o['varx'], flags, st)

	def stream(nc_=nc, ldy=n, ldye=8, ye=o['ye'], dt=_lib.NRM_F32, ldc=n, common=o['common']):
		return lib.nrm_single1_stream(y.ptr, dt, ldy, c.ptr, ldc, nc_, code.ptr, n, ny, common, ye, ldye, st)

	def cells(nc_=nc, pitch=big, ldo=ny, ldye=8, p=o['p'], odt=_lib.NRM_F64):
		return lib.nrm_single1_cells(y.ptr, _lib.NRM_F32, ldye, c.ptr, vals.ptr, rp.ptr, c.ptr, c.ptr, pitch, nc_, nx, ny, 0, p, o['stat'], o['vary'], o['alpha'], odt, ldo, o['flags'], st)

	def sweep(nc_=nc, pitch=big, ldo=ny, ldg=nx * (nc + 1), ldg2=nx, p=o['p'], odt=_lib.NRM_F64):
		return lib.nrm_single1_sweep(c.ptr, ldg, c.ptr, ldg2, c.ptr, pitch, nc_, nx, ny, 0, p, o['stat'], o['vary'], o['alpha'], odt, ldo, o['flags'], st)

	for what, call in (('select: nc > 32', lambda: select(nc_=33)), ('select: ldc < n', lambda: select(ldc=n - 1)), ('select: null cnt', lambda: select(cnt=0)),
					   ('select: covariates missing', lambda: select(cp=0)), ('select: null row_ptr', lambda: select(rowp=0)), ('select: n = 0', lambda: select(n_=0)),
					   ('common_gram: nc = 0', lambda: gram(nc_=0)), ('common_gram: nc > 32', lambda: gram(nc_=33)), ('common_gram: ldc < n', lambda: gram(ldc=n - 1)),
					   ('common_gram: null out', lambda: gram(gp=0)),
					   ('group_stats: nc > 8', lambda: gstats(nc_=9)), ('group_stats: null out', lambda: gstats(out=0)), ('group_stats: null seg', lambda: gstats(seg=0)),
					   ('group_info: nc > 8', lambda: ginfo(nc_=9, pitch=200)), ('group_info: pitch too small', lambda: ginfo(pitch=s1.HEAD + nc + nc * nc - 1)),
					   ('group_info: null gram_part', lambda: ginfo(gp=0)), ('group_info: null flags', lambda: ginfo(flags=0)),
					   ('stream: nc > 32', lambda: stream(nc_=33)), ('stream: ldy < n', lambda: stream(ldy=n - 1)), ('stream: ldye % 8', lambda: stream(ldye=12)),
					   ('stream: ldye < ny', lambda: stream(ldye=0)), ('stream: d_ye not 64-byte aligned', lambda: stream(ye=o['ye'] + 32)), ('stream: bad dtype', lambda: stream(dt=7)),
					   ('stream: ldc < n', lambda: stream(ldc=n - 1)), ('stream: null common', lambda: stream(common=0)), ('stream: null ye', lambda: stream(ye=0)),
					   ('cells: nc > 32', lambda: cells(nc_=33, pitch=2000)), ('cells: info pitch too small', lambda: cells(pitch=s1.HEAD + nc + nc * nc - 1)),
					   ('cells: ldo < ny', lambda: cells(ldo=ny - 1)), ('cells: ldye < ny', lambda: cells(ldye=ny - 1)), ('cells: null p', lambda: cells(p=0)),
					   ('cells: bad out dtype', lambda: cells(odt=7)),
					   ('sweep: info pitch too small', lambda: sweep(pitch=s1.HEAD + nc + nc * nc - 1)), ('sweep: ldo < ny', lambda: sweep(ldo=ny - 1)),
					   ('sweep: ldg too small', lambda: sweep(ldg=nx * (nc + 1) - 1)), ('sweep: ldg2 < nx', lambda: sweep(ldg2=nx - 1)), ('sweep: null p', lambda: sweep(p=0)),
					   ('sweep: bad out dtype', lambda: sweep(odt=7)), ('sweep: nc < 0', lambda: sweep(nc_=-1))):
		rc = call()
		_sync()
		print('%-36s -> %d  %s' % (what, rc, lib.nrm_last_error().decode()))
		assert rc != 0, what
		dirty = [k for k, b in outs.items() if not b.clean()]
		assert not dirty, (what, dirty)


def test_s1_zz_worst_ratios_of_this_run():
	"""The table the next rewrite of these kernels holds itself to: the worst error-to-bound ratio per kernel and output over the tests of this file that ran
	before this one in the same process (the cancellation rows: digits lost, not a ratio).  It only reports: every ratio is asserted where it is measured."""
	for key in sorted(WORST):
		print('%-44s %-14s %.3g   (%s)' % (key + WORST[key]))
	assert all(v[0] <= 1 for k, v in WORST.items() if k[1] != 'digits lost')
