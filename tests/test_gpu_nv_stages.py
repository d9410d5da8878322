"""GPU: normvar's kernels (csrc/nrm_normvar.hip) at kernel level -- nrm_normvar_weights, nrm_normvar_solve, nrm_normvar_rescale, nrm_normvar_apply and
nrm_normvar_apply_w2 called directly through the C ABI at every case of tests/nv_reference.py, every output against the longdouble reference of the same entry.

What is checked: placement (every output a Buf pre-filled with NaN, integers with -7, followed by a tail that must stay untouched: out only at rows x n at the requested
pitch, d_mom at rows x NM, d_b at rows x nc, d_scale and d_rank at rows; for weights the zero padding IS the contract: columns n .. ldo and rows rows .. rows_pad are
0.0, s1 and s2 of padded rows 0, nothing beyond rows_pad); the inputs unchanged; the exact twins bit for bit; real data inside the termwise bounds; integer ranks; the
scale exactly 1 for keepvar == 0 and wt == 0; rows with wt == 0 independent of ln w; the mark of csrc/nrm_nv_scale.h where it is decided and the marked genes' scale from
the row; flags[0] and flags[1] as counts derived from the thread map, added to; every call twice with identical bits; the entries in norm.py's order against
norm.normvar and a NormvarPlan step bit for bit; one refusal per clause of every NRM_REQUIRE; the ladder of cancellation through the public call on three routes.
tests/test_nv_reference_cpu.py shows that the comparators accept an fp64 emulation of every kernel at every case used here and reject mutations of it, and that the
cases launch every instantiation.

Every test prints its worst error-to-bound ratio per output before it asserts (pytest -rP shows them); the last test prints the table of the run.
Measured on an MI355X: see DESIGN.md section 6, "normvar at kernel level"."""
import functools

import numpy as np
import pytest

import nv_reference as nv
import stage_helpers
from stage_helpers import Buf, same, twice

pytestmark = pytest.mark.gpu

WORST = {}
LADDER = {}
F64, F32 = np.float64, np.float32
I32, I64 = np.int32, np.int64
IDS = [nv.case_id(c) for c in nv.CASES]
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
	return _lib.NRM_F64 if np.dtype(dtype) == np.dtype(F64) else _lib.NRM_F32


def _inputs(pb, extra_row=None):
	"""y, lnw, wt (and c) of a case at its layout; -> (buffers, check) where check() asserts that the call left every input as it was and that each pointer has the
	alignment the case is for."""
	L = nv.layout(pb)
	y = pb['y'] if extra_row is None else np.vstack([pb['y'], extra_row])
	bufs = dict(y=Buf(y.shape, pb['ydt'], pitch=L['ldy'], data=y, skip=L['sy']), lnw=Buf(pb['n'], F64, data=pb['lnw'], skip=L['sl']), wt=Buf(pb['rows'], F64, data=pb['wt']))
	data = dict(y=y, lnw=pb['lnw'], wt=pb['wt'])
	if pb['nc']:
		bufs['c'] = Buf((pb['nc'], pb['n']), F64, pitch=L['ldc'], data=pb['c'], skip=L['sc'])
		data['c'] = pb['c']
	for k, sk in (('y', L['sy']), ('lnw', L['sl']), ('c', L['sc'])):
		if k in bufs:
			assert (bufs[k].ptr - sk * bufs[k].dtype.itemsize) % 256 == 0, 'the allocator no longer aligns to 256 bytes: nv_reference.route assumes it'

	def check():
		for k, b in bufs.items():
			assert same(b.get().reshape(np.shape(data[k])), np.asarray(data[k], b.dtype)), 'input %s changed' % k
	return bufs, L, check


# ---- nrm_normvar_weights ---------------------------------------------------------------------------------------------------------------------------------------------
def run_weights(pb):
	torch, _lib, eng = _env()
	rows, n = pb['rows'], pb['n']
	rp = nv.rows_pad_of(rows)

	def run():
		b, L, check = _inputs(pb)
		ldo = L['ldc']
		U, V, s1, s2 = Buf((rp, ldo), F64), Buf((rp, ldo), F64), Buf(rp, F64), Buf(rp, F64)
		_lib.check(eng.lib.nrm_normvar_weights(b['y'].ptr, _code(pb['ydt']), rows, n, L['ldy'], b['lnw'].ptr, b['wt'].ptr, U.ptr, V.ptr, ldo, rp, s1.ptr, s2.ptr, eng._stream()))
		_sync()
		check()
		return dict(U=U.get(), V=V.get(), s1=s1.get().ravel(), s2=s2.get().ravel())  # (get: nothing in front of the buffers or in their tails)
	return twice(run)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('i', [i for i, c in enumerate(nv.CASES) if c['entry'] == 'weights'], ids=lambda i: IDS[i])
def test_weights(i, exact):
	pb = nv.problem(i, exact)
	got = run_weights(pb)
	rows, n = pb['rows'], pb['n']
	for k in ('U', 'V'):  # the padding is the contract: exact zeros (+0.0), which the Gram kernel reads
		assert same(got[k][:, n:], np.zeros_like(got[k][:, n:])) and same(got[k][rows:], np.zeros_like(got[k][rows:])), k + ': padding not +0.0'
	assert same(got['s1'][rows:], np.zeros(len(got['s1']) - rows)) and same(got['s2'][rows:], np.zeros(len(got['s2']) - rows))
	note('k_nv_weights' + (' exact' if exact else ''), nv.judge_weights(got, i, exact), IDS[i])


# ---- nrm_normvar_solve, nrm_normvar_rescale -------------------------------------------------------------------------------------------------------------------------------
def run_solve(pb, flags0=(3, -7, -7, -7), tol=nv.TOL, rescale=True, c_override=None):
	torch, _lib, eng = _env()
	rows, n, nc = pb['rows'], pb['n'], pb['nc']
	nm = nc * (nc + 1) // 2 + nc + 2
	if c_override is not None:
		pb = dict(pb, c=c_override)

	def run():
		b, L, check = _inputs(pb)
		mom, cb, sc, rk, fl = Buf((rows, nm), F64), Buf((rows, nc), F64), Buf(rows, F64), Buf(rows, I64), Buf(4, I32, data=list(flags0))
		_lib.check(eng.lib.nrm_normvar_solve(b['y'].ptr, _code(pb['ydt']), rows, n, L['ldy'], b['lnw'].ptr, b['wt'].ptr, b['c'].ptr, nc, L['ldc'], float(tol), pb['keepvar'],
											 mom.ptr, cb.ptr, sc.ptr, rk.ptr, fl.ptr, eng._stream()))
		_sync()
		out = dict(mom=mom.get(), b=cb.get(), scale=sc.get().ravel(), rank=rk.get().ravel(), flags=fl.get().ravel())
		if rescale:
			_lib.check(eng.lib.nrm_normvar_rescale(b['y'].ptr, _code(pb['ydt']), rows, n, L['ldy'], b['lnw'].ptr, b['wt'].ptr, b['c'].ptr, nc, L['ldc'], cb.ptr, sc.ptr, eng._stream()))
			_sync()
			out['rescaled'] = sc.get().ravel()
			assert same(cb.get(), out['b'])
		check()
		return out
	return twice(run)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('i', [i for i, c in enumerate(nv.CASES) if c['entry'] == 'solve'], ids=lambda i: IDS[i])
def test_solve(i, exact):
	pb = nv.problem(i, exact)
	got = run_solve(pb)
	ws, sv = nv.judge_solve(got['mom'], got['b'], got['scale'], got['rank'], i, exact)
	assert got['flags'].tolist() == [3 + int((got['rank'] <= 0).sum()), -7, -7, -7] and not (got['rank'] <= 0).any()
	marked = got['scale'] == nv.MARK
	assert same(got['rescaled'][~marked], got['scale'][~marked]), 'nrm_normvar_rescale moved an unmarked gene'
	ws['rescaled'], ok = nv.judge_rescale(got['rescaled'], got['b'], i, marked, exact)
	assert not (got['rescaled'][marked & ok] < 0).any()
	print('%s: %d of %d genes marked' % (IDS[i], marked.sum(), len(marked)))
	note('k_nv_moments / k_nv_solve' + (' exact' if exact else ''), ws, IDS[i])


def test_solve_counts_rank_zero_genes_and_adds_to_its_flag():
	"""A covariate that is NaN leaves no eigenvalue to keep: rank 0 for every gene (norm.py:158-159 raises), flags[0] += genes, from whatever it held."""
	i = next(i for i, c in enumerate(nv.CASES) if c['entry'] == 'solve' and c['nc'] == 3 and c['rows'] > 64)
	pb = nv.problem(i)
	c = pb['c'].copy()
	c[0, 2] = np.nan  # (data, not an address: M_g then holds NaN, |NaN| >= tol x largest is false for every eigenvalue)
	for start in (0, 11):
		got = run_solve(pb, flags0=(start, -7, -7, -7), rescale=False, c_override=c)
		assert (got['rank'] == 0).all() and got['flags'].tolist() == [start + pb['rows'], -7, -7, -7]


# ---- nrm_normvar_apply, nrm_normvar_apply_w2 ----------------------------------------------------------------------------------------------------------------------------
def run_apply(pb, flags0=(-7, 2, -7, -7), extra_row=None, y=None, lnw=None, scale=None):
	torch, _lib, eng = _env()
	rows, n, nc = pb['rows'], pb['n'], pb['nc']
	pb = dict(pb, **{k: v for k, v in (('y', y), ('lnw', lnw), ('scale', scale)) if v is not None})

	def run():
		b, L, check = _inputs(pb, extra_row)
		cb, sc = Buf((rows, nc), F64, data=pb['b']), Buf(rows, F64, data=pb['scale'])
		out, fl = Buf((rows, n), pb['odt'], pitch=L['ldo'], skip=L['so']), Buf(4, I32, data=list(flags0))
		if pb['entry'] == 'apply':
			_lib.check(eng.lib.nrm_normvar_apply(b['y'].ptr, _code(pb['ydt']), rows, n, L['ldy'], b['lnw'].ptr, b['wt'].ptr, b['c'].ptr, nc, L['ldc'], cb.ptr, sc.ptr, out.ptr,
												 _code(pb['odt']), L['ldo'], fl.ptr, eng._stream()))
		else:
			w2 = Buf((rows, n), F64, pitch=L['ldc'], data=pb['w2'])
			_lib.check(eng.lib.nrm_normvar_apply_w2(b['y'].ptr, _code(pb['ydt']), rows, n, L['ldy'], w2.ptr, L['ldc'], b['c'].ptr, nc, L['ldc'], cb.ptr, out.ptr, _code(pb['odt']),
													L['ldo'], eng._stream()))
		_sync()
		check()
		assert same(cb.get(), np.asarray(pb['b'], F64)) and same(sc.get().ravel(), np.asarray(pb['scale'], F64))
		if pb['entry'] == 'apply_w2':
			assert same(w2.get(), pb['w2'])
		return dict(out=out.get(), flags=fl.get().ravel())
	return twice(run)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('i', [i for i, c in enumerate(nv.CASES) if c['entry'] in ('apply', 'apply_w2')], ids=lambda i: IDS[i])
def test_apply(i, exact):
	pb = nv.problem(i, exact)
	got = run_apply(pb)
	assert got['flags'].tolist() == [-7, 2, -7, -7], 'finite results, or apply_w2 (which takes no flags): the counters as they were'
	note('k_nv_' + pb['entry'] + (' exact' if exact else ''), nv.judge_apply(got['out'], i, exact), IDS[i])
	if pb['entry'] == 'apply' and not exact and (pb['wt'] == 0).any():
		other = run_apply(pb, lnw=pb['lnw'] + 0.75)  # rows with wt == 0 take e = 1, whatever ln w holds: the same bits
		assert same(other['out'][pb['wt'] == 0], got['out'][pb['wt'] == 0])
		assert pb['rows'] == (pb['wt'] == 0).sum() or not same(other['out'], got['out'])


def test_apply_counts_the_waves_that_stored_a_value_that_is_not_finite():
	"""flags[1] += (workgroup, wave) pairs with a non-finite stored value, the number derived from the thread map (nv_reference.bad_waves): an inf in y in the four-cell
	loop, one in the tail loop, an fp32 output that overflows from a finite fp64 value, and a row of inf right behind the matrix, which no workgroup may count."""
	i = next(i for i, c in enumerate(nv.CASES) if c['entry'] == 'apply' and c['n'] == 1029 and c['rows'] >= 5 and c['nc'] <= 9 and c['odt'] == F64)
	pb = nv.problem(i)
	rows, n = pb['rows'], pb['n']
	assert n & ~3 == 1028 and rows % 4
	for name, cells in (('four-cell loop', [(0, 5), (0, 600), (rows - 1, 1027)]), ('tail loop', [(1, 1028)]), ('both', [(0, 5), (0, 1028), (2, 300), (rows - 1, 1028)])):
		y = pb['y'].copy()
		for g, k in cells:
			y[g, k] = np.inf
		ref = nv.apply(y, pb['lnw'], pb['wt'], pb['c'], pb['b'], pb['scale'])[0]
		want = nv.bad_waves(~np.isfinite(np.asarray(ref, F64)))
		assert want == len({(g // 4, nv.thread_of(n)[0][k] // 64) for g, k in cells})
		for start in (0, 9):
			got = run_apply(pb, flags0=(-7, start, -7, -7), y=y)
			print(name, 'flags[1]', got['flags'][1], 'from', start, 'want +', want)
			assert got['flags'].tolist() == [-7, start + want, -7, -7]
			assert np.array_equal(~np.isfinite(got['out']), ~np.isfinite(np.asarray(ref, F64)))
	got = run_apply(pb, flags0=(-7, 0, -7, -7), extra_row=np.full(n, np.inf))  # behind the last live row of the last workgroup
	assert got['flags'].tolist() == [-7, 0, -7, -7] and np.isfinite(got['out']).all()
	# fp32 output: a finite fp64 value above fp32's range
	j = next(j for j, c in enumerate(nv.CASES) if c['entry'] == 'apply' and c['odt'] == F32 and c['ydt'] == F64 and c['n'] >= 1024 and c['nc'] <= 9 and c['rows'] >= 2)
	pb = nv.problem(j)
	scale = pb['scale'].copy()
	scale[1] = 1e300
	ref = nv.apply(pb['y'], pb['lnw'], pb['wt'], pb['c'], pb['b'], scale)[0]
	assert np.isfinite(np.asarray(ref, F64)).all()
	with np.errstate(over='ignore'):
		want = nv.bad_waves(~np.isfinite(np.asarray(ref, F64).astype(F32)))
	got = run_apply(pb, flags0=(-7, 1, -7, -7), scale=scale)
	assert want >= 1 and got['flags'].tolist() == [-7, 1 + want, -7, -7] and np.isinf(got['out'][1]).all()


# ---- the entries in norm.py's order --------------------------------------------------------------------------------------------------------------------------------------
def test_entries_in_order_give_the_bits_of_the_public_call_and_of_a_plan_step():
	"""solve -> rescale -> apply into raised-pitch buffers against norm.normvar(..., device_out=True) and a NormvarPlan step on the same inputs, bit for bit; the
	inputs hold genes the rule marks (rows the covariates explain to 1e-5), so the chain shows that the rescale runs on both."""
	torch, _lib, eng = _env()
	from normalisr_amd import norm
	rng = np.random.default_rng(5)
	ng, n, nc = 37, 1029, 3
	c = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	y = rng.normal(size=(ng, n)) - 9
	y[3] = rng.normal(size=nc) @ c + 1e-5 * rng.normal(size=n)
	y[20] = 3 + 1e-5 * rng.normal(size=n)
	y = y.astype(F32)
	w, wt = np.exp(0.25 * rng.normal(size=n)), rng.uniform(0.1, 1.5, ng)
	wt[::7] = 0
	lnw = np.log(w)
	d_y = torch.from_numpy(y).cuda()
	pub = norm.normvar(d_y, c, w, wt, device_out=True)[0]
	plan = norm.NormvarPlan(d_y, c, w, wt)
	assert plan.lean
	for _ in range(3):
		stepped = plan.step()
	assert plan._graph.graph is not None and plan.check()
	ldy, ldc, ldo, nm = n + 7, n + 3, n + 5, nc * (nc + 1) // 2 + nc + 2
	by, blnw, bwt, bc = Buf((ng, n), F32, pitch=ldy, data=y), Buf(n, F64, data=lnw), Buf(ng, F64, data=wt), Buf((nc, n), F64, pitch=ldc, data=c)
	mom, cb, sc, rk, fl, out = Buf((ng, nm), F64), Buf((ng, nc), F64), Buf(ng, F64), Buf(ng, I64), Buf(4, I32, data=[0, 0, -7, -7]), Buf((ng, n), F64, pitch=ldo)
	st = eng._stream()
	_lib.check(eng.lib.nrm_normvar_solve(by.ptr, _lib.NRM_F32, ng, n, ldy, blnw.ptr, bwt.ptr, bc.ptr, nc, ldc, 1e-8, 1, mom.ptr, cb.ptr, sc.ptr, rk.ptr, fl.ptr, st))
	_sync()
	marked = sc.get().ravel() == nv.MARK
	_lib.check(eng.lib.nrm_normvar_rescale(by.ptr, _lib.NRM_F32, ng, n, ldy, blnw.ptr, bwt.ptr, bc.ptr, nc, ldc, cb.ptr, sc.ptr, st))
	_lib.check(eng.lib.nrm_normvar_apply(by.ptr, _lib.NRM_F32, ng, n, ldy, blnw.ptr, bwt.ptr, bc.ptr, nc, ldc, cb.ptr, sc.ptr, out.ptr, _lib.NRM_F64, ldo, fl.ptr, st))
	_sync()
	assert marked[3] and marked[20] and marked.sum() == 2, marked
	assert fl.get().ravel().tolist() == [0, 0, -7, -7]
	assert same(out.get(), pub.cpu().numpy()) and same(out.get(), stepped.cpu().numpy())
	ref = nv.reference_two_pass(y, lnw, wt, c)[0]
	err = np.asarray(np.abs(nv.ld(out.get()) - ref).max(axis=1) / np.abs(ref).max(axis=1), F64)
	print('chain against the longdouble two-pass reference: worst row %.3g, marked rows %s' % (err.max(), err[marked]))
	assert err.max() < nv.BAR


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
	"""One refusal per clause of every NRM_REQUIRE of the five entries: the error code, and every output untouched."""
	torch, _lib, eng = _env()
	rows, n, nc, rp = 5, 9, 3, 8
	rng = np.random.default_rng(2)
	y, lnw, wt, c = Buf((rows, n), F64, data=rng.normal(size=(rows, n))), Buf(n, F64, data=np.zeros(n)), Buf(rows, F64, data=np.ones(rows)), Buf((nc, n), F64, data=rng.normal(size=(nc, n)))
	w2, cb, sc = Buf((rows, n), F64, data=np.ones((rows, n))), Buf((rows, nc), F64, data=np.zeros((rows, nc))), Buf(rows, F64, data=np.ones(rows))
	wide = int(eng.lib.nrm_wide_covariates())
	st = eng._stream()

	def outs(**k):
		return {name: Buf(*shape) for name, shape in k.items()}

	def refuse(entry, base, changes, out):
		fn = getattr(eng.lib, entry)
		for at, v in changes:
			args = list(base)
			args[at] = v
			rc = fn(*args)
			_sync()
			assert rc != 0, (entry, 'accepted', at, v)
			assert all(b.clean() for b in out.values()), (entry, 'wrote something', at, v)
		_lib.check(fn(*base))
		_sync()
		assert not any(b.clean() for k, b in out.items() if k != 'flags'), entry  # (the counters move only when there is something to count)

	o = outs(U=((rp, n), F64), V=((rp, n), F64), s1=(rp, F64), s2=(rp, F64))
	refuse('nrm_normvar_weights', [y.ptr, _lib.NRM_F64, rows, n, n, lnw.ptr, wt.ptr, o['U'].ptr, o['V'].ptr, n, rp, o['s1'].ptr, o['s2'].ptr, st],
		   [(1, 77), (2, 0), (3, 0), (4, n - 1), (9, n - 1), (10, 4), (10, 7), (0, 0), (5, 0), (6, 0), (7, 0), (8, 0), (11, 0), (12, 0)], o)
	nm = nc * (nc + 1) // 2 + nc + 2
	o = outs(mom=((rows, nm), F64), b=((rows, nc), F64), scale=(rows, F64), rank=(rows, I64), flags=(4, I32))
	assert int(eng.lib.nrm_normvar_device_covariates()) == nv.NV_NC
	refuse('nrm_normvar_solve', [y.ptr, _lib.NRM_F64, rows, n, n, lnw.ptr, wt.ptr, c.ptr, nc, n, 1e-8, 1, o['mom'].ptr, o['b'].ptr, o['scale'].ptr, o['rank'].ptr, o['flags'].ptr, st],
		   [(1, 77), (2, 0), (3, 0), (4, n - 1), (8, 0), (8, nv.NV_NC + 1), (9, n - 1), (10, 0.0), (10, -1e-8), (0, 0), (5, 0), (6, 0), (7, 0), (12, 0), (13, 0), (14, 0), (15, 0), (16, 0)], o)
	o = dict(scale=Buf(rows, F64))
	base = [y.ptr, _lib.NRM_F64, rows, n, n, lnw.ptr, wt.ptr, c.ptr, nc, n, cb.ptr, o['scale'].ptr, st]
	for at, v in [(1, 77), (2, 0), (3, 0), (4, n - 1), (8, 0), (8, wide + 1), (9, n - 1), (0, 0), (5, 0), (6, 0), (7, 0), (10, 0), (11, 0)]:
		args = list(base)
		args[at] = v
		assert eng.lib.nrm_normvar_rescale(*args) != 0, ('nrm_normvar_rescale accepted', at, v)
	_sync()
	assert o['scale'].clean()
	mk = Buf(rows, F64, data=[nv.MARK, 1.0, nv.MARK, 2.5, nv.MARK])  # the same arguments accepted: the marked genes get a scale, the others keep their bits
	base[11] = mk.ptr
	_lib.check(eng.lib.nrm_normvar_rescale(*base))
	_sync()
	got = mk.get().ravel()
	assert got[1] == 1.0 and got[3] == 2.5 and (got[[0, 2, 4]] > 0).all(), got
	o = outs(out=((rows, n), F64), flags=(4, I32))
	refuse('nrm_normvar_apply', [y.ptr, _lib.NRM_F64, rows, n, n, lnw.ptr, wt.ptr, c.ptr, nc, n, cb.ptr, sc.ptr, o['out'].ptr, _lib.NRM_F64, n, 0, st],
		   [(1, 77), (13, 77), (2, 0), (3, 0), (4, n - 1), (14, n - 1), (8, 0), (8, wide + 1), (9, n - 1), (0, 0), (5, 0), (6, 0), (7, 0), (10, 0), (11, 0), (12, 0)], dict(out=o['out']))
	assert o['flags'].clean()  # (a null d_flags is allowed: nothing counted)
	o = outs(out=((rows, n), F32))
	refuse('nrm_normvar_apply_w2', [y.ptr, _lib.NRM_F64, rows, n, n, w2.ptr, n, c.ptr, nc, n, cb.ptr, o['out'].ptr, _lib.NRM_F32, n, st],
		   [(1, 77), (12, 77), (2, 0), (3, 0), (4, n - 1), (6, n - 1), (13, n - 1), (8, 0), (8, 65), (9, n - 1), (0, 0), (5, 0), (7, 0), (10, 0), (11, 0)], o)
	assert eng.lib.nrm_last_error().decode()


# ---- the ladder of cancellation through the public call --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder(nc, dtype, rhos):
	"""Every rung and both kinds stacked into one matrix (the rows share ln w and the covariates), with the longdouble two-pass reference.  Read-only."""
	ys, tag = [], []
	for rho in rhos:
		for kind in ('flat', 'explained'):
			y, lnw, wt, c = nv.ladder_rows(rho, kind, nc=nc, dtype=dtype)
			ys.append(y)
			tag += [(rho, kind)] * len(y)
	y, wt = np.vstack(ys), np.tile(wt, len(ys))
	ref, scale, rho_is = nv.reference_two_pass(y, lnw, wt, c)
	return y, lnw, wt, c, ref, tag, rho_is, scale


ROUTES = [('device', 3), ('NRM_DEBUG=normvar=host', 3), ('nrm_normvar_host', 12)]


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('route,nc', ROUTES, ids=[r[0] for r in ROUTES])
def test_ladder_through_the_public_call(route, nc, dtype, monkeypatch):
	"""rho = dv2 / rms(weighted row) from 1 to 1e-6, a nearly flat row and a row the covariates explain, fp32 and fp64 input: every output row within 1e-6 of its largest
	magnitude of the longdouble two-pass reference, and no call raises.  The bar is DESIGN section 2's for normvar.  rho = 1e-7 is printed and recorded, not asserted."""
	from normalisr_amd import norm

	def call(y, lnw, wt, c):
		w = np.exp(lnw)
		if route == 'nrm_normvar_host':
			return norm._normvar_host_entry(y, c, w, wt, None, 1, True, 1e-8, np.dtype(F64))[0].copy()  # (the entry recycles its result buffer)
		if route != 'device':
			monkeypatch.setenv('NRM_DEBUG', 'normvar=host')
		try:
			return norm.normvar(y, c, w, wt)[0]
		finally:
			monkeypatch.delenv('NRM_DEBUG', raising=False)

	y, lnw, wt, c, ref, tag, rho_is, _ = ladder(nc, dtype, tuple(nv.RHOS[:-1]))
	got = call(y, lnw, wt, c)
	assert got.dtype == F64 and np.isfinite(got).all()
	err = np.asarray(np.abs(nv.ld(got) - ref).max(axis=1) / np.abs(ref).max(axis=1), F64)
	worst = {}
	for t, e in zip(tag, err):
		worst[t] = max(worst.get(t, 0.0), float(e))
	for (rho, kind), e in sorted(worst.items(), reverse=True):
		print('%-24s %s rho %-6g %-10s worst row error / row maximum %.3g' % (route, np.dtype(dtype).name, rho, kind, e))
		LADDER[(route, np.dtype(dtype).name, rho, kind)] = e
	y7, lnw, wt7, c, ref7, tag7, _, _ = ladder(nc, dtype, (nv.RHOS[-1], ))
	try:
		got7 = call(y7, lnw, wt7, c)
		e7 = float(np.asarray(np.abs(nv.ld(got7) - ref7).max(axis=1) / np.abs(ref7).max(axis=1), F64).max())
	except (AssertionError, RuntimeError, ValueError):
		e7 = float('inf')
	print('%-24s %s rho 1e-07 (recorded, not asserted) worst row error / row maximum %.3g' % (route, np.dtype(dtype).name, e7))
	LADDER[(route, np.dtype(dtype).name, 1e-7, 'both')] = e7
	assert max(worst.values()) <= nv.BAR, worst


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_ladder_scale_before_and_after_the_rule_and_the_margin_of_the_unmarked(dtype):
	"""The ladder at the entries (nrm_normvar_solve, nrm_normvar_rescale; three covariates): the relative error of the scale against the longdouble two-pass reference,
	(1) in the one-pass form evaluated in fp64 on the device's own moments and coefficients -- the arithmetic of the code before the rule, printed: it crosses 1e-6 at
	rho = 1e-5 --, (2) as the two entries leave it: under 1e-6 on every rung, and the worst UNMARKED gene at least 100 x under it (the choice of tau, csrc/nrm_nv_scale.h)."""
	torch, _lib, eng = _env()
	y, lnw, wt, c, ref, tag, rho_is, want = ladder(3, dtype, tuple(nv.RHOS))
	rows, n, nc, nm = y.shape[0], y.shape[1], 3, 11
	by, bl, bw, bc = Buf((rows, n), dtype, data=y), Buf(n, F64, data=lnw), Buf(rows, F64, data=wt), Buf((nc, n), F64, data=c)
	mom, cb, sc, rk, fl = Buf((rows, nm), F64), Buf((rows, nc), F64), Buf(rows, F64), Buf(rows, I64), Buf(4, I32, data=[0, 0, -7, -7])
	_lib.check(eng.lib.nrm_normvar_solve(by.ptr, _code(dtype), rows, n, n, bl.ptr, bw.ptr, bc.ptr, nc, n, 1e-8, 1, mom.ptr, cb.ptr, sc.ptr, rk.ptr, fl.ptr, eng._stream()))
	_sync()
	m, b, marked = mom.get(), cb.get(), sc.get().ravel() == nv.MARK
	_lib.check(eng.lib.nrm_normvar_rescale(by.ptr, _code(dtype), rows, n, n, bl.ptr, bw.ptr, bc.ptr, nc, n, cb.ptr, sc.ptr, eng._stream()))
	_sync()
	after = sc.get().ravel()
	a, s1, s2 = m[:, 6:9], m[:, 9], m[:, 10]
	mean = s1 / n
	with np.errstate(divide='ignore', invalid='ignore'):  # norm.py's Gram-launch lines as they stood, on the device's sums
		before = (np.sqrt(np.maximum(s2 / n - mean * mean, 0.0)) / np.sqrt(np.maximum(s2 - np.einsum('gc,gc->g', a, b), 0.0) / n))**wt
		e0, e1 = (np.nan_to_num(np.abs(np.asarray(nv.ld(v) / want - 1, F64)), nan=np.inf) for v in (before, after))
	rung = {}
	for t, x0, x1, mk in zip(tag, e0, e1, marked):
		r = rung.setdefault(t, [0.0, 0.0, 0])
		r[0], r[1], r[2] = max(r[0], x0), max(r[1], x1), r[2] + int(mk)
	for (rho, kind), (x0, x1, k) in sorted(rung.items(), reverse=True):
		print('scale %s rho %-6g %-10s one-pass on the device\'s sums %.2e   with the rule %.2e   (%d of 10 marked)' % (np.dtype(dtype).name, rho, kind, x0, x1, k))
		LADDER[('scale, one-pass', np.dtype(dtype).name, rho, kind)] = x0
		LADDER[('scale, with the rule', np.dtype(dtype).name, rho, kind)] = x1
	unmarked = float(e1[~marked].max())
	print('worst unmarked gene on the device, %s: %.3g (%.0f x under the bar)' % (np.dtype(dtype).name, unmarked, nv.BAR / unmarked))
	LADDER[('scale, worst unmarked', np.dtype(dtype).name, 0, 'all')] = unmarked
	asserted = np.array([t[0] >= 1e-6 for t in tag])  # (rho = 1e-7 is printed and recorded, not asserted)
	assert e1[asserted].max() < nv.BAR and unmarked * 100 <= nv.BAR
	assert marked.any() and not marked.all()


def test_zz_table_of_the_run():
	"""The worst error-to-bound ratio per kernel and output over the tests above, and the ladder (pytest -rP); alone it prints nothing."""
	for (kernel, name), (ratio, case) in sorted(WORST.items()):
		print('%-40s %-12s %.3g  (%s)' % (kernel, name, ratio, case))
	for k, e in sorted(LADDER.items(), key=str):
		print('ladder %-24s %-8s rho %-6g %-10s %.3g' % (k + (e, )))
	assert all(r <= 1 for r, _ in WORST.values())
