"""GPU checks of the resident co-expression loop (normalisr_amd/levels.py; csrc/nrm_coex_levels.hip): the two kernels at the smallest shapes that can go wrong against
longdouble, CoexLevels on golden G23 against the reference's coex and against coex from scratch at every level, the paths an append can take, and coex_levels (the
function and the command) against the same steps made one by one with the public functions."""
import os
import sys

import numpy as np
import pytest

import levels_numpy as ln
from conftest import GOLDEN

if GOLDEN not in sys.path:
	sys.path.insert(0, GOLDEN)
from g23_inputs import RANKS  # noqa: E402
from levels_numpy import g23_case, of_largest  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0**-53
LD = np.longdouble


def _engine():
	from normalisr_amd import engine
	return engine.get_engine()


# ---- nrm_coex_project ------------------------------------------------------------------------------------------------------------------------------------------------
def _project(eng, x, q):
	"""A (k, nt) of nrm_coex_project for device tensors x (nt, ns; any pitch and base) and q (k, ns)."""
	from normalisr_amd import _lib
	torch = eng.torch
	nt, ns = x.shape
	k = q.shape[0]
	a = torch.full((k, nt), float('nan'), dtype=torch.float64, device=eng.device)
	_lib.check(eng.lib.nrm_coex_project(x.data_ptr(), _lib.NRM_F64 if x.dtype == torch.float64 else _lib.NRM_F32, nt, ns, x.stride(0), q.data_ptr(), k, q.stride(0),
										a.data_ptr(), a.stride(0), eng._stream()))
	torch.cuda.synchronize()
	return a.cpu().numpy()


def _layouts(eng, x):
	"""The matrix x (numpy) in HBM three ways: contiguous, with a pitch of ns + 1 (odd rows of fp32 start off a 16-byte boundary), and as a view that starts one
	element into its buffer."""
	torch = eng.torch
	nt, ns = x.shape
	t = eng.upload(x)
	wide = torch.zeros((nt, ns + 1), dtype=t.dtype, device=eng.device)
	wide[:, :ns] = t
	flat = torch.zeros((nt * ns + 1, ), dtype=t.dtype, device=eng.device)
	flat[1:] = t.reshape(-1)
	return (('contiguous', t), ('pitch ns + 1', wide[:, :ns]), ('one element in', flat[1:].view(nt, ns)))


@pytest.mark.parametrize('dtype', (np.float32, np.float64))
@pytest.mark.parametrize('nt,ns,k', ((1, 1, 1), (3, 63, 1), (5, 65, 2), (7, 1003, 3), (33, 4099, 8), (2, 70001, 3)))
def test_project_against_longdouble(nt, ns, k, dtype):
	eng = _engine()
	rng = np.random.default_rng(nt * 1000 + ns + k)
	x = (rng.standard_normal((nt, ns)) * 10.0**rng.integers(-2, 3, (nt, 1)) + rng.standard_normal((nt, 1))).astype(dtype)
	q = rng.standard_normal((k, ns))
	want = q.astype(LD) @ x.astype(LD).T
	bound = 8 * U * (np.abs(q).astype(LD) @ np.abs(x).astype(LD).T)
	d_q = eng.upload(q)
	first = None
	for name, t in _layouts(eng, x):
		assert t.stride(0) >= ns and t.stride(1) == 1
		a = _project(eng, t, d_q)
		err = np.abs(a.astype(LD) - want)
		print(nt, ns, k, np.dtype(dtype).name, name, 'largest error / bound: %.3g' % float((err / bound).max()))
		assert np.isfinite(a).all() and (err <= bound).all()
		assert np.array_equal(a, _project(eng, t, d_q))  # two calls, the same bits
		if first is None:
			first = a
		assert np.array_equal(a, first)  # and the same whatever the alignment: the order of the sums depends on the shape alone


def test_project_row_of_a_large_mean_against_a_zero_mean_direction():
	"""A row holding 1e6 + noise against a unit direction whose entries add up to zero: the answer, of the size of the noise, is what is left of terms a million
	times larger.  The bound is the same formula, 8 u sum |x_c q_c|: about 1e-7 here, 1e-7 of the answer.  The rounding of the products alone accounts for an eighth
	of it at most (u per term); the sums, being compensated, add next to nothing, so the result stays within a quarter of the bound however many terms there are."""
	eng = _engine()
	rng = np.random.default_rng(77)
	ns = 30011
	for dtype in (np.float32, np.float64):
		x = (1e6 + rng.standard_normal((2, ns))).astype(dtype)
		q = rng.standard_normal((1, ns))
		q -= q.mean()
		q /= np.sqrt((q * q).sum())
		want = q.astype(LD) @ x.astype(LD).T
		bound = 8 * U * (np.abs(q).astype(LD) @ np.abs(x).astype(LD).T)
		a = _project(eng, eng.upload(x), eng.upload(q))
		err = np.abs(a.astype(LD) - want)
		print(np.dtype(dtype).name, 'answer %.3g, error %.3g, bound %.3g' % (float(np.abs(want).max()), float(err.max()), float(bound.max())))
		assert (err <= bound).all() and float(bound.max()) < 1e-6
		assert (err <= bound / 4).all()  # (product rounding alone, u per term, is an eighth of the bound at most)


# ---- nrm_coex_downdate -----------------------------------------------------------------------------------------------------------------------------------------------
def _downdate(eng, g, ss, ss_ref, a):
	from normalisr_amd import _lib
	torch = eng.torch
	nt = ss.shape[0]
	counters = torch.zeros(2, dtype=torch.int32, device=eng.device)
	_lib.check(eng.lib.nrm_coex_downdate(g.data_ptr(), nt, g.stride(0), ss.data_ptr(), ss_ref.data_ptr(), a.data_ptr(), a.shape[0], a.stride(0), counters.data_ptr(),
										 eng._stream()))
	torch.cuda.synchronize()
	return counters.cpu().numpy()


@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('nt', (1, 63, 64, 65, 130))
def test_downdate_against_numpy(nt, k):
	eng = _engine()
	rng = np.random.default_rng(nt * 10 + k)
	ld = nt + 3
	y = rng.standard_normal((nt, nt + 5))
	g = np.full((nt, ld), 12345.0)
	g[:, :nt] = y @ y.T
	g[:, :nt] = (g[:, :nt] + g[:, :nt].T) / 2
	a = rng.standard_normal((k, nt))
	ss = 4 * (a * a).sum(axis=0) + 1
	d_g, d_ss, d_ref = eng.upload(g), eng.upload(ss), eng.upload(ss)
	c = _downdate(eng, d_g, d_ss, d_ref, eng.upload(a))
	out, ss_out = d_g.cpu().numpy(), d_ss.cpu().numpy()
	i, j = np.meshgrid(np.arange(nt), np.arange(nt), indexing='ij')
	valid = j // 64 >= i // 64
	want = g[:, :nt].astype(LD) - np.einsum('ki,kj->ij', a.astype(LD), a.astype(LD))
	bound = 2 * U * (np.abs(g[:, :nt]) + np.einsum('ki,kj->ij', np.abs(a), np.abs(a)))
	assert (np.abs(out[:, :nt].astype(LD) - want)[valid] <= bound[valid]).all()
	assert np.array_equal(out[:, :nt][~valid], g[:, :nt][~valid])  # tiles below the diagonal are not touched
	assert (out[:, nt:] == 12345.0).all()  # nor the padding columns
	same = i // 64 == j // 64
	assert np.array_equal(out[:, :nt][same], out[:, :nt].T[same])  # symmetric bit for bit where both halves are held
	up = np.triu(np.ones((nt, nt), dtype=bool))
	assert valid[up].all()  # dot[min(i, j), max(i, j)], what the symmetric sweep reads, lies in the valid part
	assert (np.abs(ss_out.astype(LD) - (ss.astype(LD) - (a.astype(LD)**2).sum(axis=0))) <= 2 * U * (np.abs(ss) + (a * a).sum(axis=0))).all()
	assert tuple(c) == (0, 0)


def test_downdate_counters_are_exact():
	"""Rows 3, 5, 64 and 100 of 130: a new sum of squares of 2^-11, 2^-9 and exactly 2^-10 of the reference (below, above and at the threshold) and one driven to
	-0.05.  [0] counts the last; [1] the first and the last (a sum that is <= 0 is below 2^-10 of a positive reference too)."""
	eng = _engine()
	nt = 130
	a = np.full((1, nt), 0.5)
	ss = np.full(nt, 1.25)
	ref = np.ones(nt)
	ss[3], ss[5], ss[100], ss[64] = 0.25 + 2.0**-11, 0.25 + 2.0**-9, 0.25 + 2.0**-10, 0.2
	d_ss = eng.upload(ss)
	c = _downdate(eng, eng.upload(np.eye(nt)), d_ss, eng.upload(ref), eng.upload(a))
	out = d_ss.cpu().numpy()
	assert out[3] == 2.0**-11 and out[5] == 2.0**-9 and out[100] == 2.0**-10 and out[64] < 0 and (np.delete(out, [3, 5, 64, 100]) == 1.0).all()
	assert tuple(c) == (1, 2)
	d_ss = eng.upload(np.where(np.arange(nt) == 7, np.nan, ss))
	assert tuple(_downdate(eng, eng.upload(np.eye(nt)), d_ss, eng.upload(ref), eng.upload(a))) == (2, 2)  # a NaN is not finite, and below nothing


# ---- the class ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _check(got, want, fp32, what, worst=None):
	"""(p, dot, var) against a reference: P to 1e-6 relative (where the reference's P is representable with room to spare, at most that elsewhere), dot and var to
	1e-10 of the largest entry for fp64 outputs and to fp32 rounding for fp32 outputs."""
	host = lambda v: np.asarray(v.cpu().numpy() if hasattr(v, 'data_ptr') else v)
	p, dot, var = (host(v) for v in got)
	want = [host(v) for v in want]
	assert p.dtype == dot.dtype == var.dtype == (np.float32 if fp32 else np.float64), what
	wp = np.asarray(want[0], dtype=np.float64)
	off = ~np.eye(len(wp), dtype=bool)
	floor = 1e-30 if fp32 else 1e-290
	big = off & (wp >= floor)
	ep = float((np.abs(p.astype(np.float64)[big] - wp[big]) / wp[big]).max()) if big.any() else 0.0
	if worst is not None:
		worst[0] = max(worst[0], ep)
	assert ep < 1e-6, (what, ep)
	assert (p[off & ~big] <= floor * (1 + 1e-4)).all() and (p >= 0).all(), what
	tol = 2.0**-23 if fp32 else 1e-10
	assert of_largest(dot, np.asarray(want[1], dtype=np.float64)) < tol and of_largest(var, np.asarray(want[2], dtype=np.float64)) < tol, what
	assert (np.diag(p) == 0).all() and (np.diag(dot) == 0).all() and np.array_equal(p, p.T), what
	return ep


@pytest.mark.parametrize('fp32', (False, True))
@pytest.mark.parametrize('resident', (False, True))
@pytest.mark.parametrize('name', ('A', 'B'))
def test_g23_through_coex_levels(golden, name, resident, fp32):
	import normalisr_amd.normalisr as norm
	from normalisr_amd import levels
	g = golden('G23_coex_levels')
	dt32, dc, rows = g23_case(g, name)
	dt = dt32 if fp32 else dt32.astype(np.float64)
	x = _engine().upload(dt) if resident else dt
	lv = levels.CoexLevels(x, dc)
	worst = [0.0]
	for k in range(5):
		if k:
			assert lv.append(rows[k - 1]) is lv
		assert lv.level == k and lv.rank == RANKS[k] and lv.dof == dt.shape[1] - 1 - RANKS[k] and lv.dc.shape == (8 + k, dt.shape[1])
		got = lv.results(device_out=resident)
		_check(got, [g['{}_{}{}'.format(name, key, k)] for key in ('p', 'dot', 'var')], fp32, 'reference, level %d' % k, worst)
		scratch = norm.coex(x, lv.dc, device_out=resident)
		assert type(got[0]) is type(scratch[0]) and type(got[2]) is type(scratch[2]) and isinstance(got[2], np.ndarray)
		_check(got, scratch, fp32, 'from scratch, level %d' % k, worst)
	assert lv.rebuilt == [False] * 4
	print(name, 'resident' if resident else 'numpy', 'fp32' if fp32 else 'fp64', 'worst P error over the levels: %.3g' % worst[0])


def _problem_a(golden):
	g = golden('G23_coex_levels')
	dt32, dc, rows = g23_case(g, 'A')
	return dt32.astype(np.float64), dc, rows


def test_paths_of_an_append(golden):
	import normalisr_amd.normalisr as norm
	from normalisr_amd import levels
	dt, dc, rows = _problem_a(golden)
	lv = levels.CoexLevels(dt, dc)
	for k in range(4):
		before, dof = lv.results(), lv.dof
		lv.append(rows[k])
		assert lv.rebuilt[-1] is False and lv.info['counters'] == (0, 0)  # generic rows, the in-span row, and gene 1 keeping 1 % of its variance (k = 1)
		if k == 2:
			assert lv.info['rho'][0] <= levels.RHO_SPAN and lv.dof == dof and lv.rank == 9
			assert all(np.array_equal(u, v) for u, v in zip(before, lv.results()))  # the in-span row: bit-identical
		else:
			assert lv.info['rho'][0] >= levels.RHO_MIN and lv.dof == dof - 1
	ss = np.asarray(lv.results()[2])
	assert ss[1] < 0.02 * np.asarray(levels.CoexLevels(dt, dc).results()[2])[1]
	# a row that keeps 1e-9 of its squared length outside the span: rebuilt, and still what coex gives
	rng = np.random.default_rng(9)
	b = ln.span_basis(lv.dc)[0]
	fresh = ln.off_span(b, rng.standard_normal(dt.shape[1]))
	inside = b.T @ rng.standard_normal(len(b))
	v = inside / np.sqrt(inside @ inside) + np.sqrt(1e-9) * fresh / np.sqrt(fresh @ fresh)
	lv.append(v)
	assert lv.rebuilt[-1] is True and 0.9e-9 < lv.info['rho'][0] < 1.1e-9 and lv.info['counters'] == (0, 0)
	_check(lv.results(), norm.coex(dt, lv.dc), False, 'rho = 1e-9')
	from normalisr_amd.association import inv_rank
	assert lv.dof == dt.shape[1] - 1 - lv.rank and lv.rank == inv_rank(lv.dc @ lv.dc.T)[1] == 10


def test_guard_trips_for_a_gene_that_keeps_a_millionth(golden):
	import normalisr_amd.normalisr as norm
	from normalisr_amd import levels
	dt, dc, rows = _problem_a(golden)
	dt = dt.copy()
	q = ln.off_span(ln.span_basis(dc)[0], rows[3])
	dt[5] = 3.0 + 1000.0 * q / np.sqrt((q * q).mean()) + np.random.default_rng(4).standard_normal(dt.shape[1])  # keeps 1e-6 of its variance once rows[3] is removed
	lv = levels.CoexLevels(dt, dc)
	lv.append(rows[0])
	assert lv.rebuilt == [False]
	lv.append(rows[3])
	assert lv.rebuilt == [False, True] and lv.info['counters'][1] >= 1 and lv.info['counters'][0] == 0 and lv.info['rho'][0] >= levels.RHO_MIN
	_check(lv.results(), norm.coex(dt, lv.dc), False, 'after the guard')
	lv.append(rows[1])  # the rebuild refreshed the reference sums: the next row updates again
	assert lv.rebuilt == [False, True, False]
	_check(lv.results(), norm.coex(dt, lv.dc), False, 'after the guard and one more row')


def test_rows_at_once_twice_dimreduce_and_bits(golden):
	import normalisr_amd.normalisr as norm
	from normalisr_amd import levels
	dt, dc, rows = _problem_a(golden)
	one = levels.CoexLevels(dt, dc)
	for k in range(3):
		one.append(rows[k])
	three = levels.CoexLevels(dt, dc).append(rows[:3])
	assert three.level == 1 and three.rebuilt == [False] and one.rebuilt == [False] * 3 and three.rank == one.rank == 9 and np.array_equal(three.dc, one.dc)
	a, b = one.results(), three.results()
	assert of_largest(b[1], a[1]) < 1e-12 and of_largest(b[2], a[2]) < 1e-12
	_check(b, a, False, 'three rows at once')
	# the same row twice: the second lies in the span
	lv = levels.CoexLevels(dt, dc).append(rows[0])
	before = lv.results()
	lv.append(rows[0])
	assert lv.rebuilt == [False, False] and lv.rank == 8 and lv.level == 2 and lv.info['rho'][0] <= levels.RHO_SPAN
	assert all(np.array_equal(u, v) for u, v in zip(before, lv.results()))
	# dimreduce passes through to dof
	lv = levels.CoexLevels(dt, dc, dimreduce=2).append(rows[0])
	assert lv.dof == dt.shape[1] - 1 - 8 - 2
	_check(lv.results(), norm.coex(dt, lv.dc, dimreduce=2), False, 'dimreduce = 2')
	# two runs, the same bits
	again = levels.CoexLevels(dt, dc)
	for k in range(3):
		again.append(rows[k])
	assert all(np.array_equal(u, v) for u, v in zip(a, again.results()))


def test_fewest_cells_and_a_nan_row():
	import normalisr_amd.normalisr as norm
	from normalisr_amd import levels
	rng = np.random.default_rng(12)
	n = 6
	dt = rng.standard_normal((5, n))
	dc = np.concatenate([rng.standard_normal((2, n)), np.ones((1, n))])
	lv = levels.CoexLevels(dt, dc)
	lv.append(rng.standard_normal(n))  # n_cell = rank + dimreduce + 2
	assert lv.rank == 4 and lv.dof == 1 and lv.rebuilt == [False]
	_check(lv.results(), norm.coex(dt, lv.dc), False, 'dof = 1')
	before = lv.results()
	with pytest.raises(ValueError, match='Insufficient number of cells'):
		lv.append(rng.standard_normal(n))
	bad = rng.standard_normal(n)
	bad[2] = np.nan
	with pytest.raises(AssertionError):
		lv.append(bad)
	assert lv.level == 1 and lv.rank == 4 and lv.dc.shape == (4, n) and lv.rebuilt == [False]
	assert all(np.array_equal(u, v) for u, v in zip(before, lv.results()))


def test_in_place_rewrite_of_the_expression(golden):
	import normalisr_amd.normalisr as norm
	from normalisr_amd import levels
	dt, dc, rows = _problem_a(golden)
	eng = _engine()
	x = eng.upload(dt)
	lv = levels.CoexLevels(x, dc).append(rows[0])
	_check(lv.results(device_out=True), norm.coex(x, lv.dc, device_out=True), False, 'before the rewrite')
	x.mul_(1.5).add_(eng.upload(np.random.default_rng(3).standard_normal(dt.shape)))
	stale = lv.results(device_out=True)  # results alone notices the rewrite too
	_check(stale, norm.coex(x, lv.dc, device_out=True), False, 'results after the rewrite')
	x.add_(eng.upload(0.5 * rows[1][None, :] * np.random.default_rng(4).standard_normal((dt.shape[0], 1))))
	for k in (1, 2, 3):
		lv.append(rows[k])
		_check(lv.results(device_out=True), norm.coex(x, lv.dc, device_out=True), False, 'level %d after the rewrite' % lv.level)
	assert lv.rebuilt == [False, True, False, False]


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------------------------------
MODULES = (('M1', 0, 20, 1.5), ('M2', 20, 35, 1.2), ('M3', 35, 47, 1.0))
QCUT = 1e-6


def _loop_problem(seed=2024):
	"""60 genes x 800 cells: three latent factors drive three gene modules of 20, 15 and 12 genes with falling strength, 13 genes of noise; gene sets: the modules and
	three sets drawn at random."""
	from normalisr_amd import enrich
	rng = np.random.default_rng(seed)
	ng, n = 60, 800
	fac = rng.standard_normal((3, n))
	dt = rng.standard_normal((ng, n)) + 2.0
	for f, (_, lo, hi, w) in enumerate(MODULES):
		dt[lo:hi] += w * fac[f]
	dc = np.concatenate([rng.standard_normal((1, n)), np.ones((1, n))])
	namet = np.array(['g%02d' % i for i in range(ng)])
	names = [m[0] for m in MODULES] + ['R1', 'R2', 'R3']
	pairs = [(t, namet[i]) for t, (_, lo, hi, _) in enumerate(MODULES) for i in range(lo, hi)]
	pairs += [(3 + t, namet[i]) for t in range(3) for i in rng.choice(ng, 10, replace=False)]
	sets = enrich.GeneSets(names, ['set ' + s for s in names], np.zeros(len(names)), pairs)
	return dt, dc, namet, sets


def _chain(dt, dc, namet, sets, levels_wanted):
	"""The same steps one by one with the public functions, from scratch at every level; asserts that no BH q-value lies within 1e-4 relative of QCUT."""
	import normalisr_amd.normalisr as norm
	from normalisr_amd import binnet, enrich, gocovt
	out, cov = [], dc
	for level in range(levels_wanted):
		p = norm.coex(dt, cov)[0]
		qv = np.concatenate([binnet.bh(row) for row in binnet.nodiag(p, split=True)])
		assert (np.abs(qv / QCUT - 1) > 1e-4).all(), 'a q-value within 1e-4 of the cutoff: choose another seed'
		net = binnet.binnet(p, QCUT)
		principals, res, top, genes = enrich.top_pathway(net, namet, sets, n=10, nmin=3)
		nxt = gocovt.pccovt(dt, cov, namet, genes)
		out.append(dict(cov=cov, net=net, principals=principals, top=top, genes=genes, cov_next=nxt))
		cov = nxt
	return out


def _same_level(rec, want):
	assert rec['principals'] == want['principals'] and rec['top'] == want['top'] and rec['genes'] == want['genes']
	assert np.array_equal(np.asarray(rec['net']), want['net']) and np.asarray(rec['net']).dtype == np.bool_
	assert np.abs(rec['cov'] - want['cov']).max() <= 1e-9 * np.abs(want['cov']).max()
	assert np.abs(rec['cov_next'] - want['cov_next']).max() <= 1e-9 * np.abs(want['cov_next']).max() and rec['cov_next'].shape == want['cov_next'].shape


def test_loop_equals_the_steps_made_one_by_one():
	from normalisr_amd import levels
	dt, dc, namet, sets = _loop_problem()
	want = _chain(dt, dc, namet, sets, 3)
	got = levels.coex_levels(dt, dc, namet, sets, QCUT, lvmax=2, n=10, nmin=3, keep=('net', 'p', 'dot', 'var'))
	assert len(got) == 3 and [r['level'] for r in got] == [0, 1, 2]
	for rec, w in zip(got, want):
		_same_level(rec, w)
		assert rec['rebuilt'] is False and rec['p'].shape == (60, 60) and rec['dot'].shape == (60, 60) and rec['var'].shape == (60, ) and 'stopped' not in rec
		assert rec['result'].top_sets(0) == rec['top']
	assert [r['top'] for r in got] == ['M1', 'M2', 'M3']  # the strongest module first
	assert got[0]['genes'] == list(namet[0:20]) and got[1]['genes'] == list(namet[20:35])
	# the resident form: a tensor in, tensors out
	eng = _engine()
	res = levels.coex_levels(eng.upload(dt), dc, namet, sets.bind(namet), QCUT, lvmax=1, n=10, nmin=3, keep=('net', 'p'), device_out=True)
	assert len(res) == 2 and res[0]['net'].is_cuda and res[0]['p'].is_cuda and 'dot' not in res[0]
	for rec, w in zip(res, want):
		assert np.array_equal(rec['net'].cpu().numpy(), w['net']) and rec['top'] == w['top']
		assert np.abs(rec['cov_next'] - w['cov_next']).max() <= 1e-9 * np.abs(w['cov_next']).max()


def test_loop_stops_where_the_network_is_empty():
	from normalisr_amd import levels
	dt, dc, namet, sets = _loop_problem()
	want = _chain(dt, dc, namet, sets, 3)
	got = levels.coex_levels(dt, dc, namet, sets, QCUT, lvmax=5, n=10, nmin=3, strict=False)
	assert len(got) == 4 and got[3]['stopped'] == 'Empty binary network.' and got[3]['level'] == 3 and 'principals' not in got[3] and 'error' not in got[3]
	assert got[3]['cov'].shape == (5, dt.shape[1])
	for rec, w in zip(got[:3], want):
		_same_level(rec, w)
	with pytest.raises(RuntimeError, match='Empty binary network.'):
		levels.coex_levels(dt, dc, namet, sets, QCUT, lvmax=5, n=10, nmin=3, strict=True)


def test_cli_coex_levels(tmp_path):
	from normalisr_amd import levels, run
	from normalisr_amd.__main__ import main
	dt, dc, namet, sets = _loop_problem()
	f = lambda name: str(tmp_path / name)
	np.save(f('exp.npy'), dt)
	np.save(f('cov.npy'), dc)
	run.file_write_txtlist(f('genes.txt'), list(namet))
	with open(f('sets.gmt'), 'w') as fh:
		for t, name in enumerate(sets.names):
			fh.write('\t'.join([name, sets.labels[t]] + [g for s, g in sets.pairs if s == t]) + '\n')
	assert main(['coex_levels', f('exp.npy'), f('cov.npy'), f('genes.txt'), str(QCUT), f('out'), '--gmt', f('sets.gmt'), '-l', '2', '-n', '10', '-m', '3', '--ext', '.npy',
				 '--pv', '--var']) == 0
	got = levels.coex_levels(dt, dc, namet, sets, QCUT, lvmax=2, n=10, nmin=3, keep=('net', 'p', 'var'))
	o = lambda name: os.path.join(f('out'), name)
	for rec in got:
		k = rec['level']
		assert list(run.file_read_txtlist(o('lv%d_master.txt' % k))) == rec['principals']
		assert list(run.file_read_txtlist(o('lv%d_pathway.txt' % k))) == rec['genes']
		assert list(run.file_read_txtlist(o('lv%d_go.txt' % k))) == [rec['top']]
		net = np.load(o('lv%d_net.npy' % k))
		assert net.dtype == np.uint8 and np.array_equal(net != 0, rec['net'])
		assert np.array_equal(np.load(o('lv%d_cov.npy' % (k + 1))), rec['cov_next'])
		assert np.array_equal(np.load(o('lv%d_pv.npy' % k)), rec['p']) and np.array_equal(np.load(o('lv%d_var.npy' % k)), rec['var'])
		assert not os.path.exists(o('lv%d_dot.npy' % k))
		with open(o('lv%d_goe.tsv' % k)) as fh:
			lines = fh.read().splitlines()
		assert lines[0].split('\t')[0] == 'name' and len(lines) == 1 + len(sets.names) and lines[1].split('\t')[7] == rec['top']
	assert not os.path.exists(o('lv0_cov.npy')) and not os.path.exists(o('lv4_cov.npy'))
