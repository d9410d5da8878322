"""GPU: norm.ComputeVarPlan with 64 .. 1024 covariates -- orthonormal bases from the host once, per iteration (B u)(B u)^T on the fp64 matrix cores and its inverse by
csrc/nrm_chol_inverse.hip, the wide entries of csrc/nrm_fitvar_plan.hip around them, one stream, one HIP graph -- against the numpy restatement
tests/front_numpy.py, what the reference returned for G22, and the public norm.compute_var on the same tensor: relerr(., ., 1.0) < 1e-9, the tolerance the public
wide call is held to (tests/test_gpu_wide_covariates.py).  Bit equality where the same kernels run on the same values.  Stage level: nrm_fitvar_wide_design against
numpy's one-operation results bit for bit, nrm_fitvar_wide_update's coefficients within the bound of a sum of n products in any order, n u sum |B1| |l|."""
import numpy as np
import pytest

import front_numpy
from conftest import relerr
from test_gpu_compute_var_plan import _problem, _t1s
from test_gpu_wide_covariates import g22, small_cases  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
U = 2.0**-53
TOL, SAFETY = 1e-8, 4.0


def ok(a, b):
	return relerr(a, b, 1.0) < 1e-9


@pytest.fixture(scope='module')
def norm():
	import normalisr_amd.normalisr as norm
	return norm


@pytest.fixture(scope='module')
def torch():
	import torch
	return torch


@pytest.fixture(scope='module')
def Plan():
	from normalisr_amd.norm import ComputeVarPlan
	return ComputeVarPlan


@pytest.fixture(scope='module')
def lib():
	from normalisr_amd import _lib
	return _lib.load()


def _scales(dt, dc, steps):
	"""The scale after every iteration of front_numpy.compute_var."""
	dt, dc = np.asarray(dt, dtype=np.float64), np.asarray(dc, dtype=np.float64)
	ns = dt.shape[1]
	c1 = np.vstack([dc, np.ones((1, ns))])
	s, out = np.ones(ns), []
	for _ in range(steps):
		y, c = dt / s, dc / s
		r = y - front_numpy._project(c, y)
		r = (r.T - r.mean(axis=1)).T
		r = (r.T / np.sqrt((r**2).mean(axis=1))).T
		z = np.log(np.sqrt((r**2).mean(axis=0)))
		s = np.exp(front_numpy._project(c1, z[None, :])[0]) * s
		s = s / s.min()
		out.append(s)
	return out


@pytest.mark.parametrize('nc', (64, 65, 131))
def test_wide_plan_small_cases(norm, torch, Plan, small_cases, nc):
	from normalisr_amd.association import inv_rank
	dt32, dc, ref = small_cases[nc]
	rank = inv_rank(dc @ dc.T)[1]
	for dt in (dt32, dt32.astype(np.float64)):
		d = torch.as_tensor(dt).cuda()
		for steps in (1, 3):
			plan = Plan(d, dc, stepmax=steps)
			assert plan.wide and plan.rank == rank and (rank < nc) == (nc == 131)  # (131: each of the three one-hot factors sums to the intercept)
			dw = plan.step()
			w = plan.results()
			pub = norm.compute_var(d, dc, stepmax=steps)
			print(nc, dt.dtype, steps, 'restatement', relerr(w, ref[steps], 1.0), 'public call', relerr(w, pub, 1.0), 'steps taken', plan.steps_taken)
			assert dw is plan.w and w.shape == (403, ) and w.min() == 1.0 and plan.steps_taken == steps
			assert ok(w, ref[steps]) and ok(w, pub)


def test_wide_plan_g22_against_the_reference(norm, torch, Plan, g22):
	for case in ('A', 'B', 'C'):  # 113, 384 and 70 covariates
		d = g22[case]
		for dt in (d['dt'], d['dt'].astype(np.float64)):
			dev = torch.as_tensor(dt).cuda()
			for steps, key in ((1, 'w1'), (3, 'w3')):
				plan = Plan(dev, d['dc'], stepmax=steps)
				plan.step()
				w = plan.results()
				pub = norm.compute_var(dev, d['dc'], stepmax=steps)
				print(case, dt.dtype, steps, 'reference', relerr(w, d[key], 1.0), 'public call', relerr(w, pub, 1.0), 'rank', plan.rank)
				assert plan.rank == d['ranks'][0]
				assert ok(w, d[key]) and ok(w, pub)


def test_wide_plan_stop_rule_on_the_device(torch, Plan, small_cases):
	dt32, dc, ref = small_cases[65]
	lc = dt32.astype(np.float64)
	d = torch.as_tensor(lc).cuda()

	def run(**ka):
		plan = Plan(d, dc, **ka)
		plan.step()
		return plan.results(), plan
	w1, p1 = run(stepmax=1)
	assert p1.steps_taken == 1
	ws, ps = run(stepmax=3, eps=1e3)  # the first step's change is below 1e3: the two iterations enqueued after it must leave everything as it is
	assert ps.steps_taken == 1 and np.array_equal(ws, w1) and ps.best_change == p1.best_change
	w3, p3 = run(stepmax=3, eps=1e-300)
	assert p3.steps_taken == 3
	t1 = _t1s(lc, dc, 3)
	print('t1 per iteration', t1, 'best change of the plan: 1 step %.17g, 3 steps %.17g' % (p1.best_change, p3.best_change))
	assert abs(p1.best_change / t1[0] - 1) <= 1e-6 and abs(p3.best_change / min(t1) - 1) <= 1e-6
	assert ok(w3, front_numpy.compute_var(lc, dc, stepmax=3, eps=1e-300))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_wide_plan_same_bits_run_to_run_and_eager_capture_replay(torch, Plan, small_cases, dtype):
	dt32, dc, ref = small_cases[131]
	d = torch.as_tensor(dt32.astype(dtype)).cuda()
	a, b = Plan(d, dc, stepmax=2), Plan(d.clone(), dc.copy(), stepmax=2)
	a.step(), b.step()
	first = a.results()
	assert np.array_equal(first, b.results())
	for k in range(2, 6):  # step 2 captures, 3 and later replay
		assert a.step() is a.w
		assert np.array_equal(a.results(), first), k
		if k >= 3:
			assert a._graph.graph is not None
	assert a._graph.enabled and a._graph.calls == 5


def test_wide_plan_follows_in_place_rewrites_with_one_graph(norm, torch, Plan, small_cases):
	rng = np.random.default_rng(78)
	dt32, dc, ref = small_cases[64]
	lc = dt32.astype(np.float64)
	d = torch.as_tensor(lc).cuda()
	plan = Plan(d, dc, stepmax=2)
	for _ in range(4):
		plan.step()
	g0 = plan._graph.graph
	before = plan.results()
	assert g0 is not None and ok(before, norm.compute_var(d, dc, stepmax=2))
	new = lc[rng.permutation(lc.shape[0])] + 0.3 * rng.normal(size=lc.shape) * rng.uniform(0.5, 2.0, lc.shape[1])
	d.data.copy_(torch.as_tensor(new).cuda())  # (.data: a write torch's version counter does not see, as a kernel of another library's would be)
	last = None
	for k in range(3):
		plan.step()
		w = plan.results()
		assert plan._graph.graph is g0 and plan._graph.enabled
		assert ok(w, front_numpy.compute_var(new, dc, stepmax=2)), k
		assert last is None or np.array_equal(w, last), k
		last = w
	assert ok(last, norm.compute_var(d, dc, stepmax=2)) and not np.array_equal(last, before)


def test_wide_plan_constant_gene(norm, torch, Plan, small_cases):
	dt32, dc, ref = small_cases[65]
	lc = dt32.astype(np.float64)
	d = torch.as_tensor(lc).cuda()
	plan = Plan(d, dc)
	for _ in range(3):
		plan.step()
	assert plan.check() and plan._graph.graph is not None
	d.data[9] = 0.0  # the covariates explain a constant row exactly: its residual is constant, its spread zero
	plan.step()
	with pytest.raises(AssertionError):
		plan.check()
	plan.step()
	with pytest.raises(AssertionError):
		plan.results()
	d.data[9] = torch.as_tensor(lc[9]).cuda()  # repaired in place
	plan.step()
	assert plan.check() and ok(plan.results(), ref[1])


def test_wide_plan_refuses_weights_beyond_the_certificate(torch, Plan):
	"""Cells whose noise follows a covariate, and a covariate in units of 1e-3 (its eigenvalue of dc dc^T, the smallest kept, is about 1e-6 of the largest): after
	the first iteration the fitted scale spreads so far that (u_max / u_min)^2 exceeds hi / (safety tol) -- the reference's rank rule may then drop a direction
	the basis keeps.  One iteration (equal weights) is fine; the second is counted on the device and check() names compute_var() as the call."""
	from normalisr_amd.norm import _fitvar_bases
	rng = np.random.default_rng(2350)
	n, nc = 500, 64
	x = rng.uniform(-1, 1, n)
	dc = np.vstack([(x - x.mean()) / x.std(), 1e-3 * rng.normal(size=(1, n)), rng.normal(size=(nc - 3, n)), np.ones((1, n))])
	dt = rng.normal(size=(40, n)) * np.exp(5.0 * x) + 3.0
	hi = _fitvar_bases(dc)[2]
	s1 = _scales(dt, dc, 1)[0]
	kappa = (s1.max() / s1.min())**2
	print('hi', hi, 'kappa after the first iteration', kappa, 'limit', hi / (SAFETY * TOL))
	assert kappa > hi / (SAFETY * TOL)
	d = torch.as_tensor(dt).cuda()
	one = Plan(d, dc, stepmax=1)
	one.step()
	assert one.check() and ok(one.results(), front_numpy.compute_var(dt, dc, stepmax=1))
	two = Plan(d, dc, stepmax=2, eps=1e-300)
	two.step()
	with pytest.raises(NotImplementedError, match=r'compute_var\(\)'):
		two.check()
	two.step()
	with pytest.raises(NotImplementedError, match=r'compute_var\(\)'):
		two.results()


def test_wide_plan_refuses_a_nearly_duplicated_row_when_the_weights_spread(norm, torch, Plan, g22):
	"""The case of test_normvar_without_a_certificate_takes_the_reference_path (tests/test_chol_inverse_cpu.py: certified for equal weights, lo = 1.60e-9): the
	first iteration runs, the second has kappa above tol / (safety lo) = 1.56 and is refused by the device's certificate."""
	from normalisr_amd.norm import _fitvar_bases
	d = g22['C']
	dc = d['dc'].astype(np.float64)
	near = np.vstack([dc, dc[3] + 1e-4 * np.random.default_rng(2222).normal(size=dc.shape[1])])
	lo = _fitvar_bases(near)[3]
	s1 = _scales(d['dt'], near, 1)[0]
	kappa = (s1.max() / s1.min())**2
	print('lo', lo, 'kappa after the first iteration', kappa, 'limit', TOL / (SAFETY * lo))
	assert kappa > TOL / (SAFETY * lo)
	dev = torch.as_tensor(d['dt']).cuda()
	one = Plan(dev, near, stepmax=1)
	one.step()
	assert one.check() and ok(one.results(), norm.compute_var(dev, near, stepmax=1))
	three = Plan(dev, near, stepmax=3)
	three.step()
	with pytest.raises(NotImplementedError, match=r'compute_var\(\)'):
		three.check()


def test_narrow_plan_runs_the_launches_it_ran(torch, Plan, lib, small_cases):
	"""63 covariates: the plan's weights are the bits of the launch list the plan had before it took more (design, pinv, moments, genes, cells, update per
	iteration, then the weights), enqueued here on the test's own buffers."""
	from normalisr_amd import _lib
	from normalisr_amd.norm import _pinv_gram_unit_rows
	dt32, dc, ref = small_cases[63]
	y = torch.as_tensor(dt32).cuda()
	steps = 3
	plan = Plan(y, dc, stepmax=steps)
	assert not plan.wide
	plan.step()
	want = plan.results()
	nt, ns = y.shape
	nc = dc.shape[0]
	f64 = dict(dtype=torch.float64, device='cuda')
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()
	c, m2i = up(dc), up(_pinv_gram_unit_rows(np.vstack([dc, np.ones((1, ns))])))
	a, b = torch.empty((nt, nc), **f64), torch.empty((nt, nc), **f64)
	mean, sc, v = torch.empty((nt, ), **f64), torch.empty((nt, ), **f64), torch.empty((ns, ), **f64)
	part = torch.empty((-(-nt // int(lib.nrm_fitvar_row_tile())), ns), **f64)
	s, best, u = torch.empty((ns, ), **f64), torch.empty((ns, ), **f64), torch.empty((ns, ), **f64)
	cw, mi = torch.empty((nc, ns), **f64), torch.empty((nc, nc), **f64)
	rank = torch.empty((1, ), dtype=torch.int64, device='cuda')
	ws = torch.empty((int(lib.nrm_fitvar_plan_workspace(ns, nc)), ), **f64)
	state, w = torch.empty((steps + 1, 4), **f64), torch.empty((ns, ), **f64)
	flags = torch.zeros((4, ), dtype=torch.int32, device='cuda')
	st, p = torch.cuda.current_stream().cuda_stream, lambda t: t.data_ptr()
	_lib.check(lib.nrm_fitvar_plan_start(ns, p(s), p(best), p(state[0]), st))
	for i in range(steps):
		now, nxt = p(state[i]), p(state[i + 1])
		_lib.check(lib.nrm_fitvar_design(p(c), nc, c.stride(0), ns, p(s), now, 1e-6, p(u), p(cw), p(ws), st))
		_lib.check(lib.nrm_fitvar_pinv(ns, nc, 1E-8, now, 1e-6, p(ws), p(mi), p(rank), st))
		_lib.check(lib.nrm_fitvar_moments(p(y), 0, nt, ns, y.stride(0), p(cw), nc, cw.stride(0), p(a), st))
		_lib.check(lib.nrm_fitvar_genes(p(y), 0, nt, ns, y.stride(0), p(u), p(c), nc, c.stride(0), p(a), p(mi), p(b), p(mean), p(sc), p(flags), st))
		_lib.check(lib.nrm_fitvar_cells(p(y), 0, nt, ns, y.stride(0), p(u), p(c), nc, c.stride(0), p(b), p(mean), p(sc), p(part), p(v), st))
		_lib.check(lib.nrm_fitvar_update(p(v), p(c), nc, c.stride(0), ns, p(m2i), p(s), p(best), now, nxt, 1e-6, p(ws), st))
	_lib.check(lib.nrm_fitvar_weights(p(best), ns, p(ws), p(w), p(flags), st))
	torch.cuda.synchronize()
	assert np.array_equal(w.cpu().numpy(), want) and (flags.cpu().numpy() == 0).all()
	assert ok(want, ref[steps])


@pytest.mark.parametrize('n', (403, 1025))
@pytest.mark.parametrize('r', (64, 129))
def test_wide_design_stage(torch, lib, n, r):
	"""u = 1 / s, Bu = B u (padded with zeros to 128 rows and 16 cells), cw = (B u) u: numpy's one-operation results, bit for bit; the certificate counter for
	limits on both sides of the weights' kappa; nothing is touched once the stop test has failed."""
	from normalisr_amd import _lib
	rng = np.random.default_rng(2360 + n + r)
	b = rng.normal(size=(r, n)) * 10.0**rng.integers(-3, 3, (r, 1))
	s = np.exp(rng.normal(0, 0.5, n))
	u = 1 / s
	kappa = (u.max() / u.min())**2
	rp, kp = -(-r // 128) * 128, -(-n // 16) * 16
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()
	d_b, d_s = up(b), up(s)
	f64 = dict(dtype=torch.float64, device='cuda')
	size = int(lib.nrm_fitvar_wide_workspace(n, r, r + 1))
	assert size > 0
	ws = torch.empty((size, ), **f64)
	st = torch.cuda.current_stream().cuda_stream

	def run(state0, hi, lo, full, fill):
		state = up([state0, 0.0, np.nan, 0.0])
		d_u, d_bu, d_cw = torch.full((n, ), fill, **f64), torch.full((rp, kp), fill, **f64), torch.full((r, n), fill, **f64)
		flags = torch.zeros((8, ), dtype=torch.int32, device='cuda')
		_lib.check(lib.nrm_fitvar_wide_design(d_b.data_ptr(), r, n, n, d_s.data_ptr(), state.data_ptr(), 1e-6, hi, lo, TOL, SAFETY, full, d_u.data_ptr(), d_bu.data_ptr(), rp, kp,
											  d_cw.data_ptr(), ws.data_ptr(), flags.data_ptr(), st))
		torch.cuda.synchronize()
		return d_u.cpu().numpy(), d_bu.cpu().numpy(), d_cw.cpu().numpy(), list(flags.cpu().numpy())
	edge = SAFETY * TOL * kappa
	gu, gbu, gcw, flags = run(1e300, edge * (1 + 1e-9), 0.0, 1, np.nan)
	bu = np.zeros((rp, kp))
	bu[:r, :n] = b * u
	assert np.array_equal(gu, u) and np.array_equal(gbu, bu) and np.array_equal(gcw, (b * u) * u)
	assert flags == [0] * 8
	assert run(1e300, edge * (1 - 1e-9), 0.0, 1, np.nan)[3] == [0, 0, 1, 0, 0, 0, 0, 0]  # the smallest kept eigenvalue too close to the rule's tolerance
	low = TOL / (SAFETY * kappa)
	assert run(1e300, 1.0, low * (1 - 1e-9), 0, np.nan)[3] == [0] * 8
	assert run(1e300, 1.0, low * (1 + 1e-9), 0, np.nan)[3] == [0, 0, 1, 0, 0, 0, 0, 0]  # the largest dropped one too close
	assert run(1e300, 1.0, low * (1 + 1e-9), 1, np.nan)[3] == [0] * 8  # (full rank: nothing is dropped)
	gu, gbu, gcw, flags = run(1e-7, edge * (1 - 1e-9), 0.0, 1, 5.0)  # stopped: bestv <= eps
	assert (gu == 5.0).all() and (gbu == 5.0).all() and (gcw == 5.0).all() and flags == [0] * 8


@pytest.mark.parametrize('n,r1', ((403, 65), (1025, 130), (2500, 66)))
def test_wide_update_stage(torch, lib, n, r1):
	"""coef = B1 log sqrt v: per-chunk partial sums added in order, whatever their order within n u sum |B1| |l| of the extended-precision sum; then the new scale,
	its minimum, the change and the state record against numpy."""
	from normalisr_amd import _lib
	rng = np.random.default_rng(2370 + n)
	b1 = np.linalg.qr(rng.normal(size=(n, r1)))[0].T.copy()
	v = np.exp(rng.normal(0, 1.0, n))
	s = np.exp(rng.normal(0, 0.3, n))
	up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()
	d_b1, d_v, d_s = up(b1), up(v), up(s)
	best = up(np.full(n, np.nan))
	state = up([[1e300, 0.0, np.nan, 0.0], [0.0] * 4])
	ws = torch.zeros((int(lib.nrm_fitvar_wide_workspace(n, r1 - 1, r1)), ), dtype=torch.float64, device='cuda')
	_lib.check(lib.nrm_fitvar_wide_update(d_v.data_ptr(), d_b1.data_ptr(), r1, n, n, d_s.data_ptr(), best.data_ptr(), state[0].data_ptr(), state[1].data_ptr(), 1e-6,
										  ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
	torch.cuda.synchronize()
	off = 2 * (-(-n // 256)) + (-(-n // 1024)) * r1  # the coefficients' place in the scratch (include/normalisr_hip.h)
	coef = ws.cpu().numpy()[off:off + r1]
	l = np.log(np.sqrt(v))
	exact = b1.astype(np.longdouble) @ l.astype(np.longdouble)
	bound = n * U * (np.abs(b1) @ np.abs(l))
	err = np.abs(coef - exact).astype(np.float64)
	print('n', n, 'r1', r1, 'largest coefficient error / bound', (err / bound).max())
	assert (err <= bound).all()
	new = np.exp(b1.T @ coef) * s
	new /= new.min()
	t1 = np.abs((new - s) / s).max()
	gs, gbest, gstate = d_s.cpu().numpy(), best.cpu().numpy(), state.cpu().numpy()
	assert relerr(gs, new, 0.0) < 1e-12 and np.array_equal(gs, gbest) and gs.min() == 1.0
	assert gstate[1][1] == 1.0 and abs(gstate[1][0] / t1 - 1) < 1e-9 and gstate[1][0] == gstate[1][2]
