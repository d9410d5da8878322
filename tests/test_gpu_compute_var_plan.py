"""GPU: norm.ComputeVarPlan -- compute_var on a resident logCPM matrix with every iteration, the stop rule and the weights on the device (csrc/nrm_fitvar_plan.hip),
one HIP graph per step -- against what the reference returned for golden G18, the numpy restatement tests/front_numpy.py and the public norm.compute_var on the
same tensor.  Tolerance: close(1e-9, floor=1), the project's bound for fp64 quantities that are not P-values; bit equality where the same kernels run on the
same values (run to run, eager / capture / replay, the stop rule).  No timing here (tests/test_zz_compute_var_plan_perf_gpu.py)."""
import numpy as np
import pytest

import front_numpy
from test_gpu_parity import close

pytestmark = pytest.mark.gpu


def ok(a, b):
	return close(a, b, 1e-9, floor=1.0)


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


def _counts(rng, ng, n, big=None):
	mu = np.exp(rng.normal(-0.8, 1.2, ng))
	x = rng.poisson(mu[:, None] * np.exp(rng.normal(0, 0.4, n))[None, :]).astype(np.int64)
	empty = x.sum(axis=0) == 0
	x[rng.integers(0, ng, n)[empty], np.nonzero(empty)[0]] = 1  # every cell has a read
	if big is not None:
		x[ng // 2, n // 3] = big
	return x


SHAPES = [  # tests/test_gpu_front.py: genes, cells, covariates (the last is the intercept), largest count forced, one-hot batches among the covariates
	(1, 64, 1, None, 0), (7, 13, 2, None, 0), (33, 65, 3, None, 0), (100, 1023, 8, None, 4), (129, 1025, 9, None, 0), (64, 257, 21, None, 4),
	(40, 4099, 5, None, 0), (300, 130, 4, None, 3), (50, 200, 1, None, 0), (20, 300, 63, None, 0), (30, 100, 3, 10**6, 0), (16, 1024, 2, None, 0),
	(45, 250, 26, 70000, 5),
]


def _problem(ng, n, nc, big, nb):
	rng = np.random.default_rng(1000 * ng + n + nc)
	x = _counts(rng, ng, n, big)
	lc = front_numpy.lcpm(x)[0]
	batch = rng.integers(0, max(nb, 1), n)
	rows = [(batch[None, :] == np.arange(nb)[:, None]).astype(np.float64)] if nb else []
	dc = np.vstack(rows + [rng.normal(size=(nc - 1 - nb, n)), np.ones((1, n))])
	assert dc.shape[0] == nc
	return lc, dc


def _t1s(dt, dc, steps):
	"""The maximum relative change of the scale in every iteration of front_numpy.compute_var (its loop, with t1 kept)."""
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
		new = np.exp(front_numpy._project(c1, z[None, :])[0]) * s
		new /= new.min()
		out.append(np.abs((new - s) / s).max())
		s = new
	return out


@pytest.mark.parametrize('steps,key', [(1, 'w1'), (3, 'w3')])
def test_g18_compute_var_plan(golden, torch, Plan, steps, key):
	g, h = golden('G18_front'), golden('G18_front_chain')
	lc, dc = g['lcpm'], h['normcov_c']
	lc32 = lc.astype(np.float32)
	for name, dt, ref in (('fp64', lc, h[key]), ('fp32', lc32, front_numpy.compute_var(lc32.astype(np.float64), dc, stepmax=steps))):
		plan = Plan(torch.as_tensor(dt).cuda(), dc, stepmax=steps)
		dw = plan.step()
		assert dw is plan.w and dw.is_cuda and dw.dtype == torch.float64 and tuple(dw.shape) == (lc.shape[1], )
		w = plan.results()
		print(name, steps, 'weights max relative error %.3g' % np.abs(w / ref - 1).max(), 'steps taken', plan.steps_taken, 'best change %.3g' % plan.best_change)
		assert isinstance(w, np.ndarray) and w.shape == (lc.shape[1], ) and w.dtype == np.float64 and w.min() == 1 and ok(w, ref), (name, steps)
		assert np.array_equal(w, dw.cpu().numpy())


@pytest.mark.parametrize('ng,n,nc,big,nb', [s for s in SHAPES if s[0] > 1])
def test_plan_random_shapes_against_numpy_and_the_public_call(norm, torch, Plan, ng, n, nc, big, nb):
	lc, dc = _problem(ng, n, nc, big, nb)
	wide = torch.zeros((ng, n + 3), dtype=torch.float64, device='cuda')
	wide[:, 1:n + 1] = torch.as_tensor(lc).cuda()
	for steps in (1, 2):
		wr = front_numpy.compute_var(lc, dc, stepmax=steps)
		for name, dt in (('contiguous', torch.as_tensor(lc).cuda()), ('unaligned rows', wide[:, 1:n + 1])):  # (the last: rows that start on no 16-byte boundary)
			plan = Plan(dt, dc, stepmax=steps)
			plan.step()
			w = plan.results()
			pub = norm.compute_var(dt, dc, stepmax=steps)
			print(ng, n, nc, steps, name, 'max relative error: numpy %.3g, public call %.3g' % (np.abs(w / wr - 1).max(), np.abs(w / pub - 1).max()))
			assert w.shape == (n, ) and w.min() == 1 and ok(w, wr) and ok(w, pub), (name, steps)


def test_plan_stop_rule_on_the_device(torch, Plan):
	lc, dc = _problem(100, 1023, 8, None, 4)
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
def test_plan_same_bits_run_to_run_and_eager_capture_replay(torch, Plan, dtype):
	lc, dc = _problem(129, 1025, 9, None, 0)
	d = torch.as_tensor(lc.astype(dtype)).cuda()
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


def test_plan_follows_in_place_rewrites_with_one_graph(norm, torch, Plan):
	"""Nothing is decided on the host, so the graph captured on the first values is the graph of every later step (tests/test_gpu_plan_rewrites.py: the
	plans that decide on the host must capture anew)."""
	rng = np.random.default_rng(77)
	lc, dc = _problem(300, 130, 4, None, 3)
	d = torch.as_tensor(lc).cuda()
	plan = Plan(d, dc, stepmax=2)
	for _ in range(4):
		plan.step()
	g0 = plan._graph.graph
	assert g0 is not None and ok(plan.results(), norm.compute_var(d, dc, stepmax=2))
	before = plan.results()
	new = lc[rng.permutation(lc.shape[0])] + 0.3 * rng.normal(size=lc.shape) * rng.uniform(0.5, 2.0, lc.shape[1])
	d.data.copy_(torch.as_tensor(new).cuda())  # (.data: a write torch's version counter does not see, as a kernel of another library's would be)
	last = None
	for k in range(5):
		plan.step()
		w = plan.results()
		assert plan._graph.graph is g0 and plan._graph.enabled
		assert ok(w, norm.compute_var(d, dc, stepmax=2)) and ok(w, front_numpy.compute_var(new, dc, stepmax=2)), k
		assert last is None or np.array_equal(w, last), k
		last = w
	assert not np.array_equal(last, before)


def test_plan_errors_from_the_device_counters(norm, torch, Plan):
	rng = np.random.default_rng(3)
	x = _counts(rng, 40, 90)
	lc = front_numpy.lcpm(x)[0]
	dc = np.vstack([rng.normal(size=(2, 90)), np.ones((1, 90))])
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
	assert plan.check() and ok(plan.results(), norm.compute_var(d, dc))


def test_plan_step_has_no_host_work(torch, Plan):
	"""The whole step -- three iterations, the stop rule, the weights -- is captured in a graph of the test's own: a synchronisation or a read-back inside it
	would end the capture with an error.  And the plan's own StepGraph captured without falling back to eager."""
	lc, dc = _problem(64, 257, 21, None, 4)
	d = torch.as_tensor(lc).cuda()
	plan = Plan(d, dc, stepmax=3, eps=1e-300)
	for _ in range(3):
		plan.step()
	assert plan._graph.enabled and plan._graph.graph is not None
	want = plan.results()
	other = Plan(d, dc, stepmax=3, eps=1e-300)
	other._launch()  # (warm-up: the kernels' code objects are loaded)
	torch.cuda.synchronize()
	g = torch.cuda.CUDAGraph()
	with torch.cuda.graph(g):
		other._launch()
	other.w.zero_()
	g.replay()
	assert np.array_equal(other.results(), want) and other.steps_taken == 3
