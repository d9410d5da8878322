"""The child side of tests/test_gpu_de_plan.py: a process in which torch cannot be imported makes every call on the library's resident de plan
(normalisr_amd.cplan.DePlan over nrm_de_plan_*) and writes what it got to an .npz; the parent compares.  `python tests/de_plan_child.py SCENARIO IN.npz OUT.npz`.
The input generators at the top are shared with the parent (which imports this module; nothing here touches torch); the frame of the child, the design forms and
the cases / replays / handback scenarios are those of tests/cabi_harness.py."""
import sys

import numpy as np

import cabi_harness as h

ROOT, KEYS = h.ROOT, h.KEYS


def screen(seed, dtype, nc, intercept=True, valued=False, full_rows=False, nx=70, ny=64, n=4100, const_rows=(9, )):
	"""The screen of tests/test_gpu_design_csr.py::_screen -- 70 design rows (two slot groups, one ragged), 64 genes, 4100 cells (three chunks of 2048, the last
	ragged), one entry in a hundred, row 9 constant -- with valued entries, other covariate sets and other sizes on request.  full_rows: row 11 holds two values
	in every cell (kept), row 12 one value (dropped)."""
	rng = np.random.default_rng(seed)
	dg = (rng.random((nx, n)) < 0.01).astype(np.float64)
	if valued:
		dg *= rng.uniform(0.5, 2.0, (nx, n))
	for r in const_rows:
		dg[r] = 0
	if full_rows:
		dg[11] = 1.0 + (rng.random(n) < 0.5)
		dg[12] = 2.0
	dt = (rng.normal(size=(ny, n)) + 0.5 * dg[0] + 0.4 * dg[1]).astype(dtype)
	if nc == 0:
		dc = np.zeros((0, n))
	elif intercept:
		dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	else:
		dc = rng.normal(size=(nc, n))
	return dg, dt, dc


def small_screen(nc, intercept, dtype='float32'):
	"""5 design rows x 19 genes x 130 cells: six entries in each design row but row 3, which is empty (de drops it).  The 24 entries of the 4 x 130 rows kept are fewer
	than one in sixteen, the density up to which the whole-problem entry takes the sparse-design kernels -- once it gets there: with so few rows and covariates
	(nx + nc <= 32) it takes the streaming kernel first unless NRM_DE_PATH=general, and the size rule wants NRM_DE_SPARSE=force."""
	rng = np.random.default_rng([61, nc])
	dg = np.zeros((5, 130))
	for i in (0, 1, 2, 4):
		dg[i, rng.choice(130, 6, replace=False)] = 1.0
	dt = (rng.normal(size=(19, 130)) + 0.5 * dg[0]).astype(dtype)
	dc = np.vstack([rng.normal(size=(nc - 1, 130)), np.ones((1, 130))]) if intercept else rng.normal(size=(nc, 130))
	return dg, dt, dc


def handback_inputs():
	"""The design of tests/test_gpu_round5.py:199-206: row 5 all but equal to a batch covariate, 40 x 70 x 6000."""
	rng = np.random.default_rng(77)
	nx, ny, n = 40, 70, 6000
	batch = (rng.random(n) < 0.03).astype(np.float64)
	dc = np.vstack([batch, rng.normal(size=(1, n)), np.ones((1, n))])
	dx = (rng.random((nx, n)) < 0.02).astype(np.float64)
	dx[5] = batch * (1.0 + 1e-6 * rng.normal(size=n))
	dy = rng.normal(size=(ny, n))
	dy[3] += 3e6 * (dx[5] - batch)
	return dx, dy, dc


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
def _inputs(c, arr):
	if 'small' in c:
		return small_screen(**c['small'])
	if 'screen' in c:
		s = dict(c['screen'])
		s['dtype'] = np.dtype(s['dtype'])
		return screen(**s)
	dg = arr[c['dg']]
	if c.get('dg_dtype'):
		dg = dg.astype(c['dg_dtype'])
	return dg, arr[c['dt']], arr[c['dc']]


def scenario_cases(job, arr, out, lib, _lib, cplan):
	return h.cases(cplan.DePlan, job, arr, out, _inputs, pinv=True)


def scenario_replays(job, arr, out, lib, _lib, cplan):
	"""Three steps, update(dt2) and two more, set_design(dg2) and two more (cabi_harness.replays)."""
	s = dict(job['screen'])
	s['dtype'] = np.dtype(s['dtype'])
	dg2, dt2, _ = screen(**dict(s, seed=s['seed'] + 1, const_rows=(20, 33)))
	return h.replays(cplan.DePlan, ('step', 'step', 'step', 'update', 'step', 'design', 'step'), screen(**s), (dg2, dt2), job['design_form'], out)


def scenario_handback(job, arr, out, lib, _lib, cplan):
	return h.handback(cplan.DePlan, handback_inputs(), out)


def scenario_bounds(job, arr, out, lib, _lib, cplan):
	s = dict(job['screen'])
	s['dtype'] = np.dtype(s['dtype'])
	dg, dt, dc = screen(**s)
	bad = dt.copy()
	bad[3, 7] = np.nan
	notes = {}
	with cplan.DePlan(dg, bad, dc) as plan:
		plan.step().step().step()
		notes['nan'] = h.raised(plan.check, catch=AssertionError)
		plan.update(dt).step()
		notes['clean_check'] = plan.check()
		h.store(out, 'after_nan', plan.results())
		notes['after_nan'] = plan.info()
	with cplan.DePlan(dg, dt, dc) as plan:
		h.store(out, 'fresh', plan.step().results())
	return notes


if __name__ == '__main__':
	h.child_main(sys.argv, globals())
