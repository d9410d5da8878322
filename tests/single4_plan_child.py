"""The child side of tests/test_gpu_single4_plan.py: a process in which torch cannot be imported makes every call on the library's resident single=4 plan
(normalisr_amd.cplan.Single4Plan over nrm_single4_plan_*) and writes what it got to an .npz; the parent compares.
`python tests/single4_plan_child.py SCENARIO IN.npz OUT.npz`.  The screen is tests/single1_plan_child.py::screen; the frame of the child, the design forms, the device copies, the
result keys and the cases / replays / handback scenarios are those of tests/cabi_harness.py.  What the top of this file defines is shared with the parent and with tests/test_single4_plan_cpu.py (which import this
module; nothing here touches torch)."""
import ctypes
import sys

import numpy as np

import cabi_harness as h
import single1_plan_child as s1c

ROOT, KEYS = h.ROOT, h.KEYS
NX, NY, N, NG0 = s1c.NX, s1c.NY, s1c.N, s1c.NG0
ZERO_ROW, ONES_ROW = s1c.ZERO_ROW, s1c.ONES_ROW
NCS = s1c.NCS
SEED = 100  # the screens are single1_plan_child.screen(SEED + nc, float64, nc)
PLANTED_GENE, HANDBACK_NC = 7, 3
TOL = 1e-8
kept_rows = s1c.kept_rows


def screen(nc, dtype=np.float64, seed=None):
	return s1c.screen(SEED + nc if seed is None else seed, np.dtype(dtype), nc)


def second_screen(nc, dtype=np.float64):
	"""Another design and other expression values of the same shape (update, set_design)."""
	return screen(nc, dtype, seed=SEED + 50 + nc)


def planted_row():
	"""An expression row all but inside the span of an intercept: 100 + 0.5 N(0, 1), |y~|^2 / |y|^2 = 2.4e-5 < 1e-4."""
	return 100.0 + 0.5 * np.random.default_rng(4).normal(size=N)


def handback_screen():
	dg, dt, dc = screen(HANDBACK_NC)
	dt = dt.copy()
	dt[PLANTED_GENE] = planted_row()
	return dg, dt, dc


def onehot_covariates():
	"""Three one-hot batches and an intercept (rank 3 of 4), and a design whose row 5 is the second batch's indicator."""
	batch = np.random.default_rng(6).integers(0, 3, N)
	return np.vstack([(batch[None, :] == np.arange(3)[:, None]).astype(np.float64), np.ones((1, N))])


def refused_designs():
	"""(covariates, {name: design}) the plan refuses: a design row copied from a one-hot covariate; two equal design rows."""
	dg, _, _ = screen(3)
	dc = onehot_covariates()
	copied, equal = dg.copy(), dg.copy()
	copied[5] = dc[1]
	equal[4] = equal[3]
	return dc, dict(copied=copied, equal=equal)


def covariates_pinv(dc, tol=TOL):
	"""The pseudo-inverse and rank of dc dc^T as Single4Plan(pinv='numpy') takes them."""
	from normalisr_amd.association import inv_rank
	dc = np.ascontiguousarray(dc, dtype=np.float64)
	if not dc.shape[0]:
		return dc, np.zeros((0, 0)), 0
	dci, dcr = inv_rank(np.matmul(dc, dc.T), tol=tol)
	return dc, np.ascontiguousarray(dci, dtype=np.float64), int(dcr)


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
def _inputs(c, arr):
	if 'screen' in c:
		s = dict(c['screen'])
		return screen(s['nc'], s.get('dtype', 'float64'), s.get('seed'))
	return arr[c['dg']], arr[c['dt']], arr[c['dc']]


def _entry(lib, _lib, dg, dt, dc):
	"""nrm_association_tests_single4_host (return_dot = 0, alpha wanted) on host arrays: the five outputs."""
	dc, dci, dcr = covariates_pinv(dc)
	dg, dt = np.ascontiguousarray(dg, dtype=np.float64), np.ascontiguousarray(dt)
	nx, n = dg.shape
	ny, nc = dt.shape[0], dc.shape[0]
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
	code = _lib.NRM_F64 if dt.dtype == np.float64 else _lib.NRM_F32
	p, st, vy = (np.empty((nx, ny), dt.dtype) for _ in range(3))
	vx, al = np.empty(nx, dt.dtype), np.zeros((nx, ny, nc), dt.dtype)
	_lib.check(lib.nrm_association_tests_single4_host(vp(dg), _lib.NRM_F64, nx, vp(dt), code, ny, vp(dc), _lib.NRM_F64, nc, n, vp(dci), dcr, 0, 0, TOL, vp(p), vp(st),
													   vp(al), vp(vx), vp(vy), code))
	return p, st, al, vx, vy


def scenario_cases(job, arr, out, lib, _lib, cplan):
	"""cabi_harness.cases; `entry`: the whole-problem entry on the rows kept too."""
	return h.cases(cplan.Single4Plan, job, arr, out, _inputs, entry=lambda dg, dt, dc: _entry(lib, _lib, dg[kept_rows()], dt, dc))


def scenario_replays(job, arr, out, lib, _lib, cplan):
	"""Five steps, update(dt2) and one more, set_design(dg2) and two more, info() after set_design kept (cabi_harness.replays)."""
	return h.replays(cplan.Single4Plan, ('step', 'step', 'step', 'step', 'step', 'update', 'design', 'step'), screen(job['nc']), second_screen(job['nc'])[:2], job['design_form'], out,
					 info_after_design=True)


def scenario_handback(job, arr, out, lib, _lib, cplan):
	return h.handback(cplan.Single4Plan, handback_screen(), out, lowmem=False)


def scenario_refusals(job, arr, out, lib, _lib, cplan):
	"""Designs the closed form has no certificate for, at construction and at set_design; too few cells; a NaN in dt."""
	dg, dt, _ = screen(3)
	dc, designs = refused_designs()
	notes = {}
	with cplan.Single4Plan(dg, dt, dc) as plan:
		h.store(out, 'first', plan.step().results())
		notes['first'] = plan.info()
	for name, d in designs.items():
		notes['create_' + name] = h.raised(lambda: cplan.Single4Plan(d, dt, dc).close())
		with cplan.Single4Plan(dg, dt, dc) as plan:
			plan.step().step()
			notes['design_' + name] = h.raised(lambda: plan.set_design(d))
			notes['step_after_' + name] = h.raised(plan.step)
			h.store(out, 'after_' + name, plan.set_design(dg).step().results())
			notes['after_' + name] = plan.info()
	notes['cells'] = h.raised(lambda: cplan.Single4Plan(dg, dt, dc, dimreduce=N - NX - 3).close())  # n == nx + rank + dimreduce
	bad = dt.copy()
	bad[3, 11] = np.nan
	with cplan.Single4Plan(dg, bad, dc) as plan:
		plan.step().step().step()
		notes['nan'] = h.raised(plan.results)
		plan.update(dt).step()
		notes['clean_check'] = h.raised(plan.check)
		h.store(out, 'after_nan', plan.results())
		notes['after_nan'] = plan.info()
	return notes


if __name__ == '__main__':
	h.child_main(sys.argv, globals())
