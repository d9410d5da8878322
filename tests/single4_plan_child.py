"""The child side of tests/test_gpu_single4_plan.py: a process in which torch cannot be imported makes every call on the library's resident single=4 plan
(normalisr_amd.cplan.Single4Plan over nrm_single4_plan_*) and writes what it got to an .npz; the parent compares.
`python tests/single4_plan_child.py SCENARIO IN.npz OUT.npz`.  The screen is tests/single1_plan_child.py::screen; the design forms, the device copies and the result
keys are those of tests/de_plan_child.py.  What the top of this file defines is shared with the parent and with tests/test_single4_plan_cpu.py (which import this
module; nothing here touches torch)."""
import ctypes
import json
import sys

import numpy as np

import de_plan_child as dpc
import single1_plan_child as s1c

ROOT = dpc.ROOT
KEYS = dpc.KEYS
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
	"""Every case: a plan on (dg, dt, dc) in each of the forms named, `steps` steps, the results (and q-values) of the last, info() at the end; `entry`: the
	whole-problem entry on the rows kept too."""
	infos = {}
	for c in job['cases']:
		dg, dt, dc = _inputs(c, arr)
		for form in c.get('forms', ['dense']):
			d, held = dpc._design(form, dg, lib, _lib, cplan)
			name = '{}.{}'.format(c['name'], form)
			with cplan.Single4Plan(d, dt, dc, dimreduce=c.get('dimreduce', 0), lowmem=c.get('lowmem', True), q=c.get('q', False), out_dtype=c.get('out_dtype')) as plan:
				for _ in range(c.get('steps', 1)):
					plan.step()
				back = plan.check()
				dpc._store(out, name, plan.results())
				if c.get('q'):
					out[name + '.q'] = plan.qvalues()
				infos[name] = dict(plan.info(), handed_back=back)
			dpc._free(lib, _lib, held)
		if c.get('entry'):
			dpc._store(out, c['name'] + '.entry', _entry(lib, _lib, dg[kept_rows()], dt, dc))
	return infos


def scenario_replays(job, arr, out, lib, _lib, cplan):
	"""Five steps, update(dt2) and one more, set_design(dg2) and two more: every step's results and info; fresh plans on the same inputs; an adopted expression
	matrix rewritten in place behind a captured step."""
	nc = job['nc']
	dg, dt, dc = screen(nc)
	dg2, dt2, _ = second_screen(nc)
	infos = {}
	with cplan.Single4Plan(dg, dt, dc, lowmem=False) as plan:
		k = 0
		for what in ('step', 'step', 'step', 'step', 'step', 'update', 'design', 'step'):
			if what == 'update':
				plan.update(dt2)
			elif what == 'design':
				plan.set_design(dpc._design(job['design_form'], dg2, lib, _lib, cplan)[0])
				infos['after_design'] = plan.info()
			plan.step()
			k += 1
			dpc._store(out, 'run{}'.format(k), plan.results())
			infos['run{}'.format(k)] = plan.info()
	for name, (g, t) in dict(fresh_a=(dg, dt), fresh_b=(dg, dt2), fresh_c=(dg2, dt2)).items():
		with cplan.Single4Plan(g, t, dc, lowmem=False) as plan:
			dpc._store(out, name, plan.step().results())
			infos[name] = plan.info()
	# an adopted expression matrix with a row pitch, rewritten in place on the plan's stream
	ny, n = dt.shape
	ld = n + 4
	ptr = dpc._pinned(lib, _lib, ny * ld * dt.itemsize)

	def fill(values, st):
		h = np.zeros((ny, ld), dtype=dt.dtype)
		h[:, :n] = values
		_lib.check(lib.nrm_upload(h.ctypes.data, ptr, h.nbytes, 0, st))
	fill(dt, None)
	with cplan.Single4Plan(dg, cplan.DeviceMatrix(ptr, (ny, n), dt.dtype, ld), dc, lowmem=False) as plan:
		for _ in range(3):
			plan.step()
		dpc._store(out, 'adopted_old', plan.results())
		infos['adopted_old'] = plan.info()
		fill(dt2, plan.device_results()['stream'])
		plan.step()
		dpc._store(out, 'adopted_new', plan.results())
		infos['adopted_new'] = plan.info()
		try:
			plan.update(dt2)
			infos['adopted_update'] = 'accepted'
		except ValueError as e:
			infos['adopted_update'] = str(e)
	_lib.check(lib.nrm_host_free(ptr))
	return infos


def scenario_handback(job, arr, out, lib, _lib, cplan):
	dg, dt, dc = handback_screen()
	infos = {}
	with cplan.Single4Plan(dg, dt, dc, lowmem=False) as plan:
		plan.step()
		infos['first_check'] = plan.check()
		infos['after_first'] = plan.info()
		dpc._store(out, 'first', plan.results())
		for k in range(3):
			plan.step()
			infos['check{}'.format(k)] = plan.check()
			dpc._store(out, 'later{}'.format(k), plan.results())
			infos['later{}'.format(k)] = plan.info()
	return infos


_raised = s1c._raised


def scenario_refusals(job, arr, out, lib, _lib, cplan):
	"""Designs the closed form has no certificate for, at construction and at set_design; too few cells; a NaN in dt."""
	dg, dt, _ = screen(3)
	dc, designs = refused_designs()
	notes = {}
	with cplan.Single4Plan(dg, dt, dc) as plan:
		dpc._store(out, 'first', plan.step().results())
		notes['first'] = plan.info()
	for name, d in designs.items():
		notes['create_' + name] = _raised(lambda: cplan.Single4Plan(d, dt, dc).close())
		with cplan.Single4Plan(dg, dt, dc) as plan:
			plan.step().step()
			notes['design_' + name] = _raised(lambda: plan.set_design(d))
			notes['step_after_' + name] = _raised(plan.step)
			dpc._store(out, 'after_' + name, plan.set_design(dg).step().results())
			notes['after_' + name] = plan.info()
	notes['cells'] = _raised(lambda: cplan.Single4Plan(dg, dt, dc, dimreduce=N - NX - 3).close())  # n == nx + rank + dimreduce
	bad = dt.copy()
	bad[3, 11] = np.nan
	with cplan.Single4Plan(dg, bad, dc) as plan:
		plan.step().step().step()
		notes['nan'] = _raised(plan.results)
		plan.update(dt).step()
		notes['clean_check'] = _raised(plan.check)
		dpc._store(out, 'after_nan', plan.results())
		notes['after_nan'] = plan.info()
	return notes


def main(argv):
	sys.modules['torch'] = None  # `import torch` raises ImportError in this process
	sys.path.insert(0, ROOT)
	from normalisr_amd import _lib, cplan
	scenario, src, dst = argv[1:4]
	arr = np.load(src)
	job = json.loads(str(arr['job']))
	lib = _lib.load()
	out = {}
	notes = globals()['scenario_' + scenario](job, arr, out, lib, _lib, cplan)
	assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]
	out['notes'] = np.array(json.dumps(notes))
	np.savez(dst, **out)
	print('child ok')


if __name__ == '__main__':
	main(sys.argv)
