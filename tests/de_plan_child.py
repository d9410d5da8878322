"""The child side of tests/test_gpu_de_plan.py: a process in which torch cannot be imported makes every call on the library's resident de plan
(normalisr_amd.cplan.DePlan over nrm_de_plan_*) and writes what it got to an .npz; the parent compares.  `python tests/de_plan_child.py SCENARIO IN.npz OUT.npz`.
The input generators at the top are shared with the parent (which imports this module; nothing here touches torch)."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('p', 'gamma', 'alpha', 'varg', 'vart')


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
def _store(out, name, res):
	for k, v in zip(KEYS, res):
		if v is not None:
			out['{}.{}'.format(name, k)] = v


def _pinned(lib, _lib, nbytes):
	p = ctypes.c_void_p()
	_lib.check(lib.nrm_host_alloc(ctypes.byref(p), max(int(nbytes), 16)))
	return p.value


def _device_copy(lib, _lib, a):
	"""`a` in device-visible memory of the library (nrm_host_alloc), filled through nrm_upload: its address."""
	a = np.ascontiguousarray(a)
	ptr = _pinned(lib, _lib, a.nbytes)
	if a.nbytes:
		_lib.check(lib.nrm_upload(a.ctypes.data, ptr, a.nbytes, 0, None))
	return ptr


def _device_csr(lib, _lib, cplan, dg, ones):
	"""The design as a cplan.DeviceCSR: canonical CSR from scipy, the three arrays uploaded by the library.  ones: no data array (every entry is 1)."""
	import scipy.sparse
	from normalisr_amd import de_sparse
	indptr, indices, data = de_sparse.canonical_design_csr(scipy.sparse.csr_matrix(dg))
	ptrs = [_device_copy(lib, _lib, indptr), _device_copy(lib, _lib, indices), None if ones else _device_copy(lib, _lib, data)]
	return cplan.DeviceCSR(ptrs[0], ptrs[1], ptrs[2], dg.shape, indices.size, data.dtype), [p for p in ptrs if p]


def _free(lib, _lib, ptrs):
	for p in ptrs:
		_lib.check(lib.nrm_host_free(p))


def _design(form, dg, lib, _lib, cplan):
	import scipy.sparse
	if form == 'dense':
		return dg, []
	if form == 'scipy':
		return scipy.sparse.csr_matrix(dg), []
	if form == 'coo':
		return scipy.sparse.coo_matrix(dg), []
	binary = bool(((dg == 0) | (dg == 1)).all())
	return _device_csr(lib, _lib, cplan, dg, ones=binary and form == 'devcsr')


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
	"""Every case: a plan on (dg, dt, dc) in each of the forms named, `steps` steps, the results (and q-values) of the last, info() at the end."""
	infos = {}
	for c in job['cases']:
		dg, dt, dc = _inputs(c, arr)
		for form in c.get('forms', ['dense']):
			d, held = _design(form, dg, lib, _lib, cplan)
			name = '{}.{}'.format(c['name'], form)
			with cplan.DePlan(d, dt, dc, dimreduce=c.get('dimreduce', 0), lowmem=c.get('lowmem', True), q=c.get('q', False), out_dtype=c.get('out_dtype'),
							  pinv=c.get('pinv', 'numpy')) as plan:
				for _ in range(c.get('steps', 1)):
					plan.step()
				back = plan.check()
				_store(out, name, plan.results())
				if c.get('q'):
					out[name + '.q'] = plan.qvalues()
				infos[name] = dict(plan.info(), handed_back=back)
			_free(lib, _lib, held)
	return infos


def scenario_replays(job, arr, out, lib, _lib, cplan):
	"""Three steps, update(dt2) and two more, set_design(dg2) and two more: every step's results and info; fresh plans on the same inputs; an adopted expression
	matrix rewritten in place behind a captured step."""
	s = dict(job['screen'])
	s['dtype'] = np.dtype(s['dtype'])
	dg, dt, dc = screen(**s)
	dg2, dt2, _ = screen(**dict(s, seed=s['seed'] + 1, const_rows=(20, 33)))
	infos = {}
	with cplan.DePlan(dg, dt, dc, lowmem=False) as plan:
		k = 0
		for what in ('step', 'step', 'step', 'update', 'step', 'design', 'step'):
			if what == 'update':
				plan.update(dt2)
			elif what == 'design':
				plan.set_design(_design(job['design_form'], dg2, lib, _lib, cplan)[0])
			plan.step()
			k += 1
			_store(out, 'run{}'.format(k), plan.results())
			infos['run{}'.format(k)] = plan.info()
	for name, (g, t) in dict(fresh_a=(dg, dt), fresh_b=(dg, dt2), fresh_c=(dg2, dt2)).items():
		with cplan.DePlan(g, t, dc, lowmem=False) as plan:
			_store(out, name, plan.step().results())
			infos[name] = plan.info()
	# an adopted expression matrix with a row pitch, rewritten in place on the plan's stream
	ny, n = dt.shape
	ld = n + 4
	ptr = _pinned(lib, _lib, ny * ld * dt.itemsize)

	def fill(values, st):
		h = np.zeros((ny, ld), dtype=dt.dtype)
		h[:, :n] = values
		_lib.check(lib.nrm_upload(h.ctypes.data, ptr, h.nbytes, 0, st))
	fill(dt, None)
	with cplan.DePlan(dg, cplan.DeviceMatrix(ptr, (ny, n), dt.dtype, ld), dc, lowmem=False) as plan:
		for _ in range(3):
			plan.step()
		_store(out, 'adopted_old', plan.results())
		infos['adopted_old'] = plan.info()
		fill(dt2, plan.device_results()['stream'])
		plan.step()
		_store(out, 'adopted_new', plan.results())
		infos['adopted_new'] = plan.info()
		try:
			plan.update(dt2)
			infos['adopted_update'] = 'accepted'
		except ValueError as e:
			infos['adopted_update'] = str(e)
	_lib.check(lib.nrm_host_free(ptr))
	return infos


def scenario_handback(job, arr, out, lib, _lib, cplan):
	dx, dy, dc = handback_inputs()
	infos = {}
	with cplan.DePlan(dx, dy, dc) as plan:
		plan.step()
		infos['first_check'] = plan.check()
		infos['after_first'] = plan.info()
		_store(out, 'first', plan.results())
		for k in range(3):
			plan.step()
			infos['check{}'.format(k)] = plan.check()
			_store(out, 'later{}'.format(k), plan.results())
			infos['later{}'.format(k)] = plan.info()
	return infos


def scenario_bounds(job, arr, out, lib, _lib, cplan):
	s = dict(job['screen'])
	s['dtype'] = np.dtype(s['dtype'])
	dg, dt, dc = screen(**s)
	bad = dt.copy()
	bad[3, 7] = np.nan
	notes = {}
	with cplan.DePlan(dg, bad, dc) as plan:
		plan.step().step().step()
		try:
			plan.check()
			notes['nan'] = 'accepted'
		except AssertionError as e:
			notes['nan'] = 'AssertionError: ' + str(e)
		plan.update(dt).step()
		notes['clean_check'] = plan.check()
		_store(out, 'after_nan', plan.results())
		notes['after_nan'] = plan.info()
	with cplan.DePlan(dg, dt, dc) as plan:
		_store(out, 'fresh', plan.step().results())
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
