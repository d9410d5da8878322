"""What the tests of the C-ABI plans and whole-problem entries share -- TEST INFRASTRUCTURE ONLY, each piece once:

  child side    the frame of a child process in which torch cannot be imported (child_main), how it stores results, device-visible copies of host arrays, the design
                forms, the adopted-matrix scenario and the cases / replays / handback scenarios of the three design plans (de, single=1, single=4);
  parent side   run_child and the comparators the parents hold the children's arrays with;
  CPU side      the declared / exported / bound check, the binds-without-torch subprocess and the one g++ ASan + UBSan build-and-run of a stand-alone host program.

Nothing here touches torch or loads the library at import: the children import this module before they block torch, the CPU files on machines without a GPU."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = ('p', 'gamma', 'alpha', 'varg', 'vart')  # what a design plan's results() returns
COEX_KEYS = ('p', 'dot', 'var')
P_TINY = 2.3e-308  # below: subnormal, compared absolutely


# ---- child side -----------------------------------------------------------------------------------------------------------------------------------------------
def without_torch(dst, run):
	"""The frame of every child: `import torch` raises ImportError from here on, the repository is importable, run(out) fills `out` with arrays and returns the
	notes; neither torch nor any torch.* module may be there afterwards.  Writes OUT.npz (the notes as JSON under 'notes') and prints `child ok`."""
	sys.modules['torch'] = None
	sys.path.insert(0, ROOT)
	out = {}
	notes = run(out)
	assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]
	out['notes'] = np.array(json.dumps(notes))
	np.savez(dst, **out)
	print('child ok')


def child_main(argv, scenarios):
	"""`python tests/X_child.py SCENARIO IN.npz OUT.npz`: scenarios['scenario_' + SCENARIO](job, arr, out, lib, _lib, cplan) under without_torch; the job is the
	JSON under 'job' of IN.npz.  scenarios: the child's globals()."""
	scenario, src, dst = argv[1:4]

	def run(out):
		from normalisr_amd import _lib, cplan
		arr = np.load(src)
		job = json.loads(str(arr['job']))
		return scenarios['scenario_' + scenario](job, arr, out, _lib.load(), _lib, cplan)
	without_torch(dst, run)


def store(out, name, res, keys=KEYS, tag=''):
	"""out['NAME.KEY' + tag] for every array of a result; what a design plan leaves out (alpha under lowmem) is None and skipped.  The coex child passes COEX_KEYS."""
	for k, v in zip(keys, res):
		if v is not None:
			out['{}.{}{}'.format(name, k, tag)] = v


def pinned(nbytes):
	"""The address of nbytes (16 at the least) of device-visible host memory of the library (nrm_host_alloc)."""
	from normalisr_amd import _lib
	p = ctypes.c_void_p()
	_lib.check(_lib.load().nrm_host_alloc(ctypes.byref(p), max(int(nbytes), 16)))
	return p.value


def device_copy(a):
	"""`a` in device-visible memory of the library (nrm_host_alloc), filled through nrm_upload: its address."""
	from normalisr_amd import _lib
	a = np.ascontiguousarray(a)
	ptr = pinned(a.nbytes)
	if a.nbytes:
		_lib.check(_lib.load().nrm_upload(a.ctypes.data, ptr, a.nbytes, 0, None))
	return ptr


def device_csr(dg, ones):
	"""The design as a cplan.DeviceCSR: canonical CSR from scipy, the three arrays uploaded by the library.  ones: no data array (every entry is 1)."""
	import scipy.sparse
	from normalisr_amd import cplan, de_sparse
	indptr, indices, data = de_sparse.canonical_design_csr(scipy.sparse.csr_matrix(dg))
	ptrs = [device_copy(indptr), device_copy(indices), None if ones else device_copy(data)]
	return cplan.DeviceCSR(ptrs[0], ptrs[1], ptrs[2], dg.shape, indices.size, data.dtype), [p for p in ptrs if p]


def free(ptrs):
	from normalisr_amd import _lib
	for p in ptrs:
		_lib.check(_lib.load().nrm_host_free(p))


def design_form(form, dg):
	"""(the design in the form named, the addresses to free afterwards).  dense; scipy (CSR); coo; devcsr (a DeviceCSR without a data array where every entry is 1);
	devcsr_data (one with a data array always)."""
	import scipy.sparse
	if form == 'dense':
		return dg, []
	if form == 'scipy':
		return scipy.sparse.csr_matrix(dg), []
	if form == 'coo':
		return scipy.sparse.coo_matrix(dg), []
	binary = bool(((dg == 0) | (dg == 1)).all())
	return device_csr(dg, ones=binary and form == 'devcsr')


def raised(call, accepted='accepted', catch=(AssertionError, ValueError, RuntimeError, NotImplementedError)):
	"""'TYPE: message' of what call() raises, or `accepted`.  The plan children catch what the bindings raise (NotImplementedError is a RuntimeError: the class name
	tells them apart) and let anything else end the child; the front-entries child passes 'no error' and Exception."""
	try:
		call()
		return accepted
	except catch as e:
		return '{}: {}'.format(type(e).__name__, e)


def adopted_matrix(a, ld, stream=None):
	"""`a` in device-visible memory of the library with row pitch ld, filled through nrm_upload on `stream` -> (cplan.DeviceMatrix, rewrite(values, stream)).  The
	caller frees .ptr."""
	from normalisr_amd import _lib, cplan
	rows, n = a.shape
	ptr = pinned(rows * ld * a.itemsize)

	def fill(values, st):
		h = np.zeros((rows, ld), dtype=a.dtype)
		h[:, :n] = values
		_lib.check(_lib.load().nrm_upload(h.ctypes.data, ptr, h.nbytes, 0, st))
	fill(a, stream)
	return cplan.DeviceMatrix(ptr, (rows, n), a.dtype, ld), fill


def update_refused(plan, values):
	"""update() on a plan that adopted its matrix: the words of its ValueError, or 'accepted'."""
	try:
		plan.update(values)
		return 'accepted'
	except ValueError as e:
		return str(e)


def adopted_rewrite(plan_cls, dg, dt, dt2, dc, out, infos, **kw):
	"""An adopted expression matrix with a row pitch (n + 4), rewritten in place on the plan's stream behind a captured step: three steps (adopted_old), the
	rewrite, one step (adopted_new); update() must be refused (adopted_update)."""
	dm, fill = adopted_matrix(dt, dt.shape[1] + 4)
	with plan_cls(dg, dm, dc, **kw) as plan:
		for _ in range(3):
			plan.step()
		store(out, 'adopted_old', plan.results())
		infos['adopted_old'] = plan.info()
		fill(dt2, plan.device_results()['stream'])
		plan.step()
		store(out, 'adopted_new', plan.results())
		infos['adopted_new'] = plan.info()
		infos['adopted_update'] = update_refused(plan, dt2)
	free([dm.ptr])


def cases(plan_cls, job, arr, out, inputs, pinv=False, handed_back=True, entry=None):
	"""Every case of the job: a plan on inputs(c, arr) = (dg, dt, dc) in each of the forms named, `steps` steps, check(), the results (and q-values) of the last,
	info() at the end.  pinv: the plan takes the keyword (single=1 and single=4 do not).  handed_back: check() returns a count, kept beside info() (Single1Plan's
	returns nothing).  entry(dg, dt, dc): the whole-problem entry's five outputs, stored as NAME.entry for a case that asks for it (single=4)."""
	infos = {}
	for c in job['cases']:
		dg, dt, dc = inputs(c, arr)
		kw = dict(dimreduce=c.get('dimreduce', 0), lowmem=c.get('lowmem', True), q=c.get('q', False), out_dtype=c.get('out_dtype'))
		if pinv:
			kw['pinv'] = c.get('pinv', 'numpy')
		for form in c.get('forms', ['dense']):
			d, held = design_form(form, dg)
			name = '{}.{}'.format(c['name'], form)
			with plan_cls(d, dt, dc, **kw) as plan:
				for _ in range(c.get('steps', 1)):
					plan.step()
				back = plan.check()
				store(out, name, plan.results())
				if c.get('q'):
					out[name + '.q'] = plan.qvalues()
				infos[name] = dict(plan.info(), handed_back=back) if handed_back else plan.info()
			free(held)
		if entry is not None and c.get('entry'):
			store(out, c['name'] + '.entry', entry(dg, dt, dc))
	return infos


def replays(plan_cls, schedule, first, second, form, out, info_after_design=False):
	"""One plan on first = (dg, dt, dc) through `schedule` -- every entry ends in a step; 'update' uploads dt2 before it, 'design' sets dg2 (in the form named)
	before it, second = (dg2, dt2) -- with every step's results and info (run1, run2, ...); fresh plans on the same inputs (fresh_a, fresh_b, fresh_c); then
	adopted_rewrite.  info_after_design: info() between set_design and the step is kept too (single=4)."""
	dg, dt, dc = first
	dg2, dt2 = second
	infos = {}
	with plan_cls(dg, dt, dc, lowmem=False) as plan:
		for k, what in enumerate(schedule, 1):
			if what == 'update':
				plan.update(dt2)
			elif what == 'design':
				plan.set_design(design_form(form, dg2)[0])
				if info_after_design:
					infos['after_design'] = plan.info()
			plan.step()
			store(out, 'run{}'.format(k), plan.results())
			infos['run{}'.format(k)] = plan.info()
	for name, (g, t) in dict(fresh_a=(dg, dt), fresh_b=(dg, dt2), fresh_c=(dg2, dt2)).items():
		with plan_cls(g, t, dc, lowmem=False) as plan:
			store(out, name, plan.step().results())
			infos[name] = plan.info()
	adopted_rewrite(plan_cls, dg, dt, dt2, dc, out, infos, lowmem=False)
	return infos


def handback(plan_cls, inputs, out, **kw):
	"""A step and its check (first_check, after_first, `first`), then three more of each (check0.., later0..)."""
	dg, dt, dc = inputs
	infos = {}
	with plan_cls(dg, dt, dc, **kw) as plan:
		plan.step()
		infos['first_check'] = plan.check()
		infos['after_first'] = plan.info()
		store(out, 'first', plan.results())
		for k in range(3):
			plan.step()
			infos['check{}'.format(k)] = plan.check()
			store(out, 'later{}'.format(k), plan.results())
			infos['later{}'.format(k)] = plan.info()
	return infos


# ---- parent side ----------------------------------------------------------------------------------------------------------------------------------------------
def start_child(child_file, args, dst, env, timeout, tail=3000):
	"""tests/CHILD_FILE with `args` in the environment `env`, one child at a time: it must end with status 0 and `child ok` -> (the arrays of dst, its notes)."""
	r = subprocess.run([sys.executable, os.path.join(HERE, child_file)] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
	assert r.returncode == 0 and 'child ok' in r.stdout, r.stdout[-tail:]
	out = np.load(dst)
	return out, json.loads(str(out['notes']))


def run_child(child_file, tmp_path, scenario, arrays, job, env=None, timeout=240):
	"""`python tests/CHILD_FILE SCENARIO IN.npz OUT.npz` with the job and the arrays in IN.npz and `env` on top of this process's environment."""
	src, dst = str(tmp_path / (scenario + '_in.npz')), str(tmp_path / (scenario + '_out.npz'))
	np.savez(src, job=np.array(json.dumps(job)), **arrays)
	return start_child(child_file, [scenario, src, dst], dst, dict(os.environ, **(env or {})), timeout)


def close(a, b, rtol=1e-6, floor=0.):
	"""Relative error under rtol, with an absolute floor beside |b|.  The defaults are those of tests/test_gpu_de_plan.py and tests/test_gpu_parity.py (1e-6, 0);
	the wide-covariate files keep a copy of their own with other defaults (1e-9, 1.0), and whoever wants those bars here names them at the call."""
	from conftest import relerr
	err = relerr(a, b, floor)
	print('  worst relative error {:.2e} (bar {:.0e}, floor {:.0e})'.format(err, rtol, floor))
	return err < rtol


def p_close(p, ref, rtol=1e-6):
	"""P-values: relative where the reference is a normal number, within 1e-307 absolutely below."""
	p, ref = np.asarray(p, dtype=np.float64), np.asarray(ref, dtype=np.float64)
	from conftest import relerr
	normal = ref >= P_TINY
	err = relerr(p[normal], ref[normal]) if normal.any() else 0.
	print('  P-values: worst relative error {:.2e}'.format(err))
	return err < rtol and bool(np.all(np.abs(p[~normal] - ref[~normal]) <= 1e-307))


def got(out, name, keys=KEYS, tag=''):
	"""The result stored under NAME.  A design plan's (KEYS): None for what was left out (alpha under lowmem).  A coex plan's (COEX_KEYS, with the tag of the
	step): all three are there, a missing one is a KeyError."""
	names = ['{}.{}{}'.format(name, k, tag) for k in keys]
	return tuple(out[n] if (n in out.files or keys is not KEYS) else None for n in names)


def same(a, b, what=''):
	"""Two design-plan results equal bit for bit: dtypes, shapes, every array."""
	for k, x, y in zip(KEYS, a, b):
		if x is None or y is None:
			assert x is None and y is None, (what, k)
			continue
		assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (what, k, float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.size else 0.)


def untested_rows_exact(res, rows):
	p, gam, a, vg, vt = res
	assert (p[rows] == 1).all() and (gam[rows] == 0).all() and (vg[rows] == 0).all() and (vt[rows] == 0).all() and (a is None or (a[rows] == 0).all())


def same_bars(got, p, gam, varg, vart, alpha=None, vtol=1e-9):
	"""single=4's bars (`_same` of tests/test_gpu_single4_rank_deficient.py): P-values 1e-6 relative, gamma vtol (floor 1e-12), varg and vart vtol, alpha vtol
	(floor 1e-9)."""
	assert p_close(got[0], p) and close(got[1], gam, vtol, 1e-12) and close(got[3], varg, vtol) and close(got[4], vart, vtol)
	if alpha is not None:
		assert close(got[2], alpha, vtol, 1e-9)


def held(got, want, dtype, nc):
	"""single=1's bars with up to 32 covariates (tests/test_gpu_single1_wide.py)."""
	tol = 1e-6 if dtype == np.float32 else 1e-9
	assert got[0].dtype == dtype
	assert p_close(got[0], want[0], 1e-6), 'P'
	assert close(got[1], want[1], tol, 1e-12), 'gamma'
	assert close(got[2], want[2], max(tol, 1e-8), 1e-9), 'alpha'
	assert close(got[3], want[3], tol), 'varx'
	assert close(got[4], want[4], tol), 'vary'


# ---- CPU side -------------------------------------------------------------------------------------------------------------------------------------------------
def vp(a):
	return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def assert_plan_names(prefix, calls, others=()):
	"""PREFIX + call for every call, and `others`: declared in include/normalisr_hip.h, exported by the library, bound by ctypes; and the header declares exactly what
	the library exports.  -> the names."""
	from normalisr_amd import _lib
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	declared = set(re.findall(r'\b(nrm_[a-z0-9_]+)\s*\(', hdr))
	lib = ctypes.CDLL(_lib.LIB_PATH)
	names = [prefix + c for c in calls] + list(others)
	for name in names:
		assert name in declared, name
		assert name in _lib.exported_symbols(), name
		assert hasattr(lib, name), name
	assert declared == set(_lib.exported_symbols())
	return names


def binds_without_torch(callables, methods, destroy_entry):
	"""A child in which `import torch` fails: normalisr_amd.cplan has the `callables`, the first of them the `methods`, the library loads and destroy(NULL) is
	fine, and torch was never asked for by name."""
	code = ("import sys; sys.modules['torch'] = None\n"
			"sys.path.insert(0, {!r})\n"
			"from normalisr_amd import cplan, _lib\n"
			"for c in {!r}:\n"
			"    assert callable(getattr(cplan, c)), c\n"
			"for m in {!r}:\n"
			"    assert callable(getattr(getattr(cplan, {!r}), m)), m\n"
			"lib = _lib.load()\n"
			"assert getattr(lib, {!r})(None) == 0\n"
			"assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]\n"
			"print('binds without torch ok')\n").format(ROOT, tuple(callables), tuple(methods), callables[0], destroy_entry)
	r = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
	assert r.returncode == 0 and 'binds without torch ok' in r.stdout, r.stdout[-2000:]


SANITIZER_FLAGS = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-pthread', '-w', '-x', 'c++']


def build_and_run_host_program(tmp_path, sources, ok_line, extra_flags=(), args=(), timeout=300, may_skip=False):
	"""The one place that builds host code under ASan + UBSan: `sources` (paths under the repository; one of them has the main) compiled by g++ into a stand-alone
	program, which is then run directly with `args` -- no environment variable is set and nothing loaded into python runs under a sanitizer.  It must end with status
	0 and print ok_line within `timeout` seconds -> its output.

	The flags are the longest line any caller had.  Callers that spelled -fno-sanitize-recover=undefined get =all (no weaker: ASan does not recover anyway), and those
	that built plain C++ without the HIP define and include path get them too (they name nothing of HIP).  may_skip: the callers that skipped where the machine
	cannot build such a program still do -- no g++, no HIP headers for a .hip source, or a one-line program that does not build with these flags; a failed build of
	the real sources is a failure, never a skip.  The other callers assert that g++ is there."""
	import pytest
	gxx = shutil.which('g++')
	flags = SANITIZER_FLAGS + list(extra_flags)
	if may_skip:
		if gxx is None or (any(s.endswith('.hip') for s in sources) and not os.path.exists('/opt/rocm/include/hip/hip_runtime.h')):
			pytest.skip('no g++ / HIP headers')
		probe = tmp_path / 'probe.cpp'
		probe.write_text('int main() { return 0; }\n')
		r = subprocess.run([gxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
		if r.returncode != 0:
			pytest.skip('g++ cannot build with the sanitizers here: ' + r.stdout[-200:])
	assert gxx is not None, 'g++ is needed to build the host arithmetic'
	exe = str(tmp_path / os.path.splitext(os.path.basename(sources[-1]))[0])
	r = subprocess.run([gxx] + flags + [os.path.join(ROOT, s) for s in sources] + ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
	assert r.returncode == 0, r.stdout[-3000:]
	r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
	assert r.returncode == 0 and ok_line in r.stdout, r.stdout[-3000:]
	return r.stdout
