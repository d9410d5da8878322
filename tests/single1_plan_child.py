"""The child side of tests/test_gpu_single1_plan.py: a process in which torch cannot be imported makes every call on the library's resident single=1 plan
(normalisr_amd.cplan.Single1Plan over nrm_single1_plan_*) and writes what it got to an .npz; the parent compares.
`python tests/single1_plan_child.py SCENARIO IN.npz OUT.npz`.  The input generators at the top are shared with the parent (which imports this module; nothing here
touches torch); the frame of the child, the design forms, the device copies, the result keys and the cases / replays scenarios are those of tests/cabi_harness.py."""
import ctypes
import sys

import numpy as np

import cabi_harness as h
import s1_wide

ROOT, KEYS = h.ROOT, h.KEYS
NX, NY, N = (s1_wide.s1.CHAIN[k] for k in ('nx', 'ny', 'n'))  # 65 groupings x 69 genes x 2051 cells
ZERO_ROW, ONES_ROW = 10, 40  # where the two rows de drops stand among the NX + 2 design rows
NG0 = NX + 2
SEEDS = dict(same=100, replays=21, q=31, raises=41, refusals=51)  # (same: + the covariate count; replays: and the next one)
NCS = [0, 3, 8, 9, 32]


def screens_used():
	"""(seed, nc) of every screen the GPU tests build: tests/test_single1_plan_cpu.py holds each to the oracle's own assertions."""
	return [(SEEDS['same'] + nc, nc) for nc in NCS] + [(SEEDS[k], 3) for k in ('replays', 'q', 'raises', 'refusals')] + [(SEEDS['replays'] + 1, 3)]


def screen(seed, dtype, nc):
	"""s1_wide.CHAIN's screen -- a ragged 64-row slot group, ny no multiple of the stream kernel's 8-column pieces, a ragged last chunk of 2048 cells; entries set with
	probability 1 / 65 -- with two rows added: one all zeros and one ALL ONES, which de drops and which must not reach the selection.  nc covariates, the intercept last."""
	rng = np.random.default_rng([seed, nc, 67])
	dx = (rng.random((NX, N)) < 1.0 / NX).astype(np.float64)
	dt = rng.normal(size=(NY, N))
	dt[:5] += 0.5 * dx[0]
	dc = np.vstack([rng.normal(size=(nc - 1, N)), np.ones((1, N))]) if nc else np.zeros((0, N))
	dg = np.insert(dx, [ZERO_ROW, ONES_ROW - 1], 0.0, axis=0)
	dg[ONES_ROW] = 1.0
	assert dg.shape == (NG0, N) and not dg[ZERO_ROW].any() and (np.delete(dg, [ZERO_ROW, ONES_ROW], axis=0) == dx).all()
	return dg, dt.astype(dtype), dc


ENTRY_NCS = [0, 3, 9]  # none; a lane per grouping; a wave per grouping
ENTRY_CONST_ROW = 4


def entry_screen(dtype, nc):
	"""The smallest screen on which the whole-problem entry and the plan can differ: 7 design rows over 203 cells, cells 0 .. 159 in one row each and cells 160 .. 202 in
	none; row 4 emptied, so that de drops it, the plan compacts and re-inflates, and its cells are shared ones too; 37 genes; nc covariates, the intercept last."""
	rng = np.random.default_rng([11, nc, 203])
	dg = np.zeros((7, 203))
	dg[rng.integers(0, 7, 160), np.arange(160)] = 1.0
	dg[ENTRY_CONST_ROW] = 0.0
	assert dg.sum(axis=0).max() == 1 and not dg[:, 160:].any() and (np.delete(dg, ENTRY_CONST_ROW, axis=0).sum(axis=1) > 3).all()
	dt = rng.normal(size=(37, 203))
	dt[:5] += 0.5 * dg[0]
	dc = np.vstack([rng.normal(size=(nc - 1, 203)), np.ones((1, 203))]) if nc else np.zeros((0, 203))
	return dg, dt.astype(dtype), dc


def kept_rows():
	return np.array([i for i in range(NG0) if i not in (ZERO_ROW, ONES_ROW)])


def one_grouping_per_cell():
	"""Every cell carries exactly one of the 65 groupings (no shared cells: grouping i is constant 1 on its own cells), beside the two rows de drops."""
	dg = np.zeros((NG0, N))
	for k, i in enumerate(kept_rows()):
		dg[i, k::NX] = 1
	dg[ONES_ROW] = 1
	return dg


def exclusive_cells(dg):
	"""Cells that carry exactly one of the groupings de keeps."""
	return int(((dg[kept_rows()] != 0).sum(axis=0) == 1).sum())


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
def _screen_of(c):
	s = dict(c['screen'])
	s['dtype'] = np.dtype(s['dtype'])
	return screen(**s)


def scenario_cases(job, arr, out, lib, _lib, cplan):
	inputs = lambda c, arr: _screen_of(c) if 'screen' in c else (arr[c['dg']], arr[c['dt']], arr[c['dc']])
	return h.cases(cplan.Single1Plan, job, arr, out, inputs, handed_back=False)


def scenario_entry(job, arr, out, lib, _lib, cplan):
	"""de(..., single=1) of the package -- with no torch in this process that is the whole-problem entry nrm_association_tests_single1_host on the rows de keeps -- and
	one step of a plan on the same arrays."""
	import normalisr_amd.normalisr as norm
	infos = {}
	for c in job['cases']:
		dg, dt, dc = entry_screen(np.dtype(c['dtype']), c['nc'])
		h.store(out, c['name'] + '.entry', norm.de(dg, dt, dc, single=1, lowmem=False))
		with cplan.Single1Plan(dg, dt, dc, lowmem=False) as plan:
			h.store(out, c['name'] + '.plan', plan.step().results())
			infos[c['name']] = plan.info()
	return infos


def scenario_replays(job, arr, out, lib, _lib, cplan):
	"""Three steps, update(dt2) and two more, set_design(dg2) and two more (cabi_harness.replays)."""
	dg2, dt2, _ = _screen_of(dict(screen=dict(job['screen'], seed=job['screen']['seed'] + 1)))
	return h.replays(cplan.Single1Plan, ('step', 'step', 'step', 'update', 'step', 'design', 'step'), _screen_of(job), (dg2, dt2), job['design_form'], out)


def scenario_raises(job, arr, out, lib, _lib, cplan):
	"""What the reference raises, from the device counters: each after three steps (the third a replay), at check()."""
	dg, dt, dc = _screen_of(job)
	notes = {}
	with cplan.Single1Plan(dg, dt, dc, dimreduce=N) as plan:
		notes['dimreduce'] = h.raised(lambda: plan.step().step().step().check())
	bad = dc.copy()
	bad[0, np.nonzero(dg[kept_rows()].sum(axis=0) == 0)[0][0]] = np.nan  # (at a cell every grouping shares)
	with cplan.Single1Plan(dg, dt, bad) as plan:
		notes['nan_covariate'] = h.raised(lambda: plan.step().step().step().check())
	with cplan.Single1Plan(one_grouping_per_cell(), dt, dc) as plan:
		notes['one_per_cell'] = h.raised(lambda: plan.step().step().step().check())
	own = np.nonzero((dg[kept_rows()] != 0).sum(axis=0) == 1)[0][0]  # a cell that belongs to exactly one grouping
	nan = dt.copy()
	nan[3, own] = np.nan
	with cplan.Single1Plan(dg, nan, dc) as plan:
		notes['nan_expression'] = h.raised(lambda: plan.step().step().step().check())
		plan.update(dt).step()
		notes['clean_check'] = h.raised(plan.check)
		h.store(out, 'after_nan', plan.results())
		notes['after_nan'] = plan.info()
	with cplan.Single1Plan(dg, dt, dc) as plan:
		h.store(out, 'fresh', plan.step().results())
	return notes


def _raw_create(lib, _lib, dt, dc, dense=None, csr=None):
	"""nrm_single1_plan_create on host arrays as they are (no canonicalisation): (what _lib.check raises, whether the handle stayed NULL)."""
	handle = ctypes.c_void_p()
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	nt, n = dt.shape
	if dense is not None:
		g = (0, vp(dense), _lib.NRM_F64, n, None, None, 0, 0, dense.shape[0])
	else:
		indptr, indices = csr
		g = (1, None, _lib.NRM_F64, 0, vp(indptr), vp(indices), int(indices.size), 0, int(indptr.size) - 1)
	rc = lib.nrm_single1_plan_create(ctypes.byref(handle), *g, vp(dt), _lib.NRM_F64, nt, n, n, 0, vp(dc), _lib.NRM_F64, dc.shape[0], 0, _lib.NRM_F64, 0, 0)
	what = h.raised(lambda: _lib.check(rc))
	null = handle.value is None
	if not null:
		lib.nrm_single1_plan_destroy(handle)
	return [what, null]


def scenario_refusals(job, arr, out, lib, _lib, cplan):
	"""Refusals that need the device, each followed by a plan that works in the same process."""
	import scipy.sparse
	dg, dt, dc = _screen_of(job)
	notes = {}
	rng = np.random.default_rng(5)
	designs = {}
	designs['negative'] = dg.copy()
	designs['negative'][3, 17] = -1.0
	designs['dense'] = (rng.random(dg.shape) < 0.3).astype(np.float64)  # more than a quarter of the entries set
	designs['two'] = dg.copy()
	designs['two'][3, 17] = 2.0
	designs['constant'] = np.zeros_like(dg)
	designs['constant'][::3] = 1.0
	m = scipy.sparse.csr_matrix(dg)
	m.sort_indices()
	indptr, indices = m.indptr.astype(np.int64), m.indices.astype(np.int32)
	falls, beyond = indptr.copy(), indices.copy()
	falls[5] = falls[4] - 1  # a decreasing indptr
	beyond[indptr[7 + 1] - 1] = N  # the last column of row 7: outside [0, n)

	def works():
		with cplan.Single1Plan(dg, dt, dc) as plan:
			return plan.step().results()
	h.store(out, 'first', works())
	for name, d in designs.items():
		notes[name] = _raw_create(lib, _lib, dt, dc, dense=np.ascontiguousarray(d))
		h.store(out, 'after_' + name, works())
	for name, c in dict(falls=(falls, indices), beyond=(indptr, beyond)).items():
		notes[name] = _raw_create(lib, _lib, dt, dc, csr=c)
		h.store(out, 'after_' + name, works())
	notes['good_csr'] = _raw_create(lib, _lib, dt, dc, csr=(indptr, indices))
	# a refused set_design leaves the plan without a design until one is accepted
	with cplan.Single1Plan(dg, dt, dc) as plan:
		notes['set_design'] = h.raised(lambda: plan.set_design(designs['two']))
		notes['step_without_design'] = h.raised(plan.step)
		h.store(out, 'after_set_design', plan.set_design(dg).step().results())
	return notes


if __name__ == '__main__':
	h.child_main(sys.argv, globals())
