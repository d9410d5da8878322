"""The child side of tests/test_gpu_front_plan.py: a process in which torch cannot be imported makes every call on the library's resident front-half plan
(normalisr_amd.cplan.FrontPlan, normalisr_amd._lib) and writes what it got to an .npz; the parent compares.  `python tests/front_plan_child.py SCENARIO IN.npz OUT.npz`.
The input generators at the top are shared with the parent (which imports this module; nothing here touches torch); the frame of the child and the adopted matrix
are those of tests/cabi_harness.py."""
import ctypes
import sys

import numpy as np

import cabi_harness as h

STAGES = ('dtn', 'dcn', 'w', 'wt', 'lcpm', 'cov')


def counts(seed, ng, n, dtype=np.int32, top=None, depth=1.0):
	"""Seeded Poisson counts with log-normal gene means and cell depths, about half of them zero; every cell has a read, every gene a zero and a non-zero entry.
	top: the value of entry [1, 2], the matrix's maximum."""
	rng = np.random.default_rng(seed)
	mu = np.exp(rng.normal(-0.3, 1.0, ng))
	x = rng.poisson(depth * mu[:, None] * np.exp(rng.normal(0.0, 0.5, n))[None, :])
	x[0, x.sum(axis=0) == 0] = 1
	x[np.arange(ng), np.arange(ng) % n] = 0  # a zero in every gene
	x[np.arange(ng), (np.arange(ng) + 1) % n] += 1
	if top is not None:
		x = np.minimum(x, top - 1)
		x[1, 2] = top
	assert (x.sum(axis=0) > 0).all() and ((x == 0).sum(axis=1) > 0).all()
	return x.astype(dtype)


def onehot(seed, k, n):
	"""k one-hot batch rows over n cells, every batch present."""
	b = np.random.default_rng(seed).integers(0, k, n)
	b[:k] = np.arange(k)
	return (b[None, :] == np.arange(k)[:, None]).astype(np.float64)


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
def _store(out, name, plan, stages=STAGES):
	dtn, dcn = plan.results()
	got = dict(dtn=dtn, dcn=dcn)
	if 'w' in stages:
		got['w'] = plan.weights()
	if 'wt' in stages:
		got['wt'] = plan.scaling()
	if 'lcpm' in stages:
		got['lcpm'] = plan.lcpm()
	if 'cov' in stages:
		got['cov'] = plan.normcov()
	for k in stages:
		out['{}.{}'.format(name, k)] = got[k]


def _plan(cplan, c, arr, reads=None):
	kw = dict(stepmax=c.get('stepmax', 1), out_dtype=np.dtype(c.get('out_dtype', 'float64')), count_cap=c.get('count_cap'))
	if c.get('ntot'):
		kw['ntot'] = c['ntot']
	return cplan.FrontPlan(arr[c['reads']] if reads is None else reads, None if c.get('cov') is None else arr[c['cov']], **kw)


def scenario_cases(job, arr, out, lib, _lib, cplan):
	"""Every case: a plan, `steps` steps with the stages after the steps named in `snaps`, info() after a check; coex: a CoexPlan adopting dtn where it lies."""
	infos = {}
	for c in job['cases']:
		with _plan(cplan, c, arr) as plan:
			for s in range(1, c.get('steps', 1) + 1):
				plan.step()
				if s in c.get('snaps', [c.get('steps', 1)]):
					_store(out, '{}@{}'.format(c['name'], s), plan)
			infos[c['name']] = plan.info()
			if c.get('coex'):
				res = plan.device_results()
				dcn = plan.results()[1]
				with cplan.CoexPlan(res['dtn'], dcn) as coex:
					coex.step()
					h.store(out, c['name'] + '.coex', coex.results(), h.COEX_KEYS)
					infos[c['name'] + '.coex'] = coex.info()
	return infos


def scenario_rewrite(job, arr, out, lib, _lib, cplan):
	"""Behind a captured graph: update(reads2) with another total and a larger maximum, and the same through an adopted matrix rewritten in place."""
	a, b, cov = arr['a'], arr['b'], arr['cov']
	c = dict(cov='cov', stepmax=2, count_cap=job['count_cap'])
	infos = {}
	with _plan(cplan, c, arr, a) as plan:
		for _ in range(3):
			plan.step()
		_store(out, 'owned_old', plan)
		plan.update(b).step()
		_store(out, 'owned_new', plan)
		infos['owned'] = plan.info()
	with _plan(cplan, c, arr, b) as plan:
		_store(out, 'fresh', plan.step())
		infos['fresh'] = plan.info()
	dm, fill = h.adopted_matrix(a, a.shape[1] + 4)
	with _plan(cplan, c, arr, dm) as plan:
		for _ in range(3):
			plan.step()
		_store(out, 'adopted_old', plan)
		fill(b, plan.device_results()['stream'])
		plan.step()
		_store(out, 'adopted_new', plan)
		infos['adopted'] = plan.info()
		infos['adopted_update'] = h.update_refused(plan, b)
	h.free([dm.ptr])
	infos['no_cap'] = h.raised(lambda: cplan.FrontPlan(dm, cov))
	return infos


def scenario_cap(job, arr, out, lib, _lib, cplan):
	below, at = arr['below'], arr['at']
	cap = job['count_cap']
	notes = {}
	with cplan.FrontPlan(below, None, count_cap=cap) as plan:
		plan.step()
		notes['below'] = h.raised(plan.check)
		_store(out, 'below', plan)
		notes['below_info'] = plan.info()
		plan.update(at).step().step()
		notes['at'] = h.raised(plan.check)
		notes['at_again'] = h.raised(plan.check)  # (the counters were cleared)
		plan.update(below).step()
		notes['after'] = h.raised(plan.check)
		_store(out, 'after', plan)
		notes['after_info'] = plan.info()
	return notes


def scenario_errors(job, arr, out, lib, _lib, cplan):
	"""One tiny matrix per refusal; after each, update() with good counts and a clean step that equals a fresh plan's."""
	good, cov = arr['good'], arr['cov']
	notes = {}
	with cplan.FrontPlan(good, cov, count_cap=256) as plan:
		_store(out, 'fresh', plan.step())
	for name in job['bad']:
		with cplan.FrontPlan(arr[name], cov, count_cap=256) as plan:
			plan.step().step().step()
			notes[name] = h.raised(plan.check)
			notes[name + '.results'] = h.raised(plan.results)
			plan.update(good).step()
			notes[name + '.after'] = h.raised(plan.check)
			_store(out, name + '.after', plan)
	return notes


def scenario_two(job, arr, out, lib, _lib, cplan):
	"""Two plans alive at once, stepped alternately with the pool emptied in between; then the pool's own accounting around a plan's life."""
	a, b, cov = arr['a'], arr['b'], arr['cov']
	notes = {}
	with cplan.FrontPlan(a, cov) as pa, cplan.FrontPlan(b, None, stepmax=2, out_dtype=np.float32) as pb:
		for i in range(4):
			pa.step()
			pb.step()
			if i == 1:
				pa.check(), pb.check()
				_lib.check(lib.nrm_release_cache())
		_store(out, 'two_a', pa)
		_store(out, 'two_b', pb)
		notes['two_a'], notes['two_b'] = pa.info(), pb.info()
	with cplan.FrontPlan(a, cov) as plan:
		_store(out, 'fresh_a', plan.step())
	with cplan.FrontPlan(b, None, stepmax=2, out_dtype=np.float32) as plan:
		_store(out, 'fresh_b', plan.step())

	def pool():
		held, used = ctypes.c_int64(-1), ctypes.c_int64(-1)
		_lib.check(lib.nrm_cache_bytes(ctypes.byref(held), ctypes.byref(used)))
		return [int(held.value), int(used.value)]
	_lib.check(lib.nrm_release_cache())
	notes['before'] = pool()
	plan = cplan.FrontPlan(a, cov)
	plan.step().step().step()
	plan.results()
	notes['alive'] = pool()
	notes['bytes'] = plan.info()['bytes']
	plan.close()
	notes['closed'] = pool()
	_lib.check(lib.nrm_release_cache())
	notes['released'] = pool()
	plan.close()  # twice is fine
	return notes


def scenario_stepmax_pair(job, arr, out, lib, _lib, cplan):
	"""Two plans of different stepmax alive at once on the same counts, stepped alternately: eager, captured, replayed."""
	notes = {}
	with cplan.FrontPlan(arr['x'], arr['cov'], stepmax=1) as p1, cplan.FrontPlan(arr['x'], arr['cov'], stepmax=3) as p3:
		for _ in range(3):
			p1.step()
			p3.step()
		_store(out, 's1', p1)
		_store(out, 's3', p3)
		notes['s1'], notes['s3'] = p1.info(), p3.info()
	return notes


if __name__ == '__main__':
	h.child_main(sys.argv, globals())
