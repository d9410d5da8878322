"""The child side of tests/test_gpu_coex_plan.py: a process in which torch cannot be imported makes every call on the library's resident coex plan
(normalisr_amd.cplan, normalisr_amd._lib) and writes what it got to an .npz; the parent compares.  `python tests/coex_plan_child.py SCENARIO IN.npz OUT.npz`.
The input generators at the top are shared with the parent (which imports this module; nothing here touches torch); the frame of the child and the adopted matrix
are those of tests/cabi_harness.py."""
import ctypes
import sys

import numpy as np

import cabi_harness as h

ROOT = h.ROOT


def spike_rows(rng, rows, n):
	"""Rows whose single spike carries all of their variance: the guard cannot certify pairs of them (tests/test_gpu_round3.py)."""
	x = 1e-3 * rng.normal(size=(rows, n))
	x[np.arange(rows), rng.choice(n, rows, replace=False)] = 50.0
	return x


def guard_inputs():
	"""The construction of test_guard_fires_inside_the_pipelined_and_chunked_paths: 40 spike rows among 2 200 at 4096 cells, fp32."""
	rng = np.random.default_rng(61)
	ng, n = 2200, 4096
	dt = rng.normal(size=(ng, n)).astype(np.float32)
	dt[:40] = spike_rows(rng, 40, n).astype(np.float32)
	dc = np.vstack([rng.normal(size=(1, n)), np.ones((1, n))]).astype(np.float32)
	return dt, dc


def expression(seed, ng, n, dtype):
	rng = np.random.default_rng(seed)
	dt = np.log1p(rng.poisson(2., (ng, n))).astype(dtype)
	dc = np.vstack([rng.normal(size=(1, n)), np.ones((1, n)), (rng.random((1, n)) < 0.4)]).astype(dtype)
	return dt, dc


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
def _store(out, name, tag, res):
	h.store(out, name, res, h.COEX_KEYS, tag)


def scenario_cases(job, arr, out, lib, _lib, cplan):
	"""Every case: a plan on (dt, dc), `steps` steps, the results after the steps named in `snaps`, info() at the end."""
	infos = {}
	for c in job['cases']:
		with cplan.CoexPlan(arr[c['dt']], arr[c['dc']], dimreduce=c.get('dimreduce', 0), out_dtype=c.get('out_dtype'), pinv=c.get('pinv', 'numpy')) as plan:
			for s in range(1, c.get('steps', 1) + 1):
				plan.step()
				if s in c.get('snaps', [c.get('steps', 1)]):
					_store(out, c['name'], s, plan.results())
			infos[c['name']] = plan.info()
	return infos


def scenario_rewrite(job, arr, out, lib, _lib, cplan):
	infos = {}
	# an adopted matrix, rewritten in place behind the third step on the plan's stream
	a, b, dc = arr['a'], arr['b'], arr['dc']
	dm, fill = h.adopted_matrix(a, a.shape[1], None)
	with cplan.CoexPlan(dm, dc) as plan:
		for _ in range(3):
			plan.step()
		_store(out, 'adopted', '_old', plan.results())
		fill(b, plan.device_results()['stream'])
		plan.step()
		_store(out, 'adopted', '_new', plan.results())
		infos['adopted'] = plan.info()
		infos['adopted_update'] = h.update_refused(plan, b)
		infos['adopted_upload_rc'] = int(lib.nrm_coex_plan_upload(plan._handle(), np.ascontiguousarray(b).ctypes.data))  # the library's own refusal
		infos['adopted_upload_msg'] = lib.nrm_last_error().decode()
	with cplan.CoexPlan(b, dc) as plan:
		_store(out, 'adopted', '_fresh', plan.step().results())
	h.free([dm.ptr])
	# an adopted matrix whose rows are 16-byte aligned but not contiguous (ld = n + 4): still the integer engine
	a, b, dc = arr['a'], arr['b'], arr['dc']
	dm, fill = h.adopted_matrix(b, b.shape[1] + 4, None)
	with cplan.CoexPlan(dm, dc) as plan:
		for _ in range(3):
			plan.step()
		_store(out, 'padded', '', plan.results())
		infos['padded'] = plan.info()
	h.free([dm.ptr])
	# update() on a plan-owned copy
	a, b, dc = arr['a2'], arr['b2'], arr['dc2']
	with cplan.CoexPlan(a, dc) as plan:
		for _ in range(3):
			plan.step()
		plan.update(b).step()
		_store(out, 'owned', '_new', plan.results())
		infos['owned'] = plan.info()
	with cplan.CoexPlan(b, dc) as plan:
		_store(out, 'owned', '_fresh', plan.step().results())
	# a pitch that is no multiple of 4: the fp64 kernel even at 4096 cells
	a, dc = arr['a3'], arr['dc3']
	dm, fill = h.adopted_matrix(a, a.shape[1] + 2, None)
	with cplan.CoexPlan(dm, dc) as plan:
		for _ in range(3):
			plan.step()
		_store(out, 'pitched', '', plan.results())
		infos['pitched'] = plan.info()
	h.free([dm.ptr])
	return infos


def scenario_guard(job, arr, out, lib, _lib, cplan):
	dt, dc = guard_inputs()
	sel = np.asarray(job['sel'])
	with cplan.CoexPlan(dt, dc, out_dtype=np.float64) as plan:
		plan.step().step()
		hits, worst = plan.check()
		info = plan.info()
		p, dot, var = plan.results()
		hits2, _ = plan.check()  # what the plan holds is certified now: nothing left to report
	out['p'], out['dot'], out['var'] = p[np.ix_(sel, sel)], dot[np.ix_(sel, sel)], var[sel]
	out['p_diag_zero'] = np.array((np.diag(p) == 0).all() and (p == p.T).all())
	return dict(hits=hits, worst=worst, hits_after=hits2, info=info)


def scenario_chain(job, arr, out, lib, _lib, cplan):
	"""coex -> binnet with the P-values never leaving HBM: nrm_binnet queued on the plan's stream behind the step, reading them where they lie; its byte matrix and
	counters go to page-locked host memory of the library (nrm_host_alloc: device-visible), all a caller without an array library has."""
	dt, dc, qcut = arr['dt'], arr['dc'], float(job['qcut'])
	ng = dt.shape[0]
	with cplan.CoexPlan(dt, dc) as plan:
		res = plan.device_results()
		mem = h.pinned(ng * ng + 32)  # the network, then the total (8 bytes) and, at +16, the flags
		h_cnt = mem + ng * ng
		for _ in range(3):  # the third is a replay
			plan.step()
			_lib.check(lib.nrm_fill_zero(h_cnt, 32, res['stream']))
			_lib.check(lib.nrm_binnet(res['p'], _lib.NRM_F64 if res['dtype'] == np.float64 else _lib.NRM_F32, ng, res['ld'], qcut, mem, ng, h_cnt, h_cnt + 16, res['stream']))
		plan.check()  # (waits for everything queued)
		out['net'] = np.frombuffer(ctypes.string_at(mem, ng * ng), dtype=np.uint8).reshape(ng, ng).copy()
		tail = ctypes.string_at(h_cnt, 32)
		out['total'] = np.frombuffer(tail[:8], dtype=np.uint64).copy()
		out['flags'] = np.frombuffer(tail[16:24], dtype=np.int32).copy()
		info = plan.info()
	h.free([mem])
	return info


def scenario_errors(job, arr, out, lib, _lib, cplan):
	a, b, dc = arr['a'], arr['b'], arr['dc']
	notes = {}
	bad = a.copy()
	bad[3, 7] = np.nan
	with cplan.CoexPlan(bad, dc) as plan:
		plan.step().step().step()
		notes['nan'] = h.raised(plan.check, catch=AssertionError)
		plan.update(a).step()
		_store(out, 'after_nan', '', plan.results())
		notes['after_nan'] = plan.info()
	# two plans alive, stepped alternately, the scratch pool emptied between their steps
	with cplan.CoexPlan(a, dc) as pa, cplan.CoexPlan(b, dc, dimreduce=1) as pb:
		for i in range(4):
			pa.step()
			pb.step()
			if i == 1:
				pa.check(), pb.check()
				_lib.check(lib.nrm_release_cache())
		_store(out, 'two_a', '', pa.results())
		_store(out, 'two_b', '', pb.results())
		notes['two_a'], notes['two_b'] = pa.info(), pb.info()
	with cplan.CoexPlan(a, dc) as plan:
		_store(out, 'fresh_a', '', plan.step().results())
	with cplan.CoexPlan(b, dc, dimreduce=1) as plan:
		_store(out, 'fresh_b', '', plan.step().results())
	return notes


def scenario_teardown(job, arr, out, lib, _lib, cplan):
	"""The pool's own accounting (nrm_cache_bytes) around a plan's life."""
	def pool():
		held, used = ctypes.c_int64(-1), ctypes.c_int64(-1)
		_lib.check(lib.nrm_cache_bytes(ctypes.byref(held), ctypes.byref(used)))
		return [int(held.value), int(used.value)]
	notes = {}
	_lib.check(lib.nrm_release_cache())
	notes['before'] = pool()
	plan = cplan.CoexPlan(arr['a'], arr['dc'])
	plan.step().step().step()
	plan.results()
	notes['alive'] = pool()
	notes['bytes'] = plan.info()['bytes']
	_lib.check(lib.nrm_release_cache())
	notes['alive_after_release'] = pool()
	plan.close()
	notes['closed'] = pool()
	_lib.check(lib.nrm_release_cache())
	notes['released'] = pool()
	plan.close()  # twice is fine
	return notes


if __name__ == '__main__':
	h.child_main(sys.argv, globals())
