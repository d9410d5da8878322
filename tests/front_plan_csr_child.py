"""The child side of tests/test_gpu_front_plan_csr.py: a process in which torch cannot be imported makes every call on the library's resident front-half plan on
CSR counts (normalisr_amd.cplan.FrontPlanCSR) -- and, beside it, on the dense plan of the same matrix -- and writes what it got to an .npz; the parent compares.
`python tests/front_plan_csr_child.py SCENARIO IN.npz OUT.npz`.  A matrix travels as its three CSR arrays exactly as stored (NAME_indptr, NAME_indices, NAME_data:
explicit zeros stay), with its shape in the job.  The generators at the top are shared with the parent (which imports this module; nothing here touches torch); the
frame of the child, the device-visible copies and the stages' store are those of tests/cabi_harness.py and tests/front_plan_child.py."""
import sys

import numpy as np

import cabi_harness as h
from front_plan_child import STAGES, _store, counts, onehot  # noqa: F401 -- the parent takes the generators from here


def csr_arrays(name, m):
	"""The three arrays of a scipy CSR matrix as stored, under the names the child reads them by."""
	return {name + '_indptr': m.indptr.astype(np.int64), name + '_indices': m.indices.astype(np.int32), name + '_data': m.data}


def seam_matrix(seed=90, ng=70, n=4133, top=70000):
	"""70 x 4133 int32 at the seams of the CSR kernels (32 rows a tile: three tiles, the last of 6 rows; 4096 cells a chunk: two chunks, the second of 37 cells; 64
	entries a wave step) as a scipy CSR matrix with stored zeros: gene 5 without a read, gene 6 with a read in every cell (so that every cell has one), genes 7 and 8
	with exactly 64 and 65 stored entries, spread over both chunks, one count of `top`, and every third stored entry of the other genes an explicit zero."""
	import scipy.sparse
	rng = np.random.default_rng(seed)
	x = counts(seed, ng, n).astype(np.int64)
	x[5] = 0
	x[6] = 1 + rng.integers(0, 4, n)
	for g, k in ((7, 64), (8, 65)):
		x[g] = 0
		x[g, np.sort(rng.choice(n, k, replace=False))[:k - 2]] = 2
		x[g, [n - 30, n - 1]] = 3  # (two of them in the short second chunk)
		assert (x[g] != 0).sum() == k
	x[1, 2] = top
	m = scipy.sparse.csr_matrix(x.astype(np.int32))
	rows = np.repeat(np.arange(ng), np.diff(m.indptr))
	zeroed = (np.arange(m.nnz) % 3 == 0) & ~np.isin(rows, (1, 6, 7, 8))
	m.data[zeroed] = 0
	dense = m.toarray()
	assert m.nnz == (x != 0).sum() and (m.data == 0).sum() > m.nnz // 4 and (dense.sum(axis=0) > 0).all() and dense.max() == top
	assert np.diff(m.indptr)[7] == 64 and np.diff(m.indptr)[8] == 65 and not dense[5].any() and dense[6].all()
	return m


def sparse_counts(seed, ng, n, density, dtype=np.int32, top=9):
	"""Seeded CSR counts 1 .. top at about `density` stored entries, canonical, every cell with a read, every gene with a zero."""
	import scipy.sparse
	rng = np.random.default_rng(seed)
	x = np.where(rng.random((ng, n)) < density, rng.integers(1, top + 1, (ng, n)), 0)
	x[rng.integers(0, ng, n), np.arange(n)] += 1
	x[np.arange(ng), np.arange(ng) % n] = 0
	x[(np.arange(n) + 1) % ng, np.arange(n)] += (x.sum(axis=0) == 0)
	assert (x.sum(axis=0) > 0).all() and ((x == 0).sum(axis=1) > 0).all()
	return scipy.sparse.csr_matrix(x.astype(dtype))


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
def _matrix(arr, name, shape):
	import scipy.sparse
	return scipy.sparse.csr_matrix((arr[name + '_data'], arr[name + '_indices'], arr[name + '_indptr']), shape=tuple(shape))


class Adopted:
	"""A CSR matrix as stored in device-visible memory of the library: indptr, and indices and data of `phys` elements each (zeroed), as a cplan.DeviceCSR; fill and
	fill_raw rewrite the arrays in place through nrm_upload on a stream -- only the entries given, what lies behind them stays."""

	def __init__(self, cplan, m, phys):
		from normalisr_amd import _lib
		self._lib, self.dtype, self.rows, self.phys = _lib, m.data.dtype, m.shape[0], int(phys)
		self.ptrs = [h.pinned((self.rows + 1) * 8), h.pinned(self.phys * 4), h.pinned(self.phys * self.dtype.itemsize)]
		self.fill_raw(np.zeros(self.rows + 1, np.int64), np.zeros(self.phys, np.int32), np.zeros(self.phys, self.dtype), None)
		self.fill(m, None)
		self.csr = cplan.DeviceCSR(self.ptrs[0], self.ptrs[1], self.ptrs[2], m.shape, m.nnz, self.dtype)

	def fill_raw(self, indptr, indices, data, stream):
		assert indptr.size == self.rows + 1 and indices.size == data.size <= self.phys
		for ptr, a in zip(self.ptrs, (indptr.astype(np.int64), indices.astype(np.int32), data.astype(self.dtype))):
			a = np.ascontiguousarray(a)
			if a.nbytes:
				self._lib.check(self._lib.load().nrm_upload(a.ctypes.data, ptr, a.nbytes, 0, stream))

	def fill(self, m, stream):
		self.fill_raw(m.indptr, m.indices, m.data, stream)

	def free(self):
		h.free(self.ptrs)


def _kw(c, arr):
	return dict(cov=None if c.get('cov') is None else arr[c['cov']], stepmax=c.get('stepmax', 1), count_cap=c.get('count_cap'))


def scenario_cases(job, arr, out, lib, _lib, cplan):
	"""Every case: its matrix through the plans named in `kinds`, `steps` steps each, the stages of the last step as NAME.KIND.*, info() as NAME.KIND -- csr and
	csr_again (two fresh CSR plans on the scipy matrix), csr_f32, adopted (the arrays as stored, stored zeros included), dense and dense_f32 (FrontPlan on
	toarray()); coex: a CoexPlan adopting the first CSR plan's dtn where it lies."""
	infos = {}
	for c in job['cases']:
		m = _matrix(arr, c['reads'], c['shape'])
		for kind in c['kinds']:
			kw = dict(_kw(c, arr), out_dtype=np.float32 if kind.endswith('_f32') else np.float64)
			held = None
			if kind.startswith('dense'):
				plan = cplan.FrontPlan(m.toarray(), **kw)
			elif kind == 'adopted':
				held = Adopted(cplan, m, m.nnz)
				plan = cplan.FrontPlanCSR(held.csr, nnz_cap=m.nnz, **kw)
			else:
				plan = cplan.FrontPlanCSR(m, **kw)
			name = '{}.{}'.format(c['name'], kind)
			with plan:
				for _ in range(c.get('steps', 2)):
					plan.step()
				_store(out, name, plan)
				infos[name] = plan.info()
				if c.get('coex') and kind == 'csr':
					with cplan.CoexPlan(plan.device_results()['dtn'], plan.results()[1]) as coex:
						coex.step()
						h.store(out, c['name'] + '.coex', coex.results(), h.COEX_KEYS)
			if held is not None:
				held.free()
	return infos


def scenario_rewrite(job, arr, out, lib, _lib, cplan):
	"""Behind a captured graph: the counts replaced by a matrix of fewer stored entries, then one of more, then the first again -- through update() on the plan's
	own arrays and through an adopted DeviceCSR rewritten in place on the plan's stream -- beside fresh plans of the same capacities on each matrix."""
	shape, cov = job['shape'], arr['cov']
	a, b, c, d = (_matrix(arr, k, shape) for k in 'abcd')
	kw = dict(cov=cov, stepmax=2, count_cap=job['count_cap'], nnz_cap=job['nnz_cap'])
	notes = {}

	def sequence(kind, plan, put):
		plan.step()
		_store(out, kind + '_first', plan)
		plan.step()
		_store(out, kind + '_a', plan)
		notes[kind + '_a'] = plan.info()
		for name, m in (('b', b), ('c', c), ('a2', a)):
			put(m)
			plan.step()
			_store(out, '{}_{}'.format(kind, name), plan)
			notes['{}_{}'.format(kind, name)] = plan.info()

	with cplan.FrontPlanCSR(a, **kw) as plan:
		sequence('own', plan, plan.update)
		notes['own_beyond'] = h.raised(lambda: plan.update(d))  # more stored entries than nnz_cap: refused before any device call ...
		dense_a, big = a.toarray(), [np.ascontiguousarray(v) for v in (d.indptr.astype(np.int64), d.indices.astype(np.int32), d.data)]
		notes['own_dense_upload'] = [lib.nrm_front_plan_upload(plan._handle(), dense_a.ctypes.data), lib.nrm_last_error().decode()]
		notes['own_c_beyond'] = [lib.nrm_front_plan_upload_csr(plan._handle(), big[0].ctypes.data, big[1].ctypes.data, big[2].ctypes.data, d.nnz), lib.nrm_last_error().decode()]
		plan.step()
		_store(out, 'own_after_refusal', plan)  # ... so the plan still holds the first matrix
		notes['own_after_refusal'] = plan.info()
	for name, m in (('a', a), ('b', b), ('c', c)):
		with cplan.FrontPlanCSR(m, **kw) as plan:
			_store(out, 'fresh_' + name, plan.step())
			notes['fresh_' + name] = plan.info()
	held = Adopted(cplan, a, job['nnz_cap'])
	with cplan.FrontPlanCSR(held.csr, **kw) as plan:
		stream = plan.device_results()['stream']
		sequence('adopted', plan, lambda m: held.fill(m, stream))
		notes['adopted_update'] = h.update_refused(plan, b)
	held.free()
	with cplan.FrontPlan(a.toarray(), cov, stepmax=2, count_cap=job['count_cap']) as plan:
		mine = [np.ascontiguousarray(v) for v in (a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data)]
		notes['dense_csr_upload'] = [lib.nrm_front_plan_upload_csr(plan._handle(), mine[0].ctypes.data, mine[1].ctypes.data, mine[2].ctypes.data, a.nnz), lib.nrm_last_error().decode()]
	return notes


def scenario_refusals(job, arr, out, lib, _lib, cplan):
	"""One adopted plan rewritten in turn with every matrix of job['bad'] (raw arrays: nothing here canonicalises them), two steps and a check for each, then the good
	matrix again, one step, a check and the stages.  The indices and data buffers physically hold twice nnz_cap elements, so that an offset a few past nnz_cap
	stays inside the allocation whatever a kernel does with it."""
	shape, cov, cap = job['shape'], arr['cov'], job['nnz_cap']
	good = _matrix(arr, 'good', shape)
	kw = dict(cov=cov, count_cap=job['count_cap'], nnz_cap=cap)
	notes = {}
	with cplan.FrontPlanCSR(good, **kw) as plan:
		_store(out, 'fresh', plan.step())
	held = Adopted(cplan, good, 2 * cap)
	with cplan.FrontPlanCSR(held.csr, **kw) as plan:
		stream = plan.device_results()['stream']
		plan.step().step()
		notes['good'] = h.raised(plan.check)
		for name in job['bad']:
			held.fill_raw(arr[name + '_indptr'], arr[name + '_indices'], arr[name + '_data'], stream)
			plan.step().step()
			notes[name] = h.raised(plan.check)
			notes[name + '.again'] = h.raised(plan.check)  # (the counters were cleared)
			held.fill(good, stream)
			plan.step()
			notes[name + '.after'] = h.raised(plan.check)
			_store(out, name + '.after', plan)
		notes['info'] = plan.info()
	held.free()
	return notes


def scenario_bytes(job, arr, out, lib, _lib, cplan):
	"""info()['bytes'] of a CSR plan and of the dense plan on the same counts, each after a step that check() accepts."""
	m = _matrix(arr, 'x', job['shape'])
	notes = {}
	with cplan.FrontPlanCSR(m) as plan:
		notes['csr_check'] = h.raised(plan.step().check)
		notes['csr'] = plan.info()
		out['csr.lcpm'] = plan.lcpm()
	with cplan.FrontPlan(m.toarray()) as plan:
		notes['dense_check'] = h.raised(plan.step().check)
		notes['dense'] = plan.info()
		out['dense.lcpm'] = plan.lcpm()
	return notes


if __name__ == '__main__':
	h.child_main(sys.argv, globals())
