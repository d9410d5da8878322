"""The resident front-half plan on CSR counts (include/normalisr_hip.h: nrm_front_plan_create_csr / _upload_csr; normalisr_amd.cplan.FrontPlanCSR) on the GPU.
Every plan call is made by a child process in which torch cannot be imported (tests/front_plan_csr_child.py); this process holds what comes back to what the
reference returned (golden G18_front, G18_front_chain) and to the dense plan of the same matrix in the same child.  Bars: those of tests/test_gpu_front_plan.py
for the dense plan -- fp64 quantities close(1e-9, floor=1), scaling factors 1e-12 absolute, P-values 1e-6 relative -- and, against the dense plan, what
tests/test_gpu_lcpm_sparse.py holds the sparse lcpm to against the dense one (the same close(1e-9, floor=1): only the order of the per-cell sum differs), with
the integer stages (the covariates before normcov's scaling come from integer totals; the scaling factors from integer zero counts) bit for bit; replays,
rewrites and refusals bit for bit.  Shapes sit at the kernels' seams: 32 rows a tile, 4096 cells a chunk, 64 entries a wave step."""
import functools

import numpy as np
import pytest
import scipy.sparse

import cabi_harness
import front_plan_csr_child as child
from cabi_harness import close, p_close

pytestmark = pytest.mark.gpu
run_child = functools.partial(cabi_harness.run_child, 'front_plan_csr_child.py', timeout=180)
STAGES = child.STAGES
MALFORMED = ('ValueError: Malformed CSR matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and '
			 'increase strictly (sum duplicates and sort the indices first).')


def ok(a, b):
	return close(a, b, 1e-9, floor=1.0)


def stages(out, name):
	return {k: out['{}.{}'.format(name, k)] for k in STAGES}


def same_bits(a, b, what):
	for k in STAGES:
		assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def test_front_plan_csr_golden_chain(golden, tmp_path):
	"""(a) G18 as scipy.sparse.csr_matrix(reads) through one CSR plan per stepmax, against what the reference returned for every stage, and coex from a CoexPlan
	that adopts dtn where it lies."""
	g, hh = golden('G18_front'), golden('G18_front_chain')
	reads, user = g['reads'], hh['cov_raw'][:4]
	m = scipy.sparse.csr_matrix(reads)
	assert reads.shape == (112, 240) and 0.3 < m.nnz / reads.size < 0.4
	cases = [dict(name='s1', reads='g', shape=m.shape, cov='user', stepmax=1, kinds=['csr'], coex=True), dict(name='s3', reads='g', shape=m.shape, cov='user', stepmax=3, kinds=['csr'])]
	out, info = run_child(tmp_path, 'cases', dict(user=user, **child.csr_arrays('g', m)), dict(cases=cases))
	print(info)
	s1, s3 = stages(out, 's1.csr'), stages(out, 's3.csr')
	for s in (s1, s3):
		assert s['lcpm'].dtype == np.float64 and ok(s['lcpm'], g['lcpm']) and ok(s['cov'], hh['normcov_c'])
		assert np.abs(s['wt'] - g['sf']).max() <= 1e-12
	assert ok(s1['w'], hh['w1']) and ok(s3['w'], hh['w3'])
	assert ok(s1['dtn'], hh['nv_exp']) and ok(s1['dcn'], hh['nv_cov'])
	assert p_close(out['s1.coex.p'], hh['coex_p']) and close(out['s1.coex.var'], hh['coex_var'], 1e-9)
	for name in ('s1.csr', 's3.csr'):
		assert info[name]['captured'] == 1 and info[name]['steps'] == 2 and info[name]['covariates'] == 8 and info[name]['max_count'] == reads.max()
		assert info[name]['count_cap'] == 1 << int(reads.max()).bit_length()


def _against_dense(out, info, name, adopted=False):
	c, d = stages(out, name + '.csr'), stages(out, name + '.dense')
	for kind in ('csr', 'dense'):
		assert info['{}.{}'.format(name, kind)]['captured'] == 1
	assert np.isfinite(d['dtn']).all() and np.isfinite(c['dtn']).all()
	for k in ('cov', 'wt'):  # the same integers through the same code
		assert c[k].dtype == d[k].dtype and np.array_equal(c[k], d[k]), (name, k)
	for k in ('lcpm', 'w', 'dtn', 'dcn'):
		assert ok(c[k], d[k]), (name, k)
	same_bits(c, stages(out, name + '.csr_again'), name + ': two fresh CSR plans')
	if adopted:  # stored zeros are entries like any other to the kernels, and count for nothing
		same_bits(c, stages(out, name + '.adopted'), name + ': the arrays as stored, zeros included')
	return c


def test_front_plan_csr_against_dense_at_the_seams(tmp_path):
	"""(b) 70 x 4133 int32 (child.seam_matrix says what it holds), CSR plan against dense plan in the same child; fp32 output is the fp64 lcpm rounded once.
	stepmax is the plans' default, 1, and the reason is the matrix, not the kernels.  The two plans' lcpm differ by one or two ulp of t1[k] in 137 cells (the
	order of the per-cell sum; at most 3.6e-15, the same for every gene of a cell) and their weights by 4e-14.  What normvar makes of that is the conditioning of
	one row: the gene without a read has lcpm T[0] - t1[k], nearly a function of the cell's total and so nearly in the span of lcpm's own covariate rows; its
	residual is small, normvar's entries for it reach 466, and every figure below is that row's -- no other row differs by more than 1.3e-11.  The CPU oracle's
	normvar on the two plans' own (lcpm, cov, w, wt) differs by 2.8e-10 of |dtn| + 1 between them at stepmax = 1 and by 2.1e-9 at stepmax = 2, where compute_var's
	second iteration has amplified the weights' difference to 9e-13: at stepmax = 2 the 1e-9 bar is out of reach on this matrix for any two implementations that
	order the sum differently (the plans differ by 1.8e-9 there; the dense plan differs from the oracle on its own inputs by 3e-9).  At stepmax = 1 the plans
	differ by 9.1e-10 in that row: inside the bar, not by much, and the same bits every run.  stepmax 3 is covered by the golden chain."""
	m = child.seam_matrix()
	cov = child.onehot(91, 2, m.shape[1])
	case = dict(name='seam', reads='m', shape=m.shape, cov='cov', stepmax=1, count_cap=131072, kinds=['csr', 'csr_again', 'adopted', 'dense', 'csr_f32'])
	out, info = run_child(tmp_path, 'cases', dict(cov=cov, **child.csr_arrays('m', m)), dict(cases=[case]))
	print(info)
	c = _against_dense(out, info, 'seam', adopted=True)
	assert info['seam.csr']['max_count'] == 70000 and info['seam.csr']['count_cap'] == 131072
	f = stages(out, 'seam.csr_f32')
	assert f['lcpm'].dtype == np.float32 and f['dtn'].dtype == np.float32 and np.array_equal(f['lcpm'], c['lcpm'].astype(np.float32))


@pytest.mark.parametrize('ng,n,dtype,seed', [(33, 65, 'int64', 92), (40, 4099, 'uint8', 93)])
def test_front_plan_csr_against_dense_other_dtypes(tmp_path, ng, n, dtype, seed):
	"""(b) 33 x 65 int64 (a second row tile of one row, a cell past the wave) and 40 x 4099 uint8 (a second chunk of three cells)."""
	m = scipy.sparse.csr_matrix(child.counts(seed, ng, n, np.dtype(dtype)))
	assert m.data.dtype == np.dtype(dtype)
	case = dict(name='d', reads='m', shape=m.shape, cov=None, stepmax=1, kinds=['csr', 'csr_again', 'dense'])
	out, info = run_child(tmp_path, 'cases', child.csr_arrays('m', m), dict(cases=[case]))
	print(info)
	_against_dense(out, info, 'd')


def test_front_plan_csr_rewrites_behind_the_graph(tmp_path):
	"""(c) After the graph exists the counts change, pattern included: fewer stored entries with another total and a larger maximum, then more, then the first matrix
	again.  Each replay is a fresh plan's first step bit for bit -- the last also the very first step's, since what lies past indptr[rows] is not read -- for the
	plan's own arrays (update) and for an adopted DeviceCSR rewritten in place; the graph is captured once."""
	shape, cap = (40, 300), 5200
	a, b, c, d = (child.sparse_counts(100 + i, *shape, dens, top=top) for i, (dens, top) in enumerate(((0.3, 9), (0.15, 200), (0.4, 9), (0.6, 9))))
	assert b.nnz < a.nnz < c.nnz <= cap < d.nnz and b.sum() != a.sum() and b.max() > a.max() and b.max() < 256
	arrays = dict(cov=child.onehot(104, 3, shape[1]))
	for k, m in zip('abcd', (a, b, c, d)):
		arrays.update(child.csr_arrays(k, m))
	out, notes = run_child(tmp_path, 'rewrite', arrays, dict(shape=shape, count_cap=256, nnz_cap=cap))
	print(notes)
	fresh = {k: stages(out, 'fresh_' + k) for k in 'abc'}
	assert not np.array_equal(fresh['a']['dtn'], fresh['b']['dtn']) and not np.array_equal(fresh['b']['dtn'], fresh['c']['dtn'])
	for kind in ('own', 'adopted'):
		for step, (run, want, top) in enumerate((('a', 'a', a), ('b', 'b', b), ('c', 'c', c), ('a2', 'a', a)), 2):
			i = notes['{}_{}'.format(kind, run)]
			assert i['captured'] == 1 and i['steps'] == step and i['max_count'] == top.max(), (kind, run, i)
			same_bits(stages(out, '{}_{}'.format(kind, run)), fresh[want], (kind, run))
		same_bits(stages(out, kind + '_a2'), stages(out, kind + '_first'), kind + ': back to the first matrix')
	assert notes['own_a']['bytes'] == notes['fresh_b']['bytes'] == notes['fresh_c']['bytes']  # the capacities size the plan, not the matrix
	assert 'adopted' in notes['adopted_update']
	assert notes['own_beyond'].startswith('ValueError') and '{} stored entries'.format(d.nnz) in notes['own_beyond'] and 'nnz_cap = {}'.format(cap) in notes['own_beyond']
	for key, words in (('own_dense_upload', 'holds CSR counts'), ('own_c_beyond', 'beyond the plan\'s nnz_cap'), ('dense_csr_upload', 'holds a dense matrix')):
		assert notes[key][0] == -1 and words in notes[key][1], (key, notes[key])  # NRM_E_ARG
	assert notes['own_after_refusal']['captured'] == 1
	same_bits(stages(out, 'own_after_refusal'), fresh['a'], 'after the refused uploads')


def _bad_matrices(good, n, nnz_cap, count_cap):
	"""The raw arrays of every matrix check() must refuse, from the arrays of a good one (canonical, int32)."""
	p, idx, val = good.indptr.astype(np.int64), good.indices.astype(np.int32), good.data.astype(np.int32)
	rows = p.size - 1
	assert (np.diff(p) >= 3).all()
	bad = {}

	def put(name, indptr=p, indices=idx, data=val):
		bad[name] = (indptr.copy(), indices.copy(), data.copy())
		return bad[name]
	_, i, v = put('dup_col_negative')  # a column repeated inside row 3 -- and a negative entry elsewhere, which a malformed matrix is reported in front of
	i[p[3] + 1] = i[p[3]]
	v[p[20]] = -1
	_, i, _ = put('col_n')  # the last column of row 4 equal to n
	i[p[5] - 1] = n
	q, _, _ = put('falling')  # indptr decreasing between rows 9 and 10
	q[10] = q[9] - 1
	q, _, _ = put('past_cap')  # indptr[rows] a few past the capacity (the buffers physically hold twice as much)
	q[rows] = nnz_cap + 5
	cell = idx == 7
	assert cell.sum() >= 2 and not cell[p[20]] and not cell[p[21]]
	for name, negative, empty in (('negative_empty_cap', True, True), ('empty_cap', False, True), ('cap', False, False)):
		_, _, v = put(name)
		v[p[21]] = count_cap  # a count at the cap
		if negative:
			v[p[20]] = -1
		if empty:
			v[cell] = 0  # every entry of cell 7 a stored zero: a cell without a read
	return bad


def test_front_plan_csr_refusals_from_the_device_counters(tmp_path):
	"""(d) A malformed matrix -- a repeated column, a column equal to n, indptr decreasing, indptr[rows] past nnz_cap -- is a ValueError in the eager CSR path's
	words, in front of everything else; a well-formed one is refused in FrontPlan's order: a negative entry, a cell without a read, a count at count_cap.  After
	each, the good matrix again and one step give the good result bit for bit: the counters were cleared, and nothing was read or written out of place."""
	shape, count_cap = (40, 300), 256
	good = child.sparse_counts(110, *shape, 0.3)
	nnz_cap = good.nnz + 40
	bad = _bad_matrices(good, shape[1], nnz_cap, count_cap)
	arrays = dict(cov=child.onehot(111, 2, shape[1]), **child.csr_arrays('good', good))
	for name, (p, i, v) in bad.items():
		arrays.update({name + '_indptr': p, name + '_indices': i, name + '_data': v})
	out, notes = run_child(tmp_path, 'refusals', arrays, dict(shape=shape, count_cap=count_cap, nnz_cap=nnz_cap, bad=list(bad)))
	print(notes)
	assert notes['good'] == 'accepted'
	for name in ('dup_col_negative', 'col_n', 'falling', 'past_cap'):
		assert notes[name] == MALFORMED, name
	assert notes['negative_empty_cap'] == 'ValueError: Negative value in d detected.'
	assert notes['empty_cap'] == 'ValueError: Found cell with no read at all. Please remove.'
	assert notes['cap'].startswith('NotImplementedError') and 'count_cap = {}'.format(count_cap) in notes['cap'] and 'largest count here is {}'.format(count_cap) in notes['cap']
	fresh = stages(out, 'fresh')
	for name in bad:
		assert notes[name + '.again'] == 'accepted' and notes[name + '.after'] == 'accepted', name
		same_bits(stages(out, name + '.after'), fresh, name)
	assert notes['info']['captured'] == 1 and notes['info']['steps'] == 2 + 3 * len(bad)


def test_front_plan_csr_takes_no_dense_counts(tmp_path):
	"""(e) 256 x 8192 int32 at about 10 % stored: info()['bytes'] of the CSR plan lies below the dense plan's.  Everything but the counts and the count pass's slabs
	is the same in both.  At up to 25 % stored entries the CSR arrays cost 8 bytes an entry, at most 2 bytes per element of the matrix, and the CSR slabs
	genes / 32 x n_cells x 8 bytes, a quarter of a byte per element, where the dense matrix alone costs 4: a plan that had taken a (genes, n_cells) buffer of counts
	as well could not lie below.  A condition, not a measurement."""
	shape = (256, 8192)
	m = child.sparse_counts(120, *shape, 0.1)
	assert 0.08 < m.nnz / (shape[0] * shape[1]) < 0.25
	out, notes = run_child(tmp_path, 'bytes', child.csr_arrays('x', m), dict(shape=shape))
	print(notes)
	assert notes['csr_check'] == 'accepted' and notes['dense_check'] == 'accepted'
	assert 0 < notes['csr']['bytes'] < notes['dense']['bytes']
	assert notes['dense']['bytes'] - notes['csr']['bytes'] > shape[0] * shape[1] * 4 // 4  # what the CSR side may cost at most leaves a quarter of the dense matrix and more
	assert ok(out['csr.lcpm'], out['dense.lcpm'])
