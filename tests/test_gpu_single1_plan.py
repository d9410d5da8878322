"""The resident single=1 plan of the C ABI (include/normalisr_hip.h: nrm_single1_plan_*; normalisr_amd/cplan.py: Single1Plan) on the GPU.  Every plan call is made by a
child process in which torch cannot be imported (tests/single1_plan_child.py); this process holds what comes back to the reference's golden vectors, to the oracle
and to normalisr_amd.single1.Single1Plan (the torch plan) on the rows de keeps.

Bars.  Golden G5 as tests/test_gpu_parity.py::test_single1_golden_and_oracle holds the public call: P-values 1e-6 relative, gamma 1e-6 (floor 1e-12), alpha 1e-6 (floor
1e-10), varg and vart 1e-9.  Golden G24 and the oracle as `held` of tests/test_gpu_single1_wide.py.  The torch plan runs the same launches in the same order on the
same lists, and a replay the launches of an eager step: against either every array is equal, bit for bit.  The ones and zeros of rows that are not tested are exact.

The screen (tests/single1_plan_child.py::screen): 65 groupings x 69 genes x 2051 cells with entries set with probability 1 / 65, and two rows de drops -- one all
zeros, one ALL ONES, which left in would leave no cell with exactly one grouping.  tests/test_single1_plan_cpu.py holds every seed used here to the oracle's own
assertions (each kept grouping varies on its selected cells, dof > 0)."""
import functools
import os

import numpy as np
import pytest

import oracle
import single1_plan_child as child
from cabi_harness import close, got, held, p_close, same, untested_rows_exact
from cabi_harness import run_child as _run_child

pytestmark = pytest.mark.gpu

run_child = functools.partial(_run_child, 'single1_plan_child.py')  # (timeout=240)
KEPT = child.kept_rows()
DROPPED = [child.ZERO_ROW, child.ONES_ROW]
SEEDS, NCS = child.SEEDS, child.NCS
FORMS = ['dense', 'scipy', 'devcsr', 'devcsr_data']  # (devcsr: no data array, every entry is 1; devcsr_data: with one)


def inflate(res, ng0, kept):
	"""de._inflate (de.py:107-122) for single=1's outputs: p = 1, gamma = alpha = varg = vart = 0 on the rows that were not tested."""
	p, gam, a, vx, vy = res
	nt = p.shape[1]
	P, G = np.ones((ng0, nt), p.dtype), np.zeros((ng0, nt), gam.dtype)
	A = None if a is None else np.zeros((ng0, nt, a.shape[2]), a.dtype)
	VG, VT = np.zeros(ng0, vx.dtype), np.zeros((ng0, nt), vy.dtype)
	P[kept], G[kept], VG[kept], VT[kept] = p, gam, vx, vy
	if a is not None:
		A[kept] = a
	return P, G, A, VG, VT


def torch_plan(dg, dt, dc, lowmem):
	"""normalisr_amd.single1.Single1Plan on the rows de keeps, one step, inflated in numpy."""
	import torch
	from normalisr_amd.single1 import Single1Plan
	plan = Single1Plan(torch.from_numpy(np.ascontiguousarray(dg[KEPT])).cuda(), torch.from_numpy(dt).cuda(), dc, return_dot=False, lowmem=lowmem)
	plan.step()
	assert plan.cells_kept() == child.exclusive_cells(dg)
	return inflate(plan.results(), dg.shape[0], KEPT), plan.cells_kept()


def test_single1_plan_c_entry_golden(golden, tmp_path):
	"""G5 (six groupings, three covariates) and G24 (seven groupings; 12 covariates of rank 11, 32 of rank 32): the reference's own arrays, every row tested, so the
	sweep writes the full-size arrays itself; fp32 inputs give fp32 outputs."""
	g5, g24 = golden('G5_single'), golden('g24')
	arrays = dict(g5_dg=g5['s1_dg'], g5_dt=g5['dt'], g5_dc=g5['dc'], dx=g24['dx'], dy=g24['dy'], c12=g24['c12_dc'], c32=g24['c32_dc'], g5_dt32=g5['dt'].astype(np.float32),
				  g5_dc32=g5['dc'].astype(np.float32))
	cases = [dict(name='g5', dg='g5_dg', dt='g5_dt', dc='g5_dc', lowmem=False, forms=['dense', 'scipy']), dict(name='g5lm', dg='g5_dg', dt='g5_dt', dc='g5_dc'),
			 dict(name='g5f32', dg='g5_dg', dt='g5_dt32', dc='g5_dc32', lowmem=False), dict(name='c12', dg='dx', dt='dy', dc='c12', lowmem=False, steps=3),
			 dict(name='c32', dg='dx', dt='dy', dc='c32', lowmem=False, steps=3)]
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	for name, v in info.items():
		print(name, v)
	for name in ('g5.dense', 'g5.scipy', 'g5lm.dense'):
		p, gam, a, vg, vt = got(out, name)
		assert info[name]['rows_kept'] == 6 and info[name]['covariates'] == 3 and info[name]['steps'] == 1 and info[name]['captured'] == 0
		assert p.shape == (6, 40) and vt.shape == (6, 40) and vg.shape == (6, ) and p.dtype == np.float64
		assert p_close(p, g5['s1_p']) and close(gam, g5['s1_gamma'], floor=1e-12)
		assert close(vg, g5['s1_varg'], 1e-9) and close(vt, g5['s1_vart'], 1e-9)
		assert (a is None) if name == 'g5lm.dense' else (a.shape == (6, 40, 3) and close(a, g5['s1_alpha'], floor=1e-10))
	same(got(out, 'g5.dense'), got(out, 'g5.scipy'), 'the design forms')
	res = got(out, 'g5f32.dense')
	assert all(x.dtype == np.float32 for x in res) and res[0].shape == (6, 40) and res[2].shape == (6, 40, 3)  # (fp32 values: held to the oracle in the next test)
	for name in ('c12', 'c32'):
		want = tuple(g24['%s_%s' % (name, k)] for k in ('p', 'gamma', 'alpha', 'varx', 'vary'))
		held(got(out, name + '.dense'), want, np.float64, want[2].shape[2])
		assert info[name + '.dense']['rows_kept'] == 7 and info[name + '.dense']['captured'] == 1


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_single1_plan_c_entry_same_bytes_as_the_torch_plan(tmp_path, dtype):
	"""0, 3, 8 (a lane per grouping), 9 and 32 (a wave per grouping) covariates with the intercept last; lowmem both ways; dense numpy, scipy CSR and device CSR arrays
	with and without a data array in: the five outputs of the torch plan on the 65 rows kept, inflated as de.py:107-122 does -- bit for bit; the oracle at the bars
	of `held`."""
	cases = []
	for nc in NCS:
		for lowmem in (True, False):
			cases.append(dict(name='c{}_{}'.format(nc, int(lowmem)), lowmem=lowmem, forms=FORMS, steps=1, screen=dict(seed=SEEDS['same'] + nc, dtype=dtype, nc=nc)))
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	for c in cases:
		dg, dt, dc = child.screen(**dict(c['screen'], dtype=np.dtype(dtype)))
		want, cells = torch_plan(dg, dt, dc, c['lowmem'])
		assert want[0].dtype == np.dtype(dtype)
		for form in FORMS:
			name = '{}.{}'.format(c['name'], form)
			v = info[name]
			assert v['rows_kept'] == 65 and v['cells_kept'] == cells and v['covariates'] == c['screen']['nc'] and v['captured'] == 0 and v['route'] == 0, (name, v)
			res = got(out, name)
			same(res, want, name)
			untested_rows_exact(res, DROPPED)
		if not c['lowmem']:
			ref = oracle.association_tests(dg[KEPT], dt.astype(np.float64), dc, single=1, return_dot=False, lowmem=False)
			res = got(out, c['name'] + '.dense')
			nc = c['screen']['nc']
			alpha = ref[2] if nc else np.zeros((65, child.NY, 0))
			held((res[0][KEPT], res[1][KEPT], res[2][KEPT], res[3][KEPT], res[4][KEPT]), (ref[0], ref[1], alpha, ref[3], ref[4]), np.dtype(dtype), nc)


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_single1_plan_c_entry_same_bytes_as_the_host_entry(tmp_path, dtype):
	"""The whole-problem entry and the plan run one step record (csrc/nrm_single1_step.h): norm.de(..., single=1, lowmem=False) in a process without torch
	(NRM_HOST_ENTRY=1: nrm_association_tests_single1_host) and cplan.Single1Plan on the same arrays give P, gamma, alpha, varg and vart equal bit for bit.
	7 design rows over 203 cells, each cell in at most one row and 43 in none, row 4 constant (the plan compacts and re-inflates); 37 genes; 0, 3 (a lane per
	grouping) and 9 (a wave per grouping) covariates."""
	cases = [dict(name='c{}'.format(nc), nc=nc, dtype=dtype) for nc in child.ENTRY_NCS]
	out, info = run_child(tmp_path, 'entry', {}, dict(cases=cases), env={'NRM_HOST_ENTRY': '1'})
	for c in cases:
		v = info[c['name']]
		print(c['name'], v)
		assert v['rows_kept'] == 6 and v['cells_kept'] == int(child.entry_screen(np.dtype(dtype), c['nc'])[0].sum()) and v['covariates'] == c['nc'] and v['steps'] == 1
		entry, plan = got(out, c['name'] + '.entry'), got(out, c['name'] + '.plan')
		assert all(x is not None and x.dtype == np.dtype(dtype) for x in entry) and entry[2].shape == (7, 37, c['nc'])
		assert np.isfinite(entry[0]).all() and (entry[0][np.arange(7) != child.ENTRY_CONST_ROW] < 1).any()
		untested_rows_exact(entry, [child.ENTRY_CONST_ROW])
		same(plan, entry, c['name'])


@pytest.mark.parametrize('design_form', ['dense', 'coo'])
def test_single1_plan_c_entry_replays(tmp_path, design_form):
	"""Three steps, update(dt2) and two more, set_design(dg2) -- another number of cells with exactly one grouping, so that the stream kernel's transposed output
	changes size -- and two more: each equals a fresh plan's single eager step on the same inputs; captured from the second step, and again after set_design; an
	adopted, pitched expression matrix rewritten in place gives the new results through the graph it already has."""
	s = dict(seed=SEEDS['replays'], dtype='float64', nc=3)
	out, info = run_child(tmp_path, 'replays', {}, dict(design_form=design_form, screen=s))
	dg = child.screen(**dict(s, dtype=np.dtype('float64')))[0]
	dg2 = child.screen(**dict(s, seed=s['seed'] + 1, dtype=np.dtype('float64')))[0]
	cells, cells2 = child.exclusive_cells(dg), child.exclusive_cells(dg2)
	assert cells != cells2
	fresh = {k: got(out, k) for k in ('fresh_a', 'fresh_b', 'fresh_c')}
	for k in fresh:
		assert info[k]['captured'] == 0 and info[k]['steps'] == 1
	for run, ref, captured, kept in ((1, 'fresh_a', 0, cells), (2, 'fresh_a', 1, cells), (3, 'fresh_a', 1, cells), (4, 'fresh_b', 1, cells), (5, 'fresh_b', 1, cells),
									 (6, 'fresh_c', 0, cells2), (7, 'fresh_c', 1, cells2)):
		name = 'run{}'.format(run)
		same(got(out, name), fresh[ref], name)
		v = info[name]
		assert v['captured'] == captured and v['steps'] == run and v['rows_kept'] == 65 and v['cells_kept'] == kept, (name, v)
	assert not np.array_equal(fresh['fresh_a'][0], fresh['fresh_b'][0]) and not np.array_equal(fresh['fresh_b'][0], fresh['fresh_c'][0])
	same(got(out, 'adopted_old'), fresh['fresh_a'], 'adopted_old')
	same(got(out, 'adopted_new'), fresh['fresh_b'], 'adopted_new')
	assert info['adopted_old']['captured'] == 1 and info['adopted_new']['captured'] == 1 and info['adopted_new']['steps'] == 4
	assert 'adopted' in info['adopted_update']


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_single1_plan_c_entry_qvalues(tmp_path, dtype):
	"""q=True: nrm_bh over all 67 x 69 = 4623 P-values (more than one tile of its sort; the 138 ones of the two dropped rows a tie group) inside the step and the
	graph: the host's binnet.bh of the plan's own P-values, bit for bit."""
	from normalisr_amd import _lib, binnet
	cases = [dict(name='q', q=True, steps=3, forms=['dense'], screen=dict(seed=SEEDS['q'], dtype=dtype, nc=3))]
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	p, q = out['q.dense.p'], out['q.dense.q']
	assert p.size == 4623 > int(_lib.load().nrm_bh_tile()) and (p[DROPPED] == 1).all() and info['q.dense']['captured'] == 1
	want = binnet.bh(p.ravel())
	assert q.dtype == p.dtype == np.dtype(dtype) and q.shape == p.shape and want.dtype == q.dtype
	assert np.array_equal(q.ravel(), want)
	assert (q >= p).all() and (q <= 1).all()


def test_single1_plan_c_entry_graph_switch_off(tmp_path):
	"""NRM_DEBUG graph=0 in the child: three steps on the 67 x 69 x 2051 screen with 3 covariates, alpha and q-values, none of them captured, and the same bits as the
	three steps -- eager, captured, replayed -- without it."""
	job = dict(cases=[dict(name='g', lowmem=False, q=True, steps=3, forms=['dense'], screen=dict(seed=SEEDS['q'], dtype='float64', nc=3))])
	(tmp_path / 'on').mkdir(), (tmp_path / 'off').mkdir()
	out, info = run_child(tmp_path / 'on', 'cases', {}, job)
	debug = ','.join([p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip()] + ['graph=0'])
	out0, info0 = run_child(tmp_path / 'off', 'cases', {}, job, env={'NRM_DEBUG': debug})
	print(info['g.dense'], info0['g.dense'])
	assert info['g.dense']['captured'] == 1 and info['g.dense']['steps'] == 3
	assert info0['g.dense']['captured'] == 0 and info0['g.dense']['steps'] == 3 and info0['g.dense']['rows_kept'] == 65
	assert info0['g.dense']['cells_kept'] == info['g.dense']['cells_kept'] > 0
	res = got(out0, 'g.dense')
	assert all(v is not None for v in res) and (res[0][DROPPED] == 1).all() and (res[0] < 1).any()
	same(res, got(out, 'g.dense'), 'graph=0')
	assert out0['g.dense.q'].dtype == out['g.dense.q'].dtype and np.array_equal(out0['g.dense.q'], out['g.dense.q'])


def test_single1_plan_c_entry_raises_what_the_reference_raises(tmp_path):
	"""From the device counters, at check() after three steps: dimreduce = n -> RuntimeError; a NaN covariate at a cell every grouping shares -> ValueError; every cell
	with exactly one grouping -> AssertionError (association.py:917-918); a NaN expression value at a grouping's own cell -> AssertionError (the results'
	assertions).  update with clean data and a step later the plan is clean and equals a fresh one."""
	out, notes = run_child(tmp_path, 'raises', {}, dict(screen=dict(seed=SEEDS['raises'], dtype='float64', nc=3)))
	print(notes)
	assert notes['dimreduce'].startswith('RuntimeError: Insufficient number of cells')
	assert notes['nan_covariate'] == 'ValueError: array must not contain infs or NaNs'
	# (the counters add up until they are looked at: all 65 groupings kept, in each of the three steps)
	assert notes['one_per_cell'].startswith('AssertionError: {} groupings take a single value on the cells selected for them'.format(3 * 65))
	assert notes['nan_expression'].startswith('AssertionError: ') and 'assertions' in notes['nan_expression']
	assert notes['clean_check'] == 'accepted' and notes['after_nan']['captured'] == 1 and notes['after_nan']['steps'] == 4
	same(got(out, 'after_nan'), got(out, 'fresh'), 'after the NaN')


def test_single1_plan_c_entry_refusals_on_the_device(tmp_path):
	"""Designs create refuses once it has looked at them on the device, in the words of the host entry; the handle stays NULL and a later plan in the same process
	gives the first one's bits."""
	out, notes = run_child(tmp_path, 'refusals', {}, dict(screen=dict(seed=SEEDS['refusals'], dtype='float64', nc=3)))
	print(notes)
	malformed = 'ValueError: Malformed CSR design matrix: indptr must rise from 0 to the number of stored entries'
	for name, want in (('negative', 'NotImplementedError: nrm_single1_plan covers designs with entries >= 0'), ('dense', 'NotImplementedError: nrm_single1_plan covers designs with entries >= 0'),
					   ('two', 'AssertionError: the largest entry of dx must be 1 (association.py:914)'), ('constant', 'ValueError: nrm_single1_plan: no design row has more than one distinct value'),
					   ('falls', malformed), ('beyond', malformed)):
		what, null = notes[name]
		assert what.startswith(want) and null, (name, what, null)
		same(got(out, 'after_' + name), got(out, 'first'), 'after ' + name)
	assert notes['good_csr'] == ['accepted', False]
	assert notes['set_design'].startswith('AssertionError: the largest entry') and notes['step_without_design'].startswith('ValueError: nrm_single1_plan_step: the plan has no design')
	same(got(out, 'after_set_design'), got(out, 'first'), 'after a refused set_design')
