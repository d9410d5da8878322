"""The resident single=4 plan of the C ABI (include/normalisr_hip.h: nrm_single4_plan_*; normalisr_amd/cplan.py: Single4Plan) on the GPU.  Every plan call is made by a
child process in which torch cannot be imported (tests/single4_plan_child.py); this process holds what comes back to the reference's golden vectors, to the oracle's
per-grouping loop and to the whole-problem entry nrm_association_tests_single4_host on the rows de keeps.

Bars: same_bars of tests/cabi_harness.py (`_same` here) -- P-values 1e-6 relative, gamma 1e-9 (floor 1e-12), varg and vart 1e-9, alpha 1e-9 (floor 1e-9).  The
plan and the entry run one step record (csrc/nrm_single4_step.h) on the same lists: P, gamma, varg and vart are equal bit for bit; alpha is summed on the device in
another order than the entry sums it on the host and is held to the bars.  A replay runs the launches of an eager step: bit for bit.  The ones and zeros of rows
that are not tested are exact.

The screen (tests/single1_plan_child.py::screen): 65 groupings x 69 genes x 2051 cells with entries set with probability 1 / 65 -- nx no multiple of the row tile, a
ragged last chunk of cells -- and two rows de drops, one all zeros and one all ones.  tests/test_single4_plan_cpu.py holds every screen used here to the conditions
these tests rely on."""
import functools
import os

import numpy as np
import pytest

import oracle
import single4_plan_child as child
from cabi_harness import got, same, untested_rows_exact
from cabi_harness import run_child as _run_child
from cabi_harness import same_bars as _same
from normalisr_amd import cplan

pytestmark = pytest.mark.gpu

run_child = functools.partial(_run_child, 'single4_plan_child.py')  # (timeout=240)
KEPT = child.kept_rows()
DROPPED = [child.ZERO_ROW, child.ONES_ROW]
FORMS = ['dense', 'scipy', 'devcsr', 'devcsr_data']  # (devcsr: no data array, every entry is 1; devcsr_data: with one)


def inflate(res, ng0, kept):
	"""de._inflate (de.py:107-122) for single=4's outputs: p = 1, gamma = alpha = varg = vart = 0 on the rows that were not tested."""
	p, gam, a, vx, vy = res
	nt = p.shape[1]
	P, G = np.ones((ng0, nt), p.dtype), np.zeros((ng0, nt), gam.dtype)
	A = None if a is None else np.zeros((ng0, nt, a.shape[2]), a.dtype)
	VG, VT = np.zeros(ng0, vx.dtype), np.zeros((ng0, nt), vy.dtype)
	P[kept], G[kept], VG[kept], VT[kept] = p, gam, vx, vy
	if a is not None:
		A[kept] = a
	return P, G, A, VG, VT


_ORACLE = {}


def oracle_inflated(dg, dt, dc, key):
	"""The oracle's per-grouping loop on the rows de keeps, inflated; computed once per screen and left unchanged."""
	if key not in _ORACLE:
		res = oracle.association_tests(dg[KEPT], np.asarray(dt, dtype=np.float64), dc, single=4, return_dot=False, lowmem=False)
		alpha = res[2] if dc.shape[0] else np.zeros((len(KEPT), dt.shape[0], 0))
		_ORACLE[key] = inflate((res[0], res[1], alpha, res[3], res[4]), dg.shape[0], KEPT)
		for a in _ORACLE[key]:
			a.setflags(write=False)
	return _ORACLE[key]


def at_the_bars(res, want, nc):
	"""The rows kept at the bars (the rows that were not tested hold exact ones and zeros -- untested_rows_exact -- against which no relative error is defined)."""
	res, want = [None if x is None else x[KEPT] for x in res], [None if x is None else x[KEPT] for x in want]
	_same(res, want[0], want[1], want[3], want[4], want[2] if (nc and res[2] is not None) else None)


def test_single4_plan_c_entry_golden(golden, tmp_path):
	"""G17 (40 x 60 x 600; 8 one-hot covariates of rank 7): de's arrays with lowmem=False, dense and scipy forms.  G17's and G10's (12 x 40 x 400, three covariates of
	full rank) per-gene dimreduce: one plan each with dimreduce = 0, 1, 2, compared on the genes whose `dr` has that value -- a gene's results depend on no other
	gene's dimreduce -- which holds a non-zero dimreduce to the reference itself."""
	g17, g10 = golden('G17_single4_onehot'), golden('G10_single4')
	arrays = dict(g17_dg=g17['dg'], g17_dt=g17['dt'], g17_dc=g17['dc'], g10_dg=g10['dg'], g10_dt=g10['dt'], g10_dc=g10['dc'])
	cases = [dict(name='g17', dg='g17_dg', dt='g17_dt', dc='g17_dc', lowmem=False, forms=['dense', 'scipy'])]
	for g in ('g17', 'g10'):
		cases += [dict(name='{}dr{}'.format(g, dr), dg=g + '_dg', dt=g + '_dt', dc=g + '_dc', dimreduce=dr) for dr in (0, 1, 2)]
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	for name, v in info.items():
		print(name, v)
	assert cplan.varying_rows(g17['dg']).all() and cplan.varying_rows(g10['dg']).all()
	for form in ('dense', 'scipy'):
		res = got(out, 'g17.' + form)
		v = info['g17.' + form]
		assert v['route'] == 0 and v['rank'] == int(g17['rc']) == 7 and v['rows_kept'] == 40 and v['dof'] == 600 - 40 - 7 and v['handed_back'] == 0
		assert res[2].shape == (40, 60, 8) and res[0].dtype == np.float64
		_same(res, g17['de_p'], g17['de_gamma'], g17['de_varg'], g17['de_vart'], g17['de_alpha'])
	same(got(out, 'g17.dense'), got(out, 'g17.scipy'), 'the design forms')
	for name, g, rank in (('g17', g17, 7), ('g10', g10, 3)):
		nx, n = g['dg'].shape
		for dr in (0, 1, 2):
			cols = np.nonzero(g['dr'] == dr)[0]
			assert cols.size > 0
			res = got(out, '{}dr{}.dense'.format(name, dr))
			assert res[2] is None and info['{}dr{}.dense'.format(name, dr)]['dof'] == n - nx - rank - dr
			_same([res[0][:, cols], res[1][:, cols], None, res[3], res[4][:, cols]], g['dr_p'][:, cols], g['dr_gamma'][:, cols], g['dr_varg'], g['dr_vart'][:, cols])


@pytest.mark.parametrize('nc', child.NCS)
def test_single4_plan_c_entry_screen(tmp_path, nc):
	"""0, 3, 8, 9 and 32 covariates with the intercept last, fp64; lowmem both ways; dense numpy, scipy CSR and device CSR arrays with and without a data array in.
	Against the oracle's per-grouping loop on the 65 rows kept, inflated as de.py:107-122 does: at the bars; dropped rows exactly 1 / 0; the four forms bit for
	bit; against nrm_association_tests_single4_host under NRM_DE_SPARSE=force on the rows kept: P, gamma, varg and vart bit for bit (the same launches), alpha at
	the bars (the entry sums it on the host, gene by gene in design-row order; the plan's k_s4_alpha sums 64 strided partial sums and a shuffle tree)."""
	cases = [dict(name='lm{}'.format(int(lowmem)), lowmem=lowmem, forms=FORMS, entry=not lowmem, screen=dict(nc=nc)) for lowmem in (True, False)]
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases), env={'NRM_DE_SPARSE': 'force'})
	dg, dt, dc = child.screen(nc)
	want = oracle_inflated(dg, dt, dc, ('screen', nc))
	for c in cases:
		first = got(out, c['name'] + '.dense')
		for form in FORMS:
			name = '{}.{}'.format(c['name'], form)
			v = info[name]
			print(name, v)
			assert v['route'] == 0 and v['rows_kept'] == 65 and v['rank'] == nc and v['dof'] == child.N - 65 - nc and v['steps'] == 1 and v['captured'] == 0, (name, v)
			assert v['reruns'] == 0 and v['handed_back'] == 0
			res = got(out, name)
			assert (res[2] is None) == c['lowmem'] and res[0].shape == (child.NG0, child.NY) and res[4].shape == (child.NG0, child.NY) and res[3].shape == (child.NG0, )
			at_the_bars(res, want, nc)
			untested_rows_exact(res, DROPPED)
			same(res, first, name)
	entry = inflate(got(out, 'lm0.entry'), child.NG0, KEPT)
	res = got(out, 'lm0.dense')
	assert res[2].shape == (child.NG0, child.NY, nc)
	for k in (0, 1, 3, 4):
		assert res[k].dtype == entry[k].dtype and np.array_equal(res[k], entry[k]), (child.KEYS[k], float(np.abs(res[k] - entry[k]).max()))
	at_the_bars(res, entry, nc)


def test_single4_plan_c_entry_fp32(tmp_path):
	"""A plan on fp32 dt with out_dtype fp32 equals, bit for bit, the arrays of a plan on the same fp32 dt with out_dtype fp64 after astype(float32): every output is
	computed in fp64 and rounded once."""
	cases = [dict(name=o, lowmem=False, out_dtype=o, screen=dict(nc=3, dtype='float32')) for o in ('float32', 'float64')]
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	r32, r64 = got(out, 'float32.dense'), got(out, 'float64.dense')
	assert all(x.dtype == np.float32 for x in r32) and all(x.dtype == np.float64 for x in r64)
	same(r32, tuple(x.astype(np.float32) for x in r64), 'rounded once')
	untested_rows_exact(r32, DROPPED)
	assert (r32[0][KEPT] < 1).any()


@pytest.mark.parametrize('design_form', ['scipy'])
def test_single4_plan_c_entry_replays(tmp_path, design_form):
	"""Five steps -- eager, captured, three launches --, update(dt2) and a step, set_design(dg2) and two steps: each equals a fresh plan's single eager step on the
	same inputs; captured from the second step, not captured after set_design until the second step on it; an adopted, pitched expression matrix rewritten in place
	gives the new results through the graph it already has."""
	out, info = run_child(tmp_path, 'replays', {}, dict(design_form=design_form, nc=3))
	fresh = {k: got(out, k) for k in ('fresh_a', 'fresh_b', 'fresh_c')}
	for k in fresh:
		assert info[k]['captured'] == 0 and info[k]['steps'] == 1
	assert info['after_design']['captured'] == 0
	for run, ref, captured in ((1, 'fresh_a', 0), (2, 'fresh_a', 1), (3, 'fresh_a', 1), (4, 'fresh_a', 1), (5, 'fresh_a', 1), (6, 'fresh_b', 1), (7, 'fresh_c', 0), (8, 'fresh_c', 1)):
		name = 'run{}'.format(run)
		same(got(out, name), fresh[ref], name)
		v = info[name]
		assert v['captured'] == captured and v['steps'] == run and v['rows_kept'] == 65 and v['route'] == 0 and v['reruns'] == 0, (name, v)
	assert not np.array_equal(fresh['fresh_a'][0], fresh['fresh_b'][0]) and not np.array_equal(fresh['fresh_b'][0], fresh['fresh_c'][0])
	same(got(out, 'adopted_old'), fresh['fresh_a'], 'adopted_old')
	same(got(out, 'adopted_new'), fresh['fresh_b'], 'adopted_new')
	assert info['adopted_old']['captured'] == 1 and info['adopted_new']['captured'] == 1 and info['adopted_new']['steps'] == 4
	assert 'adopted' in info['adopted_update']


def test_single4_plan_c_entry_graph_switch_off(tmp_path):
	"""NRM_DEBUG graph=0 in the child: three steps with alpha and q-values, none of them captured, and the same bits as the three steps -- eager, captured,
	replayed -- without it."""
	job = dict(cases=[dict(name='g', lowmem=False, q=True, steps=3, screen=dict(nc=3))])
	(tmp_path / 'on').mkdir(), (tmp_path / 'off').mkdir()
	out, info = run_child(tmp_path / 'on', 'cases', {}, job)
	debug = ','.join([p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip()] + ['graph=0'])
	out0, info0 = run_child(tmp_path / 'off', 'cases', {}, job, env={'NRM_DEBUG': debug})
	assert info['g.dense']['captured'] == 1 and info['g.dense']['steps'] == 3
	assert info0['g.dense']['captured'] == 0 and info0['g.dense']['steps'] == 3 and info0['g.dense']['rows_kept'] == 65
	res = got(out0, 'g.dense')
	assert all(v is not None for v in res) and (res[0][DROPPED] == 1).all() and (res[0] < 1).any()
	same(res, got(out, 'g.dense'), 'graph=0')
	assert np.array_equal(out0['g.dense.q'], out['g.dense.q'])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_single4_plan_c_entry_qvalues(tmp_path, dtype):
	"""q=True: nrm_bh over all 67 x 69 = 4623 P-values (more than one tile of its sort; the 138 ones of the two dropped rows a tie group) inside the step and the
	graph: the host's binnet.bh of the plan's own P-values, bit for bit."""
	from normalisr_amd import _lib, binnet
	cases = [dict(name='q', q=True, steps=3, screen=dict(nc=3, dtype=dtype))]
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	p, q = out['q.dense.p'], out['q.dense.q']
	assert p.size == 4623 > int(_lib.load().nrm_bh_tile()) and (p[DROPPED] == 1).all() and info['q.dense']['captured'] == 1
	want = binnet.bh(p.ravel())
	assert q.dtype == p.dtype == np.dtype(dtype) and q.shape == p.shape and want.dtype == q.dtype
	assert np.array_equal(q.ravel(), want)
	assert (q >= p).all() and (q <= 1).all()


def test_single4_plan_c_entry_hand_back(tmp_path):
	"""Gene 7 replaced by 100 + 0.5 N(0, 1) against three covariates with an intercept (|y~|^2 = 2.4e-5 |y|^2): the first check reports one row handed back and one
	rerun, the plan is on K1 and the fp64 Gram kernel from then on, the results -- that gene included -- are at the bars against the oracle, and three more steps
	hand nothing back."""
	out, info = run_child(tmp_path, 'handback', {}, {})
	print(info)
	assert info['first_check'] == 1
	v = info['after_first']
	assert v['reruns'] == 1 and v['route'] == 1 and v['steps'] == 1 and v['rows_kept'] == 65
	dg, dt, dc = child.handback_screen()
	want = oracle_inflated(dg, dt, dc, 'handback')
	at_the_bars(got(out, 'first'), want, child.HANDBACK_NC)
	untested_rows_exact(got(out, 'first'), DROPPED)
	for k in range(3):
		assert info['check{}'.format(k)] == 0
		v = info['later{}'.format(k)]
		assert v['reruns'] == 1 and v['route'] == 1 and v['steps'] == 2 + k and v['captured'] == 1, v  # (the rerun was the eager step on the new route)
		same(got(out, 'later{}'.format(k)), got(out, 'first'), 'later{}'.format(k))


def test_single4_plan_c_entry_refusals_and_raises(tmp_path):
	"""A design row copied from a one-hot covariate, and two equal design rows: NotImplementedError at construction and at set_design, after which the plan has no
	design until one is accepted (and then gives the first plan's bits).  n == nx + rank + dimreduce: the reference's RuntimeError.  A NaN in dt: results() raises
	the AssertionError norm.de raises, and the next step on clean values stands."""
	import normalisr_amd.normalisr as norm
	out, notes = run_child(tmp_path, 'refusals', {}, {})
	print(notes)
	assert notes['first']['rank'] == 3 and notes['first']['rows_kept'] == 65  # (three one-hot batches and an intercept: rank 3 of 4)
	for name in ('copied', 'equal'):
		assert notes['create_' + name].startswith('NotImplementedError: '), notes['create_' + name]
		assert notes['design_' + name].startswith('NotImplementedError: '), notes['design_' + name]
		assert notes['step_after_' + name].startswith('ValueError: nrm_single4_plan_step: the plan has no design')
		same(got(out, 'after_' + name), got(out, 'first'), 'after ' + name)
		assert notes['after_' + name]['captured'] == 0 and notes['after_' + name]['steps'] == 3
	assert notes['cells'].startswith('RuntimeError: Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.')
	dg, dt, _ = child.screen(3)
	dc, _ = child.refused_designs()
	bad = dt.copy()
	bad[3, 11] = np.nan
	with pytest.raises(AssertionError):
		norm.de(dg, bad, dc, single=4)
	assert notes['nan'].startswith('AssertionError: ') and 'assertions' in notes['nan']
	assert notes['clean_check'] == 'accepted' and notes['after_nan']['steps'] == 4
	same(got(out, 'after_nan'), got(out, 'first'), 'after the NaN')
