"""The resident de plan of the C ABI (include/normalisr_hip.h: nrm_de_plan_*; normalisr_amd/cplan.py: DePlan) on the GPU.  Every plan call is made by a child
process in which torch cannot be imported (tests/de_plan_child.py); this process holds what comes back to the reference's golden vectors, to the oracle and to
norm.de on the same arrays.

Bars.  P-values within 1e-6 relative (p_close; fp32: with the floor of the smallest normal fp32 number, as tests/test_gpu_parity.py holds its fp32 case).  The plan
is the sparse-design route, so gamma, alpha, varg and vart are held as tests/test_gpu_design_csr.py:399 holds that route against the reference's arithmetic: gamma
1e-6 (floor 1e-12), alpha 1e-6 (floor 1e-9), varg 1e-9 (floor 1e-15), vart 1e-7 (floor 1e-15); fp32 gamma as tests/test_gpu_parity.py: 1e-6 (floor 1e-7).  The ones
and zeros of rows that are not tested are exact.  Against norm.de under NRM_HOST_ENTRY=1 NRM_DE_SPARSE=force (the parent's route: the same lists into the same
kernels) and between a replay and a fresh plan every array is equal, bit for bit."""
import functools
import os

import numpy as np
import pytest

import de_plan_child as child
import oracle
from cabi_harness import close, got, p_close, same
from cabi_harness import run_child as _run_child

pytestmark = pytest.mark.gpu

run_child = functools.partial(_run_child, 'de_plan_child.py')  # (timeout=240)


@pytest.fixture
def parent_route(monkeypatch):
	"""norm.de as the parent commit runs it from host buffers on the sparse-design kernels."""
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	import normalisr_amd.normalisr as norm
	return norm


def test_de_plan_c_entry_golden(golden, tmp_path):
	g1, g2 = golden('G1_c1'), golden('G2_edge')
	n = g2['dt'].shape[1]
	arrays = dict(g1_dg=g1['dg'], g1_dt=g1['dt'], g1_dc=g1['dc'], dg=g2['dg'], dt=g2['dt'], dc=g2['dc'], nc0=np.zeros((0, n)), rd_dc=g2['rd_dc'], zc_dt=g2['zc_dt'], se_dt=g2['se_dt'],
				  dg32=g2['dg'].astype(np.float32), dt32=g2['dt'].astype(np.float32), dc32=g2['dc'].astype(np.float32))
	cases = [dict(name='lm1', dg='g1_dg', dt='g1_dt', dc='g1_dc', forms=['dense', 'scipy']), dict(name='lm0', dg='g1_dg', dt='g1_dt', dc='g1_dc', lowmem=False),
			 dict(name='nc0', dg='dg', dt='dt', dc='nc0'), dict(name='rd', dg='dg', dt='dt', dc='rd_dc', lowmem=False), dict(name='rd_lib', dg='dg', dt='dt', dc='rd_dc', pinv='library'),
			 dict(name='dr2', dg='dg', dt='dt', dc='dc', dimreduce=2), dict(name='int', dg='dg', dt='dt', dc='dc', dg_dtype='int64'), dict(name='zc', dg='dg', dt='zc_dt', dc='dc'),
			 dict(name='f32', dg='dg32', dt='dt32', dc='dc32'), dict(name='se', dg='dg', dt='se_dt', dc='dc')]
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	for name, v in info.items():
		print(name, v)
		assert v['route'] == 0 and v['reruns'] == 0 and v['handed_back'] == 0 and v['steps'] == 1, (name, v)
	# G1: row 2 of dg is all ones and an intercept is among the covariates -- dropped, never handed back, re-inflated exactly
	for name, lm in (('lm1.dense', 1), ('lm1.scipy', 1), ('lm0.dense', 0)):
		p, gam, a, vg, vt = got(out, name)
		k = 'de_lm{}_'.format(lm)
		assert info[name]['rows_kept'] == 3 and info[name]['rank'] == 2 and info[name]['dof'] == 300 - 1 - 2
		assert p.shape == (4, 500) and p.dtype == np.float64
		assert p_close(p, g1[k + 'p']) and close(gam, g1[k + 'gamma'], 1e-6, 1e-12)
		assert close(vg, g1[k + 'varg'], 1e-9, 1e-15) and close(vt, g1[k + 'vart'], 1e-7, 1e-15)
		assert (a is None) if lm else (a.shape == (4, 500, 2) and close(a, g1[k + 'alpha'], 1e-6, 1e-9) and (a[2] == 0).all())
		assert (p[2] == 1).all() and (gam[2] == 0).all() and vg[2] == 0 and (vt[2] == 0).all()
	p, gam, a, vg, vt = got(out, 'nc0.dense')
	assert p_close(p, g2['nc0_de_p']) and close(gam, g2['nc0_de_gamma'], 1e-6, 1e-12) and close(vg, g2['nc0_de_varg'], 1e-9, 1e-15) and close(vt, g2['nc0_de_vart'], 1e-7, 1e-15)
	assert info['nc0.dense']['rank'] == 0 and info['nc0.dense']['rows_kept'] == 5
	for name in ('rd', 'rd_lib'):  # rank 3 of 5, from numpy's SVD and from the library's own
		p, gam, a, vg, vt = got(out, name + '.dense')
		assert info[name + '.dense']['rank'] == int(g2['rd_rank']) == 3 and info[name + '.dense']['dof'] == n - 1 - 3
		assert p_close(p, g2['rd_de_p']) and close(gam, g2['rd_de_gamma'], 1e-6, 1e-12) and close(vg, g2['rd_de_varg'], 1e-9, 1e-15) and close(vt, g2['rd_de_vart'], 1e-7, 1e-15)
		assert (a is None) if name == 'rd_lib' else close(a, g2['rd_de_alpha'], 1e-6, 1e-9)
	p, gam, a, vg, vt = got(out, 'dr2.dense')
	assert p_close(p, g2['dr2_de_p']) and close(gam, g2['dr2_de_gamma'], 1e-6, 1e-12) and info['dr2.dense']['dof'] == n - 1 - 3 - 2
	p, gam, a, vg, vt = got(out, 'int.dense')
	assert p.dtype == np.float64 and p_close(p, g2['int_de_p']) and close(gam, g2['int_de_gamma'], 1e-6, 1e-12) and close(vg, g2['int_de_varg'], 1e-9, 1e-15)
	assert close(vt, g2['int_de_vart'], 1e-7, 1e-15)
	# a zero-variance gene: its variance is reported as 1 on every tested row (association.py:231-233), p = 1 and gamma = 0
	p, gam, a, vg, vt = got(out, 'zc.dense')
	assert p_close(p, g2['zc_de_p']) and close(gam, g2['zc_de_gamma'], 1e-6, 1e-12) and close(vt, g2['zc_de_vart'], 1e-7, 1e-15)
	zero = np.nonzero(g2['zc_dt'].var(axis=1) == 0)[0]
	assert zero.size > 0 and (vt[:, zero] == 1).all() and (p[:, zero] == 1).all() and (gam[:, zero] == 0).all()
	p, gam, a, vg, vt = got(out, 'f32.dense')
	assert p.dtype == np.float32 and gam.dtype == np.float32 and vg.dtype == np.float32 and vt.dtype == np.float32
	assert close(p, g2['f32_de_p'], 1e-6, 1e-38) and close(gam, g2['f32_de_gamma'], 1e-6, 1e-7) and close(vg, g2['f32_de_varg'], 1e-6) and close(vt, g2['f32_de_vart'], 1e-6)
	p, gam, a, vg, vt = got(out, 'se.dense')
	assert p_close(p, g2['se_de_p']) and close(gam, g2['se_de_gamma'], 1e-6, 1e-12) and g2['se_de_p'].min() < 1e-20


FORMS = ['dense', 'scipy', 'devcsr']
COVARIATES = [(0, True), (3, True), (9, True), (9, False)]


@pytest.mark.parametrize('valued', [False, True], ids=['binary', 'valued'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_de_plan_c_entry_same_bytes_as_the_host_entry(parent_route, tmp_path, dtype, valued):
	"""70 x 64 x 4100 with row 9 constant; covariates 0, 3, 9 with an intercept and 9 without (the stream kernel of single=1 takes the rows' sums); lowmem both
	ways; dense numpy, scipy CSR and device CSR arrays in: the five outputs of norm.de on the same arrays, bit for bit."""
	cases = []
	for nc, intercept in COVARIATES:
		for lowmem in (True, False):
			cases.append(dict(name='c{}{}{}'.format(nc, 'i' if intercept else 'n', int(lowmem)), lowmem=lowmem, forms=FORMS, steps=1,
							  screen=dict(seed=100 + nc + (0 if intercept else 50), dtype=dtype, nc=nc, intercept=intercept, valued=valued)))
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	for c in cases:
		s = dict(c['screen'], dtype=np.dtype(dtype))
		dg, dt, dc = child.screen(**s)
		want = parent_route.de(dg, dt, dc, lowmem=c['lowmem'])
		assert want[0].dtype == np.dtype(dtype) and (want[0][9] == 1).all()
		for form in FORMS:
			name = '{}.{}'.format(c['name'], form)
			assert info[name]['route'] == 0 and info[name]['reruns'] == 0 and info[name]['rows_kept'] == 69, (name, info[name])
			same(got(out, name), want, name)


def test_de_plan_c_entry_full_rows_and_several_passes(parent_route, tmp_path):
	"""A row with every cell set: two values are kept, one value is dropped (a valued design).  And 1030 design rows (more than one pass of the kernel's positions),
	130 genes, 6145 cells."""
	cases = [dict(name='full', lowmem=False, forms=FORMS, screen=dict(seed=7, dtype='float64', nc=3, valued=True, full_rows=True)),
			 dict(name='big', forms=FORMS, steps=3, screen=dict(seed=8, dtype='float32', nc=3, nx=1030, ny=130, n=6145, const_rows=[9, 1000]))]
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	for c, kept in zip(cases, (68, 1028)):
		dg, dt, dc = child.screen(**dict(c['screen'], dtype=np.dtype(c['screen']['dtype'])))
		want = parent_route.de(dg, dt, dc, lowmem=c.get('lowmem', True))
		for form in FORMS:
			name = '{}.{}'.format(c['name'], form)
			assert info[name]['route'] == 0 and info[name]['rows_kept'] == kept and info[name]['captured'] == (1 if c.get('steps', 1) > 1 else 0), (name, info[name])
			same(got(out, name), want, name)
	p, gam, a, vg, vt = got(out, 'full.dense')
	assert (p[12] == 1).all() and (gam[12] == 0).all() and (a[12] == 0).all() and vg[12] == 0 and (vt[12] == 0).all()
	assert (p[11] < 1).any() and vg[11] > 0 and (vt[11] == vt[0]).all()


@pytest.mark.parametrize('design_form', ['dense', 'coo'])
def test_de_plan_c_entry_replays(tmp_path, design_form):
	"""Three steps, update(dt2) and two more, set_design(dg2) and two more: each equals a fresh plan's single eager step on the same inputs; captured from the second
	step, and again after set_design; an adopted, pitched expression matrix rewritten in place gives the new results through the graph it already has."""
	out, info = run_child(tmp_path, 'replays', {}, dict(design_form=design_form, screen=dict(seed=21, dtype='float64', nc=3, valued=True)))
	fresh = {k: got(out, k) for k in ('fresh_a', 'fresh_b', 'fresh_c')}
	for k in fresh:
		assert info[k]['captured'] == 0 and info[k]['steps'] == 1
	for run, ref, captured, kept in ((1, 'fresh_a', 0, 69), (2, 'fresh_a', 1, 69), (3, 'fresh_a', 1, 69), (4, 'fresh_b', 1, 69), (5, 'fresh_b', 1, 69), (6, 'fresh_c', 0, 68),
									 (7, 'fresh_c', 1, 68)):
		name = 'run{}'.format(run)
		same(got(out, name), fresh[ref], name)
		assert info[name]['captured'] == captured and info[name]['steps'] == run and info[name]['rows_kept'] == kept and info[name]['reruns'] == 0, (name, info[name])
	assert not np.array_equal(fresh['fresh_a'][0], fresh['fresh_b'][0]) and not np.array_equal(fresh['fresh_b'][0], fresh['fresh_c'][0])
	same(got(out, 'adopted_old'), fresh['fresh_a'], 'adopted_old')
	same(got(out, 'adopted_new'), fresh['fresh_b'], 'adopted_new')
	assert info['adopted_old']['captured'] == 1 and info['adopted_new']['captured'] == 1 and info['adopted_new']['steps'] == 4
	assert 'adopted' in info['adopted_update']


def test_de_plan_c_entry_hands_a_design_row_near_the_covariate_span_back(tmp_path):
	"""Row 5 of the design all but equals a batch covariate (tests/test_gpu_round5.py:199-206): the first check reports the hand-back and has redone the step on K1
	and the fp64 Gram kernel; results as the oracle's at that test's bars; three more steps stay on that route, reruns stays 1."""
	dx, dy, dc = child.handback_inputs()
	ref = oracle.association_tests(dx, dy, dc, return_dot=False)
	assert ref[0][5].min() < 1e-6
	out, info = run_child(tmp_path, 'handback', {}, {})
	print(info)
	assert info['first_check'] > 0 and info['after_first']['route'] == 1 and info['after_first']['reruns'] == 1 and info['after_first']['rows_kept'] == 40
	for name in ('first', 'later0', 'later1', 'later2'):
		p, gam, a, vg, vt = got(out, name)
		assert p_close(p, ref[0]) and close(gam, ref[1], 1e-6, 1e-9) and close(vg, ref[3], 1e-6), name
		assert close(vt, np.broadcast_to(ref[4], vt.shape), 1e-6), name
	for k in range(3):
		v = info['later{}'.format(k)]
		assert info['check{}'.format(k)] == 0 and v['route'] == 1 and v['reruns'] == 1 and v['steps'] == 2 + k, v
	assert info['later2']['captured'] == 1
	same(got(out, 'later2'), got(out, 'first'), 'the dense route repeats its bits')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_de_plan_c_entry_qvalues(tmp_path, dtype):
	"""q=True: nrm_bh over all 70 x 64 = 4480 P-values (more than one tile of its sort; the 64 ones of the dropped row a tie group) inside the step and the graph:
	the host's binnet.bh of the plan's own P-values, bit for bit."""
	from normalisr_amd import _lib, binnet
	cases = [dict(name='q', q=True, steps=3, forms=['dense'], screen=dict(seed=31, dtype=dtype, nc=3))]
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases))
	p, q = out['q.dense.p'], out['q.dense.q']
	assert p.size == 4480 > int(_lib.load().nrm_bh_tile()) and (p[9] == 1).all() and info['q.dense']['captured'] == 1
	want = binnet.bh(p.ravel())
	assert q.dtype == p.dtype == np.dtype(dtype) and q.shape == p.shape and want.dtype == q.dtype
	assert np.array_equal(q.ravel(), want)
	assert (q >= p).all() and (q <= 1).all()


def test_de_plan_c_entry_graph_switch_off(tmp_path):
	"""NRM_DEBUG graph=0 in the child: three steps on the 70 x 64 screen with alpha and q-values, none of them captured, and the same bits as the three steps --
	eager, captured, replayed -- without it."""
	job = dict(cases=[dict(name='g', lowmem=False, q=True, steps=3, forms=['dense'], screen=dict(seed=51, dtype='float64', nc=3, valued=True))])
	(tmp_path / 'on').mkdir(), (tmp_path / 'off').mkdir()
	out, info = run_child(tmp_path / 'on', 'cases', {}, job)
	debug = ','.join([p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip()] + ['graph=0'])
	out0, info0 = run_child(tmp_path / 'off', 'cases', {}, job, env={'NRM_DEBUG': debug})
	print(info['g.dense'], info0['g.dense'])
	assert info['g.dense']['captured'] == 1 and info['g.dense']['steps'] == 3
	assert info0['g.dense']['captured'] == 0 and info0['g.dense']['steps'] == 3 and info0['g.dense']['rows_kept'] == 69
	res = got(out0, 'g.dense')
	assert all(v is not None for v in res) and (res[0][9] == 1).all() and (res[0] < 1).any()
	same(res, got(out, 'g.dense'), 'graph=0')
	assert out0['g.dense.q'].dtype == out['g.dense.q'].dtype and np.array_equal(out0['g.dense.q'], out['g.dense.q'])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_de_plan_c_entry_graph_switch_off_same_bytes_as_the_host_entry(parent_route, monkeypatch, tmp_path, dtype):
	"""The whole-problem entry and the plan run one step record (csrc/nrm_de_sparse_step.h): NRM_DEBUG graph=0 in the child, 5 design rows (one empty) x 19 genes x
	130 cells, three eager steps against norm.de on the same arrays, bit for bit.  One covariate, the intercept: the fused table with a constant covariate.  Six
	without an intercept: the fused table without one (six is within nrm_de_sparse_fused_covariates() = 8).  Nine without: the rows' sums from the stream kernel of
	single=1.  fp32 is the issue's case; fp64 is there because rounding to fp32 can hide another algorithm's last bits.

	The entry's route.  With 4 rows kept and at most 9 covariates nrm_association_tests_host would take the streaming kernel (nx + nc <= 32) and never reach
	nrm_host_de_sparse: NRM_DE_PATH=general switches that off, NRM_DE_SPARSE=force overrides the size rule, the density is under one in sixteen and nothing is handed
	back (nrm_last_guard).  That it then ran the sparse-design kernels shows in fp64: under NRM_DE_SPARSE=0, K1 and the fp64 Gram kernel, gamma has other bits."""
	import ctypes
	from normalisr_amd import _lib
	lib = _lib.load()
	assert 6 <= int(lib.nrm_de_sparse_fused_covariates()) < 9 <= int(lib.nrm_de_sparse_max_covariates())
	monkeypatch.setenv('NRM_DE_PATH', 'general')
	cases = [dict(name='c{}{}'.format(nc, 'i' if intercept else 'n'), lowmem=False, steps=3, forms=['dense'], small=dict(nc=nc, intercept=intercept, dtype=dtype))
			 for nc, intercept in ((1, True), (6, False), (9, False))]
	debug = ','.join([p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip()] + ['graph=0'])
	out, info = run_child(tmp_path, 'cases', {}, dict(cases=cases), env={'NRM_DEBUG': debug})
	for c in cases:
		name = c['name'] + '.dense'
		print(name, info[name])
		assert info[name]['captured'] == 0 and info[name]['steps'] == 3 and info[name]['route'] == 0 and info[name]['reruns'] == 0 and info[name]['rows_kept'] == 4
		dg, dt, dc = child.small_screen(**c['small'])
		assert 16 * int((dg != 0).sum()) <= 4 * dg.shape[1]
		want = parent_route.de(dg, dt, dc, lowmem=False)
		hits = ctypes.c_int64(-1)
		_lib.check(lib.nrm_last_guard(ctypes.byref(hits), None))
		assert hits.value == 0, 'the entry handed rows back to the dense kernels'
		assert want[0].dtype == np.dtype(dtype) and (want[0][3] == 1).all() and (want[0] < 1).any() and want[2].shape == (5, 19, c['small']['nc'])
		same(got(out, name), want, name)
		if dtype == 'float64':
			monkeypatch.setenv('NRM_DE_SPARSE', '0')
			dense = parent_route.de(dg, dt, dc, lowmem=False)
			monkeypatch.setenv('NRM_DE_SPARSE', 'force')
			assert np.allclose(dense[1], want[1], rtol=1e-6, atol=1e-12) and not np.array_equal(dense[1], want[1]), name


def test_de_plan_c_entry_bounds(tmp_path):
	"""A NaN planted in one expression value: check() raises AssertionError (the reference's assertions, counted on the device); update and a step later the plan
	is clean and equals a fresh one."""
	out, notes = run_child(tmp_path, 'bounds', {}, dict(screen=dict(seed=41, dtype='float64', nc=3)))
	print(notes)
	assert notes['nan'].startswith('AssertionError: ') and 'assertions' in notes['nan']
	assert notes['clean_check'] == 0 and notes['after_nan']['route'] == 0 and notes['after_nan']['reruns'] == 0
	same(got(out, 'after_nan'), got(out, 'fresh'), 'after the NaN')
