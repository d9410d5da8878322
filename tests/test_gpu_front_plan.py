"""The resident front-half plan of the C ABI (include/normalisr_hip.h: nrm_front_plan_*; normalisr_amd.cplan.FrontPlan) on the GPU: counts in, (dtn, dcn) out as one
HIP graph.  Every plan call is made by a child process in which torch cannot be imported (tests/front_plan_child.py); this process holds what comes back to what the
reference returned (golden G18_front, G18_front_chain) and, for the ragged shapes, to the numpy restatements of tests/front_numpy.py, normcov below and the CPU
oracle's normvar.  Bars are the project's: fp64 quantities close(1e-9, floor=1) (tests/test_gpu_front_entries.py), scaling factors 1e-12 absolute, P-values 1e-6
relative (cabi_harness.p_close), fp32 output 1e-6 (tests/test_gpu_parity.py's fp32 cases); replays and rewrites bit for bit."""
import functools
import os

import numpy as np
import pytest

import cabi_harness
import front_numpy
import front_plan_child as child
import oracle
from cabi_harness import close, p_close

pytestmark = pytest.mark.gpu
run_child = functools.partial(cabi_harness.run_child, 'front_plan_child.py', timeout=180)
STAGES = child.STAGES


def ok(a, b):
	return close(a, b, 1e-9, floor=1.0)


def normcov(dc):
	"""norm.py:4-53 with c=True in numpy: rows holding only 0 and 1 left alone, the others centred and divided by sqrt(mean(dev^2)), the ones row appended."""
	dc = np.asarray(dc, dtype=np.float64)
	assert not (dc == dc[:, :1]).all(axis=1).any()
	cont = ((dc != 0) & (dc != 1)).any(axis=1)
	out = dc.copy()
	dev = dc[cont] - dc[cont].mean(axis=1)[:, None]
	out[cont] = dev / np.sqrt((dev**2).mean(axis=1))[:, None]
	return np.vstack([out, np.ones((1, dc.shape[1]))])


def scaled_covariates(dc, w):
	"""norm.py:261-273 with cat=1."""
	t = ((dc != 0) & (dc != 1)).any(axis=1) | (dc == 1).all(axis=1)
	out = dc.copy()
	out[t] = dc[t] * w
	return out


@functools.lru_cache(maxsize=None)
def _chain(key):
	"""The whole chain in numpy for the arrays registered under `key`, computed once: (lcpm, normcov, w, wt, dtn, dcn)."""
	x, user, stepmax = _INPUTS[key]
	lc, cov = front_numpy.lcpm(x)
	dc = normcov(cov if user is None else np.vstack([user, cov]))
	w = front_numpy.compute_var(lc, dc, stepmax=stepmax)
	wt = front_numpy.scaling_factor(x)
	dtn, dcn = oracle.normvar(lc, dc, w, wt)[:2]
	assert np.allclose(dcn, scaled_covariates(dc, w), rtol=1e-13, atol=0)
	return lc, dc, w, wt, dtn, dcn


_INPUTS = {}


def stages(out, name):
	return {k: out['{}.{}'.format(name, k)] for k in STAGES}


def same_bits(a, b, what):
	for k in STAGES:
		assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def debug_with(switch):
	return ','.join([p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip()] + [switch])


def test_front_plan_golden_chain(golden, tmp_path):
	"""G18 through one plan per stepmax, against what the reference returned for every stage, and coex from a CoexPlan that adopts dtn where it lies."""
	g, hh = golden('G18_front'), golden('G18_front_chain')
	reads, user = g['reads'], hh['cov_raw'][:4]
	assert reads.dtype == np.int32 and reads.max() > 255 and user.shape[0] + 4 == hh['normcov_c'].shape[0] == 8
	cases = [dict(name='s1', reads='reads', cov='user', stepmax=1, coex=True), dict(name='s3', reads='reads', cov='user', stepmax=3)]
	out, info = run_child(tmp_path, 'cases', dict(reads=reads, user=user), dict(cases=cases))
	print(info)
	s1, s3 = stages(out, 's1@1'), stages(out, 's3@1')
	for s in (s1, s3):
		assert s['lcpm'].dtype == np.float64 and ok(s['lcpm'], g['lcpm']) and ok(s['cov'], hh['normcov_c'])
		assert np.abs(s['wt'] - g['sf']).max() <= 1e-12
	assert ok(s1['w'], hh['w1']) and ok(s3['w'], hh['w3']) and s1['w'].min() == 1
	assert ok(s1['dtn'], hh['nv_exp']) and ok(s1['dcn'], hh['nv_cov'])
	assert p_close(out['s1.coex.p'], hh['coex_p']) and close(out['s1.coex.var'], hh['coex_var'], 1e-9)
	# steps taken: what ComputeVarPlan takes on the same input (every iteration while the best change stays above eps: tests/test_gpu_compute_var_plan.py)
	import torch
	from normalisr_amd.norm import ComputeVarPlan
	for name, steps in (('s1', 1), ('s3', 3)):
		plan = ComputeVarPlan(torch.as_tensor(g['lcpm']).cuda(), hh['normcov_c'], stepmax=steps)
		plan.step()
		plan.results()
		assert info[name]['cv_steps'] == plan.steps_taken == steps
		assert info[name]['covariates'] == 8 and info[name]['max_count'] == reads.max() and info[name]['count_cap'] == 1 << int(reads.max()).bit_length()


def test_front_plan_fp32_output(golden, tmp_path):
	g, hh = golden('G18_front'), golden('G18_front_chain')
	cases = [dict(name='f64', reads='reads', cov='user'), dict(name='f32', reads='reads', cov='user', out_dtype='float32')]
	out, info = run_child(tmp_path, 'cases', dict(reads=g['reads'], user=hh['cov_raw'][:4]), dict(cases=cases))
	a, b = stages(out, 'f64@1'), stages(out, 'f32@1')
	assert b['lcpm'].dtype == np.float32 and b['dtn'].dtype == np.float32 and b['dcn'].dtype == np.float64
	assert np.array_equal(b['lcpm'], a['lcpm'].astype(np.float32))  # rounded once, at the store
	# dtn: the project's fp32 bar, 1e-6, beside an absolute floor at the scale of what was rounded.  The fp32 plan's lcpm carries 2^-24 of entries of up to
	# max |lcpm|, normvar multiplies a cell by at most max(w) (w ** wt, wt <= 1) before it removes the covariates, and dtn is that residual: an entry the
	# regression has brought near zero carries the rounding of its operands undiminished, so no bound relative to the entry alone can hold (the numpy
	# restatement of the chain on lcpm rounded to fp32 differs from the fp64 one by the same 7e-2 of such entries, 8e-6 absolutely).
	floor = float(np.abs(a['lcpm']).max() * a['w'].max())
	assert close(b['dtn'], a['dtn'], 1e-6, floor=floor)


def test_front_plan_replay_is_the_step(tmp_path):
	"""Four steps -- eager, captured, replayed, replayed: the same bits after each; and with the graph switched off, the same bits again."""
	x, user = child.counts(3, 37, 203), child.onehot(4, 2, 203)
	cases = [dict(name='r', reads='x', cov='user', stepmax=2, steps=4, snaps=[1, 2, 3, 4])]
	(tmp_path / 'on').mkdir(), (tmp_path / 'off').mkdir()
	out, info = run_child(tmp_path / 'on', 'cases', dict(x=x, user=user), dict(cases=cases))
	out0, info0 = run_child(tmp_path / 'off', 'cases', dict(x=x, user=user), dict(cases=cases), env={'NRM_DEBUG': debug_with('graph=0')})
	print(info, info0)
	assert info['r']['captured'] == 1 and info['r']['steps'] == 4 and info0['r']['captured'] == 0 and info0['r']['steps'] == 4
	first = stages(out, 'r@1')
	assert np.isfinite(first['dtn']).all()
	for s in (2, 3, 4):
		same_bits(first, stages(out, 'r@{}'.format(s)), s)
	for s in (1, 4):
		same_bits(first, stages(out0, 'r@{}'.format(s)), ('graph=0', s))


def test_front_plan_nothing_baked_into_the_graph(tmp_path):
	"""After the graph exists the counts change -- another total and a larger maximum below the cap: the next replay is a fresh plan's first step bit for bit, for
	the plan's own copy (update) and for an adopted matrix rewritten in place.  A graph that captured t0, len or a covariate row as a launch argument fails here."""
	a, b = child.counts(5, 37, 203, top=40), child.counts(6, 37, 203, top=200, depth=1.7)
	assert b.max() > a.max() and b.sum() != a.sum() and b.max() < 256
	out, info = run_child(tmp_path, 'rewrite', dict(a=a, b=b, cov=child.onehot(7, 3, 203)), dict(count_cap=256))
	print(info)
	fresh = stages(out, 'fresh')
	for kind in ('owned', 'adopted'):
		assert info[kind]['captured'] == 1 and info[kind]['steps'] == 4 and info[kind]['max_count'] == b.max()
		same_bits(stages(out, kind + '_new'), fresh, kind)
		assert not np.array_equal(out[kind + '_old.dtn'], out[kind + '_new.dtn'])
	same_bits(stages(out, 'owned_old'), stages(out, 'adopted_old'), 'a pitched adopted matrix')
	assert 'adopted' in info['adopted_update'] and info['no_cap'].startswith('ValueError') and 'count_cap' in info['no_cap']


RAGGED = [
	dict(name='r37x203', ng=37, n=203, dtype='int32', user=(2, False), stepmax=2),  # genes off every row tile, cells off the four-per-thread grouping and below 256
	dict(name='r5x64', ng=5, n=64, dtype='int32', user=None, stepmax=1),  # cov=None: four covariates
	dict(name='u8', ng=37, n=203, dtype='uint8', user=None, stepmax=1),
	dict(name='i16', ng=40, n=300, dtype='int16', user=(2, True), stepmax=3),  # one continuous user row beside a one-hot pair; more than one workgroup of cells
]


def _ragged_inputs(c, i):
	x = child.counts(20 + i, c['ng'], c['n'], np.dtype(c['dtype']), depth=3.0 if c['ng'] == 5 else 1.0)
	user = None
	if c['user'] is not None:
		user = child.onehot(30 + i, c['user'][0], c['n'])
		if c['user'][1]:
			user = np.vstack([np.random.default_rng(40 + i).normal(5.0, 2.0, (1, c['n'])), user])
	return x, user


def test_front_plan_ragged_shapes(tmp_path):
	arrays, cases = {}, []
	for i, c in enumerate(RAGGED):
		x, user = _ragged_inputs(c, i)
		arrays[c['name'] + '_x'] = x
		if user is not None:
			arrays[c['name'] + '_u'] = user
		_INPUTS[c['name']] = (x, user, c['stepmax'])
		cases.append(dict(name=c['name'], reads=c['name'] + '_x', cov=None if user is None else c['name'] + '_u', stepmax=c['stepmax'], steps=2))
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	for c in RAGGED:
		print(c['name'], info[c['name']])
		got = stages(out, c['name'] + '@2')
		lc, dc, w, wt, dtn, dcn = _chain(c['name'])
		assert info[c['name']]['covariates'] == dc.shape[0] and info[c['name']]['captured'] == 1
		assert ok(got['lcpm'], lc) and ok(got['cov'], dc) and ok(got['w'], w) and np.abs(got['wt'] - wt).max() <= 1e-12
		assert ok(got['dtn'], dtn) and ok(got['dcn'], dcn)


def test_front_plan_the_cap(tmp_path):
	"""A maximum of count_cap - 1 passes; a maximum equal to count_cap is refused by check() with both numbers, and the plan serves again after update."""
	cap = 64
	below, at = child.counts(50, 37, 203, top=cap - 1), child.counts(50, 37, 203, top=cap)
	assert below.max() == cap - 1 and at.max() == cap
	_INPUTS['cap'] = (below, None, 1)
	out, notes = run_child(tmp_path, 'cap', dict(below=below, at=at), dict(count_cap=cap))
	print(notes)
	assert notes['below'] == 'accepted' and notes['below_info']['max_count'] == cap - 1 and notes['below_info']['count_cap'] == cap
	assert notes['at'].startswith('NotImplementedError') and str(cap) in notes['at'] and 'largest count here is {}'.format(cap) in notes['at']
	assert notes['at_again'] == 'accepted' and notes['after'] == 'accepted'
	same_bits(stages(out, 'after'), stages(out, 'below'), 'after the refusal')
	lc, dc, w, wt, dtn, dcn = _chain('cap')
	assert ok(out['below.lcpm'], lc) and ok(out['below.dtn'], dtn)


def test_front_plan_errors_through_check(tmp_path):
	"""One tiny matrix per refusal: the reference's exception type and words, and a clean step on the same plan afterwards.  compute_var's refusal of a gene with
	a constant residual needs a spread that is zero to the bit (csrc/nrm_fitvar.hip: sc_g == 0), which no count matrix reaches through lcpm -- its rows carry the
	rounding of T[x] - t1 -- so its counter, type and words are held on the CPU (tests/test_front_plan_cpu.py: nrm_front_plan_status), not here."""
	good = child.counts(60, 12, 96)
	cov = child.onehot(61, 2, 96)
	bad = {}
	bad['negative'] = good.copy()
	bad['negative'][3, 5] = -1
	bad['empty_cell'] = good.copy()
	bad['empty_cell'][:, 7] = 0
	bad['all_zero'] = np.zeros_like(good)
	eq = np.zeros_like(good)  # every cell the same total, spread differently: lcpm's own ln total row is constant
	third = np.arange(96) % 3 == 0
	eq[np.arange(96) % 12, np.arange(96)] = np.where(third, 4, 6)
	eq[(np.arange(96) + 1) % 12, np.arange(96)] = np.where(third, 2, 0)
	assert (eq.sum(axis=0) == 6).all() and (eq >= 0).all()
	bad['equal_totals'] = eq
	out, notes = run_child(tmp_path, 'errors', dict(good=good, cov=cov, **bad), dict(bad=sorted(bad)))
	print(notes)
	assert notes['negative'] == 'ValueError: Negative value in d detected.'
	assert notes['empty_cell'] == 'ValueError: Found cell with no read at all. Please remove.'
	assert notes['all_zero'].startswith('AssertionError') and 'no read' in notes['all_zero']
	assert notes['equal_totals'] == 'ValueError: Detected constant covariate. Please only provide full-rank covariate without constant covariate.'
	fresh = stages(out, 'fresh')
	for name in bad:
		assert notes[name + '.results'] == 'accepted'  # (check() cleared the counters; what the plan holds for such counts is for the caller to discard)
		assert notes[name + '.after'] == 'accepted', name
		same_bits(stages(out, name + '.after'), fresh, name)


def test_front_plan_two_stepmax_side_by_side(tmp_path):
	"""Two plans with stepmax 1 and 3 alive at once on the same 70 x 131 counts (three row tiles, the last ragged): each keeps a compute_var state block of its own
	length (csrc/nrm_fitvar_step.h: 4 (stepmax + 1) + n doubles).  What does not depend on stepmax -- lcpm, the covariates, the scaling factors -- is the same to the
	bit, each plan's iteration count lies within its own stepmax, and both finish with finite results."""
	x, cov = child.counts(80, 70, 131), child.onehot(81, 2, 131)
	out, info = run_child(tmp_path, 'stepmax_pair', dict(x=x, cov=cov), {})
	print(info)
	s1, s3 = stages(out, 's1'), stages(out, 's3')
	for k in ('lcpm', 'cov', 'wt'):
		assert s1[k].dtype == s3[k].dtype and np.array_equal(s1[k], s3[k]), k
	assert 1 <= info['s1']['cv_steps'] <= 1 and 1 <= info['s3']['cv_steps'] <= 3
	for s, i in ((s1, info['s1']), (s3, info['s3'])):
		assert i['captured'] == 1 and i['steps'] == 3 and i['covariates'] == 6
		assert s['w'].shape == (131, ) and np.isfinite(s['w']).all() and s['w'].min() > 0 and np.isfinite(s['dtn']).all() and np.isfinite(s['dcn']).all()
	assert info['s3']['bytes'] - info['s1']['bytes'] == 4 * 2 * 8  # the two state records more, and nothing else


def test_front_plan_two_plans_and_teardown(tmp_path):
	a, b, cov = child.counts(70, 37, 203), child.counts(71, 40, 300), child.onehot(72, 2, 203)
	out, n = run_child(tmp_path, 'two', dict(a=a, b=b, cov=cov), {})
	print(n)
	for k in ('a', 'b'):
		assert n['two_' + k]['captured'] == 1 and n['two_' + k]['steps'] == 4
		same_bits(stages(out, 'two_' + k), stages(out, 'fresh_' + k), k)
	assert out['two_b.dtn'].dtype == np.float32
	assert n['before'] == [0, 0]
	assert n['alive'][1] >= n['bytes'] > 0 and n['alive'][0] >= n['alive'][1]
	assert n['closed'][1] == 0  # destroy gives everything back to the pool ...
	assert n['released'] == [0, 0]  # ... and nrm_release_cache then frees it: no device memory held
