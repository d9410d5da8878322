"""The resident coex plan of the C ABI (include/normalisr_hip.h: nrm_coex_plan_*; normalisr_amd/cplan.py) on the GPU.  Every plan call is made by a child process
in which torch cannot be imported (tests/coex_plan_child.py: normalisr_amd._lib and .cplan only); this process holds what comes back to the reference's golden
vectors, to the oracle and to norm.coex on the same arrays.  Bars: P-values within 1e-6 relative (the project's), covariances and variances within 1e-9 of their
largest entry, zeros / ones / symmetry exact, replays bit for bit."""
import functools
import os

import numpy as np
import pytest

import cabi_harness
import coex_plan_child as child
import oracle
from cabi_harness import p_close

pytestmark = pytest.mark.gpu

run_child = functools.partial(cabi_harness.run_child, 'coex_plan_child.py', timeout=180)
got = lambda out, name, tag='': cabi_harness.got(out, name, cabi_harness.COEX_KEYS, tag)


def p_close32(p, ref, rtol=1e-6):
	"""fp32 P-values: relative with the floor of the smallest normal fp32 number, as the fp32 cases of tests/test_gpu_parity.py."""
	p, ref = np.asarray(p, dtype=np.float64), np.asarray(ref, dtype=np.float64)
	err = float(np.max(np.abs(p - ref) / (np.abs(ref) + 1e-38)))
	print('  P-values (fp32): worst relative error {:.2e}'.format(err))
	return err < rtol


def scale_close(a, ref, rtol=1e-9):
	a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
	err = float(np.abs(a - ref).max() / np.abs(ref).max())
	print('  worst error over the largest entry {:.2e}'.format(err))
	return err <= rtol


def exact_structure(p, d):
	return bool((np.diag(p) == 0).all() and (np.diag(d) == 0).all() and (p == p.T).all() and (d == d.T).all())


def test_coex_plan_c_entry_golden_fp64_route(golden, tmp_path):
	g1, g2 = golden('G1_c1'), golden('G2_edge')
	ns = int(g1['coex_n'])
	dt, dc, n = g2['dt'], g2['dc'], g2['dt'].shape[1]
	arrays = dict(g1_dt=g1['dt'][:ns], g1_dc=g1['dc'], dt40=dt[:40], dt45=dt[:45], dc=dc, nc0=np.zeros((0, n)), rd_dc=g2['rd_dc'], zc_dt=g2['zc_dt'])
	cases = [dict(name='g1', dt='g1_dt', dc='g1_dc'), dict(name='nc0', dt='dt40', dc='nc0'), dict(name='rd', dt='dt40', dc='rd_dc'), dict(name='rd_lib', dt='dt40', dc='rd_dc', pinv='library'),
			 dict(name='dr2', dt='dt40', dc='dc', dimreduce=2), dict(name='tile', dt='dt45', dc='dc'), dict(name='zc', dt='zc_dt', dc='dc')]
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	for c in cases:
		assert info[c['name']]['engine'] == 0 and info[c['name']]['steps'] == 1, info[c['name']]
		p, d, v = got(out, c['name'], 1)
		assert p.dtype == np.float64 and d.dtype == np.float64 and v.dtype == np.float64 and exact_structure(p, d), c['name']
	p, d, v = got(out, 'g1', 1)
	assert p.shape == (ns, ns) and p_close(p, g1['coex_p']) and scale_close(d, g1['coex_dot']) and scale_close(v, g1['coex_var'])
	assert info['g1']['rank'] == 2 and info['g1']['dof'] == 300 - 1 - 2
	p, d, v = got(out, 'nc0', 1)
	assert p_close(p, g2['nc0_coex_p']) and scale_close(d, g2['nc0_coex_dot']) and scale_close(v, g2['nc0_coex_var']) and info['nc0']['rank'] == 0
	for name in ('rd', 'rd_lib'):  # rank 3 of 5, from numpy's SVD and from the library's own
		p, d, v = got(out, name, 1)
		assert info[name]['rank'] == int(g2['rd_rank']) == 3 and info[name]['dof'] == n - 1 - 3
		assert p_close(p, g2['rd_coex_p']) and scale_close(d, g2['rd_coex_dot']) and scale_close(v, g2['rd_coex_var'])
	assert p_close(got(out, 'dr2', 1)[0], g2['dr2_coex_p']) and info['dr2']['dof'] == n - 1 - 3 - 2
	p, d, v = got(out, 'tile', 1)
	assert p.shape == (45, 45) and p_close(p, g2['tile_coex_p']) and scale_close(d, g2['tile_coex_dot']) and scale_close(v, g2['tile_coex_vy'])
	# constant rows: variance reported as 1, p = 1, dot = 0 (association.py:231-233), through k_plan_var; the collinear pair's R^2 -> 1 gives p = 0
	p, d, v = got(out, 'zc', 1)
	assert v[5] == 1 and (p[5] == np.where(np.arange(30) == 5, 0, 1)).all() and (d[5] == 0).all()
	assert p[6, 7] == 0. and p[7, 6] == 0.
	ok = np.ones_like(p, dtype=bool)
	ok[6, 7] = ok[7, 6] = False
	assert p_close(p[ok], g2['zc_coex_p'][ok]) and scale_close(d, g2['zc_coex_dot']) and scale_close(v, g2['zc_coex_var'])


def test_coex_plan_c_entry_golden_integer_route(golden, tmp_path):
	g = golden('G11_i8hard')
	kinds = ('intercept', 'onehot', 'collinear', 'none')
	arrays = dict(dt=g['dt'], **{'dc_' + k: g['dc_' + k] for k in kinds})
	cases = [dict(name=k, dt='dt', dc='dc_' + k) for k in kinds] + [dict(name='onehot_lib', dt='dt', dc='dc_onehot', pinv='library')]
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	ranks = dict(intercept=1, onehot=4, collinear=3, none=0, onehot_lib=4)
	for c in cases:
		name, kind = c['name'], c['dc'][3:]
		print(name, info[name])
		assert info[name]['engine'] == 6 and info[name]['reruns'] == 0
		assert info[name]['rank'] == ranks[name] and info[name]['dof'] == 4096 - 1 - ranks[name]  # the library's own rank gives coex's dof
		p, d, v = got(out, name, 1)
		assert exact_structure(p, d)
		assert p_close(p, g['coex_{}_p'.format(kind)]) and scale_close(d, g['coex_{}_dot'.format(kind)]) and scale_close(v, g['coex_{}_var'.format(kind)])


REPLAY = [  # ng: one and two ragged row tiles; n = 2052: integer engine, no multiple of NRM_K_TILE; 2050: fp64 kernel above 2048 cells (n % 4 != 0); 300: fp64 kernel
	dict(name='i8_f32', ng=130, n=2052, dtype='float32', out_dtype=None, engine=6),
	dict(name='i8_f64_out32', ng=257, n=2052, dtype='float64', out_dtype='float32', engine=6),
	dict(name='f64_2050', ng=130, n=2050, dtype='float64', out_dtype=None, engine=0),
	dict(name='f64_f32_out64', ng=257, n=300, dtype='float32', out_dtype='float64', engine=0),
	dict(name='f64_300', ng=130, n=300, dtype='float64', out_dtype=None, engine=0),
]


def test_coex_plan_c_entry_replay_is_the_step(tmp_path):
	"""Five steps per case -- eager, captured, three replays: the results after steps 1, 2 and 5 are the same bits, and they are norm.coex's P-values."""
	import normalisr_amd.normalisr as norm
	arrays, cases = {}, []
	for i, c in enumerate(REPLAY):
		arrays[c['name'] + '_dt'], arrays[c['name'] + '_dc'] = child.expression(100 + i, c['ng'], c['n'], c['dtype'])
		cases.append(dict(name=c['name'], dt=c['name'] + '_dt', dc=c['name'] + '_dc', out_dtype=c['out_dtype'], steps=5, snaps=[1, 2, 5]))
	out, info = run_child(tmp_path, 'cases', arrays, dict(cases=cases))
	for c in REPLAY:
		name = c['name']
		print(name, info[name])
		assert info[name]['captured'] == 1 and info[name]['steps'] == 5 and info[name]['engine'] == c['engine'] and info[name]['reruns'] == 0
		first = got(out, name, 1)
		want = np.dtype(c['out_dtype'] or c['dtype'])
		for a in first:
			assert a.dtype == want
		for s in (2, 5):
			for a, b in zip(first, got(out, name, s)):
				assert np.array_equal(a, b, equal_nan=True), (name, s)
		p, d, v = first
		assert exact_structure(p, d) and np.isfinite(p).all()
		pr, dr, vr = norm.coex(arrays[name + '_dt'], arrays[name + '_dc'])
		assert (p_close32 if np.float32 in (want, pr.dtype) else p_close)(p, pr), name
		tol = 1e-9 if want == np.float64 and pr.dtype == np.float64 else 1e-6  # (fp32 results carry 6e-8 of rounding each)
		assert scale_close(d, dr, tol) and scale_close(v, vr, tol)


def debug_with(switch):
	"""NRM_DEBUG for a child: the keys this process has, and `switch`."""
	return ','.join([p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip()] + [switch])


def test_coex_plan_c_entry_graph_switch_off(golden, tmp_path):
	"""NRM_DEBUG graph=0 in the child: three steps on G1, none of them captured, and the same bits as the three steps -- eager, captured, replayed -- without it."""
	g1 = golden('G1_c1')
	ns = int(g1['coex_n'])
	arrays = dict(dt=g1['dt'][:ns], dc=g1['dc'])
	job = dict(cases=[dict(name='g1', dt='dt', dc='dc', steps=3, snaps=[3])])
	(tmp_path / 'on').mkdir(), (tmp_path / 'off').mkdir()
	out, info = run_child(tmp_path / 'on', 'cases', arrays, job)
	out0, info0 = run_child(tmp_path / 'off', 'cases', arrays, job, env={'NRM_DEBUG': debug_with('graph=0')})
	print(info['g1'], info0['g1'])
	assert info['g1']['captured'] == 1 and info['g1']['steps'] == 3
	assert info0['g1']['captured'] == 0 and info0['g1']['steps'] == 3
	for a, b in zip(got(out0, 'g1', 3), got(out, 'g1', 3)):
		assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
	assert p_close(got(out0, 'g1', 3)[0], g1['coex_p'])


def test_coex_plan_c_entry_in_place_rewrite(golden, tmp_path):
	import normalisr_amd.normalisr as norm
	g = golden('G11_i8hard')
	a, dc = child.expression(7, 130, 2052, 'float32')
	b = child.expression(8, 130, 2052, 'float32')[0]
	a2, dc2 = child.expression(9, 257, 300, 'float64')
	b2 = child.expression(10, 257, 300, 'float64')[0]
	out, info = run_child(tmp_path, 'rewrite', dict(a=a, b=b, dc=dc, a2=a2, b2=b2, dc2=dc2, a3=g['dt'], dc3=g['dc_onehot']), {})
	print(info)
	# an adopted matrix rewritten in place: the next replay is a fresh plan's first step, bit for bit; still one capture
	assert info['adopted']['engine'] == 6 and info['adopted']['captured'] == 1 and info['adopted']['steps'] == 4
	for x, y in zip(got(out, 'adopted', '_new'), got(out, 'adopted', '_fresh')):
		assert np.array_equal(x, y)
	assert not np.array_equal(out['adopted.p_old'], out['adopted.p_new'])
	assert p_close32(out['adopted.p_new'], norm.coex(b, dc)[0])
	assert 'adopted' in info['adopted_update']  # update() refuses an adopted matrix (ValueError), and so does the library (NRM_E_ARG)
	assert info['adopted_upload_rc'] == -1 and 'adopted' in info['adopted_upload_msg']
	# the same values behind a padded pitch (ld = n + 4, rows still 16-byte aligned): the integer engine, and the contiguous plan's bits
	assert info['padded']['engine'] == 6 and info['padded']['captured'] == 1
	for x, y in zip(got(out, 'padded'), got(out, 'adopted', '_fresh')):
		assert np.array_equal(x, y)
	# update() on a plan-owned copy
	assert info['owned']['engine'] == 0 and info['owned']['captured'] == 1 and info['owned']['steps'] == 4
	for x, y in zip(got(out, 'owned', '_new'), got(out, 'owned', '_fresh')):
		assert np.array_equal(x, y)
	assert p_close(out['owned.p_new'], norm.coex(b2, dc2)[0])
	# a pitch that is no multiple of 4 at 4096 cells: the fp64 kernel, and the golden vectors
	assert info['pitched']['engine'] == 0 and info['pitched']['captured'] == 1
	p, d, v = got(out, 'pitched')
	assert exact_structure(p, d) and p_close(p, g['coex_onehot_p']) and scale_close(d, g['coex_onehot_dot']) and scale_close(v, g['coex_onehot_var'])


@pytest.mark.parametrize('tol', ['3e-9', '0'])
def test_coex_plan_c_entry_guard_reruns_on_fp64(tol, tmp_path):
	"""The construction of test_guard_fires_inside_the_pipelined_and_chunked_paths (tests/test_gpu_round3.py): at a tolerance of 3e-9 the guard cannot certify the
	pairs of spike rows, check() says so and redoes the step on the fp64 kernel once; at 0 there is no guard and no rerun.  Either way the oracle to 1e-6."""
	dt, dc = child.guard_inputs()
	ng = dt.shape[0]
	sel = np.r_[0:60, 1000:1040, ng - 30:ng]
	out, r = run_child(tmp_path, 'guard', {}, dict(sel=sel.tolist()), env={'NRM_I8_GUARD_TOL': tol})
	print(r)
	assert r['info']['engine'] == 6 and r['info']['captured'] == 1
	if tol == '0':
		assert r['hits'] == 0 and r['info']['reruns'] == 0
	else:
		assert r['hits'] > 0  # the precondition: the guard fired
		assert r['info']['reruns'] == 1 and r['hits_after'] == 0
	po, do, vo = oracle.coex(dt[sel].astype(np.float64), dc.astype(np.float64))
	off = ~np.eye(len(sel), dtype=bool)
	assert bool(out['p_diag_zero'])
	ok = p_close(out['p'][off], po[off])  # (printed either way; without the guard nothing is claimed for the spike rows' pairs)
	assert scale_close(out['var'], vo)
	if tol != '0':
		assert ok


def test_coex_plan_c_entry_chain_binnet_in_hbm(tmp_path):
	import normalisr_amd.normalisr as norm
	dt, dc = child.expression(21, 300, 2500, 'float64')
	qcut = 0.2
	out, info = run_child(tmp_path, 'chain', dict(dt=dt, dc=dc), dict(qcut=qcut))
	print(info)
	assert info['engine'] == 6 and info['captured'] == 1
	want = np.asarray(norm.binnet(norm.coex(dt, dc)[0], qcut))
	assert out['flags'][0] == 0 and int(out['total'][0]) == int(want.sum()) > 0
	assert np.array_equal(out['net'].astype(bool), want)


def test_coex_plan_c_entry_errors_and_two_plans(tmp_path):
	a, dc = child.expression(31, 130, 300, 'float64')
	b = child.expression(32, 130, 300, 'float64')[0]
	out, notes = run_child(tmp_path, 'errors', dict(a=a, b=b, dc=dc), {})
	print(notes)
	assert notes['nan'].startswith('AssertionError') and 'non-finite' in notes['nan']
	for x, y in zip(got(out, 'after_nan'), got(out, 'fresh_a')):  # usable again after update() with clean values
		assert np.array_equal(x, y)
	for k in ('a', 'b'):  # two plans stepped alternately, the pool emptied between steps: each its own fresh computation
		assert notes['two_' + k]['captured'] == 1 and notes['two_' + k]['steps'] == 4
		for x, y in zip(got(out, 'two_' + k), got(out, 'fresh_' + k)):
			assert np.array_equal(x, y)
	po, do, vo = oracle.coex(b, dc, dimreduce=1)
	assert p_close(out['fresh_b.p'], po) and scale_close(out['fresh_b.dot'], do)


def test_coex_plan_c_entry_teardown_returns_the_pool(tmp_path):
	a, dc = child.expression(41, 257, 2052, 'float32')
	out, n = run_child(tmp_path, 'teardown', dict(a=a, dc=dc), {})
	print(n)
	assert n['before'] == [0, 0]
	assert n['alive'][1] >= n['bytes'] > 0 and n['alive'][0] >= n['alive'][1]
	assert n['alive_after_release'][1] == n['alive'][1] and n['alive_after_release'][0] == n['alive'][1]  # a live plan's buffers stay; idle blocks go
	assert n['closed'][1] == 0  # destroy gives everything back to the pool ...
	assert n['released'] == [0, 0]  # ... and nrm_release_cache then frees it: no device memory held
