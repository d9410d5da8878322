"""CPU-only checks of the resident co-expression loop (normalisr_amd/levels.py, `normalisr coex_levels`): the numpy restatement of tests/levels_numpy.py -- the
independent check of the GPU tests -- against what the reference's coex returned on every cumulative covariate set (golden G23, tests/golden/make_g23.py), the
append decision as a pure function, every argument error before any device call, the parser and the library's two entries."""
import os
import sys

import numpy as np
import pytest

import levels_numpy as ln
from conftest import GOLDEN, ROOT

if GOLDEN not in sys.path:
	sys.path.insert(0, GOLDEN)
from g23_inputs import RANKS  # noqa: E402
from levels_numpy import g23_case, of_largest, p_errors  # noqa: E402


@pytest.mark.parametrize('name', ('A', 'B'))
def test_numpy_restatement_matches_the_reference_at_every_level(golden, name):
	g = golden('G23_coex_levels')
	dt, dc, rows = g23_case(g, name)
	lv = ln.Levels(dt.astype(np.float64), dc)
	for k in range(5):
		if k:
			lv.append(rows[k - 1])
		assert lv.rank == RANKS[k] and lv.dof == dt.shape[1] - 1 - RANKS[k]
		p, dot, var = lv.results()
		ep, small = p_errors(p, g['{}_p{}'.format(name, k)])
		ed, ev = of_largest(dot, g['{}_dot{}'.format(name, k)]), of_largest(var, g['{}_var{}'.format(name, k)])
		print(name, k, 'P %.3g relative, %.3g below 1e-290; dot %.3g, var %.3g of the largest' % (ep, small, ed, ev))
		assert ep < 1e-9 and small < 1e-289 and ed < 1e-10 and ev < 1e-10
		assert (np.diag(p) == 0).all() and (np.diag(dot) == 0).all()
	assert lv.rebuilt == [False] * 4 and lv.info['counters'] == (0, 0)
	# the update against the from-scratch Gram matrix of the same level, in longdouble: the identity itself
	gl, sl, _, r = ln.gram(dt, np.concatenate([dc, rows]), np.longdouble)
	assert r == 10
	assert of_largest(lv.g, np.asarray(gl, dtype=np.float64)) < 1e-11 and of_largest(lv.ss, np.asarray(sl, dtype=np.float64)) < 1e-11


def test_fixture_is_what_the_issue_describes(golden):
	g = golden('G23_coex_levels')
	assert g['A_dt'].shape == (48, 700) and g['A_dt'].dtype == np.float32 and g['A_dc'].shape == (8, 700) and g['A_rows'].shape == (4, 700)
	assert g['A_p4'].shape == (48, 48) and g['B_p4'].shape == (24, 24) and g['B_var0'].shape == (24, )
	for name in ('A', 'B'):
		keeps = g[name + '_var2'][1] / g[name + '_var1'][1]
		assert 0.005 < keeps < 0.02  # gene 1 keeps 1 % of its variance when the second row is removed
		assert np.array_equal(g[name + '_p2'], g[name + '_p3']) or of_largest(g[name + '_dot3'], g[name + '_dot2']) < 1e-12  # the third row is in the span
	dt = g['A_dt'].astype(np.float64)
	assert dt[2].mean() / dt[2].std() > 800


def test_append_decision_is_a_pure_function(golden):
	from normalisr_amd import levels
	from normalisr_amd.association import inv_rank
	g = golden('G23_coex_levels')
	for name in ('A', 'B'):
		dt, dc, rows = g23_case(g, name)
		cov = dc
		b, r = levels.covariate_basis(cov)
		assert r == 7 and b.shape == (7, dc.shape[1]) and np.abs(b @ b.T - np.eye(7)).max() < 1e-14
		for k in range(4):
			plan = levels.plan_append(b, cov, rows[k:k + 1])
			mine = ln.decide(ln.span_basis(cov)[0], cov, rows[k:k + 1])
			both = np.concatenate([cov, rows[k:k + 1]])
			assert plan['rank'] == mine['rank'] == RANKS[k + 1] == inv_rank(both @ both.T)[1]
			assert plan['update'] and mine['update'] and np.array_equal(plan['rho'] >= levels.RHO_MIN, mine['rho'] >= ln.RHO_MIN)
			again = levels.plan_append(b, cov, rows[k:k + 1])
			assert np.array_equal(again['rho'], plan['rho']) and np.array_equal(again['q'], plan['q'])  # the same arguments, the same answer
			if k == 2:  # the in-span row adds nothing
				assert plan['rho'][0] <= levels.RHO_SPAN and plan['q'].shape == (0, dc.shape[1]) and mine['q'] == []
			else:
				q = plan['q']
				assert q.shape == (1, dc.shape[1]) and abs(float(q[0] @ q[0]) - 1) < 1e-14 and np.abs(b @ q[0]).max() < 1e-14
				assert np.abs(q[0] - np.asarray(mine['q'][0])).max() < 1e-12
				b = np.concatenate([b, q])
			cov = both
		# a row that keeps 1e-9 of its squared length outside the span asks for a rebuild, whatever the rank says
		rng = np.random.default_rng(5)
		fresh = ln.off_span(b, rng.standard_normal(dc.shape[1]))
		inside = b.T @ rng.standard_normal(len(b))
		v = inside / np.sqrt(inside @ inside) + np.sqrt(1e-9) * fresh / np.sqrt(fresh @ fresh)
		plan = levels.plan_append(b, cov, v[None, :])
		assert 0.9e-9 < plan['rho'][0] < 1.1e-9 and not plan['update'] and plan['q'].shape[0] == 0
		assert not ln.decide(b, cov, v[None, :])['update']
		# three rows at once: the same directions as one by one
		b0 = levels.covariate_basis(dc)[0]
		plan = levels.plan_append(b0, dc, rows[:3])
		assert plan['update'] and plan['rank'] == 9 and plan['q'].shape[0] == 2 and np.abs(plan['q'] @ plan['q'].T - np.eye(2)).max() < 1e-14
		assert plan['rho'][2] <= levels.RHO_SPAN and np.abs(plan['q'] - b[7:9]).max() < 1e-12
		# the same row twice in one call: the second lies in the span of the first
		plan = levels.plan_append(b0, dc, rows[[0, 0]])
		assert plan['update'] and plan['rank'] == 8 and plan['q'].shape[0] == 1 and plan['rho'][1] <= levels.RHO_SPAN
		# two rows a part in 1e8 away from parallel: neither new nor in the span -> rebuild
		assert not levels.plan_append(b0, dc, np.stack([rows[0], rows[0] + 1e-4 * rows[1]]))['update']
		# a zero row lies in the span
		plan = levels.plan_append(b0, dc, np.zeros((1, dc.shape[1])))
		assert plan['update'] and plan['rank'] == 7 and plan['q'].shape[0] == 0


def test_guard_counters_of_the_restatement():
	ref = np.array([1.0, 1.0, 1.0, 1.0, 0.0])
	new = np.array([2.0**-11, 2.0**-9, -1e-3, np.nan, 0.0])
	assert ln.guard(new, ref) == (3, 2)  # not finite or <= 0: rows 2, 3, 4; below 2^-10 of the reference: rows 0 and 2


def test_argument_errors_match_coex_before_any_device_call(monkeypatch):
	from normalisr_amd import _lib, engine, levels
	from normalisr_amd.association import association_tests

	def no_device(*a, **ka):
		raise AssertionError('the device was touched before the arguments were checked')
	monkeypatch.setattr(_lib, 'load', no_device)
	monkeypatch.setattr(engine, 'get_engine', no_device)
	rng = np.random.default_rng(1)
	dt, dc = rng.standard_normal((5, 12)), np.concatenate([rng.standard_normal((2, 12)), np.ones((1, 12))])
	nan = dc.copy()
	nan[0, 3] = np.nan
	cases = [(dt[0], dc, 0), (dt, dc[0], 0), (dt, dc[:, :11], 0), (dt[:0], dc, 0), (dt, dc, 1.5), (dt, dc, 8), (dt, np.concatenate([dc, rng.standard_normal((8, 12))]), 0),
			 (dt, nan, 0)]
	for x, c, d in cases:
		with pytest.raises(Exception) as want:
			association_tests(x, None, c, dimreduce=d)
		assert not str(want.value).startswith('the device was touched'), want.value
		with pytest.raises(type(want.value)) as got:
			levels.CoexLevels(x, c, dimreduce=d)
		assert str(got.value) == str(want.value)
		with pytest.raises(type(want.value)) as got:
			levels.coex_levels(x, c, ['g%d' % i for i in range(len(x))], None, 0.05, dimreduce=d)
		assert str(got.value) == str(want.value)
	with pytest.raises(AssertionError, match='array must not contain infs or NaNs'):  # (an AssertionError as well: what append's callers are told to expect)
		levels.CoexLevels(dt, nan)
	names = ['a', 'b', 'c', 'd', 'e']
	with pytest.raises(ValueError, match='Q-value cutoff must be between 0 and 1'):
		levels.coex_levels(dt, dc, names, None, 1.0)
	with pytest.raises(ValueError, match='Wrong shape for net or namet'):
		levels.coex_levels(dt, dc, names[:4], None, 0.05)
	with pytest.raises(ValueError, match='Number of principal genes'):
		levels.coex_levels(dt, dc, names, None, 0.05, n=5)
	with pytest.raises(ValueError, match='keep names'):
		levels.coex_levels(dt, dc, names, None, 0.05, n=2, keep=('net', 'alpha'))
	with pytest.raises(ValueError, match='lvmax'):
		levels.coex_levels(dt, dc, names, None, 0.05, n=2, lvmax=-1)

	# append: the checks of coex on the enlarged covariates, on an object whose device state is never reached
	lv = levels.CoexLevels.__new__(levels.CoexLevels)
	lv.nt, lv.ns, lv.dc, lv.dimreduce, lv.level, lv.rebuilt = 5, 12, dc, 0, 0, []
	row = rng.standard_normal(12)
	bad = row.copy()
	bad[5] = np.inf
	for rows in (bad, np.stack([row, bad])):
		with pytest.raises(AssertionError, match='array must not contain infs or NaNs'):
			lv.append(rows)
		with pytest.raises(ValueError, match='array must not contain infs or NaNs'):  # coex's own class and text (inv_rank)
			lv.append(rows)
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions'):
		lv.append(row[:11])
	with pytest.raises(ValueError, match='Incorrect dx/dy/dc size'):
		lv.append(np.zeros((1, 1, 12)))
	with pytest.raises(ValueError, match='Insufficient number of cells: must be greater than degrees of freedom removed \\+ covariate \\+ 1.'):
		lv.append(rng.standard_normal((8, 12)))
	assert lv.dc is dc and lv.level == 0 and lv.rebuilt == []


def test_library_declares_the_two_entries():
	from normalisr_amd import _lib
	lib = _lib.load()
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	for name in ('nrm_coex_project', 'nrm_coex_downdate'):
		assert name in _lib.exported_symbols() and hasattr(lib, name) and name + '(' in hdr
	assert 'association.py:224-235' in hdr[hdr.index('nrm_coex_project:') - 1500:hdr.index('nrm_coex_project:')]
	# argument checks of the entries answer before any launch
	F32, F64, E = _lib.NRM_F32, _lib.NRM_F64, _lib.NRM_E_ARG
	assert lib.nrm_coex_project(16, F32, 4, 10, 9, 16, 1, 10, 16, 4, 0) == E  # a pitch below the row
	assert lib.nrm_coex_project(16, F32, 4, 10, 10, 16, 0, 10, 16, 4, 0) == E and lib.nrm_coex_project(16, F32, 4, 10, 10, 16, 9, 10, 16, 4, 0) == E  # 1 to 8 directions
	assert lib.nrm_coex_project(20, F64, 4, 10, 10, 16, 1, 10, 16, 4, 0) == E  # fp64 rows off their 8-byte boundary
	assert lib.nrm_coex_project(16, 7, 4, 10, 10, 16, 1, 10, 16, 4, 0) == E and lib.nrm_coex_project(16, F32, 4, 10, 10, 16, 1, 10, 16, 3, 0) == E
	assert lib.nrm_coex_project(0, F32, 4, 10, 10, 16, 1, 10, 16, 4, 0) == E
	assert lib.nrm_coex_downdate(16, 4, 3, 16, 16, 16, 1, 4, 16, 0) == E  # G narrower than its rows
	assert lib.nrm_coex_downdate(16, 4, 4, 16, 16, 16, 0, 4, 16, 0) == E and lib.nrm_coex_downdate(16, 4, 4, 16, 16, 16, 1, 3, 16, 0) == E
	assert lib.nrm_coex_downdate(16, 4, 4, 16, 0, 16, 1, 4, 16, 0) == E and lib.nrm_coex_downdate(16, 4, 4, 16, 16, 16, 1, 4, 18, 0) == E


def test_parser_and_runner_of_coex_levels(tmp_path):
	from normalisr_amd.__main__ import build_parser
	from normalisr_amd import run
	p = build_parser()
	ns = vars(p.parse_args(['coex_levels', 'e', 'c', 'g', '1E-3', 'out', '--gmt', 'sets.gmt']))
	assert (ns['cmd'], ns['exp_in'], ns['cov_in'], ns['genes_in'], ns['qcut'], ns['out_dir'], ns['gmt']) == ('coex_levels', 'e', 'c', 'g', 1e-3, 'out', 'sets.gmt')
	assert (ns['lvmax'], ns['n'], ns['nmin'], ns['dimr'], ns['ext'], ns['pv'], ns['dot'], ns['var'], ns['key']) == (5, 100, 5, None, '.tsv', False, False, False, 'id')
	ns = vars(p.parse_args(['coex_levels', 'e', 'c', 'g', '0.1', 'out', '--go', 'o.obo', 'a.gaf', '--key', 'symbol', '-l', '2', '-n', '10', '-m', '3', '-d', '1', '--ext', '.npy',
							'--pv', '--dot', '--var']))
	assert (ns['go'], ns['key'], ns['lvmax'], ns['n'], ns['nmin'], ns['dimr'], ns['ext'], ns['pv'], ns['dot'], ns['var']) == (['o.obo', 'a.gaf'], 'symbol', 2, 10, 3, 1, '.npy', True,
																															 True, True)
	with pytest.raises(SystemExit):
		p.parse_args(['coex_levels', 'e', 'c', 'g', '0.1', 'out'])  # neither --gmt nor --go
	assert callable(run.coex_levels)
	# the command checks its arguments before any device call and writes nothing
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('e.tsv'), np.arange(20.0).reshape(4, 5), delimiter='\t', fmt='%.8G')
	np.savetxt(f('c.tsv'), np.ones((1, 4)), delimiter='\t', fmt='%.8G')
	run.file_write_txtlist(f('g.txt'), ['a', 'b', 'c', 'd'])
	with open(f('s.gmt'), 'w') as fh:
		fh.write('S1\tfirst\ta\tb\n')
	args = dict(exp_in=f('e.tsv'), cov_in=f('c.tsv'), genes_in=f('g.txt'), qcut=0.05, out_dir=f('out'), gmt=f('s.gmt'), go=None, key='id', lvmax=1, n=2, nmin=1, dimr=None,
				ext='.tsv', pv=False, dot=False, var=False)
	with pytest.raises(ValueError, match='Unmatching dx/dy/dc dimensions'):
		run.coex_levels(args)
	assert not os.path.exists(f('out'))


def test_module_is_exported_and_the_facade_is_unchanged():
	import importlib
	import normalisr_amd
	assert 'levels' in normalisr_amd.__all__
	assert importlib.import_module('normalisr.levels') is importlib.import_module('normalisr_amd.levels')
	import normalisr_amd.normalisr as norm
	assert 'coex_levels' not in vars(norm) and 'CoexLevels' not in vars(norm)
