"""CPU: the kernel-level reference of normvar (tests/nv_reference.py) is anchored to the project's model (oracle.normvar), accepts an fp64 emulation of every kernel in
the kernel's own order at EVERY case tests/test_gpu_nv_stages.py runs, rejects mutations of that emulation, makes every integer rank of its cases a fact, launches
every instantiation csrc/nrm_normvar.hip compiles, and shows on the ladder of cancellation what the one-pass scale loses and the rule of csrc/nrm_nv_scale.h keeps."""
import os
import re

import numpy as np
import pytest

import oracle
import nv_reference as nv

F32, F64 = np.float32, np.float64
WORST = {}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'normalisr_amd', 'csrc')
IDS = [nv.case_id(c) for c in nv.CASES]


def note(stage, ws):
	for k, w in ws.items():
		WORST[(stage, k)] = max(WORST.get((stage, k), 0.0), w.ratio)
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (stage, bad)


def composed(dt, dc, w, wt, keepvar=True, tol=nv.TOL):
	"""weights -> moments -> solve -> apply in longdouble, with the scale both ways."""
	lnw = np.log(nv.ld(w))
	mom, _ = nv.moments(dt, lnw, wt, dc)
	sv = nv.solve(mom, dc.shape[0], dt.shape[1], wt, tol, keepvar)
	tp = nv.scale_two_pass(dt, lnw, wt, dc, sv['b'])
	return nv.apply(dt, lnw, wt, dc, sv['b'], sv['scale'])[0], sv, tp, mom


def seeded(seed, ng=12, n=400, nc=3):
	rng = np.random.default_rng(seed)
	dt = rng.normal(size=(ng, n)) * rng.uniform(0.5, 2, (ng, 1)) - 9
	w, wt = np.exp(0.25 * rng.normal(size=n)), rng.uniform(0, 1.5, ng)
	wt[::5] = 0
	return dt, np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))]), w, wt


@pytest.mark.parametrize('which', ['G9', 'seed 3', 'seed 4'])
def test_composed_reference_agrees_with_the_oracle(golden, which):
	"""The chain of the entry references gives oracle.normvar's result, and scale_two_pass the oracle's dv and dv2.  The allowance is the oracle's own fp64: a result
	element is a residual of n + nc terms against the weighted row, scaled: (n + 4 nc + 8) u x cond(M_g) x (|y e| + sum |b c e|) x scale, which the test takes as
	1e-11 of the row's largest magnitude at these shapes (n <= 400, cond <= 1e3) -- measured and printed, and the comparison is not vacuous."""
	if which == 'G9':
		g = golden('G9_normvar')
		dt, dc, w, wt = (np.asarray(g[k], F64) for k in ('dt', 'dc', 'w', 'wt'))
	else:
		dt, dc, w, wt = seeded(int(which[-1]))
	want = oracle.normvar(dt, dc, w, wt)[0]
	plain = oracle.normvar(dt, dc, w, wt, keepvar=False)[0]
	out, sv, tp, mom = composed(dt, dc, w, wt)
	err = np.asarray(np.abs(out - want).max(axis=1), F64) / np.abs(want).max(axis=1)
	print('%s: composed reference against oracle.normvar, worst row error / row maximum %.3g' % (which, err.max()))
	assert 0 < err.max() < 1e-11
	w2 = w[None, :]**wt[:, None]
	w2[wt == 0] = 1
	dv = np.sqrt((((dt * w2).T - (dt * w2).mean(axis=1))**2).mean(axis=0))  # the oracle's line for norm.py:248-249
	dv2 = np.sqrt((plain**2).mean(axis=1))  # ... and for norm.py:255 on its own residuals
	e1, e2 = np.abs(np.asarray(tp['dv'] / dv - 1, F64)).max(), np.abs(np.asarray(tp['dv2'] / dv2 - 1, F64)).max()
	print('%s: scale_two_pass against the oracle: dv %.3g, dv2 %.3g; one-pass against two-pass scale %.3g' % (which, e1, e2, np.abs(np.asarray(sv['scale'] / tp['scale'] - 1, F64)).max()))
	assert e1 < 1e-13 and e2 < 1e-11
	assert not sv['marked'].any() and np.abs(np.asarray(sv['scale'] / tp['scale'] - 1, F64)).max() < 1e-11  # (rows at rho ~ 1: the two forms agree)


# ---- the emulation inside the bounds at every GPU case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('i', range(len(nv.CASES)), ids=IDS)
def test_emulation_inside_the_bounds(i, exact):
	got = nv.emulate(i, exact)
	ws = nv.judge_case(got, i, exact)
	if nv.CASES[i]['entry'] == 'solve':  # the marked genes' scale from the row (k_nv_rescale in its own order)
		pb = nv.problem(i, exact)
		marked = got['scale'] == nv.MARK
		with np.errstate(all='ignore'):
			again = nv.emu_rescale(pb['y'], pb['lnw'], pb['wt'], pb['c'], got['b'], got['scale'])
		assert nv.same_bits(again[~marked], got['scale'][~marked]).all()
		ws['rescaled'] = nv.judge_rescale(again, got['b'], i, marked, exact)[0]
	note(nv.CASES[i]['entry'] + (' exact' if exact else ''), ws)


def test_exact_twins_are_exact():
	"""On the twins every product and partial sum is an integer (or a dyadic) below 2^53: the longdouble reference IS the fp64 result in any order."""
	for i, c in enumerate(nv.CASES):
		pb = nv.problem(i, True)
		assert (pb['lnw'] == 0).all() and (pb['y'] == np.round(pb['y'])).all()
		if c['nc']:
			assert (pb['c'] == np.round(pb['c'])).all()
		if c['entry'] == 'solve':
			mom = nv.moments(pb['y'], pb['lnw'], pb['wt'], pb['c'])[0]
			assert (np.abs(mom) < 2.0**53).all() and (mom == np.round(mom)).all()
		if c['entry'] == 'apply':
			assert (pb['b'] * 4 == np.round(pb['b'] * 4)).all() and (np.log2(pb['scale']) == np.round(np.log2(pb['scale']))).all()


def test_every_rank_is_a_fact():
	"""Every eigenvalue of every gene's M_g lies at least 1e3 away from tol x the largest, as a factor, on both sides; and the table holds each kind of deficiency."""
	kinds = set()
	for i, c in enumerate(nv.CASES):
		if c['entry'] != 'solve':
			continue
		for exact in (False, True):
			pb = nv.problem(i, exact)
			sv = nv.solve(np.asarray(nv.reference(i, exact)[0], F64), c['nc'], c['n'], pb['wt'], nv.TOL, c['keepvar'])
			assert (sv['gap'] >= 1e3).all(), (nv.case_id(c), sv['gap'].min())
			kinds.add((c['cov'], 'deficient' if (sv['rank'] < c['nc']).any() else 'full'))
	print(sorted(kinds))
	assert {('full', 'full'), ('full', 'deficient'), ('repeat', 'deficient'), ('onehot', 'deficient'), ('zero', 'full')} <= kinds  # (zero: inv_rank keeps every zero eigenvalue)


# ---- mutations -------------------------------------------------------------------------------------------------------------------------------------------------------
def find(entry, **want):
	for i, c in enumerate(nv.CASES):
		if c['entry'] == entry and all((v(c[k]) if isinstance(v, type(find)) else c[k] == v) for k, v in want.items()):
			return i
	raise KeyError((entry, want))


MUTATIONS = [  # (entry, mutation, how to choose the case)
	('weights', 'tail cells dropped', dict(n=1029)),
	('weights', 'one wave left out', dict(n=1029)),
	('weights', 'e for e^2 in U', dict(n=7)),
	('weights', 'wt of the neighbouring row', dict(n=1029)),
	('weights', 'padding columns of U left', dict(layout='aligned', n=7)),
	('weights', 'padding rows of V left', dict(n=7)),
	('solve', 'tail cells dropped', dict(n=1029)),
	('solve', 'one wave left out', dict(n=2053)),
	('solve', 'pairs in tril order', dict(nc=3, n=lambda n: n > 7)),
	('solve', 'e for e^2 in a', dict(nc=2, n=lambda n: n > 7)),
	('solve', 'wt of the neighbouring row', dict(n=lambda n: n > 7, keepvar=1, rows=lambda r: r > 2)),
	('solve', 'last covariate missing from the fit', dict(nc=3, n=lambda n: n > 7)),
	('solve', 'mean divided by the pitch', dict(n=lambda n: n > 7, keepvar=1, cov='full', rows=lambda r: r > 1, layout=lambda v: v != 'minimal')),
	('solve', 'second gene of an odd last pair dropped', dict(rows=lambda r: r % 2 == 0)),
	('apply', 'tail cells dropped', dict(n=1029)),
	('apply', 'scale of the neighbouring row', dict(rows=lambda r: r > 1)),
	('apply', 'wt of the neighbouring row', dict(rows=lambda r: r > 1)),
	('apply', 'last covariate missing from the fit', dict(nc=9)),
	('apply', 'WIDE table read at pitch 64', dict(nc=65, rows=lambda r: r > 1)),
	('apply', 'fp32 output truncated, not rounded', dict(odt=F32)),
	('apply_w2', 'last covariate missing from the fit', dict(nc=63)),
	('apply_w2', 'w2 of the neighbouring row', dict(rows=lambda r: r > 1)),
]


@pytest.mark.parametrize('entry,mut,want', MUTATIONS, ids=['%s: %s' % m[:2] for m in MUTATIONS])
def test_mutations_are_rejected(entry, mut, want):
	"""Each mutation of the emulation leaves at least one bound -- on real data AND on the exact twin where the mutation moves a value there (named below)."""
	i = find(entry, **want)
	ws = nv.judge_case(nv.emulate(i, False, mut), i, False)
	bad = {k: w.ratio for k, w in ws.items() if not w.ratio <= 1}
	print(nv.case_id(nv.CASES[i]), mut, bad)
	assert bad, (entry, mut)
	if mut in ('tail cells dropped', 'one wave left out', 'pairs in tril order', 'last covariate missing from the fit', 'padding columns of U left', 'scale of the neighbouring row'):
		ws = nv.judge_case(nv.emulate(i, True, mut), i, True)
		assert any(not w.ratio <= 1 for w in ws.values()), (entry, mut, 'exact twin')


def test_flag_mutation_is_rejected_and_the_count_follows_the_thread_map():
	"""flags[1] += (workgroup, wave) pairs that stored a non-finite value: a planted inf in the four-cell loop and one in the tail loop of the same row land in different
	waves only when their threads do; set-instead-of-added shows once the counter starts non-zero; a row past the last workgroup's live rows stores nothing."""
	i = find('apply', n=1029, odt=F64, nc=lambda q: q <= 9)
	pb = dict(nv.problem(i))
	y = pb['y'].copy()
	y[0, 5] = np.inf  # thread 1 of the four-cell loop: wave 0
	y[0, 1028] = np.inf  # the tail loop (n4 = 1028), thread 0: wave 0 again -> still one pair
	y[0, 600] = np.inf  # thread 150: wave 2
	rows = y.shape[0]
	y[rows - 1, 1027] = -np.inf  # the second iteration of thread 0, wave 0: a new pair only in another workgroup
	want = 2 + (1 if (rows - 1) // 4 != 0 else 0)
	args = (y, pb['lnw'], pb['wt'], pb['c'], pb['b'], pb['scale'], pb['odt'])
	assert nv.emu_apply(*args, flags1=0)['flags1'] == want
	assert nv.emu_apply(*args, flags1=5)['flags1'] == want + 5
	assert nv.emu_apply(*args, flags1=5, mut='flags[1] set instead of added')['flags1'] != want + 5
	th, tail = nv.thread_of(1029)
	assert th[5] == 1 and th[600] == 150 and th[1028] == 0 and tail[1028] and not tail[1027] and th[1023] == 255 and th[1027] == 0
	m = nv.map_four(1029)
	assert sorted(m[m >= 0].tolist()) == list(range(1029)) and m[0].tolist() == [0, 1, 2, 3, 1024, 1025, 1026, 1027, 1028] and m[1].tolist() == [4, 5, 6, 7, -1, -1, -1, -1, -1]


def test_properties_pinned_from_the_kernel_text():
	"""Mutations that cannot reach an output as data are pinned as text: flags[1] is added to by atomicAdd, never stored; the mean divides by n (the shared rule takes n,
	the solve passes the cell count); the WIDE table's pitch is nc; genes past the end store nothing; the moments' waves are added in the documented order."""
	src = open(os.path.join(CSRC, 'nrm_normvar.hip')).read()
	rule = open(os.path.join(CSRC, 'nrm_nv_scale.h')).read()
	assert 'atomicAdd(&flags[1], 1)' in src and not re.search(r'flags\[1\]\s*=[^=]', src)
	assert 'atomicAdd(&flags[0], 1)' in src and not re.search(r'flags\[0\]\s*=[^=]', src)
	assert 'const int ldb = WIDE ? nc : 64;' in src
	# an fp32 output rounded through fp32 twice is the same value (the cast is idempotent): no data shows it.  What is pinned is that the result is ONE cast of the fp64
	# expression, never an fp32 intermediate
	assert 'const OutT o = (OutT)(sc[r] * e * (yv - fit));' in src and '(OutT)((double)y[(row0 + r) * ldy + k] - w2[(row0 + r) * ldw + k] * fit[r])' in src
	assert not re.search(r'\(float\)', src)
	assert 'const double mean = s1 / n;' in rule and 'nrm_nv_scale(mo[NP + NC], mo[NP + NC + 1], ab, (double)n, wt[g])' in src
	assert '((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid]' in src and 'g0 + tid / NM < rows' in src
	assert '#define NRM_NV_TAU 0x1p-20' in rule and nv.TAU == 2.0**-20 and '#define NRM_NV_MARK (-1.0)' in rule and nv.MARK == -1.0
	from normalisr_amd import norm
	assert norm.NV_TAU == nv.TAU and norm.NV_MARK == nv.MARK


# ---- the routes --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_launches_every_instantiation():
	got = set()
	for c in nv.CASES:
		got |= nv.route(c)
	want = nv.all_instantiations()
	by = {}
	for k in want:
		by[k[0]] = by.get(k[0], 0) + 1
	print('instantiations:', by, 'covered', len(got & want), 'of', len(want))
	assert by == {'k_nv_moments': 32, 'k_nv_solve': 8, 'k_nv_apply': 16, 'k_nv_apply_w2': 4, 'k_nv_weights': 2}
	assert got == want, sorted(want - got, key=str)
	# the edges the issue names, each in at least one case of the entry it belongs to
	for entry, key, values in (('weights', 'n', nv.CELLS), ('weights', 'rows', nv.GENES), ('solve', 'nc', range(1, 9)), ('apply', 'nc', nv.APPLY_NC), ('apply_w2', 'nc', nv.W2_NC)):
		have = {c[key] for c in nv.CASES if c['entry'] == entry}
		assert set(values) <= have, (entry, key, set(values) - have)
	for entry in ('solve', 'apply'):
		assert {c['n'] for c in nv.CASES if c['entry'] == entry} >= {1, 3, 4, 7, 1024, 1029, 2053}, entry
		assert {c['rows'] for c in nv.CASES if c['entry'] == entry} >= {1, 2, 3, 5, 9, 65, 130}, entry
		assert {c['layout'] for c in nv.CASES if c['entry'] == entry} >= set(nv.LAYOUTS) - ({'out off'} if entry == 'solve' else set()), entry
	assert any(c['nc'] == 1024 and c['n'] == 5 and c['rows'] == 5 for c in nv.CASES)
	assert {c['keepvar'] for c in nv.CASES if c['entry'] == 'solve'} == {0, 1} and {c['cov'] for c in nv.CASES if c['entry'] == 'solve'} == set(nv.COVS)


# ---- the ladder ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ladder_of_cancellation():
	"""rho = dv2 / rms(weighted row) from 1 to 1e-7, a nearly flat row and a row the covariates explain: the relative error of the scale against the longdouble two-pass
	reference.  The one-pass form crosses the project's bar of 1e-6 at rho = 1e-5 (eps / rho^2); the two-pass form stays five orders under it; the rule of
	csrc/nrm_nv_scale.h (one-pass unless a difference is below 2^-20 of its minuend) keeps every rung down to 1e-6 under the bar, its worst UNMARKED gene at least
	100 x under it."""
	table, unmarked = {}, 0.0
	for rho in nv.RHOS:
		for kind in ('flat', 'explained'):
			y, lnw, wt, c = nv.ladder_rows(rho, kind)
			ref = nv.reference_two_pass(y, lnw, wt, c)[1]
			row = {}
			for form in ('one', 'two', 'rule'):
				sc, marked = nv.emu_scale(y, lnw, wt, c, form)
				with np.errstate(all='ignore'):
					err = np.nan_to_num(np.abs(np.asarray(nv.ld(sc) / ref - 1, F64)), nan=np.inf)
				row[form] = err.max()
				if form == 'rule' and (~marked).any():
					unmarked = max(unmarked, err[~marked].max())
			table[(rho, kind)] = row
			print('rho %-6g %-10s one-pass %.2e   two-pass %.2e   rule %.2e (%d of %d marked)' % (rho, kind, row['one'], row['two'], row['rule'], marked.sum(), len(marked)))
	print('worst unmarked gene under the rule: %.3g (%.0f x under the bar)' % (unmarked, nv.BAR / unmarked))
	for kind in ('flat', 'explained'):
		assert table[(1e-4, kind)]['one'] < nv.BAR < table[(1e-5, kind)]['one']  # the crossing
		assert all(table[(rho, kind)]['two'] < nv.BAR * 1e-4 for rho in nv.RHOS)
		assert all(table[(rho, kind)]['rule'] < nv.BAR for rho in nv.RHOS if rho >= 1e-6)
	assert unmarked * 100 <= nv.BAR


def test_zz_print_the_worst_ratios():
	for k in sorted(WORST):
		print('%-16s %-12s worst emulation error / bound %.3g' % (k[0], k[1], WORST[k]))
	assert all(v <= 1 for v in WORST.values())
