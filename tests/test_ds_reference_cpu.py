"""CPU: the entry-level reference of the sparse-design de kernels (tests/ds_reference.py) is anchored to the project's model (oracle.association_tests, which
residualises first), accepts an fp64 emulation of every kernel in the kernel's own order at EVERY case tests/test_gpu_ds_stages.py runs, rejects mutations of that
emulation, decides its planted threshold rows, and those cases launch all 32 instantiations of k_de_sparse.  The worst emulation-to-bound ratio printed here settles
ds_reference.SLACK."""
import functools
import os
import re

import numpy as np
import pytest

import oracle
import ds_reference as ds

F32, F64 = np.float32, np.float64
WORST = {}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'normalisr_amd', 'csrc')


def note(stage, ws):
	for k, w in ws.items():
		WORST[(stage, k)] = max(WORST.get((stage, k), 0.0), w.ratio)
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (stage, bad)


@functools.lru_cache(maxsize=None)
def problem(i, exact):
	pb = ds.problem(ds.CASES[i], exact)
	pb['lists'] = ds.cpu_lists(pb['X'])
	assert pb['lists']['binary'] == pb['binary']
	return pb


def emulate(pb, mut=None, ldd=None):
	c = pb
	return ds.emu_de_sparse(pb['Y'], pb['common_in'], pb['C'], pb['dci'], pb['lists'], pb['bx'], c['cidx'], c['cval'], c['by_gene'], ldd, mut)


def find(name, **want):
	for i, c in enumerate(ds.CASES):
		if c['name'] == name and all(c[k] == v for k, v in want.items()):
			return i
	raise KeyError(name)


# ---- the anchor ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('valued', [False, True], ids=['ones', 'valued'])
@pytest.mark.parametrize('nc', [0, 1, 5, 9])
def test_composed_reference_agrees_with_the_oracle(nc, valued):
	"""design_stats -> de_sparse in longdouble against oracle.association_tests(single=0): n varx, n vary and n dot are |x~|^2, |y~|^2 and x~ . y~ of rows
	residualised FIRST, with the oracle's own inverse.  Two allowances, both counted: (1) the references evaluate the difference form on the fp64 dci handed in,
	which differs from the residual-first value by b_y . (G b_x - a_x) -- measured here in longdouble and held to cond(G) nc u of the termwise absolute product;
	(2) the oracle's fp64 arithmetic: a residual element is x_k - sum_c b_c C_ck with b from two matrix products over n and nc terms, then a sum over n cells:
	(n + 2 nc + 2) u on sum_k (|y_k| + sum_c |b_yc C_ck|) (|x_k| + sum_c |b_xc C_ck|), plus the same cond(G) nc u for its own inverse."""
	n, nx, ny = 300, 7, 5
	c = ds._case('anchor', n, ny, nx, nc, nc - 1, 1.0, F64, valued)
	pb = ds.problem(c, False, seed=7)
	X, Y, C, ref = pb['X'], pb['Y'], pb['C'], pb['ref']
	row_ptr, cells, vals = ds.csr(X)
	st = ds.design_stats(row_ptr, cells, vals, C, pb['dci'], nc)
	p, dot, alpha, varx, vary = oracle.association_tests(X, Y, C, single=0, return_dot=True, lowmem=True)
	Xl, Yl, Cl = ds.ld(X), ds.ld(Y), ds.ld(C)
	rx, ry = Xl - st['coef'] @ Cl, Yl - ref['coefy'] @ Cl
	ax, ay = np.abs(Xl) + np.abs(st['coef']) @ np.abs(Cl), np.abs(Yl) + np.abs(ref['coefy']) @ np.abs(Cl)
	kap = float(np.linalg.cond(C @ C.T)) if nc else 0.0
	cu = (n + 2 * nc + 2) * ds.U + kap * nc * ds.U
	first = dict(dot=rx @ ry.T, ss=(rx * rx).sum(axis=1), ssy=(ry * ry).sum(axis=1))
	absd = dict(dot=ax @ ay.T, ss=(ax * ax).sum(axis=1), ssy=(ay * ay).sum(axis=1))
	live = np.asarray(st['ss'], F64) > 1e-6 * np.asarray(absd['ss'], F64)  # (the oracle turns a variance of 0 into 1: the empty row and the row of ones stay out)
	assert live.sum() >= nx - 3  # (two empty rows, and the row of ones when there is an intercept)
	got = dict(dot=n * ds.ld(dot), ss=n * ds.ld(varx), ssy=n * ds.ld(vary))
	mine = dict(dot=(ref['dot'], ref['dot_bound']), ss=(st['ss_form'], st['ss_bound']), ssy=(ref['ssy'], ref['ssy_bound']))
	ws = {}
	for k in ('dot', 'ss', 'ssy'):
		sel = live if k == 'ss' else (live[:, None] & np.ones(ny, bool)[None] if k == 'dot' else np.ones(ny, bool))
		value, bound = mine[k]
		form = np.abs(first[k] - value)
		ws[k + ' form'] = ds.worst(form[sel], (kap * nc * ds.U * absd[k] + bound)[sel], 'difference form against residual first')
		ws[k] = ds.worst(np.abs(got[k] - value)[sel], (bound + form + cu * absd[k])[sel], k)
	print({k: w.ratio for k, w in ws.items()})
	note('oracle', ws)
	assert all(w.ratio > 0 for k, w in ws.items() if 'form' not in k) or nc == 0  # (the comparison is not vacuous)


# ---- the emulation inside the bounds at every GPU case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('i', range(len(ds.CASES)), ids=lambda i: ds.case_id(ds.CASES[i]))
def test_emulation_de_sparse(i, exact):
	pb = problem(i, exact)
	got = emulate(pb)
	ws = ds.judge_de_sparse(got, pb['ref'], exact)
	if pb['kind'] == 'self' and not exact:  # (the twin's integer bx are not the design's coefficients: nothing is symmetric there)
		ws['symmetry'] = ds.judge_symmetry(got['dot'], pb['ref'])
	if pb['kind'] == 'cond' and not exact:
		ds.print_cancel_table('emulation, ' + np.dtype(pb['dtype']).name, got, pb['ref'])
	note('de_sparse', ws)
	ctr = ds.ct(pb['C'], pb['nc'], pb['cidx'], pb['n'])
	assert ctr is None or ctr.size == ds.ct_doubles(pb['n'], pb['nc'], pb['cidx'] if 0 <= pb['cidx'] < pb['nc'] else -1)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('case', ds.STATS, ids=str)
def test_emulation_design_stats(case, exact):
	nx, nc, valued = case
	C = ds.covariates(nc, ds.STATS_N, nc - 1, 1.0, exact, indicator=True)
	dci = ds.inverse(C, exact)
	row_ptr, cells, vals = ds.csr(ds.stats_design(nx, valued, exact, C))
	ref = ds.design_stats(row_ptr, cells, vals, C, dci, nc, exact)
	note('design_stats', ds.judge_design_stats(ds.emu_design_stats(row_ptr, cells, vals, C, dci, nc), ref, exact))
	if not exact and nx == 130 and nc >= 2:
		assert ref['undecided'] == 0 and ref['flag_lo'] == 1, ref  # the row equal to the indicator is flagged, the row at ratio 2e-4 (valued) is not
		if valued:
			r = float(ref['ss'][nx - 2] / ((vals[row_ptr[nx - 2]:row_ptr[nx - 1]]**2).sum()))
			assert 1.5e-4 < r < 2.5e-4, r
	assert set(np.diff(row_ptr)) >= (set(ds.STATS_LENS) if nx > 1 else {65})


# ---- the planted threshold rows ------------------------------------------------------------------------------------------------------------------------------------
def test_threshold_rows_are_decided():
	for i, c in enumerate(ds.CASES):
		ref = problem(i, False)['ref']
		assert ref['undecided'] <= 2, (ds.case_id(c), ref['undecided'])
		if c['kind'] == 'cond':
			ratio = np.asarray(ref['yy'] / np.where(ref['q'] > 0, ref['q'], 1), F64)
			assert ref['undecided'] == 0 and ref['flag_lo'] == 3, ref['flag_lo']  # mean / sd = 1000, the row inside the span, the row at 0.5e-4
			assert 0.3e-4 < ratio[5] < 0.7e-4 and 1.5e-4 < ratio[6] < 2.7e-4 and ratio[2] < 2e-6 and abs(ratio[4]) < 1e-10 and ref['q'][3] == 0 and ref['ssy'][3] == 0, ratio
			lost = -np.log10(ratio[:3])
			assert lost[0] < 1 and 2.5 < lost[1] < 3.5 and 5.5 < lost[2], lost  # |y|^2 / |y~|^2 = 1 + (mean / sd)^2


# ---- mutations -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_mutations_are_rejected():
	"""Each mutation of the emulation is rejected by the comparator that should catch it, on a case of the table (the unmutated emulation passes every case above)."""
	caught = {}
	plan = [  # (mutation, case, exact, output)
		('cells past n not zeroed', find('nx1025'), True, 'common'), ('cells past n not zeroed', find('nx1025'), False, 'ssy'),
		('clamp into another row', find('nx1025'), False, 'dot'), ('clamp into another row', find('nx1025-f64'), True, 'ssy'),
		('cval left out', find('nx1025'), False, 'common'), ('cval left out', find('cov-ng1-3'), True, 'dot'),
		('cidx not skipped', find('cov-ng1-3'), False, 'common'), ('cidx not skipped', find('cov-ng1-3'), True, 'coefy'),
		('9th entry dropped', find('nx1025'), False, 'dot'), ('9th entry dropped', find('cov-ng1-3'), True, 'dot'),
		('sum not carried', find('nx1025'), False, 'dot'), ('sum not carried', find('cov-ng1-3'), True, 'dot'),
		('by_gene pitch', find('nx1025'), False, 'dot'),
		('second pass zeros', find('nx1025'), False, 'dot'), ('second pass zeros', find('nx1025-common'), True, 'dot'),
		('float accumulator', find('nx1025'), False, 'dot'), ('float accumulator', find('conditioning', dtype=F64), False, 'dot'),
		('threshold 1e-3', find('conditioning', dtype=F32), False, 'flags[2]'), ('threshold 1e-3', find('conditioning', dtype=F64), False, 'flags[2]'),
		('ssy not clamped', find('conditioning', dtype=F32), True, 'ssy')]
	for mut, i, exact, key in plan:
		pb = problem(i, exact)
		ldd = (pb['nx'] if pb['by_gene'] else pb['ny']) + 5
		assert all(w.ratio <= 1 for w in ds.judge_de_sparse(emulate(pb, None, ldd), pb['ref'], exact).values())
		caught['%s / %s %s' % (mut, key, 'exact' if exact else 'real')] = ds.judge_de_sparse(emulate(pb, mut, ldd), pb['ref'], exact)[key].ratio > 1
	# a negative ssy is rejected on real data whatever its size
	pb = problem(find('conditioning', dtype=F64), False)
	got = emulate(pb)
	got['ssy'][4] = -1e-300
	caught['ssy negative / real'] = ds.judge_de_sparse(got, pb['ref'], False)['ssy'].ratio > 1
	# nrm_design_stats
	C = ds.covariates(5, ds.STATS_N, 4, 1.0, False, indicator=True)
	dci = ds.inverse(C, False)
	row_ptr, cells, vals = ds.csr(ds.stats_design(130, True, False, C))
	ref = ds.design_stats(row_ptr, cells, vals, C, dci, 5)
	caught['threshold 1e-3 / design flags'] = ds.judge_design_stats(ds.emu_design_stats(row_ptr, cells, vals, C, dci, 5, mut='threshold 1e-3'), ref, False)['flags[2]'].ratio > 1
	print(caught)
	assert all(caught.values()), [k for k, v in caught.items() if not v]


def test_rows_2_and_3_of_the_fp64_operand_cannot_reach_an_output():
	"""k_de_sparse<double> zeroes the matrix operand of the lanes with lane & 2 (a workgroup has two rows).  Left out, those lanes would repeat rows 0 and 1 in
	columns 2 and 3 of every 4 x 4 block -- and nothing else changes: the instruction keeps its columns apart (D[b][i][j] takes B[b][.][j] only), fold() and
	fold_rows() add over the lane bits 2..5 and never across lane & 3, and total() reads wsum[.. + 4 i + r] with r < R = 2 only.  So no comparator CAN reject that
	mutation; what is pinned instead is the property it rests on, from the kernel's text: the reads of wsum stay below R in the row index."""
	src = open(os.path.join(CSRC, 'nrm_de_sparse.hip')).read()
	assert 't += wsum[(w * (NG + 2) + which) * 16 + i * 4 + r];' in src and re.search(r'if \(tid < R\) \{\s*const int r = tid;', src)
	assert 'yd = (lane & 2) ? 0.0 : (double)lw[(h + u) * 32];' in src
	# the folds move no value between lanes that differ in lane & 3: every exchange is over a multiple of 4 lanes
	assert re.findall(r'__shfl_xor\(v, (\w+), 64\)', src) == ['4', '8', 'o'] and 'for (int o = 4; o < 64; o <<= 1)' in src


# ---- coverage of the instantiations ------------------------------------------------------------------------------------------------------------------------------
def test_gpu_cases_launch_every_instantiation():
	src = open(os.path.join(CSRC, 'nrm_de_sparse.hip')).read()
	launches = set(re.findall(r'DS_LAUNCH\((true|false), (-?\d+)\); break;', src))
	gos = set(re.findall(r'DS_GO\((float|double), (true|false)\)', src))
	assert len(launches) == 8 and len(gos) == 4
	assert 'k_de_sparse<T, AL, BINARY, NGV>' in src and 'const int ngv = g0 == 0 ? ng : -1;' in src and 'g0 += (DS_T / 64) * DS_G' in src
	assert 'ng = (int)((m + 3) / 4);' in src and 'int ng = -1, cidx = -1;' in src
	want = {'k_de_sparse<%s, %s, %s, %s>' % (t, al, b, g) for t, b in gos for al, g in launches}
	assert len(want) == 32
	# ALIGNED: the launcher's own condition, token for token, is what ds.de_aligned restates (the GPU file asserts it per case on the pointers it passes)
	rule = re.search(r'const bool aligned = (.*?);', src, re.S).group(1)
	assert ' '.join(rule.split()) == '((uintptr_t)d_y % 16 == 0) && (ldy * sizeof(T)) % 16 == 0 && n % DsVec<T>::V == 0'
	for y, ldy, size, n in ((0, 4, 4, 4), (4, 4, 4, 4), (0, 5, 4, 4), (0, 8, 4, 5), (0, 2, 8, 2), (8, 2, 8, 2), (0, 3, 8, 2), (0, 4, 8, 3), (0, 4, 4, 6), (0, 2, 8, 6)):
		assert ds.de_aligned(y, ldy, size, n) == ((y % 16 == 0) and (ldy * size) % 16 == 0 and n % (16 // size) == 0)
	got = set()
	for i, c in enumerate(ds.CASES):
		for exact in (True, False):
			pb = problem(i, exact)
			got |= ds.de_instantiations(c, pb['binary'])
		ldy, skip = ds.pitches(c)
		size = np.dtype(c['dtype']).itemsize
		assert ds.de_aligned(skip * size, ldy, size, c['n']) == ds.case_aligned(c) and ldy >= c['n']
	assert got == want, (want - got, got - want)
	# the mechanisms the sizes are for
	cs = ds.CASES
	assert {c['n'] for c in cs} == set(ds.CELLS) and {c['ny'] for c in cs} >= set(ds.NYS) and {c['nx'] for c in cs} == {1, 63, 65, 1024, 1025}
	assert {(c['dtype'], c['mis']) for c in cs if c['mis']} == {(t, m) for t in (F32, F64) for m in ('y', 'ldy')}
	assert all(c['n'] % (16 // np.dtype(c['dtype']).itemsize) == 0 for c in cs if c['mis'])  # each cause alone
	assert {(c['nc'], c['cidx']) for c in cs if c['fused']} >= {(0, -1), (1, 0), (1, -1), (4, -1), (5, 0), (5, 2), (5, 4), (9, 8)}
	assert {c['nc'] for c in cs if not c['fused']} == {3, 9, 32} and {c['cval'] for c in cs} == {1.0, 2.5, -0.5}
	assert {c['by_gene'] for c in cs} == {0, 1} and not all(c['coefy'] for c in cs) and not all(c['flags'] for c in cs)
	X = problem(find('nx1025'), False)['X']
	nnz = (X != 0).sum(axis=1)
	assert set(ds.ROW_LENS) <= set(nnz) and X[:, 0].any() and X[:, -1].any() and X[:, 2047].any() and X[:, 2048].any()
	assert not X[-1, ds.CH:].any() and X[-1].any() and not X[-2, :3 * ds.CH].any() and X[-2].any()  # the first chunk only, the last chunk only
	assert ((X[-3] != 0) & (X[-4] != 0)).sum() >= 9


def test_zz_slack_rule():
	"""SLACK is the worst emulation-to-unslackened-bound ratio of this file's run, rounded up to a power of two, at most 4 (run after the tests above in the same
	process; alone it checks the cap only)."""
	emu = {k: v for k, v in WORST.items() if k[0] != 'oracle' and np.isfinite(v)}
	for k in sorted(WORST):
		print('%-14s %-12s worst error / bound %.3g' % (k + (WORST[k], )))
	assert ds.SLACK in (1.0, 2.0, 4.0)
	if emu:
		worst = max(emu.values()) * ds.SLACK
		print('worst emulation / unslackened bound: %.3g' % worst)
		assert ds.SLACK == max(1.0, 2.0**np.ceil(np.log2(worst))), worst
