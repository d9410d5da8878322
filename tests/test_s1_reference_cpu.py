"""CPU: the stage reference of single=1 (tests/s1_reference.py) is anchored to the project's model (the oracle's per-grouping loop), accepts an fp64 emulation
of every kernel in the kernel's own order of operations at EVERY shape tests/test_gpu_s1_stages.py uses, rejects mutations of that emulation, and those shapes
launch every instantiation of k_s1_stream, k_s1_cells and k_s1_group_info.  The worst emulation-to-bound ratio printed here settles s1_reference.SLACK."""
import os
import re

import numpy as np
import pytest

import oracle
import s1_reference as s1

F32, F64 = np.float32, np.float64
WORST = {}


def note(stage, ws, odt=F64):
	"""(fp32 outputs are kept apart: their bound is little more than the output's own rounding, so their ratios sit just below 1 by construction.)"""
	stage += ' (fp32 out)' if odt == F32 else ''
	for k, w in ws.items():
		WORST[(stage, k)] = max(WORST.get((stage, k), 0.0), w.ratio)
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (stage, bad)


# ---- the anchor --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nc,duplicate', [(0, False), (1, False), (5, False), (12, False), (5, True)])
def test_composed_reference_agrees_with_the_oracle(nc, duplicate):
	"""select -> group_stats -> group_info -> stream -> cells in longdouble against oracle.association_tests(single=1): valued entries, six cells with two
	groupings, 0 / 1 / 5 / 12 covariates and a covariate given twice.  P, gamma, alpha, varx, vary inside the stage bounds plus the oracle's own fp64
	arithmetic, counted the same way: it sums over the ns_i cells of S_i, takes nc-long products and a few scalar operations -- (ns_i + nc + 2) u on the
	absolute terms of each quantity -- and its pseudo-inverse comes from an SVD, which the M+ bound of group_info covers (|dM+| |a| in alpha)."""
	pb = s1.cells_problem(13, nc, F64, seed=3, lens=[3, 5, 8, 17], zero_gene=False, duplicate=duplicate)
	dx = s1.dense(pb['row_ptr'], pb['cells'], pb['vals'], pb['n'])
	assert dx.max() == 1 and (dx > 0).sum(axis=0).max() == 2
	p, gamma, alpha, varx, vary = oracle.association_tests(dx, pb['Y'].astype(F64), pb['C'], single=1, return_dot=False, lowmem=False)
	ref, gi = s1.cells_reference(pb, 0), pb['gi']
	f = lambda v: np.asarray(v, F64)
	ns, vx = f(gi['ns'])[:, None], f(gi['vx'])[:, None]
	cu = (ns + nc + 2) * s1.U
	own_vy = cu * ref['yy_abs'] / ns
	own_g = cu * ref['xy_abs'] / (ns * vx) + cu * np.abs(f(ref['gam']))
	own_al = np.einsum('ice,iye->iyc', gi['inv_bound'], np.abs(f(ref['a']))) + cu[:, :, None] * ref['alpha_abs'] + own_g[:, :, None] * np.abs(f(gi['ccx']))[:, None, :]
	got = dict(stat=gamma, vary=vary, alpha=alpha if nc else None)
	ref2 = dict(ref, stat_bound=ref['stat_bound'] + own_g, vy_bound=ref['vy_bound'] + own_vy, alpha_bound=ref['alpha_bound'] + own_al)
	ws = s1.judge_pairs(got, ref2, F64)
	ws['varx'] = s1.worst(np.abs(s1.ld(varx) - gi['vx']), gi['vx_bound'] + cu[:, 0] * gi['vx_abs'], 'varx')
	if duplicate:
		assert (np.asarray(gi['rank']) == nc - 1).all()
	picks = s1.p_subset(ref, pb['dof'], pb['plants'].values(), limit=12)
	assert set(pb['plants'].values()) <= set(picks)
	with np.errstate(divide='ignore', invalid='ignore'):
		own_r2 = f(ref['r2']) * (2 * own_g / np.abs(f(ref['gam'])) + own_vy / f(ref['vy']))
	ref3 = dict(ref, r2_bound=ref['r2_bound'] + np.where(np.isfinite(own_r2), own_r2, 0.0))  # (the oracle's R^2, from its own gamma and vary)
	ws['p'] = s1.judge_p(p, ref3, pb['dof'], picks, F64)
	print({k: w.ratio for k, w in ws.items()})
	note('oracle', ws)


# ---- the emulation inside the bounds at every GPU shape -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', s1.SELECT, ids=str)
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
def test_emulation_select(case, exact):
	n, nx, nc, valued = case
	row_ptr, cells, vals = s1.design(n, nx, 0, valued, exact)
	C = s1.covariates(nc, n, 0, exact) if nc else None
	ref = s1.select(row_ptr, cells, vals, n, C)
	note('select', s1.judge_select(s1.emu_select(row_ptr, cells, vals, n, C), ref, exact))
	if n >= 255:  # the shapes do what they are for: long rows whose kept entries are in several ballots, cells with 0, 1, 2, 3 entries
		assert set(np.unique(np.minimum(ref['cnt'], 3))) == {0, 1, 2, 3} or nx <= 3
		assert nx < 6 or ((np.diff(ref['seg'])[:6] > 0).sum() >= 4)


@pytest.mark.parametrize('nc', s1.GS_NC)
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
def test_emulation_group_stats(nc, exact):
	pb = s1.gs_problem(nc, 0, exact)
	ref, bound = s1.group_stats(pb['seg'], pb['cells'], pb['xe'], pb['C'], nc)
	got = s1.emu_group_stats(pb['seg'], pb['cells'], pb['xe'], pb['C'], nc)
	note('group_stats', dict(gs=s1.bits(got, np.asarray(ref, F64), 'gs (exact)') if exact else s1.worst(np.abs(s1.ld(got) - ref), bound, 'gs')))


def _gi(nx, nc, variant, mut=None):
	pb = s1.gi_problem(nx, nc, variant)
	ref = s1.group_info(pb['gs'], pb['gpart'], pb['rowinfo'], pb['n_common'], nc, pb['dimreduce'])
	info, varx, flags = s1.emu_group_info(pb['gs'], pb['gpart'], pb['rowinfo'], pb['n_common'], nc, pb['dimreduce'], mut=mut)
	ws = s1.judge_group_info(info, varx, flags, ref, nc)
	ws['dof'] = s1.bits(info[:, 2].copy(), ref['dof'], 'dof')
	return pb, ref, ws


@pytest.mark.parametrize('nc', s1.GI_NC)
@pytest.mark.parametrize('nx', s1.GI_NX)
def test_emulation_group_info(nx, nc):
	for variant in s1.GI_VARIANTS:
		pb, ref, ws = _gi(nx, nc, variant)
		note('group_info', ws)
		if variant == 'duplicate' and nc > 1:
			assert (ref['rank'][~ref['fallback']] == nc - 1).all()
		if variant == 'plain' and nx >= 4:
			assert ref['vx'][1] == 1 and ref['flags'][2] == 1 and ref['flags'][4] == (1 if nc else 0)
		if variant == 'no shared cells':
			assert ref['flags'][3] > 0 or nc < 2
			assert ref['flags'][2] == (1 if nx >= 4 else 0)


@pytest.mark.parametrize('case', s1.stream_cases(), ids=lambda c: '%d-%d-%d-%s-%s-%d' % (c[0], c[1], c[2], c[3].__name__, c[4], c[5]))
def test_emulation_stream(case):
	n, ny, nc, dtype, mis, ldye = case
	for exact in (True, False):
		pb = s1.stream_problem(n, ny, nc, dtype, 0, exact)
		ref = s1.stream(pb['Y'], pb['C'], pb['code'], nc, pb['n_kept'], ldye)
		common, ye = s1.emu_stream(pb['Y'], pb['C'], pb['code'], nc, pb['n_kept'], ldye)
		note('stream', s1.judge_stream(common, ye, ref, ny, exact))


@pytest.mark.parametrize('case', s1.cells_cases(), ids=lambda c: 'ny%d-nc%d-%s-%s-%d-%d' % (c[0], c[1], c[2].__name__, c[3].__name__, c[4], c[5]))
def test_emulation_cells(case):
	ny, nc, ydt, odt, rd, al = case
	pb = s1.cells_problem(ny, nc, ydt)
	ref = s1.cells_reference(pb, rd)
	got, fl = s1.emu_cells(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], pb['common'], pb['info'], nc, ny, rd)
	got = {k: (None if v is None else v.astype(odt)) for k, v in got.items()}
	note('cells', s1.judge_pairs(got, ref, odt, fl), odt)
	if ny > 1:
		assert ref['flag0'] == pb['nx']  # the zero gene, and only it


def test_emulation_cells_cancellation_and_flag1():
	ny, nc = s1.CANCEL_SHAPE
	for ydt in s1.CANCEL_DTYPES:  # (the GPU file runs the case with the output type of the input)
		pb = s1.cells_problem(ny, nc, ydt, mean_over_sd=s1.CANCEL, zero_gene=False)
		ref = s1.cells_reference(pb, 0)
		got, fl = s1.emu_cells(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], pb['common'], pb['info'], nc, ny, 0)
		got = {k: (None if v is None else v.astype(ydt)) for k, v in got.items()}
		note('cells cancellation', s1.judge_pairs(got, ref, ydt, fl), ydt)
	pb = s1.cells_problem(ny, nc, F64, mean_over_sd=s1.CANCEL, zero_gene=False)
	ref = s1.cells_reference(pb, 0)
	lost = np.log10(ref['q_over_yy'])
	assert lost[:, 0].max() < 1 and 2.5 < lost[:, 1].min() and 5.5 < lost[:, 2].min(), lost[:, :3]  # mean / sd = 1, 30, 1000: |q| / |yy| = 1 + (mean / sd)^2
	# the reference's closed form is the residual-first form (association.py:357-360) to longdouble accuracy times that cancellation
	rf = s1.residual_first(pb)
	assert (np.abs(rf - ref['yy']) <= 64 * s1.ULD * np.asarray(ref['q_over_yy'], F64) * np.abs(rf) * pb['n']).all()
	# q handed in too small: R^2 > 1 + 1e-8 on exactly the pairs the reference names
	pb = s1.cells_problem(ny, nc, F64, zero_gene=False)
	ref0 = s1.cells_reference(pb, 0)
	common = pb['common'].copy()
	common[nc, :4] -= s1.q_cut(ref0, pb['nx'] - 1)[:4]
	ref = s1.cells_reference(pb, 0, common)
	got, fl = s1.emu_cells(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], common, pb['info'], nc, ny, 0)
	assert ref['flag1'] >= 4 and ref['flag0'] == 0
	note('cells R2 above one', s1.judge_pairs(got, ref, F64, fl))


@pytest.mark.parametrize('variant', s1.SWEEP_VARIANTS, ids=lambda v: '%s-%s-dot%d' % (v[0].__name__, v[1].__name__, v[2]))
@pytest.mark.parametrize('nc', s1.SWEEP_NC)
def test_emulation_sweep_is_cells_on_the_same_sums(nc, variant):
	"""The masked-Gram sweep finishes (a, xy, q) as k_s1_cells does: the emulation with empty segments and the sums handed in (a and q as `common`, xy as `xy0`) is
	inside the bounds of pairs() with no input error, grouping by grouping, in both variants the GPU file runs."""
	ydt, odt, rd = variant
	ny = s1.SWEEP_NY
	pb = s1.cells_problem(ny, nc, ydt)
	a, _, xy, _, q, _ = s1.cell_sums(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], pb['common'], nc, ny)
	a64, xy64, q64 = np.asarray(a, F64), np.asarray(xy, F64), np.asarray(q, F64)
	z = np.zeros_like(xy64)
	ref = s1.pairs(s1.ld(a64), np.zeros(a64.shape), s1.ld(xy64), z, s1.ld(q64), z, pb['info'], nc, rd)
	for i in range(pb['nx']):
		seg = np.zeros(2, np.int64)
		common = np.concatenate([a64[i].T, q64[i][None]], axis=0)
		got, fl = s1.emu_cells(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], seg, common, pb['info'][i:i + 1], nc, ny, rd, xy0=xy64[i:i + 1])
		got = {k: (None if v is None else v.astype(odt)) for k, v in got.items()}
		one = {k: (v[i:i + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (pb['nx'], ) else v) for k, v in ref.items()}
		one.update(flag0=int((~one['finite']).sum()), flag1=int((one['finite'] & (np.asarray(one['r2'], F64) > 1 + 1e-8)).sum()))
		note('sweep', s1.judge_pairs(got, one, odt, fl), odt)


def test_emulation_chain():
	"""The chain of the GPU file (s1.CHAIN), stage by stage as there: each stage's emulation on the previous stage's emulated outputs, judged by the stage's
	reference on those same inputs."""
	cp = s1.chain_problem()
	nx, ny, n, nc, C, Y = (cp[k] for k in ('nx', 'ny', 'n', 'nc', 'C', 'Y'))
	sel = s1.emu_select(cp['row_ptr'], cp['cells'], None, n, C)
	note('chain: select', s1.judge_select(sel, s1.select(cp['row_ptr'], cp['cells'], None, n, C), False))
	gs = s1.emu_group_stats(sel['seg'], sel['idx'], sel['xe'], C, nc)
	gs_ref, gs_bound = s1.group_stats(sel['seg'], sel['idx'], sel['xe'], C, nc)
	note('chain: group_stats', dict(gs=s1.worst(np.abs(s1.ld(gs) - gs_ref), gs_bound, 'gs')))
	gpart = s1.emu_common_gram(sel['cnt'], C)[0]
	info, varx, flags = s1.emu_group_info(gs, gpart, sel['rowinfo'], sel['n_common'], nc, 0)
	gi_ref = s1.group_info(gs, gpart, sel['rowinfo'], sel['n_common'], nc, 0)
	ws = s1.judge_group_info(info, varx, flags, gi_ref, nc)
	ws['dof'] = s1.bits(info[:, 2].copy(), gi_ref['dof'], 'dof')
	note('chain: group_info', ws)
	common, ye = s1.emu_stream(Y, C, sel['code'], nc, sel['n_kept'], cp['ldye'])
	note('chain: stream', s1.judge_stream(common, ye, s1.stream(Y, C, sel['code'], nc, sel['n_kept'], cp['ldye']), ny, False))
	pb = dict(nx=nx, ny=ny, nc=nc, sel=sel, ye=np.where(np.isnan(ye), 0, ye), common=common, info=info)
	ref = s1.cells_reference(pb, cp['return_dot'])
	got, fl = s1.emu_cells(pb['ye'], sel['ce'], sel['xe'], sel['seg'], common, info, nc, ny, cp['return_dot'])
	got = {k: (None if v is None else v.astype(cp['out_dtype'])) for k, v in got.items()}
	note('chain: cells', s1.judge_pairs(got, ref, cp['out_dtype'], fl), cp['out_dtype'])


def test_the_reference_spreads_ln_p():
	"""The P subset of the GPU file: at (ny 257, nc 5) the reference alone yields at least 200 distinct finite ln P values, and the subset holds every planted pair."""
	pb = s1.cells_problem(257, 5, F64)
	ref = s1.cells_reference(pb, 0)
	lp = s1.ln_p_estimates(ref, pb['dof'])
	assert np.isfinite(lp).all() and len(np.unique(lp)) >= 200
	picks = s1.p_subset(ref, pb['dof'], pb['plants'].values(), limit=220)
	assert set(pb['plants'].values()) <= set(picks) and len(picks) >= 200, len(picks)


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_mutations_are_rejected():
	"""Each mutation of the emulation is rejected by the comparator that should catch it (and the unmutated emulation passes the same case)."""
	caught = {}
	# select
	row_ptr, cells, vals = s1.design(700, 65, 0, True, True)
	C = s1.covariates(9, 700, 0, True)
	ref = s1.select(row_ptr, cells, vals, 700, C)
	assert all(w.ratio <= 1 for w in s1.judge_select(s1.emu_select(row_ptr, cells, vals, 700, C), ref, True).values())
	for mut, key in (('seg off by one', 'seg'), ('skip counted as common', 'sel_info'), ('skip counted as common', 'gram')):
		caught[mut + ' / ' + key] = s1.judge_select(s1.emu_select(row_ptr, cells, vals, 700, C, mut=mut), ref, True)[key].ratio > 1
	# stream
	for mut, (n, ny, nc), key in (('tail dropped', (2051, 13, 5), 'common'), ('tail dropped', (3, 8, 0), 'common'), ('reach-back one too high', (1024, 13, 12), 'common'),
								  ('padding rows land in another row', (1024, 13, 5), 'YE padding'), ('q not masked', (1024, 8, 3), 'common')):
		for exact in (True, False):
			pb = s1.stream_problem(n, ny, nc, F32, 0, exact)
			ref = s1.stream(pb['Y'], pb['C'], pb['code'], nc, pb['n_kept'], 16)
			ws = s1.judge_stream(*s1.emu_stream(pb['Y'], pb['C'], pb['code'], nc, pb['n_kept'], 16, mut=mut), ref, ny, exact)
			caught['%s / %s %s' % (mut, key, 'exact' if exact else 'real')] = ws[key].ratio > 1
	# 'q accumulated with the masked value on both factors' gives the same sums on finite data (the masked value is y or 0): nothing to reject, and it is not
	pb = s1.stream_problem(1024, 8, 3, F64, 0, False)
	one, two = s1.emu_stream(pb['Y'], pb['C'], pb['code'], 3, pb['n_kept'], 8), s1.emu_stream(pb['Y'], pb['C'], pb['code'], 3, pb['n_kept'], 8, mut='q masked on both factors')
	assert s1.same_bits(one[0], two[0]).all()
	# cells
	pb = s1.cells_problem(257, 5, F64)
	ref = s1.cells_reference(pb, 0)
	for mut, key in (('ccx and ccy swapped', 'alpha'), ('float accumulator', 'stat'), ('float accumulator', 'vary')):
		got, fl = s1.emu_cells(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], pb['common'], pb['info'], 5, 257, 0, mut=mut)
		caught[mut + ' / ' + key] = s1.judge_pairs(got, ref, F64, fl)[key].ratio > 1
	# group_info
	for mut, variant, key in (('rank tolerance 1e-6', 'nearly dependent', 'dof'), ('vx 0 -> 1 left out', 'plain', 'vx'), ('dof off by one', 'plain', 'dof'),
							  ('min/max not extended by 0', 'plain', 'flags')):
		caught[mut + ' / ' + key] = _gi(65, 5, variant, mut)[2][key].ratio > 1
	print(caught)
	assert all(caught.values()), [k for k, v in caught.items() if not v]


# ---- coverage of the instantiations ------------------------------------------------------------------------------------------------------------------------------
def test_gpu_cases_launch_every_instantiation():
	"""The instantiations named by the dispatch code of csrc/nrm_single1.hip (its S1_FIRST, S1_CASE and S1_GI lists, read from the source) against the ones the
	GPU cases reach by the dispatch rules restated in s1_reference."""
	src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'normalisr_amd', 'csrc', 'nrm_single1.hip')).read()
	first = {int(a): int(b) for a, b in re.findall(r'^\s*S1_FIRST\((\d+), (\d+)\)', src, re.M)}
	assert sorted(first) == list(range(9))
	assert 's1_stream_go<T, S1_NCB, 4, false>' in src and '#define S1_NCB 8' in src
	# ALIGNED: the launcher's own condition, token for token, is what s1.stream_aligned restates (the GPU file asserts it per case on the pointers it passes)
	rule = re.search(r'const bool aligned = (.*?);', src, re.S).group(1)
	assert ' '.join(rule.split()) == ('((uintptr_t)d_y % 16 == 0) && (ldy * sizeof(T)) % 16 == 0 && ((uintptr_t)d_code % 16 == 0) && '
									  '(NC == 0 || (((uintptr_t)d_c % 16 == 0) && ldc % 2 == 0))')
	for args in ((0, 4, 4, 0, 0, 2, 1), (4, 4, 4, 0, 0, 2, 1), (0, 3, 4, 0, 0, 2, 1), (0, 4, 4, 4, 0, 2, 1), (0, 4, 4, 0, 8, 2, 1), (0, 4, 4, 0, 0, 3, 1), (0, 4, 4, 0, 8, 3, 0), (0, 1, 8, 0, 0, 2, 1)):
		y, ldy, size, code, c, ldc, ncv = args
		assert s1.stream_aligned(*args) == ((y % 16 == 0) and (ldy * size) % 16 == 0 and (code % 16 == 0) and (ncv == 0 or ((c % 16 == 0) and ldc % 2 == 0)))
	want = set()
	for t in ('float', 'double'):
		for al in ('true', 'false'):
			want |= {'k_s1_stream<%s, %d, %d, %s, true>' % (t, nc, r, al) for nc, r in first.items()}
			want.add('k_s1_stream<%s, 8, 4, %s, false>' % (t, al))
	got = set()
	for n, ny, nc, dtype, mis, ldye in s1.stream_cases():
		got |= set(s1.stream_instantiations(nc, dtype, mis is None))
	assert got == want, (want - got, got - want)
	# the mechanisms the sizes are for
	cases = s1.stream_cases()
	assert any(n == 2051 and ny == 69 and nc <= 5 for n, ny, nc, *_ in cases) and any(n == 2051 and ny == 69 and nc > 5 for n, ny, nc, *_ in cases)
	assert {m for *_, m, _ in cases} == {None, 'y', 'ldy', 'ldc', 'code'}
	assert {(n, ny) for n, ny, *_ in cases} == {(n, ny) for n in s1.STREAM_N for ny in s1.STREAM_NY}
	assert any(nc % 8 and nc > 8 for _, _, nc, *_ in cases)
	ncts = sorted(int(v) for v in re.findall(r'^\s*S1_CASE\((-?\d+)\)', src, re.M))
	assert ncts == [-1] + list(range(9))
	want = {'k_s1_cells<%s, %d>' % (t, v) for t in ('float', 'double') for v in ncts}
	got = {s1.cells_instantiation(nc, ydt) for _, nc, ydt, *_ in s1.cells_cases()}
	assert got == want, (want - got, got - want)
	gi = [int(v) for v in re.findall(r'S1_GI\((\d)\)', src)]
	assert sorted(gi) == list(range(9)) and {s1.group_info_instantiation(nc) for nc in s1.GI_NC} == {'k_s1_group_info<%d>' % v for v in gi}


def test_zz_slack_rule():
	"""SLACK is the worst emulation-to-unslackened-bound ratio of this file's run, rounded up to a power of two, at most 4 (run after the tests above in the same
	process; alone it checks the cap only)."""
	emu = {k: v for k, v in WORST.items() if k[0] != 'oracle' and np.isfinite(v)}
	for k in sorted(WORST):
		print('%-20s %-12s worst error / bound %.3g' % (k + (WORST[k], )))
	assert s1.SLACK in (1.0, 2.0, 4.0)
	if emu:
		worst = max(emu.values()) * s1.SLACK
		print('worst emulation / unslackened bound: %.3g (fp64 outputs alone: %.3g)' % (worst, max(v for k, v in emu.items() if 'fp32 out' not in k[0]) * s1.SLACK))
		assert s1.SLACK == max(1.0, 2.0**np.ceil(np.log2(worst))), worst
