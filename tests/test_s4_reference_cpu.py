"""The reference of the single=4 kernels and of the fp64 Gram kernel (tests/s4_reference.py) checked on the CPU, so that tests/test_gpu_s4_stages.py can be trusted:

  * the comparators accept an fp64 emulation of every kernel at every shape the GPU file uses, and reject every listed mutation of it;
  * (a) the Python port of the Gram schedule equals gram_plan / gram_pieces_of of csrc/nrm_host_logic.h field by field (a stand-alone host program under
    g++ -fsanitize=address,undefined, tests/host/gram_port_sanitize.cpp), and at 512 workgroup slots the gram cases reach every branch of the schedule;
  * (b) the sweep cases launch both k_s4_sweep instantiations;
  * (c) every guard case has pairs of all three classes, a gene that must be hit and one that must not, and no undecided pair.

The last test prints the worst ratio of emulation to unslackened bound per stage: s4_reference.SLACK is settled from it."""
import numpy as np
import pytest

import s4_reference as s4
from cabi_harness import build_and_run_host_program

WORST = {}
F64, F32 = np.float64, np.float32


def accept(stage, ws):
	for k, w in ws.items():
		WORST[(stage, k)] = max(WORST.get((stage, k), 0.0), w.ratio / s4.SLACK if np.isfinite(w.ratio) else w.ratio)
		assert w.ratio <= 1, (stage, k, w)


def reject(stage, ws, mutation):
	assert any(not w.ratio <= 1 for w in ws.values()), '%s: mutation %r passes the comparators' % (stage, mutation)


# ---- (a) the schedule --------------------------------------------------------------------------------------------------------------------------------------------
def _launches():
	out = []
	for nwg in (512, 608, 208):
		for c in s4.GRAM:
			name, m_pad, n_pad, k_pad, sym, m_rows, n_rows, row0, row1, whole = c
			out.append((m_pad, n_pad, k_pad // s4.GK, sym, m_rows, n_rows, row0, m_pad if row1 is None else row1, nwg, int(whole)))
		rng = np.random.default_rng(nwg)
		for _ in range(60):
			sym = int(rng.integers(0, 2))
			ntm = int(rng.integers(1, 40))
			ntn = ntm if sym else int(rng.integers(1, 40))
			nkt = int(rng.integers(1, 500))
			nb = (ntm + 7) // 8
			b0 = int(rng.integers(0, nb))
			b1 = int(rng.integers(b0 + 1, nb + 1))
			m_pad, n_pad = ntm * 128, ntn * 128
			m_rows = int(rng.integers(m_pad - 127, m_pad + 1))
			out.append((m_pad, n_pad, nkt, sym, m_rows, m_rows if sym else int(rng.integers(n_pad - 127, n_pad + 1)), b0 * 1024, min(b1 * 1024, m_pad), nwg, int(rng.integers(0, 2)) if not sym and b0 == 0 and b1 == nb else 0))
	return out


def test_schedule_port_equals_gram_plan_under_address_and_ub_sanitizers(tmp_path):
	"""Every field of GramSched and every workgroup's piece list (checksum), for the gram cases and 60 random launches each at 512, 608 and 208 slots."""
	launches = _launches()
	inp = tmp_path / 'launches.txt'
	inp.write_text(''.join(' '.join(str(v) for v in l) + '\n' for l in launches))
	out = build_and_run_host_program(tmp_path, ['tests/host/gram_port_sanitize.cpp'], 'gram schedule printed: %d launches' % len(launches), args=[str(inp)], may_skip=True)
	lines = out.strip().split('\n')[:-1]
	assert len(lines) == len(launches)
	for l, line in zip(launches, lines):
		s = s4.gram_schedule(*l[:9], whole=bool(l[9]))
		want = [int(v) for v in line.split()]
		got = [s[k] for k in s4.FIELDS] + [s4.pieces_hash(s)]
		assert got == want, (l, dict(zip(s4.FIELDS + ['pieces'], zip(got, want))))


def test_gram_cases_reach_every_branch_of_the_schedule_at_512_slots():
	reached = set()
	for c in s4.GRAM:
		reached |= s4.branches(s4.gram_case(c, 512))
	want = {'all-stream-k', 'stored-whole', 'straddle', 'parts2', 'parts4', 'parts8', 'whole-tiles', 'whole+remainder', 'symmetric-ragged', 'band'}
	assert want <= reached, want - reached
	# every piece list covers every k-tile of every tile of the launch exactly once, and what the fix-up reads is what the pieces wrote
	for c in s4.GRAM:
		s = s4.gram_case(c, 512)
		tm = s4.tile_map(s)
		assert sorted(tm) == list(range(s['tiles']))
		for t, pcs in tm.items():
			assert sorted((k0, k1) for k0, k1, _ in pcs)[0][0] == 0 and sum(k1 - k0 for k0, k1, _ in pcs) == s['nkt']
		for b in range(s['tiles_al'] + s['tiles_sk']):
			r = s4.fixup_reads(s, b)
			t = s['tiles_dp'] + b
			if r is None:
				assert [p[2] for p in tm[t]] == [None]
			else:
				assert r[0] == t and r[1] == [p[2] for p in tm[t]], (c[0], b, r, tm[t])


# ---- gram ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _judge_gram(c, s, exact, out, rows):
	ws = s4.judge_gram(out, s4.gram(c, s, exact, rows), exact)
	ws['placement'] = s4.judge_gram_placement(c, s, out, rows)
	return ws


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('case', s4.GRAM, ids=lambda c: c[0])
def test_gram_emulation_accepted(case, exact):
	s = s4.gram_case(case, 512)
	rows = s4.gram_rows(case)
	if len(rows) > 12:  # (the emulation is a Python loop over pieces and cells: twelve of the reference's rows, the first and the last among them)
		rows = rows[np.unique(np.linspace(0, len(rows) - 1, 12).astype(int))]
	accept('gram', _judge_gram(case, s, exact, s4.emu_gram(case, s, exact, rows), rows))


GRAM_MUTATIONS = [('drop-slab', 'one-tile-40'), ('drop-slab', 'parts8'), ('drop-second-piece', 'straddle'), ('swizzle', 'stored-whole'), ('edge', 'finite:whole-ragged16')]


@pytest.mark.parametrize('mutation,name', GRAM_MUTATIONS, ids=lambda v: v)
def test_gram_mutations_rejected(mutation, name):
	case = [c for c in s4.GRAM if c[0] == name][0]
	s = s4.gram_case(case, 512)
	rows = s4.gram_rows(case)
	rows = rows[np.unique(np.linspace(0, len(rows) - 1, 6).astype(int))] if len(rows) > 6 else rows
	if mutation == 'edge':
		rows = np.arange(140, 150)
	for exact in (True, False):
		reject('gram', _judge_gram(case, s, exact, s4.emu_gram(case, s, exact, rows, mutate=mutation), rows), mutation)


# ---- fix_dot -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ns', s4.FIX_NS)
def test_fix_dot_emulation_accepted_mutation_rejected(ns):
	for rows in s4.FIX_ROWS:
		for cols in s4.FIX_COLS:
			for exact in (True, False):
				dot, fr, fc, n = s4.fix_problem(rows, cols, ns, exact)
				ref = s4.fix_dot(dot, fr, fc, ns, n, exact)
				accept('fix_dot', s4.judge_fix_dot(s4.emu_fix_dot(dot, fr, fc, ns, n), ref, exact))
				if ns == 5:
					reject('fix_dot', s4.judge_fix_dot(s4.emu_fix_dot(dot, fr, fc, ns, n, mutate='top'), ref, exact), 'six planes\' prefix sums at five')


# ---- spd -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nx,nxp', s4.SPD)
def test_spd_emulations_accepted_mutations_rejected(nx, nxp):
	m = s4.spd_matrix(nx)
	ldm = nx + 3
	md = np.full((nx, ldm), np.nan)
	md[:, :nx] = np.triu(m)
	md[:, :nx][np.tril_indices(nx, -1)] = np.nan
	ref = s4.spd_prepare(md, nx, nxp)
	mp = s4.emu_spd_sym(md, nx, nxp)
	scal = s4.emu_spd_scale(s4.emu_spd_rows(mp, nx), np.diagonal(mp)[:nx], nx)
	full = mp.copy()
	pad = np.arange(nx, nxp)
	full[pad, pad] = scal[1]
	accept('spd_prepare', s4.judge_spd_prepare(full, np.array(scal), ref, nx, nxp))
	for mut in ('edge', 'transpose'):
		if mut == 'transpose' and nx <= 32:  # (no off-diagonal tile holds a value)
			continue
		bad = s4.emu_spd_sym(md, nx, nxp, mutate=mut)
		bad[pad, pad] = scal[1]
		if mut == 'edge' and nx == nxp:
			continue
		reject('spd_prepare', s4.judge_spd_prepare(bad, np.array(scal), ref, nx, nxp), 'k_spd_sym ' + mut)
	# NaN: off the diagonal -> scal[0]; on it -> scal[1] (and scal[0]); an fmax that swallows it is rejected
	if nx >= 2:
		for (i, j) in ((0, nx - 1), (nx // 2, nx // 2)):
			mn = md.copy()
			mn[i, j] = np.nan
			rn = s4.spd_prepare(mn, nx, nxp)
			assert np.isnan(rn['norm1']) and np.isnan(rn['mean']) == (i == j)
			mpn = s4.emu_spd_sym(mn, nx, nxp)
			rowsum = s4.emu_spd_rows(mpn, nx)
			sc = np.array(s4.emu_spd_scale(rowsum, np.diagonal(mpn)[:nx], nx))
			mpn[pad, pad] = sc[1]
			accept('spd_prepare NaN', {k: w for k, w in s4.judge_spd_prepare(mpn, sc, rn, nx, nxp).items() if k in ('norm1', 'mean')})
			sc = np.array(s4.emu_spd_scale(rowsum, np.diagonal(mpn)[:nx], nx, mutate='fmax'))
			reject('spd_prepare NaN', {k: w for k, w in s4.judge_spd_prepare(mpn, sc, rn, nx, nxp).items() if k in ('norm1', 'mean')}, 'fmax swallows NaN')
	# one Newton-Schulz step's small kernels on the matrices this start gives
	x = s4.spd_start(full, nxp, 1, scal[0])
	t = full @ x
	rr = s4.spd_transpose_residual(t, nxp)
	accept('spd_residual', dict(res=s4.worst(np.abs(s4.ld([s4.emu_spd_residual(t, nxp)]) - rr['res']), np.asarray([rr['res_bound']]), 'res')))
	xn = x @ t.T
	fin = s4.spd_finish(xn, nx, nxp, np.diagonal(m).copy())
	emu_n = s4.emu_spd_finish(xn, nx, nxp)
	small = np.vstack([np.diagonal(emu_n)[:nx], s4.emu_spd_rows(emu_n, nx, np.diagonal(m).copy()), s4.emu_spd_rows(emu_n, nx)])
	accept('spd_finish', s4.judge_spd_finish(emu_n, small, fin))
	for mut in ('untransposed', 'edge'):
		if mut == 'edge' and nx == nxp:
			continue
		if mut == 'untransposed' and nx == 1:
			continue
		reject('spd_finish', s4.judge_spd_finish(s4.emu_spd_finish(xn, nx, nxp, mutate=mut), small, fin), 'k_spd_finish ' + mut)


@pytest.mark.parametrize('count', s4.UPDATE_COUNTS)
def test_update_emulation_accepted_dropped_tail_rejected(count):
	rng = np.random.default_rng(count)
	x, xt = rng.normal(size=count), rng.normal(size=count)
	want = s4.spd_update(x, xt)
	accept('spd_update', dict(x=s4.bits(s4.emu_spd_update(x, xt), want, '2 x - xt')))
	if count % 2:
		reject('spd_update', dict(x=s4.bits(s4.emu_spd_update(x, xt, mutate='tail'), want, '2 x - xt')), 'no scalar tail')


# ---- (b) rss and the sweep -------------------------------------------------------------------------------------------------------------------------------------------
def test_sweep_cases_launch_both_instantiations_and_every_edge():
	cases = s4.sweep_cases()
	assert {(np.dtype(c[4]).name, c[5]) for c in cases} == {('float64', 0), ('float32', 1)}
	assert {c[0] for c in cases} == set(s4.SWEEP_N) and {c[1] for c in cases} == set(s4.SWEEP_N)
	assert {c[2] for c in cases} == {0, 5} and {c[3] for c in cases} == set(s4.SWEEP_DOF)
	for dt, rd in s4.SWEEP_VARIANTS:
		sp = set()
		for c in cases:
			if (c[4], c[5]) == (dt, rd):
				pb = s4.sweep_problem(*c[:4])
				sp |= set(pb.special) | set(pb.plants) | ({'dxx0'} if (pb.dxx == 0).any() else set())
		assert {'ulps', 'r2', 'nan', 'inf', 'dxx0', 'p_one', 'p_1e30', 'p_sub32', 'p_sub64', 'p_zero'} <= sp, sp


@pytest.mark.parametrize('case', s4.sweep_cases(), ids=lambda c: 'nx%d-ny%d-m+%d-dof%d-%s-dot%d' % (c[0], c[1], c[2], c[3], np.dtype(c[4]).name, c[5]))
def test_sweep_emulation_accepted_mutations_rejected(case):
	nx, ny, extra, dof, dtype, rd = case
	pb = s4.sweep_problem(nx, ny, extra, dof)
	rr = s4.rss(pb)
	rs = s4.emu_rss(pb)
	accept('rss', dict(rss=s4.judge_values(rs, rr['rss'], rr['bound'], 'rss')))
	if 'ulps' in pb.special:
		assert 0 > rs[pb.special['ulps']] > -1e-14
	reject('rss', dict(rss=s4.judge_values(s4.emu_rss(pb, mutate='edge'), rr['rss'], rr['bound'], 'rss')), 'k < m - 1')
	ref = s4.sweep(pb, rs, rd, dtype)
	assert ref['undecided'] == 0
	e = s4.emu_sweep(pb, rs, rd, dtype)
	ws = {k: s4.judge_values(e[k], ref['out'][k], ref['bound'][k], k) for k in ('stat', 'vary')}
	ws['flags'] = s4.Worst(0.0 if e['flags'] == ref['flags'] else np.inf, None, 'flags %r == %r' % (e['flags'], ref['flags']))
	accept('sweep', ws)
	if pb.special:
		assert ref['flags'][0] > 0 and ref['flags'][1] > 0
	for mut in ('vx0', 'return_dot', 'edge', 'transposed'):
		if (mut == 'vx0' and not (pb.dxx == 0).any()) or (mut == 'edge' and not extra) or (mut == 'transposed' and (nx != ny or nx == 1)):
			continue
		b = s4.emu_sweep(pb, rs, rd, dtype, mutate=mut)
		ws = {k: s4.judge_values(b[k], ref['out'][k], ref['bound'][k], k) for k in ('stat', 'vary')}
		reject('sweep', ws, mut)


# ---- (c) the guard -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('name', s4.GUARD_CASES)
def test_guard_cases_valid_emulation_accepted_mutations_rejected(name, dtype):
	pb, fy, kappa, cstar, gstar, ns, budget = s4.guard_case(name)
	rs = s4.emu_rss(pb)
	g = s4.guard(pb, rs, fy, kappa, cstar, gstar, ns, budget, dtype)
	assert g['undecided'] == 0, 'share of undecided pairs must be 0'
	nz_over = g['counted'].sum()
	assert g['under'].any() and nz_over > 0 and g['exempt'].any(), 'all three classes'
	assert len(g['must']) > 0 and len(g['must_not']) > 0
	assert g['hits'][0] == g['hits'][1]
	# stored P of the emulation: zero exactly where the reference's class says zero (no over pair is in between)
	r2 = np.asarray(s4.sweep(pb, rs, 0, F64)['out']['r2'], dtype=F64)
	p = np.ones(r2.shape, dtype=dtype)
	for i, j in np.argwhere(g['over']):
		p[i, j] = 1.0 if s4.k3._nonzero_class(float(r2[i, j]), pb.dof, dtype) > 0 else 0.0
	e = s4.emu_guard(pb, rs, fy, kappa, cstar, gstar, ns, budget, dtype, p)
	accept('guard', s4.check_guard([0, 0, e['flags2'], e['flags3']], 0, e['hits'], g))
	for mut in ('factor', 'exemption', 'axis', 'worst-all'):
		b = s4.emu_guard(pb, rs, fy, kappa, cstar, gstar, ns, budget, dtype, p, mutate=mut)
		reject('guard', s4.check_guard([0, 0, b['flags2'], b['flags3']], 0, b['hits'], g), mut)


# ---- design scalars ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nx', s4.SCALARS_NX)
def test_design_scalar_cases_hold_every_kind_of_row(nx):
	small = s4.scalars_input(nx)
	ref = s4.design_scalars(small, nx, 4096)
	assert ref['count'] >= 1
	if nx > 6:
		assert ref['count'] >= 6 and (ref['dxx'] == 0).any() and (ref['varx'][ref['dxx'] == 0] == 1).all() and np.isnan(ref['dxx']).any() and np.isinf(ref['dxx']).any()


def test_zz_table_and_slack():
	"""Prints the worst emulation-to-bound ratio per stage and output; SLACK is that, rounded up to a power of two and capped at 4."""
	for k in sorted(WORST):
		print('%-20s %-14s worst error / bound %.3g' % (k + (WORST[k], )))
	fin = [v for v in WORST.values() if np.isfinite(v)]
	if fin:
		need = max(fin)
		slack = min(4.0, 2.0**max(0, int(np.ceil(np.log2(max(need, 1e-300))))))
		print('worst %.3g -> SLACK %g' % (need, slack))
		assert s4.SLACK == slack
