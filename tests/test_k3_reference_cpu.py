"""CPU: the K3 reference of tests/k3_reference.py is right, its comparators work, the conditions the GPU tests rely on hold.

An fp64 numpy emulation of the sweeps (written from the kernels' structure: prefix sums, the `top` index arithmetic, the swap below the diagonal, the
per-pair guard with a float square root) must be accepted by every comparator at every shape and scalar set tests/test_gpu_k3_stages.py uses, and fourteen
mutations of it -- the mistakes a rewrite of K3 could make -- must each be rejected by at least one.  The emulation's P-value is scipy's beta.cdf (what the
reference package calls, association.py:249); the comparator that needs the device's own function (bit equality with nrm_pvalues_from_r2) gets it handed in."""
import numpy as np
import pytest
from scipy import special

import k3_reference as k3
from k3_reference import model

F64, F32 = np.float64, np.float32


def p_host(r2, dof):
	x = 1.0 - np.asarray(r2, dtype=np.float64)
	with np.errstate(invalid='ignore'):
		p = special.betainc(dof / 2.0, 0.5, np.clip(x, 0.0, 1.0))
	return np.where(np.isnan(x), np.nan, np.where(x <= 0, 0.0, np.where(x >= 1, 1.0, p)))


def corr64(fx, fy, top, n, mut=None):
	"""nrm_fix_corr: sum_s u_x[s] V_y[top - s] / n in fp64, V the prefix sums (no fma: within the bound; exact on exact problems)."""
	if mut == 'top+1':
		top += 1
	if mut == 'top-1':
		top -= 1
	ux = np.zeros((fx.shape[0], 7))
	uy = np.zeros((fy.shape[0], 7))
	ux[:, :5], uy[:, :5] = fx[:, :5], fy[:, :5]
	v = np.cumsum(uy, axis=1)
	if mut == 'u for V':
		v = uy
	acc = np.zeros((fx.shape[0], fy.shape[0]))
	for s in range(5):
		if 0 <= top - s:
			acc = acc + np.outer(ux[:, s], v[:, top - s])
	return acc * (1.0 / n)


def emulate(pb, entry, dtype, stat_kind=0, want_rt=False, budget=0.0, prefill=(0, 0, 0, 0), mut=None):
	"""entry 'sym' (k_assoc_sweep_sym), 'generic' (k_assoc_sweep), 'mirror' (k_assoc_sweep_mirror).  Returns (outs, flags) as the GPU tests' runners do; an
	element the kernel would not write stays NaN."""
	n, dof = float(pb.n), pb.dof
	d = np.array(pb.dot, dtype=np.float64)
	c = corr64(pb.fx, pb.fy, pb.top, pb.n, mut) if pb.ns else np.zeros_like(d)
	if pb.sym:
		up = np.triu(d + c, 1)
		low = np.triu(d, 1).T if mut == 'no correction below the diagonal' else up.T  # (below the diagonal the roles are swapped: the mirror image's value)
		d1 = up + low
	else:
		d1 = d + c
	rule = (lambda s: s) if mut == '0 -> n dropped' else (lambda s: np.where(s == 0, n, s))
	vx, vy = rule(pb.ssx), rule(pb.ssy)
	with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
		vv = np.outer(vx, vy)
		r2 = (d1 * d1) / vv
		p = p_host(r2, dof)
		stat = d1 / vx[:, None] if (stat_kind or mut == 'stat over vx') else d1 / n
		rr = d1 / np.sqrt(vv)
		rc = np.minimum(r2, 1.0)
		tt = np.sqrt(dof * rc / (1.0 - rc))
		if mut != 'sign of t lost':
			tt = np.copysign(tt, d1)
	outs = dict(p=p, stat=stat)
	if want_rt:
		outs.update(r=rr, t=tt)
	if pb.sym and mut != 'non-zero diagonal':
		for a in outs.values():
			a[np.arange(pb.nx), np.arange(pb.nx)] = 0.0
	with np.errstate(over='ignore'):
		outs = {k: a.astype(dtype) for k, a in outs.items()}
	if mut == 'untransposed' and entry == 'sym':
		for a in outs.values():
			for bi in range(pb.nx // 64):
				for bj in range(bi + 1, pb.nx // 64):
					a[bj * 64:bj * 64 + 64, bi * 64:bi * 64 + 64] = a[bi * 64:bi * 64 + 64, bj * 64:bj * 64 + 64]
	if mut == 'ragged column dropped' and pb.ny % 64:
		for a in outs.values():
			a[:, pb.ny // 64 * 64:] = np.nan
	m = pb.pairs()
	flags = np.array(prefill, dtype=np.int64)
	with np.errstate(invalid='ignore'):
		flags[0] += int((m & ~(np.isfinite(r2) & np.isfinite(vx)[:, None] & np.isfinite(vy)[None, :])).any())
		flags[1] += int((m & (r2 > 1.0 + 1e-8)).any())
	if pb.ns and budget > 0:
		if entry == 'sym' and mut != 'lower triangle counted':
			m = m & np.triu(np.ones_like(m), 1)
		K = model.k_const(pb.ns)
		dr = K * np.outer(pb.fx[:, 5], pb.fy[:, 5]) + (pb.fx[:, 6][:, None] + pb.fy[:, 6][None, :])
		with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
			ar = (np.sqrt(r2.astype(F32)) * F32(1.0000002)).astype(F64)
			om = np.maximum(1.0 - r2, 1e-150)
			num, den = dr * (dof * ar + np.sqrt(dof)), om * om
			err = (num.astype(F32) / den.astype(F32)).astype(F64)
		over = m & (num > budget * den)
		nz = (p != 0) if entry == 'generic' else (outs['p'] != 0)
		lo = np.maximum(ar - dr, 0.0)
		unexempt = over & ~nz & (p_host(lo * lo, dof) != 0)
		hits = int((over & nz).sum()) + (0 if mut == 'exemption without its test' else int(unexempt.sum()))
		if entry == 'mirror' and mut == 'lower triangle counted':
			hits *= 2
		counted = m & (~over | nz)
		if mut == 'worst from certified threads only':
			bad_col = np.zeros_like(m)
			for t0 in range(0, pb.nx, 64):
				bad_col[t0:t0 + 64] = over[t0:t0 + 64].any(axis=0)[None, :]
			counted &= ~bad_col
		w = F32(err[counted].max()) if counted.any() else F32(0)
		if flags[2] < (1 << 30) or mut == 'counter not saturating':
			flags[2] += hits
		flags[3] = max(int(flags[3]), int(w.view(np.int32)))
	return outs, flags.astype(np.int32)


def verdicts(pb, entry, dtype, stat_kind=0, want_rt=False, mut=None):
	ref = k3.reference(pb)
	outs, fl = emulate(pb, entry, dtype, stat_kind, want_rt, mut=mut)
	pe = None
	if pb.exact:
		pe = p_host(ref['r2_64'], pb.dof)
		if pb.sym:
			pe[np.arange(pb.nx), np.arange(pb.nx)] = 0.0
	# (the mpmath subset holds the DEVICE function to G12's tolerance, which scipy's beta.cdf does not meet everywhere: that comparator has a test of its own below)
	ws = k3.judge(outs, pb, ref, dtype, stat_kind, pe, mp_subset=False)
	if stat_kind == 1 and pb.sym:
		ws.pop('stat symmetry')
	return ws, fl


def rejected(ws):
	return sorted(k for k, w in ws.items() if not w.ratio <= 1)


# ---- the comparators accept the emulation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('scal', k3.SCALARS, ids=lambda s: 'n%d-dof%d' % s)
def test_comparators_accept_the_emulation_at_every_gpu_shape(scal, exact):
	n, dof = scal
	worst = 0.0
	for ns in k3.NSS:
		for ng in k3.SYM_NG:
			pb = k3.problem(exact, True, ng, ng, n, dof, ns)
			for entry, kind, rt in (('sym', 0, False), ('generic', 0, True), ('generic', 1, False)):
				for dtype in (F64, F32):
					ws, fl = verdicts(pb, entry, dtype, kind, rt)
					assert not rejected(ws) and (fl == 0).all(), (ng, ns, entry, dtype, rejected(ws), fl)
					worst = max(worst, max(w.ratio for w in ws.values()))
		for sym, shapes in ((False, k3.RECT), (False, [s[:2] for s in k3.MIRROR])):
			for nx, ny in shapes:
				pb = k3.problem(exact, sym, nx, ny, n, dof, ns)
				for dtype in (F64, F32):
					ws, fl = verdicts(pb, 'generic', dtype, 1, True)
					assert not rejected(ws) and (fl == 0).all(), (nx, ny, ns, dtype, rejected(ws), fl)
					worst = max(worst, max(w.ratio for w in ws.values()))
	print('worst error / bound of the emulation: %.3g' % worst)


def test_mpmath_subset_comparator():
	"""The subset comparator itself: mpmath's own values rounded to double pass, the same values 1e-12 off do not."""
	pb = k3.problem(True, True, 200, 200, 4096, 4093, 6)
	ref = k3.reference(pb)
	p = np.zeros((200, 200))
	sub = k3.subset(pb, ref['r2_64'])
	assert len(sub) <= 200 and set(pb.plants.values()) <= set(sub)
	for i, j in sub:
		p[i, j] = float(k3.p_mp(float(ref['r2_64'][i, j]), pb.dof))
	assert k3.compare_p_subset(p, pb, ref['r2_64'], F64).ratio <= 1
	assert k3.compare_p_subset(p * (1 + 1e-12), pb, ref['r2_64'], F64).ratio > 1
	assert k3.compare_p_subset(p.astype(F32), pb, ref['r2_64'], F32).ratio <= 1


# ---- the mutations -----------------------------------------------------------------------------------------------------------------------------------------------
SWEEP_MUTATIONS = {
	'top+1': ('sym', 0, False),
	'top-1': ('sym', 0, False),
	'no correction below the diagonal': ('generic', 0, True),
	'u for V': ('sym', 0, False),
	'0 -> n dropped': ('generic', 1, True),
	'non-zero diagonal': ('sym', 0, False),
	'untransposed': ('sym', 0, False),
	'ragged column dropped': ('sym', 0, False),
	'stat over vx': ('generic', 0, True),
	'sign of t lost': ('generic', 0, True),
}


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('ns', [5, 6])
@pytest.mark.parametrize('mut', sorted(SWEEP_MUTATIONS))
def test_sweep_mutation_is_rejected(mut, ns, exact):
	entry, kind, rt = SWEEP_MUTATIONS[mut]
	pb = k3.problem(exact, True, 200, 200, 4096, 4093, ns)
	ws, _ = verdicts(pb, entry, F64, kind, rt)
	assert not rejected(ws)
	ws, _ = verdicts(pb, entry, F64, kind, rt, mut=mut)
	print(mut, '-> rejected by', rejected(ws))
	assert rejected(ws), mut


def guard_verdict(name, entry, dtype, mut=None, prefill=(0, 0, 0, 0)):
	pb, budget, kind = k3.guard_case(name)
	ref = k3.reference(pb)
	domain = {'sym': 'unordered', 'generic': 'ordered' if pb.sym else 'rect', 'mirror': 'rect'}[entry]
	g = k3.guard_reference(pb, ref, budget, domain, F64 if entry == 'generic' else dtype)
	_, fl = emulate(pb, entry, dtype, budget=budget, prefill=prefill, mut=mut)
	return g, fl, k3.check_guard(fl, prefill[2], g)


@pytest.mark.parametrize('name', k3.GUARD_CASES)
def test_guard_cases_are_decided_and_the_emulation_is_accepted(name):
	"""Zero undecided pairs, the classes as designed, and the emulation's per-pair count and maximum inside the intervals -- for every kernel the GPU test runs."""
	pb, budget, kind = k3.guard_case(name)
	entries = ('sym', 'generic') if kind == 'sym' else (('mirror', ) if kind == 'mirror' else ('generic', ))
	for entry in entries:
		for dtype in (F64, F32):
			g, fl, (a, b) = guard_verdict(name, entry, dtype, prefill=(0, 0, 7, 0))
			print(name, entry, dtype.__name__, 'over %d (non-zero P %d, zero P counted %d, exempt %d)' % (g['over'].sum(), g['n_nz'], g['n_z'], g['n_exempt']), a.what, b.what)
			assert g['undecided'] == 0
			assert a.ratio <= 1 and b.ratio <= 1, (a, b)
			assert g['under'].any()
			if name == 'exempt':
				assert g['hits'] == (0, 0) and g['n_exempt'] >= 1 and fl[2] == 7
			elif name == 'large-g':
				assert g['n_z'] >= 1 and g['hits'][0] >= 1
			else:  # all three classes, for either stored type: under (above), over with P != 0, over with P == 0 (counted after the exemption test, or exempt)
				assert g['n_nz'] > 0 and g['n_z'] + g['n_exempt'] > 0, 'all three classes'
	if kind == 'sym':  # the generic kernel's count within twice the unordered interval (what the GPU test asserts)
		g = k3.guard_reference(pb, k3.reference(pb), budget, 'unordered', F64)
		_, fl = emulate(pb, 'generic', F64, budget=budget)
		assert 2 * g['hits'][0] <= fl[2] <= 2 * g['hits'][1]


@pytest.mark.parametrize('mut,name,entry', [('lower triangle counted', 'sym6', 'sym'), ('lower triangle counted', 'mirror6', 'mirror'),
											('exemption without its test', 'large-g', 'sym'), ('exemption without its test', 'sym5', 'sym'),
											('worst from certified threads only', 'sym6', 'sym'), ('worst from certified threads only', 'large-g', 'sym')])
def test_guard_mutation_is_rejected(mut, name, entry):
	g, fl, (a, b) = guard_verdict(name, entry, F64, mut=mut)
	print(mut, name, a.what, b.what)
	assert a.ratio > 1 or b.ratio > 1


def test_guard_counter_saturates_and_the_mutation_is_seen():
	_, fl, _ = guard_verdict('sym6', 'sym', F64, prefill=(0, 0, 1 << 30, 0))
	assert fl[2] == 1 << 30
	_, fl, _ = guard_verdict('sym6', 'sym', F64, mut='counter not saturating', prefill=(0, 0, 1 << 30, 0))
	assert fl[2] != 1 << 30


def test_flags_expectation_follows_the_data():
	pb = k3.problem(False, True, 130, 130, 4096, 4093, 6, ones=False).copy()
	assert (emulate(pb, 'sym', F64)[1] == 0).all()
	q = pb.copy()
	q.dot[np.arange(130), np.arange(130)] = np.nan
	assert (emulate(q, 'sym', F64)[1] == 0).all(), 'NaN on a symmetric diagonal must not flag'
	q = pb.copy()
	q.set_r(3, 129, np.sqrt(1 + 2e-8))
	assert list(emulate(q, 'sym', F64)[1][:2] > 0) == [False, True]
	q.set_r(3, 129, np.sqrt(1 + 5e-9))
	assert (emulate(q, 'sym', F64)[1] == 0).all()
	q = pb.copy()
	q.dot[3, 129] = q.dot[129, 3] = np.nan
	assert list(emulate(q, 'sym', F64)[1][:2] > 0) == [True, False]


# ---- the reference is right --------------------------------------------------------------------------------------------------------------------------------------
def test_exact_problems_are_exact():
	"""Python integers: every partial sum of the correction is an integer multiple of 2^-52 / n below 2^53 of them, in any order; the fp64 corr is the exact one;
	the planted R^2 sit where they should."""
	from fractions import Fraction
	for ns in (5, 6):
		for n, dof in k3.SCALARS:
			pb = k3.problem(True, False, 65, 130, n, dof, ns)
			S = np.rint(np.ldexp(pb.fx[:, :5], 26 - 8 * np.arange(5))).astype(np.int64)
			T = np.rint(np.ldexp(pb.fy[:, :5], 26 - 8 * np.arange(5))).astype(np.int64)
			assert np.array_equal(np.ldexp(S.astype(F64), 8 * np.arange(5) - 26), pb.fx[:, :5]) and np.abs(S).max() <= 256 and np.abs(T).max() <= 256
			# the largest sum of absolute values of any subset of terms, in units of 2^-52
			worst = max(sum(abs(int(S[i, s])) * abs(int(T[j, t])) << (8 * (s + t)) for s in range(ns - 1) for t in range(ns - 1 - s)) for i in range(0, 65, 7) for j in range(0, 130, 11))
			assert worst < 2**53
			c64 = corr64(pb.fx, pb.fy, pb.top, n)
			for i in range(0, 65, 7):
				for j in range(0, 130, 11):
					want = Fraction(sum(int(S[i, s]) * int(T[j, t]) << (8 * (s + t)) for s in range(ns - 1) for t in range(ns - 1 - s)), 2**52 * n)
					assert Fraction(float(c64[i, j])) == want
					assert Fraction(float(k3._corr(pb.fx, pb.fy, ns, n, F64)[0][i, j])) == want
			ref = k3.reference(pb)
			for name, want in (('q_lo', 0.25 - 2.0**-54), ('q_eq', 0.25), ('q_hi', 0.25 + 2.0**-52), ('zero', 0.0), ('under', 0.0), ('one', 1.0)):
				assert ref['r2_64'][pb.plants[name]] == want, (name, ns, n)
			lo, hi = ref['r2_64'][pb.plants['u_lo']], ref['r2_64'][pb.plants['u_hi']]
			assert -np.log1p(-lo) < k3.UMAX < -np.log1p(-hi) and hi - lo < 1e-11
			assert 1 + 4e-9 < ref['r2_64'][pb.plants['one_plus']] < 1 + 6e-9
			assert np.array_equal(np.asarray(ref['out']['r2'], dtype=F64) == 0, ref['r2_64'] == 0)


def test_plants_cover_the_edges_and_every_subset_holds_them():
	for sym, shapes in ((True, [(g, g) for g in k3.SYM_NG if g > 1]), (False, k3.RECT[1:] + [s[:2] for s in k3.MIRROR])):
		for nx, ny in shapes:
			pb = k3.problem(False, sym, nx, ny, 4096, 4093, 6)
			ref = k3.reference(pb)
			pos = set(pb.plants.values())
			assert {'zero', 'under', 'q_lo', 'q_eq', 'q_hi', 'u_lo', 'u_hi', 'one', 'one_plus'} <= set(pb.plants)
			assert any(j == ny - 1 for _, j in pos) and (sym or any(i == nx - 1 for i, _ in pos)), 'last row and column'
			if ny >= 66:
				cols = {j for _, j in pos} | ({i for i, _ in pos} if sym else set())
				assert 63 in cols and 64 in cols, 'both sides of a tile boundary'
			assert (pb.ssx == 0).sum() >= (1 if nx >= 5 else 0) and (pb.ssy == 0).sum() == 1
			assert pos <= set(k3.subset(pb, np.asarray(ref['out']['r2'], dtype=F64))) and len(k3.subset(pb, np.asarray(ref['out']['r2'], dtype=F64))) <= 200


def test_reference_correction_and_bound_against_the_error_model():
	"""On quantised real rows the reference's correction is tools/i8_error_model.mean_correction and its dr is analyse_pair's bound."""
	rng = np.random.default_rng(3)
	n = 512
	for ns in (5, 6):
		x = np.where(rng.random((6, n)) < 0.05, rng.normal(size=(6, n)) + 3, 0.0)
		x -= x.mean(axis=1, keepdims=True)
		recs, stats = [], []
		for row in x:
			q, sh = model.quantise(row, ns)
			st = model.row_stats(model.digits(q, ns), q, sh, n, ns)
			stats.append(st)
			recs.append(list(st['u']) + [0.0] * (5 - len(st['u'])) + [st['c'], st['g'], 1.0])
		f = np.array(recs)
		ss = (x * x).sum(axis=1)
		pb = k3.Problem(sym=True, nx=6, ny=6, n=n, dof=float(n - 2), ns=ns, exact=False, dot=x @ x.T, ssx=ss, ssy=ss, fx=f, fy=f, plants={})
		corr = k3._corr(f, f, ns, n)[0]
		g = k3.guard_reference(pb, k3.reference(pb), 1e300, 'unordered', F64)
		for i in range(6):
			for j in range(i + 1, 6):
				want = model.mean_correction(stats[i], stats[j], n, ns)
				assert abs(float(corr[i, j]) - want) <= 1e-14 * max(abs(want), 1e-300) + 1e-30
				assert abs(float(g['dr'][i, j]) / model.analyse_pair(x[i], x[j], ns)['bound'] - 1) < 1e-12


def test_reference_pvalues_against_the_oracle():
	"""A small coex problem without records: the reference's R^2 through mpmath equals oracle.coex's P-values."""
	import oracle
	rng = np.random.default_rng(7)
	ng, n = 12, 64
	dt = rng.normal(size=(ng, n)) + rng.normal(size=(ng, 1)) * rng.normal(size=(1, n))
	dc = np.ones((1, n))
	po, do, vo = oracle.coex(dt, dc)
	x = dt - dt.mean(axis=1, keepdims=True)
	ss = (x * x).sum(axis=1)
	pb = k3.Problem(sym=True, nx=ng, ny=ng, n=n, dof=float(n - 2), ns=0, exact=False, dot=x @ x.T, ssx=ss, ssy=ss, fx=None, fy=None, plants={})
	ref = k3.reference(pb)
	for i in range(ng):
		for j in range(ng):
			want = 0.0 if i == j else float(k3.p_mp(float(ref['out']['r2'][i, j]), pb.dof))
			assert abs(po[i, j] - want) <= 1e-9 * want + 1e-300, (i, j, po[i, j], want)
	assert np.allclose(np.asarray(ref['out']['stat0'], dtype=F64), do, rtol=1e-10, atol=1e-14)


# ---- the streaming de sweep ----------------------------------------------------------------------------------------------------------------------------------------
def emulate_de(dp, const_last, kind, mut=None):
	raw = k3.de_raw(dp['G'], dp['nc'], const_last)
	nc, nx, n, dof = dp['nc'], dp['nx'], float(dp['n']), dp['dof']
	g = raw.copy()
	if const_last and mut != 'const_last move omitted':
		g[:, nc - 1] = raw[:, 31]
		g[:, nc:] = raw[:, nc - 1:31]
	a = g[:, :nc]
	by = a @ dp['dci'].T if (nc and dp['rank'] > 0) else np.zeros((dp['ny'], nc))
	sy = np.maximum(dp['ssraw'] - (a * by).sum(axis=1), 0.0)
	vy = np.where(sy == 0, n, sy)
	vx = np.where(dp['ssx'] == 0, n, dp['ssx'])
	d = g[:, nc:nc + nx].T
	with np.errstate(divide='ignore', invalid='ignore'):
		r2 = d * d / np.outer(vx, vy)
		rc = np.minimum(r2, 1.0)
		return dict(p=p_host(r2, dof), stat=d / vx[:, None] if kind else d / n, r=d / np.sqrt(np.outer(vx, vy)), t=np.copysign(np.sqrt(dof * rc / (1 - rc)), d)), sy, by


@pytest.mark.parametrize('nc,nx', k3.DE)
def test_de_reference_accepts_the_emulation_and_rejects_the_omitted_move(nc, nx):
	for n, dof in ((4096, 4093), (32, 16)):
		for rank in ((0, ) if nc == 0 else (0, nc)):
			dp = k3.de_problem(nc, nx, n, dof, rank)
			ref = k3.de_reference(dp)
			if rank and nc:
				assert (ref['margin'] > 1000 * ref['e_sy']).all() and (ref['ssy'][:4] == 0).all(), 'every row is far from the clamp, rows 0-3 beyond it'
			assert (ref['ssy'][:4] == 0).all()
			for const_last in ((0, ) if nc == 0 else (0, 1)):
				for kind in (0, 1):
					outs, sy, by = emulate_de(dp, const_last, kind)
					ws = {k: k3.compare(outs[k], ref, k if k != 'stat' else 'stat%d' % kind, F64) for k in ('stat', 'r', 't')}
					ws['ssy'] = k3.worst(np.abs(k3.ld(sy) - ref['ssy']), ref['ssy_bound'], 'ssy')
					ws['by'] = k3.worst(np.abs(k3.ld(by) - ref['by']), ref['by_bound'], 'by')
					assert not rejected(ws), (nc, nx, rank, const_last, kind, ws)
					if const_last:
						outs, sy, by = emulate_de(dp, const_last, kind, mut='const_last move omitted')
						ws = {k: k3.compare(outs[k], ref, k if k != 'stat' else 'stat%d' % kind, F64) for k in ('stat', 'r', 't')}
						assert rejected(ws)


def test_alpha_reference():
	rng = np.random.default_rng(1)
	stat, ssx, bx, by = rng.normal(size=(5, 9)), np.array([2.0, 0.0, 3.0, 4.0, 5.0]), rng.normal(size=(5, 3)), rng.normal(size=(9, 3))
	for kind in (0, 1):
		ref, bound = k3.alpha_reference(stat, kind, ssx, 16, bx, by)
		g = stat * (16.0 / np.where(ssx == 0, 16.0, ssx))[:, None] if kind == 0 else stat
		got = by[None] - g[:, :, None] * bx[:, None, :]
		assert k3.worst(np.abs(k3.ld(got) - ref), bound, 'alpha').ratio <= 1
		assert k3.worst(np.abs(k3.ld(got * (1 + 1e-14)) - ref), bound, 'alpha').ratio > 1


# ---- launch conditions ---------------------------------------------------------------------------------------------------------------------------------------------
def test_gpu_cases_launch_every_instantiation_and_tile_branch():
	"""From the launcher's conditions (nrm_assoc_sweep_band: the sym kernel when symmetric, stat_kind 0 and neither r nor t is asked for; else the generic one)."""
	seen = set()
	for dtype in (F64, F32):
		for kind, rt in ((0, False), (0, True), (1, False)):  # test_k3_symmetric
			seen.add(k3.instantiation('sweep', dtype, 1, kind, rt))
		for kind, rt in ((0, False), (1, True)):  # test_k3_rectangular
			seen.add(k3.instantiation('sweep', dtype, 0, kind, rt))
		seen.update(k3.instantiation(e, dtype) for e in ('mirror', 'de', 'alpha'))
	print('\n'.join(sorted(seen)))
	assert seen == {'k_assoc_sweep<double>', 'k_assoc_sweep<float>', 'k_assoc_sweep_sym<double, 32>', 'k_assoc_sweep_sym<float, 32>', 'k_assoc_sweep_mirror<double>',
					'k_assoc_sweep_mirror<float>', 'k_de_small_sweep<double>', 'k_de_small_sweep<float>', 'k_alpha<double, double>', 'k_alpha<float, float>'}
	branches = set()
	for ng in k3.SYM_NG:
		branches |= k3.tile_branches(ng, ng, 1)
	for nx, ny in k3.RECT:
		branches |= k3.tile_branches(nx, ny, 0)
	assert branches == {'rect', 'upper', 'diagonal', 'mirrored', 'ragged'}
	assert k3.tile_branches(64, 64, 1) == {'diagonal'} and 'ragged' in k3.tile_branches(65, 65, 1)
