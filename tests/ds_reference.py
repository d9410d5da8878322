"""Reference of the sparse-design de kernels (csrc/nrm_de_sparse.hip: k_design_stats, k_ds_ct, k_de_sparse), entry by entry -- TEST INFRASTRUCTURE ONLY.

numpy in longdouble (64-bit mantissa on x86); no GPU.  One plain function per C entry, taking what the entry takes, so that no bound carries an earlier stage's
error (the fp64 values handed in -- dci, bx, common -- are exact inputs):

    design_stats   nrm_design_stats     ss = |x - b C|^2 with the residual formed FIRST (association.py:224-230), coef = b = (x C^T) dci, the flags[2] count
    ct             k_ds_ct              the non-constant covariates cell by cell in fours: a copy with zeros, nrm_de_sparse_ct_doubles long
    de_sparse      nrm_de_sparse        common (a = y C^T, |y|^2), ssy = max(|y|^2 - a . b_y, 0), coefy = b_y = a dci, dot = y . x - a . b_x, the flags[2] count

Running-error bounds (u = 2^-53; every count is taken with u + 2^-64: the reference rounds the same terms once more in longdouble).  A sum of m terms in ANY
order has m - 1 additions on its longest path, plus one rounding per product (the matrix instruction is not assumed to fuse; the CPU emulation has no fma):
    a_c = sum_k C_ck y_k, |y|^2, cval sum_k y_k     n (u) x sum |terms|                         (n cells; the constant covariate: n - 1 additions, one product)
    S_x = sum_{k in x} v_k y_k                       len(x) x sum |terms|
    b_c = sum_e a_e dci_ec                           d_b_c = sum_e d_a_e |dci_ec| + nc u sum_e |a_e dci_ec|
    yy = |y|^2 - sum_c a_c b_c                       d_yy = d_q + sum_c (d_a_c |b_c| + |a_c| d_b_c + d_a_c d_b_c) + (nc + 1) u (|y|^2 + sum_c |a_c b_c|)    (nc = 0: d_q)
    dot = S - sum_c a_c bx_c                         d_dot = d_S + sum_c d_a_c |bx_c| + (nc + 1) u (|S| + sum_c |a_c bx_c|)                                  (nc = 0: d_S)
    common handed in (d_ct = NULL): d_a = d_q = 0.   ssy = max(yy, 0) moves towards the reference (which is >= 0 up to d_yy); a negative ssy is never accepted.
    design_stats: the same with len(x) for n; its ss is judged against the residual-first value, so the bound also carries what the dci handed in lacks of
    being the inverse of C C^T, exactly (longdouble): |x - b C|^2 - (|x|^2 - a . b) = b . (G b - a), G = C C^T -> + sum_c |b_c| |(G b - a)_c|.
These bounds carry the cancellation of the differences (|y|^2 against a . b_y): a relative tolerance on the result would hide a lost digit.

flags[2]: a row is counted when !(yy >= 1e-4 |y|^2) and |y|^2 > 0.  The reference decides a row when |yy - 1e-4 |y|^2| exceeds d_yy + 1e-4 d_q + u 1e-4 |y|^2;
the count must lie between the decided flagged rows and that plus the undecided ones (at most two per case: asserted on the CPU).

Exact twins: small-integer Y, C, dci, bx and design values make every fp64 sum exact, so common, ssy, coefy, dot, ss, coef are compared bit for bit (ss with
the difference form the kernel evaluates, since an integer dci is no inverse).  Valued cases keep small-integer VALUES in their twin (the sums stay exact and the
twin launches the same instantiation as the real case).

SLACK multiplies every bound; the CPU file (tests/test_ds_reference_cpu.py) settles it from the fp64 emulation (emu_*) of each kernel in the kernel's own order.
Measured there over every case: worst ratio 0.80 (`common` at n = 1, where the count is the kernel's own) -> SLACK = 1.  A device ratio above 1 is a finding
about the kernel."""
import os
import sys

import numpy as np

from k3_reference import LD, U, Worst, ld, worst, same_bits, bits  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

SLACK = 1.0
ULD = 2.0**-64
UU = U + ULD
F32, F64 = np.float32, np.float64
CH, DS_T, DS_G = 2048, 512, 2  # nrm_design.h
PASS = DS_T * DS_G
THR = 1e-4


def round_up(v, m):
	return (v + m - 1) // m * m


# ---- the cases of the GPU file (imported by both test files) ------------------------------------------------------------------------------------------------------
def _case(name, n, ny, nx, nc=0, cidx=-1, cval=1.0, dtype=F32, valued=False, mis=None, fused=True, by_gene=0, coefy=True, flags=True, pad=0, kind=None):
	return dict(name=name, n=n, ny=ny, nx=nx, nc=nc, cidx=cidx, cval=cval, dtype=dtype, valued=valued, mis=mis, fused=fused, by_gene=by_gene, coefy=coefy, flags=flags,
				pad=pad, kind=kind)


COVS = {  # how the covariates reach each NG: (nc, cidx, cval, fused)
	0: [(0, -1, 1.0, True), (1, 0, 2.5, True)],
	1: [(1, -1, 1.0, True), (4, -1, 1.0, True), (5, 0, 1.0, True), (5, 2, -0.5, True), (5, 4, 2.5, True)],
	2: [(9, 8, 1.0, True), (9, 3, -0.5, True), (8, -1, 1.0, True)],
	-1: [(3, 1, 1.0, False), (9, -1, 1.0, False), (32, 31, 1.0, False)]}
CELLS = [1, 3, 2047, 2048, 2049, 4100, 6145]
NYS = [1, 2, 3, 4, 5, 9]
NXS = [1, 63, 65]


def cases():
	out, i = [], 0
	# every instantiation: type x aligned x binary x NG, the other sizes cycling through their lists
	for dtype in (F32, F64):
		for valued in (False, True):
			for ng in (0, 1, 2, -1):
				for al in (True, False):
					V = 16 // np.dtype(dtype).itemsize
					nc, cidx, cval, fused = COVS[ng][i % len(COVS[ng])]
					n = [c for c in CELLS if (c % V == 0) == al][i % (2 if al else 5)]
					out.append(_case('sweep%d' % i, n, NYS[i % 6], NXS[i % 3], nc, cidx, cval, dtype, valued, None, fused, by_gene=i & 1, pad=(i >> 1) & 1))
					i += 1
	# each remaining way of reaching a covariate layout
	for ng, lst in COVS.items():
		for j, (nc, cidx, cval, fused) in enumerate(lst):
			out.append(_case('cov-ng%d-%d' % (ng, j), 2049 + 2051 * (j & 1), 5, 65, nc, cidx, cval, F32 if j & 1 else F64, bool(j & 1), None, fused, by_gene=j & 1, pad=1))
	# each cause of ALIGNED = false alone (n % V == 0, the pitch a multiple of V, the pointer aligned: all but one)
	for dtype in (F32, F64):
		for mis in ('y', 'ldy'):
			out.append(_case('mis-%s' % mis, 2048, 5, 65, 5, 4, 1.0, dtype, False, mis))
	# design rows: one full pass, two passes (17 groups: one live group in the second, positions beyond nslots)
	out.append(_case('nx1024', 2048, 2, 1024, 5, 0, 1.0, F32, False))
	out.append(_case('nx1025', 6145, 9, 1025, 5, 2, 2.5, F32, True, by_gene=1, pad=1))
	out.append(_case('nx1025-f64', 2049, 3, 1025, 9, 8, 1.0, F64, False))
	out.append(_case('nx1025-common', 4100, 5, 1025, 3, 0, 1.0, F32, False, fused=False))
	# outputs absent
	out.append(_case('no-coefy', 4100, 5, 65, 5, 4, 1.0, F32, False, coefy=False))
	out.append(_case('no-flags', 2049, 4, 63, 5, 4, 1.0, F64, True, flags=False, by_gene=1))
	# conditioning (an intercept): mean / sd 1, 30, 1000, a zero row, a row inside the span, rows planted at ratio 0.5e-4 and 2e-4
	for dtype in (F32, F64):
		out.append(_case('conditioning', 4100, 9, 65, 4, 3, 1.0, dtype, False, kind='cond'))
	# the single=4 plan's design side: Y is the dense fp64 design itself
	out.append(_case('single4-design', 2049, 65, 65, 3, 2, 1.0, F64, True, kind='self', by_gene=1, pad=1))
	out.append(_case('single4-design-01', 4100, 63, 63, 3, 0, 1.0, F64, False, kind='self'))
	return out


CASES = cases()
CANCEL = [1, 30, 1000]
STATS = [(nx, nc, valued) for nx in (1, 130) for nc in (0, 1, 5, 32) for valued in (False, True)]  # nrm_design_stats
STATS_LENS = [0, 1, 63, 64, 65, 200]
STATS_N = 700
CHAIN = dict(nx=65, ny=9, n=4100, nc=5)
ROW_LENS = [0, 1, 7, 8, 9, 300]


def case_id(c):
	return '%s-n%d-ny%d-nx%d-nc%d-c%d-%s-%s%s' % (c['name'], c['n'], c['ny'], c['nx'], c['nc'], c['cidx'], np.dtype(c['dtype']).name, 'valued' if c['valued'] else 'ones',
													  '' if c['fused'] else '-common')


def de_aligned(y_ptr, ldy, itemsize, n):
	"""ds_go's `aligned` (compared with the source text token for token in the CPU file)."""
	V = 16 // itemsize
	return ((y_ptr % 16 == 0) and (ldy * itemsize) % 16 == 0 and n % V == 0)


def pitches(c):
	"""(ldy, skip of Y in elements) of a case: each cause of ALIGNED = false alone."""
	V = 16 // np.dtype(c['dtype']).itemsize
	ldy = round_up(c['n'], V) + V * c['pad']
	if c['mis'] == 'ldy':
		ldy += 1
	return ldy, (1 if c['mis'] == 'y' else 0)


def case_aligned(c):
	return c['mis'] is None and c['n'] % (16 // np.dtype(c['dtype']).itemsize) == 0


def de_instantiations(c, binary):
	"""What nrm_de_sparse launches for a case: the first pass with NG = groups of 4 non-constant covariates (d_ct given) or -1, later passes with -1."""
	t = 'float' if np.dtype(c['dtype']) == F32 else 'double'
	m = c['nc'] - (1 if 0 <= c['cidx'] < c['nc'] else 0)
	ng = (m + 3) // 4 if c['fused'] else -1
	assert ng in (-1, 0, 1, 2)
	names = set()
	for g0 in range(0, round_up(c['nx'], 64) // 64, (DS_T // 64) * DS_G):
		names.add('k_de_sparse<%s, %s, %s, %d>' % (t, 'true' if case_aligned(c) else 'false', 'true' if binary else 'false', ng if g0 == 0 else -1))
	return names


# ---- data ------------------------------------------------------------------------------------------------------------------------------------------------------------
def design(n, nx, valued, exact, seed=0):
	"""(nx, n) fp64: rows of 0, 1, 7, 8, 9 and 300 entries inside one chunk (the chunk moving with the row), entries at cell 0, n - 1, 2047 and 2048; with 10 rows and
	more: a row with entries in the first chunk only, one in the last only (their sums travel through every re-deal), two rows sharing cells."""
	rng = np.random.default_rng(1000 + seed)
	nch = (n + CH - 1) // CH
	X = np.zeros((nx, n))

	def val(k):
		if not valued:
			return np.ones(k)
		if exact:
			return rng.choice([-3.0, -2.0, -1.0, 2.0, 3.0], k)
		return rng.normal(size=k) + 0.25

	for i in range(nx):
		c = (i // 6 + i) % nch
		lo, hi = c * CH, min(n, (c + 1) * CH)
		L = min(ROW_LENS[i % 6], hi - lo)
		X[i, lo + rng.choice(hi - lo, L, replace=False)] = val(L)
	edge = [k for k in (0, 2047, 2048, n - 1) if 0 <= k < n]
	X[min(1, nx - 1), edge] = val(len(edge))
	if nx >= 10:
		X[nx - 1] = 0
		X[nx - 1, rng.choice(min(n, CH), min(5, n), replace=False)] = val(min(5, n))
		X[nx - 2] = 0
		lo = (nch - 1) * CH
		X[nx - 2, lo + rng.choice(n - lo, min(5, n - lo), replace=False)] = val(min(5, n - lo))
		X[nx - 2, n - 1] = val(1)[0]
		sh = rng.choice(n, min(12, n), replace=False)
		X[nx - 3] = 0
		X[nx - 4] = 0
		X[nx - 3, sh] = val(len(sh))
		X[nx - 4, sh[:9]] = val(len(sh[:9]))
	return X


def csr(X):
	row_ptr = np.zeros(X.shape[0] + 1, np.int64)
	row_ptr[1:] = np.cumsum((X != 0).sum(axis=1))
	r, k = np.nonzero(X)
	vals = X[r, k].astype(F64)
	return row_ptr, k.astype(np.int32), (None if (vals == 1).all() else vals)


def stats_design(nx, valued, exact, C=None, seed=0):
	"""CSR for nrm_design_stats: rows of 0, 1, 63, 64, 65, 200 entries in STATS_N cells; real data with covariates: row nx - 1 equals the indicator covariate
	C[0] (flagged) and row nx - 2 is that indicator with +-sqrt(2e-4) on its cells (ratio about 2e-4: not flagged)."""
	rng = np.random.default_rng(2000 + seed)
	n = STATS_N
	X = np.zeros((nx, n))
	for i in range(nx):
		L = STATS_LENS[i % 6] if nx > 1 else 65
		v = np.ones(L) if not valued else (rng.choice([-3.0, -2.0, -1.0, 2.0, 3.0], L) if exact else rng.normal(size=L) + 0.25)
		X[i, rng.choice(n, L, replace=False)] = v
	if C is not None and not exact and nx >= 10 and C.shape[0]:
		X[nx - 1] = C[0]
		if valued:
			on = np.nonzero(C[0])[0]
			X[nx - 2] = 0
			X[nx - 2, on] = 1 + np.sqrt(2e-4) * np.where(np.arange(len(on)) & 1, 1.0, -1.0)
	return X


def covariates(nc, n, cidx, cval, exact, seed=0, indicator=False):
	rng = np.random.default_rng(3000 + seed)
	C = rng.integers(-3, 4, (nc, n)).astype(F64) if exact else rng.normal(size=(nc, n))
	if indicator and nc:  # (nrm_design_stats: a batch indicator a design row can coincide with)
		C[0] = 0
		C[0, rng.choice(n, min(200, n), replace=False)] = 1
	if 0 <= cidx < nc:
		C[cidx] = cval
	return C


def inverse(C, exact, seed=0):
	"""dci as handed to the entries: the fp64 inverse of C C^T; exact twins: small integers, NOT symmetric (b_c = sum_e a_e dci[e][c] is told apart from its transpose)."""
	nc = C.shape[0]
	if exact:
		return np.random.default_rng(4000 + seed).integers(-2, 3, (nc, nc)).astype(F64)
	if nc == 0:
		return np.zeros((0, 0))
	d = np.linalg.pinv(C @ C.T, hermitian=True)
	return (d + d.T) / 2  # (symmetric to the bit: the single=4 case compares dot[i, j] with dot[j, i])


def expression(c, C, exact, seed=0):
	ny, n, dtype = c['ny'], c['n'], c['dtype']
	rng = np.random.default_rng(5000 + seed)
	if exact:
		return rng.integers(-3, 4, (ny, n)).astype(dtype)
	Y = rng.normal(size=(ny, n)) + 1.0
	if c['kind'] == 'cond':
		assert ny == 9 and c['cidx'] >= 0 and n >= 64
		z = rng.normal(size=(ny, n))
		for r, m in enumerate(CANCEL):
			Y[r] = m + z[r]
		Y[3] = 0
		Y[4] = rng.normal(size=c['nc']) @ C  # inside the span of the covariates (up to its rounding to the rows' type)
		Y[5] = np.sqrt(1 / 0.5e-4 - 1) + z[5]  # |y~|^2 / |y|^2 about 0.5e-4: flagged
		Y[6] = np.sqrt(1 / 2e-4 - 1) + z[6]  # about 2e-4: not flagged
	return Y.astype(dtype)


def problem(c, exact, seed=0):
	"""Everything nrm_de_sparse takes for a case, and its reference."""
	n, nx, nc = c['n'], c['nx'], c['nc']
	X = design(n, nx, c['valued'], exact, seed)
	C = covariates(nc, n, c['cidx'], c['cval'], exact, seed)
	dci = inverse(C, exact, seed)
	row_ptr, cells, vals = csr(X)
	Y = X.copy() if c['kind'] == 'self' else expression(c, C, exact, seed)
	if exact:
		bx = np.random.default_rng(6000 + seed).integers(-2, 3, (nx, nc)).astype(F64)
	else:
		bx = np.asarray(design_stats(row_ptr, cells, vals, C, dci, nc)['coef'], F64)
	common_in = None
	if not c['fused']:
		first = de_sparse(Y, None, C, dci, X, bx, c['cidx'], c['cval'])
		common_in = np.asarray(first['common'], F64)
	ref = de_sparse(Y, common_in, C, dci, X, bx, c['cidx'], c['cval'], by_gene=c['by_gene'], exact=exact)
	return dict(c, X=X, C=C, dci=dci, Y=Y, bx=bx, common_in=common_in, ref=ref, exact=exact, binary=vals is None)


# ---- the references ---------------------------------------------------------------------------------------------------------------------------------------------------
def _flag_count(yy, q, dyy, dq, exact):
	if exact:  # every sum is exact: the kernel's own test on the same fp64 values
		f = ~(np.asarray(yy, F64) >= THR * np.asarray(q, F64)) & (np.asarray(q, F64) > 0)
		return int(f.sum()), int(f.sum()), 0
	t = LD(THR) * q
	decided = (np.abs(yy - t) > SLACK * (dyy + THR * dq + UU * THR * q)) | (q == 0)
	lo = int((decided & (yy < t) & (q > 0)).sum())
	und = int((~decided).sum())
	return lo, lo + und, und


def design_stats(row_ptr, cells, vals, C, dci, nc, exact=False):
	nx = len(row_ptr) - 1
	Cl, dl = ld(C)[:nc], ld(dci)
	G = Cl @ Cl.T if nc else None
	ss, form, dss, xxs = (np.zeros(nx, LD) for _ in range(4))
	coef, dcoef = np.zeros((nx, nc), LD), np.zeros((nx, nc), LD)
	for i in range(nx):
		k = cells[row_ptr[i]:row_ptr[i + 1]]
		v = ld(np.ones(len(k)) if vals is None else vals[row_ptr[i]:row_ptr[i + 1]])
		L = len(k)
		xx = (v * v).sum()
		xxs[i] = xx
		if not nc:
			ss[i], form[i], dss[i] = xx, xx, L * UU * xx
			continue
		a, a_abs = Cl[:, k] @ v, np.abs(Cl[:, k]) @ np.abs(v)
		da = L * UU * a_abs
		b = a @ dl
		db = da @ np.abs(dl) + nc * UU * (np.abs(a) @ np.abs(dl))
		x = np.zeros(Cl.shape[1], LD)
		x[k] = v
		res = x - b @ Cl
		ss[i], form[i] = (res * res).sum(), xx - (a * b).sum()
		ab = (np.abs(a) * np.abs(b)).sum()
		dss[i] = L * UU * xx + (da * np.abs(b) + np.abs(a) * db + da * db).sum() + (nc + 1) * UU * (xx + ab) + (np.abs(b) * np.abs(G @ b - a)).sum()
		coef[i], dcoef[i] = b, db
	lo, hi, und = _flag_count(form, xxs, dss, np.diff(row_ptr) * UU * xxs, exact)
	return dict(ss=np.maximum(ss, 0), ss_form=np.maximum(form, 0), ss_bound=dss, coef=coef, coef_bound=dcoef, flag_lo=lo, flag_hi=hi, undecided=und)


def judge_design_stats(got, ref, exact):
	"""got: ss (nx), coef (nx, nc) or None, flag (int or None)."""
	ws = {}
	if exact:
		ws['ss'] = bits(got['ss'], np.asarray(ref['ss_form'], F64), 'ss (exact)')
		if got.get('coef') is not None:
			ws['coef'] = bits(got['coef'], np.asarray(ref['coef'], F64), 'coef (exact)')
	else:
		neg = bool((got['ss'] < 0).any())
		w = worst(np.abs(ld(got['ss']) - ref['ss']), SLACK * ref['ss_bound'], 'ss')
		ws['ss'] = Worst(np.inf, None, 'ss negative') if neg else w
		if got.get('coef') is not None:
			ws['coef'] = worst(np.abs(ld(got['coef']) - ref['coef']), SLACK * ref['coef_bound'], 'coef')
	if got.get('flag') is not None:
		ok = ref['flag_lo'] <= got['flag'] <= ref['flag_hi']
		ws['flags[2]'] = Worst(0.0 if ok else np.inf, None, 'count %d in [%d, %d]' % (got['flag'], ref['flag_lo'], ref['flag_hi']))
	return ws


def ct_doubles(n, nc, cidx):
	m = nc - (1 if cidx >= 0 else 0)
	return max((m + 3) // 4 * round_up(n, CH) * 4, 1)


def ct(C, nc, cidx, n):
	"""[group of 4][cell][4]: the covariates without the constant one, in their order; zeros for cells >= n and the last group's empty places.  No group: None
	(the scratch of one double stays as it was)."""
	cidx = cidx if 0 <= cidx < nc else -1
	m = nc - (1 if cidx >= 0 else 0)
	ng, ncells = (m + 3) // 4, round_up(n, CH)
	if ng == 0:
		return None
	out = np.zeros((ng, ncells, 4))
	for j in range(m):
		out[j // 4, :n, j % 4] = C[j + (1 if cidx >= 0 and j >= cidx else 0), :n]
	return out.ravel()


def de_sparse(Y, common_in, C, dci, X, bx, cidx, cval, by_gene=0, exact=False):
	"""dot is returned as (nx, ny), or (ny, nx) with by_gene."""
	ny, n = Y.shape
	nx, nc = X.shape[0], C.shape[0]
	cidx = cidx if 0 <= cidx < nc else -1
	Yl, Cl, dl, bl = ld(Y), ld(C), ld(dci), ld(bx)
	if common_in is None:
		a, a_abs = Yl @ Cl.T, np.abs(Yl) @ np.abs(Cl).T
		if cidx >= 0:
			a[:, cidx], a_abs[:, cidx] = LD(cval) * Yl.sum(axis=1), abs(LD(cval)) * np.abs(Yl).sum(axis=1)
		q = (Yl * Yl).sum(axis=1)
		da, dq = n * UU * a_abs, n * UU * q
		common, dcommon = np.concatenate([a.T, q[None]]), np.concatenate([da.T, dq[None]])
	else:
		a, q = ld(common_in[:nc]).T.copy(), ld(common_in[nc]).copy()
		da, dq = np.zeros_like(a), np.zeros_like(q)
		common = dcommon = None
	if nc:
		b = a @ dl
		db = da @ np.abs(dl) + nc * UU * (np.abs(a) @ np.abs(dl))
		yy = q - (a * b).sum(axis=1)
		dyy = dq + (da * np.abs(b) + np.abs(a) * db + da * db).sum(axis=1) + (nc + 1) * UU * (q + (np.abs(a) * np.abs(b)).sum(axis=1))
	else:
		b, db, yy, dyy = np.zeros((ny, 0), LD), np.zeros((ny, 0), LD), q.copy(), dq.copy()
	S, S_abs, L = np.zeros((ny, nx), LD), np.zeros((ny, nx), LD), np.zeros(nx)
	Xl = ld(X)
	for i in range(nx):
		k = np.nonzero(X[i])[0]
		L[i] = len(k)
		if len(k):
			S[:, i], S_abs[:, i] = Yl[:, k] @ Xl[i, k], np.abs(Yl[:, k]) @ np.abs(Xl[i, k])
	dot, ddot = S.copy(), L[None, :] * UU * S_abs
	if nc:
		dot = S - a @ bl.T
		ddot = ddot + da @ np.abs(bl).T + (nc + 1) * UU * (S_abs + np.abs(a) @ np.abs(bl).T)
	lo, hi, und = _flag_count(yy, q, dyy, dq, exact)
	tr = (lambda m: m) if by_gene else (lambda m: m.T)
	return dict(common=common, common_bound=dcommon, ssy=np.maximum(yy, 0), yy=yy, q=q, ssy_bound=dyy, coefy=b, coefy_bound=db, dot=tr(dot), dot_bound=tr(ddot),
				flag_lo=lo, flag_hi=hi, undecided=und)


def judge_de_sparse(got, ref, exact):
	"""got: dot in ref's layout, ssy, and common / coefy / flag where the call has them (None otherwise)."""
	ws = {}
	for k in ('common', 'ssy', 'coefy', 'dot'):
		if got.get(k) is None or (k == 'common' and ref['common'] is None):
			continue
		if got[k].size == 0:
			continue
		if exact:
			ws[k] = bits(np.asarray(got[k], F64), np.asarray(ref[k], F64), k + ' (exact)')
		else:
			ws[k] = worst(np.abs(ld(got[k]) - ref[k]), SLACK * ref[k + '_bound'], k)
	if not exact and (got['ssy'] < 0).any():
		ws['ssy'] = Worst(np.inf, None, 'ssy negative')
	if got.get('flag') is not None:
		ok = ref['flag_lo'] <= got['flag'] <= ref['flag_hi']
		ws['flags[2]'] = Worst(0.0 if ok else np.inf, None, 'count %d in [%d, %d]' % (got['flag'], ref['flag_lo'], ref['flag_hi']))
	return ws


def judge_symmetry(dot, ref):
	"""The single=4 plan's use (Y is the design): dot[i, j] against dot[j, i] inside the sum of their bounds (bit for bit where both bounds are 0)."""
	return worst(np.abs(ld(dot) - ld(dot).T), SLACK * (ref['dot_bound'] + ref['dot_bound'].T), 'dot[i, j] - dot[j, i]')


def cancel_table(got, ref):
	"""The rows with mean / sd = 1, 30, 1000 of a conditioning case (dot as (nx, ny)): (mean / sd, log10(|y|^2 / |y~|^2), relative error of ssy, its error / bound,
	the largest error of the row's products over the largest product, their worst error / bound) -- what the differences |y|^2 - a . b_y and x . y - a . b_x cost."""
	rows = []
	for r, m in enumerate(CANCEL):
		e = abs(LD(got['ssy'][r]) - ref['ssy'][r])
		ed = np.abs(ld(got['dot'][:, r]) - ref['dot'][:, r])
		rows.append((m, float(np.log10(ref['q'][r] / ref['ssy'][r])), float(e / ref['ssy'][r]), float(e / ref['ssy_bound'][r]), float(ed.max() / np.abs(ref['dot'][:, r]).max()),
					 worst(ed, ref['dot_bound'][:, r], 'dot').ratio))
	return rows


def print_cancel_table(where, got, ref):
	for row in cancel_table(got, ref):
		print('%s: mean/sd %-5g log10(q/yy) %.2f  ssy relative error %.2g (error / bound %.3g)  dot: largest error / largest product %.2g (error / bound %.3g)' % ((where, ) + row))


# ---- fp64 emulations in the kernels' own order (numpy: no fma, every product rounded) --------------------------------------------------------------------------------
def cpu_lists(X):
	"""The lists of a design as tests/tools/lists_reference.py builds them (torch on the CPU), as numpy arrays."""
	import torch
	import lists_reference as lr
	old = lr.MAX_DENSITY  # (the builder refuses dense designs; the tiny cases -- one row, one cell -- are dense)
	lr.MAX_DENSITY = 1.0
	try:
		L = lr.ReferenceLists(torch.from_numpy(np.ascontiguousarray(X)))
	finally:
		lr.MAX_DENSITY = old
	assert L.ok
	return dict(ell=L.ell.numpy(), vals=None if L.vals is None else L.vals.numpy(), base=L.base.numpy(), w=L.w.numpy(), sig=L.sig.numpy(), slot2x=L.slot2x.numpy(),
				ngroups=L.ngroups, binary=L.binary)


def _tree(v):
	"""Butterfly / shift tree over axis 0 (a power of two): pairs, then pairs of pairs."""
	while v.shape[0] > 1:
		v = v[0::2] + v[1::2]
	return v[0]


def emu_design_stats(row_ptr, cells, vals, C, dci, nc, mut=None):
	nx = len(row_ptr) - 1
	ss, coef, flag = np.zeros(nx), np.zeros((nx, nc)), 0
	for i in range(nx):
		k = cells[row_ptr[i]:row_ptr[i + 1]]
		v = np.ones(len(k)) if vals is None else np.asarray(vals[row_ptr[i]:row_ptr[i + 1]], F64)
		xx, a = np.zeros(64), np.zeros((64, nc))
		for e0 in range(0, len(k), 64):  # lane-strided
			m = min(64, len(k) - e0)
			xx[:m] = xx[:m] + v[e0:e0 + m] * v[e0:e0 + m]
			if nc:
				a[:m] = a[:m] + v[e0:e0 + m, None] * C[:nc, k[e0:e0 + m]].T
		for o in (32, 16, 8, 4, 2, 1):  # v[l] += v[l + o]
			xx, a = xx[:o] + xx[o:2 * o], a[:o] + a[o:2 * o]
		xx, a = xx[0], a[0]
		s = xx
		for c in range(nc):
			b = 0.0
			for e in range(nc):
				b = b + a[e] * dci[e, c]
			coef[i, c] = b
			s = s - a[c] * b
		ss[i] = s if (s > 0 or mut == 'ssy not clamped') else 0.0
		if not (s >= (1e-3 if mut == 'threshold 1e-3' else THR) * xx) and xx > 0:
			flag += 1
	return dict(ss=ss, coef=coef if nc else None, flag=flag)


def emu_de_sparse(Y, common_in, C, dci, Ls, bx, cidx, cval, by_gene=0, ldd=None, mut=None):
	"""k_de_sparse in its own order: per workgroup row the matrix-core sums (4 x 4 x 4 blocks per lane, folded by 4 and 8, the eight waves in order; |y|^2 and the
	plain sum per lane, a 16-lane butterfly, the waves in order), the gathers per position in list order in blocks of 8, the sums moving with the re-deal of every
	chunk, the second pass reading `common`.  Returns what the entry writes; dot through a NaN buffer of pitch ldd in the requested layout."""
	ny, n = Y.shape
	nc = C.shape[0]
	nx = bx.shape[0]
	cidx = cidx if 0 <= cidx < nc else -1
	R = 4 if Y.dtype == F32 else 2
	nch = (n + CH - 1) // CH
	Yd = np.zeros((ny, nch * CH))
	Yd[:, :n] = Y
	if mut == 'cells past n not zeroed':
		Yd[:, n:] = Y[:, :1]  # (the loads past n read cell 0)
	sig, ngroups = Ls['sig'], Ls['ngroups']
	nslots = ngroups * 64
	common = None
	if common_in is None:
		m = nc - (1 if cidx >= 0 else 0)
		ng = (m + 3) // 4
		if mut == 'cidx not skipped' and ng:
			ctr = np.zeros((ng, nch * CH, 4))
			for j in range(m):
				ctr[j // 4, :n, j % 4] = C[j, :n]
		else:
			ctr = ct(C, nc, cidx, n)
			ctr = None if ctr is None else ctr.reshape(ng, nch * CH, 4)
		da = np.zeros((max(ng, 1), 8, 4, 4, ny))  # [group][wave][block b][covariate i][row]
		dq, dk = np.zeros((8, 16, ny)), np.zeros((8, 16, ny))  # [wave][lane >> 2][row]
		for c in range(nch):
			Yc = Yd[:, c * CH:(c + 1) * CH].reshape(ny, 8, 16, 4, 4)  # [row][wave][cell group][k][b]: cell b + 4 k of the group
			for h in range(16):
				yd = Yc[:, :, h].transpose(1, 2, 3, 0)  # [wave][k][b][row]
				ydl = yd.reshape(8, 16, ny)
				dq = dq + ydl * ydl
				dk = dk + ydl
				for g in range(ng):
					A = ctr[g, c * CH:(c + 1) * CH].reshape(8, 16, 4, 4, 4)[:, h]  # [wave][k][b][i]
					for k in range(4):
						da[g] = da[g] + A[:, k, :, :, None] * yd[:, k, :, None, :]
		folded = (da[:, :, 0] + da[:, :, 1]) + (da[:, :, 2] + da[:, :, 3])  # xor 4, xor 8 -> [group][wave][i][row]

		def waves(v):  # the eight waves in order
			t = np.zeros(v.shape[1:])
			for w in range(8):
				t = t + v[w]
			return t

		tot = [waves(folded[g]) for g in range(max(ng, 1))]  # [i][row]
		yraw = waves(np.stack([_tree(dq[w]) for w in range(8)]))
		ksum = waves(np.stack([_tree(dk[w]) for w in range(8)]))
		as_ = np.zeros((ny, nc))
		j = 0
		for c in range(nc):
			if c == cidx:
				as_[:, c] = ksum if mut == 'cval left out' else cval * ksum
			else:
				as_[:, c] = tot[j >> 2][j & 3]
				j += 1
		common = np.concatenate([as_.T, yraw[None]])
	else:
		as_, yraw = np.asarray(common_in[:nc], F64).T.copy(), np.asarray(common_in[nc], F64).copy()
	# the first pass's epilogue
	yy = yraw.copy()
	coefy = np.zeros((ny, nc))
	for c in range(nc):
		b = np.zeros(ny)
		for e in range(nc):
			b = b + as_[:, e] * dci[e, c]
		coefy[:, c] = b
		yy = yy - as_[:, c] * b
	ssy = yy.copy() if mut == 'ssy not clamped' else np.where(yy > 0, yy, 0.0)
	flag = int((~(yy >= (1e-3 if mut == 'threshold 1e-3' else THR) * yraw) & (yraw > 0)).sum())
	# the gathers: position p of chunk c works for slot sig[c][p]
	acc = F32 if mut == 'float accumulator' else F64
	Spos = np.zeros((nslots, ny), acc)
	for c in range(nch):
		if c > 0 and mut != 'sum not carried':
			by_slot = np.zeros_like(Spos)
			by_slot[sig[c - 1]] = Spos
			Spos = by_slot[sig[c]]
		rec = np.concatenate([Yd[:, c * CH:(c + 1) * CH], np.zeros((ny, 1))], axis=1)
		for g in range(ngroups):
			b0, wd = int(Ls['base'][c * ngroups + g]), int(Ls['w'][c * ngroups + g])
			blk = Ls['ell'][b0:b0 + wd * 64].reshape(wd // 8, 64, 8)
			val = None if Ls['vals'] is None else Ls['vals'][b0:b0 + wd * 64].reshape(wd // 8, 64, 8)
			for jb in range(wd // 8 if mut != '9th entry dropped' else min(1, wd // 8)):
				for u in range(8):
					r = rec[:, blk[jb, :, u].astype(np.int64)].T  # (64, ny)
					if val is not None:
						r = r * val[jb, :, u][:, None]
					Spos[g * 64:(g + 1) * 64] = (Spos[g * 64:(g + 1) * 64] + r).astype(acc)
	S = np.zeros((nslots, ny))
	S[sig[nch - 1]] = Spos
	x_of = Ls['slot2x']
	dot = np.full((nx, ny), np.nan)
	for s in range(nslots):
		x = x_of[s]
		if x < 0:
			continue
		d = S[s].copy()
		if not (mut == 'second pass zeros' and s >= PASS):
			for c in range(nc):
				d = d - as_[:, c] * bx[x, c]
		dot[x] = d
	if mut == 'clamp into another row':  # the padded rows of the last workgroup (clamped to row ny - 1) storing their results
		for y in range(ny, round_up(ny, R)):
			dot[:, y % ny], ssy[y % ny] = dot[:, ny - 1], ssy[ny - 1]
	# placement
	rows, cols = (ny, nx) if by_gene else (nx, ny)
	ldd = cols if ldd is None else ldd
	flat = np.full(rows * ldd + ldd, np.nan)
	xi, yi = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
	if by_gene:
		at = yi * (nx if mut == 'by_gene pitch' else ldd) + xi
	else:
		at = xi * ldd + yi
	flat[at.ravel()] = dot.ravel()
	placed = flat[:rows * ldd].reshape(rows, ldd)[:, :cols]
	return dict(common=common, ssy=ssy, coefy=coefy if nc else None, dot=placed.copy(), flag=flag)
