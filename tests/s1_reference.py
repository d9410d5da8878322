"""Reference of the single=1 kernels (csrc/nrm_single1.hip and the selection in csrc/nrm_design_lists.hip), stage by stage -- TEST INFRASTRUCTURE ONLY.

numpy in longdouble (64-bit mantissa on x86) and mpmath at 60 digits for P-values; no torch, no GPU.  One plain function per C entry, taking what the entry
takes and returning what it writes, in its layout:

    select       nrm_single1_select / nrm_single1_common_gram   (association.py:914-918)        integers, copies, and the shared cells' Gram matrix
    group_stats  nrm_single1_group_stats                        (:350-364, the grouping's own cells)
    group_info   nrm_single1_group_info                         (:350-374: M_i^+ and rank by the rule of :77-80, ccx, vx, ns, dof, the counters)
    stream       nrm_single1_stream                             (the sums over the shared cells; YE)
    pairs        nrm_single1_cells / nrm_single1_sweep          (a, xy, q -> yy, vy, gamma, R^2, alpha; P by mpmath on a subset)

Every stage is judged on the inputs it was GIVEN (the fp64 values in HBM are exact inputs), so no bound carries an earlier stage's error.

Running-error bounds (u = 2^-53).  Each is u x (sum of the absolute values of the terms) x (the depth of the operation chain the kernel documents), the chain
being: a thread's fma chain of L terms (L roundings; the fp64 emulation of the CPU test has no fma and rounds the product too: L + 1), the 64-lane tree (6), the
four waves in order (3), and where partial blocks are added in order, their number minus one.  16 x 2^-64 of the absolute sum is added for the reference itself.
    Gram of the shared cells   L = ceil(n / (256 gb)),  depth L + 1 + 6 + 3 + (gb - 1)          (gb = 64 blocks, added in block order)
    group_stats                L = ceil(len / 64),      depth L + 1 + 6
    stream (common)            L = ceil(ceil(n / V) / 256) V + 1 (tail), depth L + 1 + 6 + 3
    cells: a, xy0, q           L = len + 1 (the shared part first),       depth L + 1
    pairs, from d_a, d_xy0, d_q above (0 for the masked-Gram sweep, whose a, xy, q are inputs), |.| taken termwise so that the bound CARRIES THE CANCELLATION:
      ccy_c = sum_e M+_ce a_e     d_ccy_c = sum_e |M+_ce| d_a_e + (nc + 1) u sum_e |M+_ce a_e|
      ady = a . ccy               d_ady = sum_c (d_a_c |ccy_c| + |a_c| d_ccy_c) + (nc + 1) u sum_c |a_c ccy_c|         adx likewise with ccx (an exact input)
      yy = q - ady                d_yy = d_q + d_ady + u |yy|                  xy = xy0 - adx      d_xy = d_xy0 + d_adx + u |xy|
      vy = yy / ns                d_vy = d_yy / ns + u |vy|
      gamma = xy / (ns vx)        d_g = d_xy / (ns vx) + 2 u |gamma|           stat = gamma | gamma vx: + u |stat|
      R^2 = gamma^2 vx / vy       d_R2 = (2 |gamma| d_g + d_g^2) vx / (vy - d_vy) + R^2 d_vy / (vy - d_vy) + 4 u R^2
      alpha_c = ccy_c - gamma ccx_c      d_alpha = d_ccy_c + d_g |ccx_c| + u (|ccy_c| + 2 |gamma ccx_c|)
    fp32 outputs add 2^-24 |value| + 2^-150.
    group_info: M = (sum of the partial blocks in order) + own: depth gb + 1 on |terms|.  M+ is compared as the pseudo-inverse of the longdouble M: a backward
      stable eigen-solver returns the pseudo-inverse of M + E, ||E|| <= p(nc) u ||M||, so |dM+| <= p(nc) u kappa ||M+||_2 elementwise (kappa over the kept
      eigenvalues) with p(nc) = 24 nc: a count, not a second slack -- an element meets 2 (nc - 1) rotations a sweep at three roundings each, about six sweeps,
      36 nc in the worst case, of which the reconstruction and the fp64 eigen-solver behind the reference itself take their share; errors of rotations
      do not add up in the worst case, and the measured ratios are 0.03 - 0.04: this bound would let a solver that loses a digit and a half pass on M+
      alone (ccx, vx and every pair's alpha downstream have bounds of their own); ccx = M+ xc: |dM+| |xc| + (nc + 1) u |M+| |xc|; vx = (xx - xc . ccx) / ns as yy above.
    P: the tolerance test_pvalue_function_against_mpmath applies to golden G12 (k3_reference.p_tolerance) plus (dof / 2) d_R2 / (1 - R^2).

SLACK multiplies every bound.  It is settled on the CPU (tests/test_s1_reference_cpu.py: the worst ratio of the fp64 emulation to the unslackened bound over
every shape the GPU file uses, rounded up to a power of two, capped at 4).  Measured there over every shape, the chain's, both sweep variants
and both cancellation runs included: worst ratio 0.998 (fp32 outputs, whose rounding alone comes within a hair of its 2^-24 |value|; 0.443 over the fp64
outputs) -> SLACK = 1.  A device ratio above 1 is a finding
about the kernel."""
import math

import numpy as np

import k3_reference as k3
from k3_reference import LD, U, Worst, ld, worst, same_bits, bits  # noqa: F401

SLACK = 1.0
ULD = 2.0**-64
COMMON, SKIP = -2, -1  # NRM_S1_COMMON, NRM_S1_SKIP
HEAD = 26
GB = 64  # nrm_single1_select_gram_blocks()
F32, F64 = np.float32, np.float64

# ---- the shapes of the GPU file (imported by both test files) -------------------------------------------------------------------------------------------------
ROW_LENS = [0, 1, 63, 64, 65, 200]
SELECT = [  # (n, nx, nc, valued)
	(1, 1, 0, False), (1, 3, 3, True), (255, 3, 8, False), (256, 65, 9, True), (700, 65, 20, False), (700, 1030, 32, True), (700, 3, 0, True)]
GS_LENS = [0, 1, 63, 64, 65, 130]
GS_NC = list(range(9))
GI_NX = [1, 64, 65, 130]
GI_NC = list(range(9))
STREAM_N = [3, 1024, 2051]
STREAM_NY = [1, 8, 13, 69]
STREAM_NC = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 20, 32]
MISALIGN = ['y', 'ldy', 'ldc', 'code']
CELL_LENS = [0, 1, 7, 8, 9, 17]
CELLS_NY = [1, 257]
CELLS_NC = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 32]
SWEEP_NC = [0, 5, 12]
CANCEL = [1, 30, 1000]  # mean / sd of the cancellation case's genes
CHAIN = dict(nx=65, ny=69, n=2051, nc=5)


def stream_cases():
	"""(n, ny, nc, dtype, misalign or None, ldye): every nc in both dtypes aligned and with one misalignment (each kind in turn); n and ny cycle with coprime
	periods so that every (n, ny) occurs, (2051, 69) -- 9 row blocks at R = 8 on a grid of 16, 18 at R = 4 on 24 -- among them."""
	out, i = [], 0
	for nc in STREAM_NC:
		for dtype in (F32, F64):
			for mis in (None, 'x'):
				n, ny = STREAM_N[i % 3], STREAM_NY[i % 4]
				if mis:
					kinds = [m for m in MISALIGN if nc or m != 'ldc']
					mis = kinds[(i // 2) % len(kinds)]
				out.append((n, ny, nc, dtype, mis, (ny + 7) // 8 * 8 + (16 if i % 2 else 0)))
				i += 1
	out.append((2051, 69, 5, F32, None, 72))
	out.append((2051, 69, 12, F64, 'code', 88))
	return out


def cells_cases():
	"""(ny, nc, y dtype, out dtype, return_dot, alpha): per nc the four (input, output) types; ny alternates with the output type and flips with nc, return_dot
	alternates with the input type and flips with nc // 2, so that every (ny, output type) and every (return_dot, input type) occurs -- fp32 outputs get the
	planted pairs, the zero gene and a second block of genes too; the P spread's case (257, 5, ., fp64) is among them."""
	out = []
	for nc in CELLS_NC:
		for j, ydt in enumerate((F32, F64)):
			for k, odt in enumerate((F32, F64)):
				out.append((CELLS_NY[(k + nc + 1) % 2], nc, ydt, odt, (j + nc // 2) % 2, bool((j + k + nc // 4) % 2) or nc in (9, 32)))
	return out


SWEEP_VARIANTS = [(F64, F64, 0), (F32, F32, 1)]  # (y dtype, out dtype, return_dot) of the masked-Gram sweep's cases
SWEEP_NY = 13
CANCEL_DTYPES = [F64, F32]
CANCEL_SHAPE = (9, 3)  # (ny, nc)


def stream_aligned(y_ptr, ldy, itemsize, code_ptr, c_ptr, ldc, nc):
	"""s1_stream_go's choice of ALIGNED, restated (tests/test_s1_reference_cpu.py holds the restatement to the source text)."""
	return y_ptr % 16 == 0 and (ldy * itemsize) % 16 == 0 and code_ptr % 16 == 0 and (nc == 0 or (c_ptr % 16 == 0 and ldc % 2 == 0))


# ---- which instantiations a case launches: the dispatch rules of nrm_single1.hip, restated -----------------------------------------------------------------
def stream_instantiations(nc, dtype, aligned):
	"""s1_stream<T>: the first pass takes min(nc, 8) covariates with R = 8 up to five of them and R = 4 from six; then passes of 8 with R = 4, FIRST = false."""
	t = 'float' if np.dtype(dtype) == F32 else 'double'
	a = 'true' if aligned else 'false'
	first = min(nc, 8)
	out = ['k_s1_stream<%s, %d, %d, %s, true>' % (t, first, 8 if first <= 5 else 4, a)]
	if nc > 8:
		out.append('k_s1_stream<%s, 8, 4, %s, false>' % (t, a))
	return out


def stream_passes(nc):
	"""(comp0, covariates) of every pass; the last one reaches back when nc % 8 != 0."""
	out = [(0, min(nc, 8))]
	c0 = 8
	while c0 < nc:
		out.append((c0 if c0 + 8 <= nc else nc - 8, 8))
		c0 += 8
	return out


def cells_instantiation(nc, dtype):
	return 'k_s1_cells<%s, %d>' % ('float' if np.dtype(dtype) == F32 else 'double', nc if nc <= 8 else -1)


def group_info_instantiation(nc):
	return 'k_s1_group_info<%d>' % nc


# ---- problems --------------------------------------------------------------------------------------------------------------------------------------------------
def _values(rng, shape, exact, dtype=F64, lo=-3, hi=4):
	if exact:
		return rng.integers(lo, hi, size=shape).astype(dtype)
	return rng.normal(size=shape).astype(dtype)


def design(n, nx, seed=0, valued=False, exact=True, lens=None):
	"""CSR lists of a design with entries > 0: (row_ptr int64, cells int32 ascending inside a row, vals fp64 or None).  The first rows have ROW_LENS entries
	(clipped to n), the others 0, 1 or 2, so that cells with 0, 1, 2, 3 and more entries occur and kept entries are scattered through long rows."""
	rng = np.random.default_rng([seed, n, nx, 17])
	lens = list(ROW_LENS if lens is None else lens)
	rows = []
	for i in range(nx):
		m = min(lens[i] if i < len(lens) else int(rng.integers(0, 3)), n)
		rows.append(np.sort(rng.choice(n, size=m, replace=False)).astype(np.int32))
	row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
	cells = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
	vals = None
	if valued:
		vals = (rng.integers(1, 4, size=cells.size).astype(F64) if exact else rng.uniform(0.25, 1.0, size=cells.size))
	return row_ptr, cells, vals


def dense(row_ptr, cells, vals, n):
	dx = np.zeros((len(row_ptr) - 1, n))
	for i in range(len(row_ptr) - 1):
		a, b = row_ptr[i], row_ptr[i + 1]
		dx[i, cells[a:b]] = 1.0 if vals is None else vals[a:b]
	return dx


def covariates(nc, n, seed=0, exact=True, intercept=False, duplicate=False):
	rng = np.random.default_rng([seed, nc, n, 23])
	C = _values(rng, (nc, n), exact)
	if intercept and nc:
		C[0] = 1.0
	if duplicate and nc > 1:
		C[nc - 1] = C[0]
	return C


def expression(ny, n, dtype, seed=0, exact=True, lcpm=True):
	"""exact: small integers; real: log-CPM-like rows (a mean of a few units, a spread below one, many cells at the row's floor)."""
	rng = np.random.default_rng([seed, ny, n, 29])
	if exact:
		return _values(rng, (ny, n), True, dtype, -4, 5)
	if not lcpm:
		return rng.normal(size=(ny, n)).astype(dtype)
	mu, sd = rng.uniform(0.5, 6, (ny, 1)), rng.uniform(0.2, 1.0, (ny, 1))
	return np.maximum(mu + sd * rng.normal(size=(ny, n)), mu - sd).astype(dtype)


# ---- select ----------------------------------------------------------------------------------------------------------------------------------------------------
def select(row_ptr, cells, vals, n, C):
	"""Every output of nrm_single1_select.  gram: the (nc, nc) longdouble Gram matrix of the shared cells; gram_abs: its absolute terms; gram_bound."""
	nx = len(row_ptr) - 1
	nc = 0 if C is None else C.shape[0]
	cnt = np.bincount(cells, minlength=n).astype(np.int32)
	code = np.where(cnt == 0, COMMON, SKIP).astype(np.int32)
	seg = np.zeros(nx + 1, np.int64)
	idx, xe = [], []
	rowinfo = np.zeros((nx, 3))
	for i in range(nx):
		a, b = int(row_ptr[i]), int(row_ptr[i + 1])
		k = cells[a:b]
		keep = cnt[k] == 1
		v = (np.ones(b - a) if vals is None else vals[a:b])[keep]
		code[k[keep]] = len(idx) + np.arange(keep.sum())
		idx.extend(int(c) for c in k[keep])
		xe.extend(v)
		seg[i + 1] = len(idx)
		rowinfo[i] = (keep.sum(), v.min() if v.size else np.inf, v.max() if v.size else -np.inf)
	idx, xe = np.array(idx, np.int64), np.array(xe, F64)
	res = dict(cnt=cnt, code=code, seg=seg, idx=idx, xe=xe, ce=(C[:, idx].T.copy() if nc else np.zeros((len(idx), 0))), rowinfo=rowinfo, n_common=int((cnt == 0).sum()),
			   n_kept=len(idx))
	if nc:
		res.update(common_gram(cnt, C))
	return res


def common_gram(cnt, C):
	n = C.shape[1]
	Cn = ld(C[:, cnt == 0])
	gram, gabs = Cn @ Cn.T, np.abs(Cn) @ np.abs(Cn).T
	depth = math.ceil(n / (256 * GB)) + 1 + 6 + 3 + GB - 1
	return dict(gram=gram, gram_abs=gabs, gram_bound=SLACK * U * depth * gabs + 16 * ULD * gabs)


def gram_from_parts(part, nc):
	"""part (npairs, gb, 64) as the kernel leaves it -> the (nc, nc) matrix, the blocks added in block order (as k_s1_group_info and the host do)."""
	nb = (nc + 7) // 8
	m = np.zeros((nb * 8, nb * 8))
	p = 0
	for bi in range(nb):
		for bj in range(bi, nb):
			t = np.zeros(64)
			for g in range(part.shape[1]):
				t = t + part[p, g]
			m[bi * 8:bi * 8 + 8, bj * 8:bj * 8 + 8] = t.reshape(8, 8)
			m[bj * 8:bj * 8 + 8, bi * 8:bi * 8 + 8] = t.reshape(8, 8).T
			p += 1
	return m[:nc, :nc]


INT_OUTPUTS = ('cnt', 'code', 'seg', 'idx', 'xe', 'ce', 'rowinfo')


def judge_select(got, ref, exact_gram):
	"""got: dict with the names of INT_OUTPUTS (idx, xe, ce cut at n_kept), n_common, n_kept, gram (or None)."""
	ws = {}
	for k in INT_OUTPUTS:
		g, r = np.asarray(got[k]), np.asarray(ref[k])
		ws[k] = Worst(np.inf, None, k + ': shape') if g.shape != r.shape else bits(g, r.astype(g.dtype), k)
	ws['sel_info'] = Worst(0.0 if (got['n_common'], got['n_kept']) == (ref['n_common'], ref['n_kept']) else np.inf, None, 'sel_info[3], [4]')
	if got.get('gram') is not None:
		if exact_gram:
			ws['gram'] = bits(np.asarray(got['gram'], F64), np.asarray(ref['gram'], F64), 'gram (exact)')
		else:
			ws['gram'] = worst(np.abs(ld(got['gram']) - ref['gram']), ref['gram_bound'], 'gram')
	return ws


# ---- group_stats -----------------------------------------------------------------------------------------------------------------------------------------------
def group_stats(seg, cells, xe, C, nc):
	"""(nx, nc (nc + 1) / 2 + nc + 1) longdouble: C_c C_d (c <= d, row by row), C_c x, x x over the grouping's own cells; and the bound."""
	nx = len(seg) - 1
	npk = nc * (nc + 1) // 2 + nc + 1
	out, ab, depth = np.zeros((nx, npk), LD), np.zeros((nx, npk), LD), np.zeros((nx, 1))
	iu = np.triu_indices(nc)
	for i in range(nx):
		a, b = int(seg[i]), int(seg[i + 1])
		x = ld(xe[a:b])
		cv = ld(C[:, cells[a:b]]) if nc else np.zeros((0, b - a), LD)
		for dst, f in ((out, lambda v: v), (ab, np.abs)):
			dst[i, :len(iu[0])] = (f(cv) @ f(cv).T)[iu]
			dst[i, len(iu[0]):len(iu[0]) + nc] = f(cv) @ f(x)
			dst[i, -1] = f(x) @ f(x)
		depth[i] = math.ceil((b - a) / 64) + 1 + 6
	return out, SLACK * U * depth * ab + 16 * ULD * ab


# ---- group_info ------------------------------------------------------------------------------------------------------------------------------------------------
def inv_rank_ld(M, tol=1e-8):
	"""The reference's rule (association.py:77-80) on the symmetric M: eigen-decomposition in fp64, |eigenvalues| below tol x the largest dropped.  Returns
	(M+ in longdouble -- refined by two Newton steps X + X (P - M X) restricted to the kept subspace --, rank, kappa over the kept, ||M+||_2)."""
	nc = M.shape[0]
	m64 = np.asarray(0.5 * (M + M.T), F64)
	w, v = np.linalg.eigh(m64)
	smax = np.abs(w).max() if nc else 0.0
	keep = np.abs(w) >= tol * smax
	r = int(keep.sum())
	if r == 0:
		return np.zeros((nc, nc), LD), 0, 1.0, 0.0
	vk, wk = ld(v[:, keep]), ld(w[keep])
	X = (vk / wk) @ vk.T
	P = vk @ vk.T
	if r == nc:
		P = np.eye(nc, dtype=LD)
	for _ in range(2):
		X = X + X @ (P - ld(M) @ X)
		X = 0.5 * (X + X.T)
	return X, r, float(np.abs(w[keep]).max() / np.abs(w[keep]).min()), float(1.0 / np.abs(w[keep]).min())


def group_info(gs, gpart, rowinfo, n_common, nc, dimreduce, gram=None):
	"""The record fields nrm_single1_group_info derives (plan excluded: bit for bit nrm_pvalue_plan_fill_many at dof), their bounds, and the counters.
	gs (nx, np) fp64, gpart (gb, 64) fp64 or None; gram: the shared cells' (nc, nc) matrix itself instead of gpart (more than 8 covariates: no kernel, the
	record is data to the sweeps)."""
	nx = gs.shape[0]
	npair = nc * (nc + 1) // 2
	iu = np.triu_indices(nc)
	mcc = np.zeros((nc, nc), LD)
	mcc_abs = np.zeros((nc, nc), LD)
	if nc and gram is not None:
		mcc, mcc_abs = ld(gram), np.abs(ld(gram))
	elif nc:
		s, sa = ld(gpart).sum(axis=0).reshape(8, 8), np.abs(ld(gpart)).sum(axis=0).reshape(8, 8)
		mcc[iu], mcc_abs[iu] = s[iu], sa[iu]
		mcc, mcc_abs = np.triu(mcc) + np.triu(mcc, 1).T, np.triu(mcc_abs) + np.triu(mcc_abs, 1).T
	res = dict(ns=np.zeros(nx, LD), vx=np.zeros(nx, LD), vx_raw=np.zeros(nx, LD), vx_abs=np.zeros(nx), dof=np.zeros(nx), rank=np.zeros(nx, np.int64), ccx=np.zeros((nx, nc), LD), inv=np.zeros((nx, nc, nc), LD),
			   vx_bound=np.zeros(nx), ccx_bound=np.zeros((nx, nc)), inv_bound=np.zeros((nx, nc, nc)), flags=np.zeros(8, np.int64), fallback=np.zeros(nx, bool))
	for i in range(nx):
		ns = LD(n_common) + LD(rowinfo[i, 0])
		lo, hi = rowinfo[i, 1], rowinfo[i, 2]
		if n_common > 0:
			lo, hi = min(lo, 0.0), max(hi, 0.0)
		if not hi > lo:
			res['flags'][2] += 1
		xx, xx_abs = LD(gs[i, npair + nc]), abs(LD(gs[i, npair + nc]))
		rk = 0
		if nc:
			own = np.zeros((nc, nc), LD)
			own[iu] = ld(gs[i, :npair])
			own = np.triu(own) + np.triu(own, 1).T
			M = own + mcc
			if not np.isfinite(np.asarray(M, F64)).all():
				res['flags'][4] += 1
				res['fallback'][i] = True
				M = np.eye(nc, dtype=LD)
			inv, rk, kappa, n2 = inv_rank_ld(M)
			# M itself as the kernel forms it: gb additions of the partial blocks and one of the grouping's own, then the solver's backward error
			dM = float(np.max((GB + 1) * U * (mcc_abs + np.abs(own)))) if not res['fallback'][i] else 0.0
			dinv = SLACK * (24 * nc * U * kappa * n2 + n2 * n2 * dM * nc) * np.ones((nc, nc))
			xc = ld(gs[i, npair:npair + nc])
			ccx = inv @ xc
			dccx = dinv @ np.abs(np.asarray(xc, F64)) + SLACK * (nc + 1) * U * np.asarray(np.abs(inv) @ np.abs(xc), F64)
			dot = xc @ ccx
			ddot = float(np.abs(np.asarray(xc, F64)) @ dccx + SLACK * (nc + 1) * U * float(np.abs(xc) @ np.abs(ccx)))
			xx = xx - dot
			xx_abs = xx_abs + np.abs(xc) @ np.abs(ccx)
			res['ccx'][i], res['inv'][i], res['ccx_bound'][i], res['inv_bound'][i] = ccx, inv, dccx, dinv
		else:
			ddot = 0.0
		vx = xx / ns
		res['vx_bound'][i] = (ddot + SLACK * U * float(abs(xx))) / float(ns) + SLACK * U * float(abs(vx)) + 16 * ULD * float(xx_abs) / float(ns)
		res['vx_raw'][i] = vx
		res['vx_abs'][i] = float(xx_abs) / float(ns)
		if vx == 0:
			vx = LD(1)
		dof = float(ns) - 1.0 - rk - dimreduce
		if not dof > 0:
			res['flags'][3] += 1
			dof = 1.0
		res['ns'][i], res['vx'][i], res['dof'][i], res['rank'][i] = ns, vx, dof, rk
	return res


def judge_group_info(info, varx, flags, ref, nc):
	"""info (nx, pitch) as the kernel wrote it (the plan columns are compared by the caller)."""
	ws = {}
	ws['ns'] = bits(info[:, 0].copy(), np.asarray(ref['ns'], F64), 'ns')
	# vx = 0 -> 1 is a discontinuity: where the value before the rule is within its bound of 0 (x lies in the span of the covariates on S_i: as many
	# covariates as cells) either side of the rule is right -- the value within its bound, or exactly 1; everywhere else there is one answer
	err = np.abs(ld(info[:, 1]) - ref['vx'])
	near0 = np.abs(np.asarray(ref['vx_raw'], F64)) <= ref['vx_bound']
	err = np.where(near0, np.minimum(np.abs(ld(info[:, 1]) - ref['vx_raw']), np.abs(ld(info[:, 1]) - 1)), err)
	err = np.where(info[:, 1] == 0, np.inf, err)  # (never 0 itself: that is what the rule is for)
	ws['vx'] = worst(err, ref['vx_bound'], 'vx')
	ws['varx'] = bits(varx.copy(), info[:, 1].copy(), 'varx == rec[1]')
	if nc:
		ws['ccx'] = worst(np.abs(ld(info[:, HEAD:HEAD + nc]) - ref['ccx']), ref['ccx_bound'], 'ccx')
		ws['M+'] = worst(np.abs(ld(info[:, HEAD + nc:HEAD + nc + nc * nc]).reshape(info.shape[0], nc, nc) - ref['inv']), ref['inv_bound'], 'M+')
	ws['flags'] = Worst(0.0 if np.array_equal(np.asarray(flags[2:5], np.int64), ref['flags'][2:5]) else np.inf, None, 'flags[2..4] %s want %s' % (list(flags[2:5]), list(ref['flags'][2:5])))
	return ws


def record(ref, i, nc, plan=None):
	"""The fp64 record of grouping i from a group_info reference (plan: 24 doubles, or zeros)."""
	rec = np.zeros(HEAD + nc + nc * nc)
	rec[0], rec[1] = float(ref['ns'][i]), float(ref['vx'][i])
	if plan is not None:
		rec[2:HEAD] = plan
	rec[HEAD:HEAD + nc] = np.asarray(ref['ccx'][i], F64)
	rec[HEAD + nc:] = np.asarray(ref['inv'][i], F64).ravel()
	return rec


# ---- stream ----------------------------------------------------------------------------------------------------------------------------------------------------
def stream(Y, C, code, nc, n_kept, ldye):
	"""common (nc + 1, ny) longdouble with its bound, and YE (n_kept, ldye): the values at the kept cells in columns < ny, NaN elsewhere (columns ny.. may also
	hold row ny - 1's value: ye_pad)."""
	ny, n = Y.shape
	V = 4 if Y.dtype == F32 else 2
	m = code == COMMON
	Yn = ld(Y[:, m])
	Cn = ld(C[:, m]) if nc else np.zeros((0, int(m.sum())), LD)
	common = np.concatenate([Cn @ Yn.T, (Yn * Yn).sum(axis=1)[None]], axis=0)
	cab = np.concatenate([np.abs(Cn) @ np.abs(Yn).T, (Yn * Yn).sum(axis=1)[None]], axis=0)
	depth = math.ceil(math.ceil(n / V) / 256) * V + 1 + 1 + 6 + 3
	ye = np.full((n_kept, ldye), np.nan, Y.dtype)
	ye_pad = np.full((n_kept, ldye), np.nan, Y.dtype)
	k = np.nonzero(code >= 0)[0]
	ye[code[k], :ny] = Y[:, k].T
	ye_pad[code[k], :] = Y[ny - 1, k][:, None]
	return dict(common=common, common_bound=SLACK * U * depth * cab + 16 * ULD * cab, ye=ye, ye_pad=ye_pad)


def judge_stream(common, ye, ref, ny, exact):
	ws = {}
	if exact:
		ws['common'] = bits(np.asarray(common, F64), np.asarray(ref['common'], F64), 'common (exact)')
	else:
		ws['common'] = worst(np.abs(ld(common) - ref['common']), ref['common_bound'], 'common')
	ws['YE'] = bits(ye[:, :ny].copy(), ref['ye'][:, :ny].copy(), 'YE at the kept cells')
	pad = ye[:, ny:]
	ok = np.isnan(pad) | same_bits(pad.copy(), ref['ye_pad'][:, ny:].copy())
	ws['YE padding'] = Worst(0.0 if ok.all() else np.inf, tuple(np.argwhere(~ok)[0]) if not ok.all() else None, 'columns ny..ldye: NaN or row ny - 1')
	return ws


# ---- pairs: cells and the masked-Gram sweep ---------------------------------------------------------------------------------------------------------------
def cell_sums(YE, CE, xe, seg, common, nc, ny):
	"""a (nx, ny, nc), xy0, q (nx, ny) in longdouble and their running-error bounds (cells: the shared part first, then the grouping's own cells in order)."""
	nx = len(seg) - 1
	a, da = np.zeros((nx, ny, nc), LD), np.zeros((nx, ny, nc))
	xy, dxy, q, dq = np.zeros((nx, ny), LD), np.zeros((nx, ny)), np.zeros((nx, ny), LD), np.zeros((nx, ny))
	for i in range(nx):
		s, e = int(seg[i]), int(seg[i + 1])
		v = ld(YE[s:e, :ny])  # (len, ny)
		ce, x = ld(CE[s:e]).reshape(e - s, nc), ld(xe[s:e])
		depth = e - s + 2
		a[i] = ld(common[:nc]).T + v.T @ ce
		ab = np.abs(ld(common[:nc])).T + np.abs(v).T @ np.abs(ce)
		da[i] = SLACK * U * depth * ab + 16 * ULD * ab
		xy[i] = v.T @ x
		ab = np.abs(v).T @ np.abs(x)
		dxy[i] = SLACK * U * depth * ab + 16 * ULD * ab
		q[i] = ld(common[nc]) + (v * v).sum(axis=0)
		dq[i] = (SLACK * U * depth + 16 * ULD) * np.asarray(np.abs(ld(common[nc])) + (v * v).sum(axis=0), F64)  # (|terms|: a common[qrow] handed in may be negative)
	return a, da, xy, dxy, q, dq


def pairs(a, da, xy0, dxy0, q, dq, info, nc, return_dot):
	"""The closed form of every pair from (a, xy0, q) and the groupings' records (info (nx, >= HEAD + nc + nc^2) fp64: exact inputs)."""
	f = lambda v: np.asarray(v, F64)
	ns, vx = ld(info[:, 0])[:, None], ld(info[:, 1])[:, None]
	ccx = ld(info[:, HEAD:HEAD + nc])[:, None, :]  # (nx, 1, nc)
	mi = ld(info[:, HEAD + nc:HEAD + nc + nc * nc]).reshape(info.shape[0], nc, nc)
	ccy = np.einsum('ice,iye->iyc', mi, a)
	k = SLACK * (nc + 1) * U
	dccy = np.einsum('ice,iye->iyc', f(np.abs(mi)), da) + k * f(np.einsum('ice,iye->iyc', np.abs(mi), np.abs(a)))
	ady, adx = (a * ccy).sum(axis=2), (a * ccx).sum(axis=2)
	dady = (da * f(np.abs(ccy)) + f(np.abs(a)) * dccy).sum(axis=2) + k * f((np.abs(a * ccy)).sum(axis=2))
	dadx = (da * f(np.abs(ccx))).sum(axis=2) + k * f(np.abs(a * ccx).sum(axis=2))
	yy, xy = q - ady, xy0 - adx
	dyy = dq + dady + SLACK * U * f(np.abs(yy)) + 16 * ULD * f(np.abs(q) + np.abs(a * ccy).sum(axis=2))
	dxy = dxy0 + dadx + SLACK * U * f(np.abs(xy)) + 16 * ULD * f(np.abs(xy0) + np.abs(a * ccx).sum(axis=2))
	with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
		vy = yy / ns
		dvy = dyy / f(ns) + SLACK * U * f(np.abs(vy))
		gam = xy / (ns * vx)
		dg = dxy / f(ns * vx) + SLACK * 2 * U * f(np.abs(gam))
		r2 = gam * gam * vx / vy
		room = np.maximum(f(vy) - dvy, 0.0)
		dr2 = np.where(room > 0, ((2 * f(np.abs(gam)) * dg + dg * dg) * f(vx) + f(r2) * dvy) / room, np.inf) + SLACK * 4 * U * f(r2)
		stat = gam * vx if return_dot else gam
		dstat = dg * (f(vx) if return_dot else 1.0) + SLACK * U * f(np.abs(stat))
		alpha = ccy - gam[:, :, None] * ccx
		dalpha = dccy + dg[:, :, None] * f(np.abs(ccx)) + SLACK * U * f(np.abs(ccy) + 2 * np.abs(gam[:, :, None] * ccx))
	r2_64 = f(r2)
	finite = np.isfinite(r2_64) & np.isfinite(f(vy))
	return dict(yy=yy, vy=vy, gam=gam, r2=r2, stat=stat, alpha=alpha, alpha_abs=f(np.abs(ccy) + np.abs(gam[:, :, None] * ccx)),
				yy_abs=f(np.abs(q) + np.abs(a * ccy).sum(axis=2)), xy_abs=f(np.abs(xy0) + np.abs(a * ccx).sum(axis=2)), vy_bound=dvy, stat_bound=dstat, r2_bound=dr2, alpha_bound=dalpha, yy_bound=dyy,
				flag0=int((~finite).sum()), flag1=int((finite & (r2_64 > 1.0 + 1e-8)).sum()), finite=finite,
				q_over_yy=f(np.abs(q)) / np.maximum(f(np.abs(yy)), 1e-300))


def _f32(bound, value, dtype):
	return bound + (2.0**-24 * np.abs(np.asarray(value, F64)) + 2.0**-150 if np.dtype(dtype) == F32 else 0.0)


def judge_pairs(got, ref, out_dtype, flags=None):
	"""got: stat, vary (nx, ny), alpha (nx, ny, nc) or None -- EVERY pair; non-finite reference values must come back non-finite."""
	ws = {}
	for name, key in (('stat', 'stat'), ('vary', 'vy')) + ((('alpha', 'alpha'), ) if got.get('alpha') is not None else ()):
		r, b = ref[key], _f32(ref[key + '_bound'], ref[key], out_dtype)
		g = ld(got[name])
		fin = np.isfinite(np.asarray(r, F64))
		err = np.where(fin, np.abs(g - np.where(fin, r, 0)), np.where(np.isfinite(np.asarray(g, F64)), np.inf, 0.0))
		ws[name] = worst(err, np.where(fin, b, 1.0), name)
	if flags is not None:
		ok = int(flags[0]) == ref['flag0'] and int(flags[1]) == ref['flag1']
		ws['flags'] = Worst(0.0 if ok else np.inf, None, 'flags[0], [1] = %d, %d want %d, %d' % (flags[0], flags[1], ref['flag0'], ref['flag1']))
	return ws


def p_subset(ref, dof, plants=(), limit=24):
	"""The planted pairs and an even spread over ln P of the finite pairs with R^2 < 1."""
	r2 = np.asarray(ref['r2'], F64)
	ok = ref['finite'] & (r2 >= 0) & (r2 < 1)
	idx = np.argwhere(ok)
	picks = [tuple(p) for p in plants]
	if idx.size:
		lp = np.asarray(dof)[idx[:, 0]] / 2 * np.log1p(-r2[ok])
		order = np.argsort(lp)
		for L in np.linspace(0, max(-700.0, float(lp.min())), limit // 4):  # evenly over the range of ln P ...
			picks.append(tuple(int(v) for v in idx[order[min(np.searchsorted(lp[order], L), order.size - 1)]]))
		for k in np.linspace(0, order.size - 1, limit).astype(int):  # ... and evenly over the values that occur
			picks.append(tuple(int(v) for v in idx[order[k]]))
	return list(dict.fromkeys(picks))


def ln_p_estimates(ref, dof):
	r2 = np.asarray(ref['r2'], F64)
	ok = ref['finite'] & (r2 >= 0) & (r2 < 1)
	return (np.asarray(dof)[:, None] / 2 * np.log1p(-np.where(ok, r2, 0)))[ok]


def judge_p(p_got, ref, dof, picks, out_dtype):
	"""P at the picks against mpmath at the reference's R^2 rounded to double: G12's tolerance plus (dof / 2) (d_R2 + roundings of R^2 and 1 - R^2) / (1 - R^2)."""
	errs, bounds = [], []
	for (i, y) in picks:
		x, d = float(ref['r2'][i, y]), float(ref['r2_bound'][i, y])
		want = k3.p_mp(x, float(dof[i]))
		got = float(p_got[i, y])
		if x + 2 * d >= 1:  # within its bound of 1: P is monotone, 0 <= p <= P(R^2 - bound) is all that holds
			top = float(k3.p_mp(max(x - 2 * d - 2 * U, 0.0), float(dof[i]))) * (1 + 1e-6) + 1e-300
			errs.append((got if top < 1 else 0.0) if 0 <= got <= 1 else np.inf)  # (a bound that reaches R^2 = 0 says 0 <= p <= 1 and no more)
			bounds.append(top)
			continue
		tol = (k3.p_tolerance(want, float(dof[i])) if want > 0 else 0.0) + float(dof[i]) / 2 * (d + U * x + float(np.spacing(1 - x))) / (1 - x)
		errs.append(abs(got - float(want)))
		bounds.append(_f32(tol * float(want) + 1e-300, float(want), out_dtype))
	w = worst(np.array(errs), np.array(bounds, F64), 'p (mpmath subset)')
	return Worst(w.ratio, picks[w.where[0]] if w.where else None, w.what)


# ---- a cells problem: segments of CELL_LENS, planted pairs, a zero gene ------------------------------------------------------------------------------------------
def cells_problem(ny, nc, ydt, seed=0, exact=False, n_common=40, lens=None, intercept=True, mean_over_sd=None, zero_gene=True, duplicate=False):
	"""Everything nrm_single1_cells reads, built from an actual screen: a design whose grouping i owns lens[i] cells, n_common shared cells, covariates (the
	first an intercept), expression values; the selection, the groupings' records and the shared sums from the stage references (rounded to fp64: the
	inputs of this stage).  Planted pairs on the last grouping (genes 0..3: R^2 = 1e-6, 1/4 -, 1/4 +, 1 - 1e-9), gene ny - 1 all zero."""
	lens = list(CELL_LENS if lens is None else lens)
	nx = len(lens)
	n = n_common + sum(lens) + 6  # six cells carry two groupings
	rng = np.random.default_rng([seed, ny, nc, 31])
	perm = rng.permutation(n)
	own = np.split(perm[n_common:n_common + sum(lens)], np.cumsum(lens)[:-1])
	double = perm[n_common + sum(lens):]
	rows = [np.sort(np.concatenate([own[i], double if i in (nx - 1, nx - 2) else []])).astype(np.int32) for i in range(nx)]
	row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
	cells = np.concatenate(rows).astype(np.int32)
	C = covariates(nc, n, seed, exact, intercept=intercept, duplicate=duplicate)
	vals = None if exact else np.where(rng.uniform(size=cells.size) < 0.5, 1.0, rng.uniform(0.25, 1.0, size=cells.size))
	sel = select(row_ptr, cells, vals, n, C if nc else None)
	Y = expression(ny, n, ydt, seed, exact)
	plants = {}
	if mean_over_sd is not None:
		for y in range(ny):
			r = mean_over_sd[y % len(mean_over_sd)]
			Y[y] = (r + rng.normal(size=n)).astype(ydt)
	elif not exact and ny >= 8:
		i = nx - 1
		S = np.concatenate([np.nonzero(sel['code'] == COMMON)[0], sel['idx'][sel['seg'][i]:sel['seg'][i + 1]]])
		xs = np.zeros(len(S))
		xs[n_common:] = sel['xe'][sel['seg'][i]:sel['seg'][i + 1]]
		Cs = C[:, S].T if nc else np.zeros((len(S), 0))
		res = lambda v: v - Cs @ np.linalg.lstsq(Cs, v, rcond=None)[0] if nc else v
		xt = res(xs)
		for y, r2 in enumerate((1e-6, 0.25 - 1e-6, 0.25 + 1e-6, 1 - 1e-9)):
			e = res(rng.normal(size=len(S)))
			e = e - xt * (e @ xt) / (xt @ xt)
			Y[y] = 0
			Y[y, S] = (math.sqrt(r2) * xt / np.linalg.norm(xt) + math.sqrt(1 - r2) * e / np.linalg.norm(e)).astype(ydt)
			plants[('near 0', 'quarter -', 'quarter +', 'near 1')[y]] = (i, y)
	if zero_gene and ny > 1:
		Y[ny - 1] = 0
	ldye = (ny + 7) // 8 * 8
	st = stream(Y, C, sel['code'], nc, sel['n_kept'], ldye)
	gs, _ = group_stats(sel['seg'], sel['idx'], sel['xe'], C, nc)
	gpart = None
	if nc:
		gpart = np.zeros((GB, 64))
		g8 = np.zeros((8, 8))
		g8[:min(nc, 8), :min(nc, 8)] = np.asarray(sel['gram'], F64)[:8, :8]
		gpart[0] = g8.ravel()
	if nc <= 8:
		gi = group_info(np.asarray(gs, F64), gpart, sel['rowinfo'], sel['n_common'], nc, 0)
	else:  # (the device has no group_info beyond 8 covariates; the record is data to the sweep: built here with the same rule)
		gi = group_info_wide(np.asarray(gs, F64), np.asarray(sel['gram'], F64), sel['rowinfo'], sel['n_common'], nc)
	info = np.stack([record(gi, i, nc) for i in range(nx)])
	ye = np.where(np.isnan(st['ye']), 0, st['ye']).astype(ydt)
	return dict(nx=nx, ny=ny, nc=nc, n=n, row_ptr=row_ptr, cells=cells, vals=vals, C=C, Y=Y, sel=sel, ye=ye, ldye=ldye, common=np.asarray(st['common'], F64), info=info,
				dof=gi['dof'], plants=plants, gi=gi, gs=np.asarray(gs, F64), gpart=gpart)


def group_info_wide(gs, gram, rowinfo, n_common, nc):
	"""group_info for more than 8 covariates (no kernel: the host does this in the product), from the shared cells' Gram matrix itself."""
	return group_info(gs, None, rowinfo, n_common, nc, 0, gram=gram)


def cells_reference(pb, return_dot, common=None):
	a, da, xy, dxy, q, dq = cell_sums(pb['ye'], pb['sel']['ce'], pb['sel']['xe'], pb['sel']['seg'], pb['common'] if common is None else common, pb['nc'], pb['ny'])
	ref = pairs(a, da, xy, dxy, q, dq, pb['info'], pb['nc'], return_dot)
	ref.update(a=a, xy0=xy, q=q)
	return ref


def q_cut(ref, i, target=1.5):
	"""What to take off common[qrow] of every gene so that grouping i's R^2 becomes `target` (yy' = yy R^2 / target)."""
	return np.asarray(ref['yy'][i] * (1 - ref['r2'][i] / target), F64)


def residual_first(pb):
	"""yy the way the reference takes it (association.py:357-360): the residual first, then its sum of squares -- in longdouble, for the digits-lost column."""
	nx, ny, nc = pb['nx'], pb['ny'], pb['nc']
	out = np.zeros((nx, ny), LD)
	sel = pb['sel']
	for i in range(nx):
		S = np.concatenate([np.nonzero(sel['code'] == COMMON)[0], sel['idx'][sel['seg'][i]:sel['seg'][i + 1]]])
		Ys, Cs = ld(pb['Y'][:, S]), ld(pb['C'][:, S])
		mi = ld(pb['info'][i, HEAD + nc:HEAD + nc + nc * nc]).reshape(nc, nc)
		r = Ys - (Ys @ Cs.T) @ mi @ Cs
		out[i] = (r * r).sum(axis=1)
	return out


# ---- fp64 emulations of the kernels, in their own order of operations (no fma: the product is rounded too) -------------------------------------------------
def _tree(t):
	"""__shfl_down tree over the last axis of 64 lanes: lane 0's value."""
	t = np.array(t, F64)
	for o in (32, 16, 8, 4, 2, 1):
		t = t.copy()
		t[..., :64 - o] = t[..., :64 - o] + t[..., o:]
	return t[..., 0]


def emu_select(row_ptr, cells, vals, n, C, mut=None):
	"""The five kernels of nrm_single1_select as they run: counts, ballots with a running offset, the scan, the codes, the placement."""
	nx = len(row_ptr) - 1
	nc = 0 if C is None else C.shape[0]
	cnt = np.zeros(n, np.int32)
	np.add.at(cnt, cells, 1)
	seg = np.zeros(nx + 1, np.int64)
	rowinfo = np.zeros((nx, 3))
	keepm = []
	for i in range(nx):
		a, b = int(row_ptr[i]), int(row_ptr[i + 1])
		kept, lo, hi = 0, np.inf, -np.inf
		masks = []
		for e0 in range(a, b, 64):
			e = np.arange(e0, min(e0 + 64, b))
			keep = cnt[cells[e]] == 1
			v = np.ones(len(e)) if vals is None else vals[e]
			if keep.any():
				lo, hi = min(lo, v[keep].min()), max(hi, v[keep].max())
			masks.append((e, keep, kept))
			kept += int(keep.sum())
		keepm.append(masks)
		seg[i + 1] = kept
		rowinfo[i] = (kept, lo, hi)
	seg[1:] = np.cumsum(seg[1:])
	if mut == 'seg off by one' and nx > 1:
		seg[1:-1] += (seg[1:-1] < seg[-1])
	common = cnt == 0
	if mut == 'skip counted as common':
		common = cnt != 1
	code = np.where(cnt == 0, COMMON, SKIP).astype(np.int32)
	nk = int(seg[-1])
	idx, xe, ce = np.full(nk, -7, np.int64), np.full(nk, np.nan), np.full((nk, nc), np.nan)
	for i in range(nx):
		for e, keep, kept in keepm[i]:
			pos = seg[i] + kept + np.cumsum(keep) - keep  # popcount of the ballot below the lane
			for j in np.nonzero(keep)[0]:
				p = int(pos[j])
				if p >= nk:
					continue
				k = cells[e[j]]
				idx[p], xe[p], code[k] = k, (1.0 if vals is None else vals[e[j]]), p
				if nc:
					ce[p] = C[:, k]
	res = dict(cnt=cnt, code=code, seg=seg, idx=idx, xe=xe, ce=ce, rowinfo=rowinfo, n_common=int(common.sum()), n_kept=nk, gram=None)
	if nc:
		res['gram'] = gram_from_parts(emu_common_gram(cnt if mut != 'skip counted as common' else np.where(cnt == 1, 1, 0), C), nc)
	return res


def emu_common_gram(cnt, C):
	nc, n = C.shape
	nb = (nc + 7) // 8
	Cp = np.zeros((nb * 8, n))
	Cp[:nc] = C
	part = np.zeros((nb * (nb + 1) // 2, GB, 64))
	p = 0
	for bi in range(nb):
		for bj in range(bi, nb):
			for g in range(min(GB, (n + 255) // 256)):  # (the other blocks have no cell: their sums are 0)
				acc = np.zeros((256, 64))
				for k0 in range(g * 256, n, GB * 256):
					k = np.arange(k0, min(k0 + 256, n))
					m = cnt[k] == 0
					t = (Cp[bi * 8:bi * 8 + 8, k][:, None, :] * Cp[bj * 8:bj * 8 + 8, k][None, :, :]).reshape(64, -1).T
					acc[:len(k)] = acc[:len(k)] + np.where(m[:, None], t, 0.0)
				w = _tree(acc.reshape(4, 64, 64).transpose(0, 2, 1))  # (4 waves, 64 sums)
				part[p, g] = ((w[0] + w[1]) + w[2]) + w[3]
			p += 1
	return part


def emu_group_stats(seg, cells, xe, C, nc):
	nx = len(seg) - 1
	iu = np.triu_indices(nc)
	out = np.zeros((nx, nc * (nc + 1) // 2 + nc + 1))
	for i in range(nx):
		acc = np.zeros((out.shape[1], 64))
		for e0 in range(int(seg[i]), int(seg[i + 1]), 64):
			e = np.arange(e0, min(e0 + 64, int(seg[i + 1])))
			cv, x = (C[:, cells[e]] if nc else np.zeros((0, len(e)))), xe[e]
			t = np.concatenate([(cv[:, None, :] * cv[None, :, :])[iu], cv * x, (x * x)[None]], axis=0)
			acc[:, :len(e)] = acc[:, :len(e)] + t
		out[i] = _tree(acc)
	return out


def jacobi_pinv(m, tol=1e-8):
	"""nrm_small_pinv_one of csrc/nrm_jacobi.h, statement by statement, in Python floats (fp64)."""
	n = m.shape[0]
	a = [[0.5 * (float(m[i, j]) + float(m[j, i])) for j in range(n)] for i in range(n)]
	v = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
	for _ in range(60):
		off = diag = 0.0
		for i in range(n):
			diag += a[i][i] * a[i][i]
			for j in range(i + 1, n):
				off += a[i][j] * a[i][j]
		if off == 0.0 or off <= 1e-34 * diag:
			break
		for p in range(n - 1):
			for q in range(p + 1, n):
				apq = a[p][q]
				if apq == 0.0:
					continue
				theta = (a[q][q] - a[p][p]) / (2.0 * apq)
				t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
				c = 1.0 / math.sqrt(t * t + 1.0)
				s = t * c
				for k in range(n):
					akp, akq = a[k][p], a[k][q]
					a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
				for k in range(n):
					apk, aqk = a[p][k], a[q][k]
					a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
				a[p][q] = a[q][p] = 0.0
				for k in range(n):
					vkp, vkq = v[k][p], v[k][q]
					v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
	w = [a[i][i] for i in range(n)]
	smax = max([abs(x) for x in w] + [0.0])
	keep = [abs(x) >= tol * smax for x in w]
	iw = [1.0 / w[i] if keep[i] else 0.0 for i in range(n)]
	inv = np.zeros((n, n))
	for i in range(n):
		for j in range(i + 1):
			t = 0.0
			for k in range(n):
				if iw[k] != 0.0:
					t += v[i][k] * iw[k] * v[j][k]
			inv[i, j] = inv[j, i] = t
	return inv, sum(keep)


def emu_group_info(gs, gpart, rowinfo, n_common, nc, dimreduce, pitch=None, mut=None):
	nx = gs.shape[0]
	npair = nc * (nc + 1) // 2
	pitch = pitch or HEAD + nc + nc * nc
	info, varx, flags = np.full((nx, pitch), np.nan), np.full(nx, np.nan), np.zeros(8, np.int64)
	mcc = np.zeros(64)
	if nc:
		for g in range(gpart.shape[0]):
			mcc = mcc + gpart[g]
	for i in range(nx):
		ns = float(n_common) + rowinfo[i, 0]
		lo, hi = rowinfo[i, 1], rowinfo[i, 2]
		if n_common > 0 and mut != 'min/max not extended by 0':
			lo, hi = min(lo, 0.0), max(hi, 0.0)
		if not hi > lo:
			flags[2] += 1
		xx = gs[i, npair + nc]
		rk = 0
		if nc:
			m = np.zeros((nc, nc))
			w = 0
			for c in range(nc):
				for d in range(c, nc):
					m[c, d] = m[d, c] = gs[i, w] + mcc[c * 8 + d]
					w += 1
			if not np.isfinite(m).all():
				flags[4] += 1
				m = np.eye(nc)
			inv, rk = jacobi_pinv(m, 1e-6 if mut == 'rank tolerance 1e-6' else 1e-8)
			if rk == 0:
				inv[:] = 0
			xc = gs[i, npair:npair + nc]
			dot = 0.0
			for c in range(nc):
				t = 0.0
				for d in range(nc):
					t += inv[c, d] * xc[d]
				info[i, HEAD + c] = t
				dot += xc[c] * t
			xx -= dot
			info[i, HEAD + nc:HEAD + nc + nc * nc] = inv.ravel()
		vx = xx / ns
		if vx == 0.0 and mut != 'vx 0 -> 1 left out':
			vx = 1.0
		dof = ns - 1.0 - rk - dimreduce - (1 if mut == 'dof off by one' else 0)
		if not dof > 0:
			flags[3] += 1
			dof = 1.0
		info[i, 0], info[i, 1], varx[i] = ns, vx, vx
		info[i, 2] = dof  # (the plan's place: the emulation leaves dof there for the tests that compare it)
	return info, varx, flags


def emu_stream(Y, C, code, nc, n_kept, ldye, mut=None):
	"""k_s1_stream pass by pass: thread tid takes the groups tid, tid + 256, ... of V cells, then one cell of the tail; the lane tree, the four waves in order."""
	ny, n = Y.shape
	V = 4 if Y.dtype == F32 else 2
	common = np.full((nc + 1, ny), np.nan)
	ye = np.full((n_kept, ldye), np.nan, Y.dtype)
	groups = n // V
	for pi, (comp0, NC) in enumerate(stream_passes(nc)):
		first = pi == 0
		R = 8 if (first and NC <= 5) else 4
		nblk = ((ny + R - 1) // R + 7) // 8 * 8
		per = (nblk + 7) // 8
		for b in range(nblk):
			y0 = ((b % 8) * per + b // 8) * R
			if y0 >= ny:
				continue
			rows = np.minimum(y0 + np.arange(R), ny - 1)
			acc = np.zeros((R, NC + 1, 256))
			cells_of = [np.arange(g0 * V, min(g0 + 256, groups) * V).reshape(-1, V) for g0 in range(0, groups, 256)]
			order = [ks[:, v] for ks in cells_of for v in range(V)]
			if mut != 'tail dropped' and groups * V < n:
				order.append(np.arange(groups * V, n))
			for k in order:
				m = code[k] == COMMON
				yd = Y[rows][:, k].astype(F64)
				ym = np.where(m, yd, 0.0)
				t = acc[:, :, :len(k)]
				if first:
					t[:, NC] = t[:, NC] + {'q masked on both factors': ym * ym, 'q not masked': yd * yd}.get(mut, ym * yd)
				for c in range(NC):
					t[:, c] = t[:, c] + ym * C[comp0 + c, k]
				if first:
					kk = k[code[k] >= 0]
					for r in range(R):
						dst = code[kk]
						if mut == 'padding rows land in another row' and y0 + r >= ny:
							dst = (dst + 1) % max(n_kept, 1)
						ye[dst, y0 + r] = Y[rows[r], kk]
			w = _tree(acc.reshape(R, NC + 1, 4, 64))
			tot = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
			for r in range(R):
				if y0 + r < ny:
					c0 = comp0 + (1 if (mut == 'reach-back one too high' and not first and comp0 % 8) else 0)
					common[c0:c0 + NC, y0 + r] = tot[r, :NC]
					if first:
						common[nc, y0 + r] = tot[r, NC]
	return common, ye


def emu_cells(YE, CE, xe, seg, common, info, nc, ny, return_dot, mut=None, xy0=None):
	"""k_s1_cells per thread: the shared sums, the grouping's cells in order, the closed form; vectorised over the genes.  Returns stat, vary, alpha, r2, flags."""
	nx = len(seg) - 1
	acc = F32 if mut == 'float accumulator' else F64
	stat, vary, alpha, r2o = np.zeros((nx, ny)), np.zeros((nx, ny)), np.zeros((nx, ny, nc)), np.zeros((nx, ny))
	flags = np.zeros(8, np.int64)
	for i in range(nx):
		ns, vx = info[i, 0], info[i, 1]
		ccx, mi = info[i, HEAD:HEAD + nc], info[i, HEAD + nc:HEAD + nc + nc * nc].reshape(nc, nc)
		a = [common[c, :ny].astype(acc) for c in range(nc)]
		xy, q = (np.zeros(ny, acc) if xy0 is None else xy0[i].astype(acc)), common[nc, :ny].astype(acc)  # (xy0: the masked-Gram sweep's own xy)
		for k in range(int(seg[i]), int(seg[i + 1])):
			v = YE[k, :ny].astype(acc)
			for c in range(nc):
				a[c] = a[c] + v * acc(CE[k, c])
			xy = xy + v * acc(xe[k])
			q = q + v * v
		a, xy, q = [t.astype(F64) for t in a], xy.astype(F64), q.astype(F64)
		ady, adx, ccy = np.zeros(ny), np.zeros(ny), []
		for c in range(nc):
			t = np.zeros(ny)
			for e in range(nc):
				t = t + mi[c, e] * a[e]
			ccy.append(t)
			ady = ady + a[c] * t
			adx = adx + a[c] * ccx[c]
		with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
			yy = q - ady
			xy = xy - adx
			vy = yy / ns
			gam = xy / (ns * vx)
			r2 = gam * gam * vx / vy
		bad = ~np.isfinite(r2) | ~np.isfinite(vy)
		flags[0] += int(bad.sum())
		flags[1] += int((~bad & (r2 > 1.0 + 1e-8)).sum())
		stat[i], vary[i], r2o[i] = (gam * vx if return_dot else gam), vy, r2
		for c in range(nc):
			alpha[i, :, c] = (ccx[c] - gam * ccy[c]) if mut == 'ccx and ccy swapped' else (ccy[c] - gam * ccx[c])
	return dict(stat=stat, vary=vary, alpha=alpha if nc else None, r2=r2o), flags


# ---- problems of the other stages ------------------------------------------------------------------------------------------------------------------------------
GI_VARIANTS = ['plain', 'duplicate', 'zero covariate', 'no shared cells', 'nearly dependent']


def gi_problem(nx, nc, variant, seed=0):
	"""What nrm_single1_group_info reads, from an actual design (grouping i owns 2 + i % 5 cells with distinct values; 30 shared cells, or none).  'plain' with
	nx >= 4 also carries: row 1 keeps nothing (xx = 0: vx 0 -> 1; flagged), row 2 takes the single value 0.5 on its own cells (not flagged: the shared cells
	add 0; without shared cells it is flagged), row 3 has an infinite Gram entry (nc > 0: flags[4], the identity instead).  Without shared cells ns <= nc + 1 for
	most rows: dof <= 0."""
	rng = np.random.default_rng([seed, nx, nc, 37])
	lens = [2 + i % 5 for i in range(nx)]
	n_common = 0 if variant == 'no shared cells' else 30
	n = n_common + sum(lens)
	C = rng.normal(size=(nc, n))
	if nc:
		C[0] = 1.0
	if variant == 'duplicate' and nc > 1:
		C[nc - 1] = C[0]
	if variant == 'zero covariate' and nc > 1:
		C[1] = 0.0
	if variant == 'nearly dependent' and nc > 1:
		C[nc - 1] = C[nc - 2] + 1e-3 * rng.normal(size=n)
	seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
	cells = (n_common + np.arange(sum(lens))).astype(np.int64)
	xe = rng.uniform(0.25, 1.0, size=sum(lens))
	gs = np.asarray(group_stats(seg, cells, xe, C, nc)[0], F64)
	gpart = None
	if nc:
		g8 = np.zeros((8, 8))
		cn = C[:, :n_common]
		g8[:nc, :nc] = cn @ cn.T
		gpart = rng.normal(size=(GB, 64)) * 1e-3 * (n_common > 0)  # partial blocks that only add up to the matrix
		gpart[0] += g8.ravel() - gpart.sum(axis=0)
	rowinfo = np.array([[lens[i], xe[seg[i]:seg[i + 1]].min(), xe[seg[i]:seg[i + 1]].max()] for i in range(nx)])
	if variant == 'plain' and nx >= 4:
		npair = nc * (nc + 1) // 2
		gs[1, npair:] = 0.0
		gs[1, :npair] = 0.0
		rowinfo[1] = (0, np.inf, -np.inf)
		rowinfo[2, 1:] = 0.5
		if nc:
			gs[3, 0] = np.inf
	if variant == 'no shared cells' and nx >= 4:
		rowinfo[2, 1:] = 0.5  # the single value again: flagged now, no shared cell adds a 0
	return dict(gs=gs, gpart=gpart, rowinfo=rowinfo, n_common=n_common, nc=nc, nx=nx, dimreduce=1 if variant == 'plain' else 0)


def gs_problem(nc, seed=0, exact=False):
	"""Segments of GS_LENS over 200 cells in a scattered order."""
	rng = np.random.default_rng([seed, nc, 41])
	n = 400
	seg = np.concatenate([[0], np.cumsum(GS_LENS)]).astype(np.int64)
	cells = rng.permutation(n)[:seg[-1]].astype(np.int64)
	xe = rng.integers(1, 4, size=seg[-1]).astype(F64) if exact else rng.uniform(0.25, 1, size=seg[-1])
	return dict(seg=seg, cells=cells, xe=xe, C=covariates(nc, n, seed, exact), nc=nc, n=n)


def stream_problem(n, ny, nc, dtype, seed=0, exact=False):
	"""A cell in three common, one in three kept (positions in a scattered order), the others skipped."""
	rng = np.random.default_rng([seed, n, ny, nc, 43])
	kind = rng.integers(0, 3, size=n)
	code = np.where(kind == 0, COMMON, SKIP).astype(np.int32)
	kept = np.nonzero(kind == 1)[0]
	code[kept] = rng.permutation(len(kept))
	return dict(Y=expression(ny, n, dtype, seed, exact), C=covariates(nc, n, seed, exact), code=code, n_kept=len(kept), n=n, ny=ny, nc=nc)


def sweep_inputs(a, xy0, q, nc, pad=3):
	"""G (ny, nx (nc + 1) + pad), G2 (ny, nx + pad) as nrm_single1_sweep reads them, from (nx, ny, ..) sums rounded to fp64; NaN in the padding."""
	nx, ny = xy0.shape
	G = np.full((ny, nx * (nc + 1) + pad), np.nan)
	G2 = np.full((ny, nx + pad), np.nan)
	for i in range(nx):
		G[:, i * (nc + 1):i * (nc + 1) + nc] = np.asarray(a[i], F64)
		G[:, i * (nc + 1) + nc] = np.asarray(xy0[i], F64)
		G2[:, i] = np.asarray(q[i], F64)
	return G, G2


def chain_problem():
	"""The screen of the chain test (CHAIN: 65 groupings x 69 genes x 2051 cells x 5 covariates, fp32 rows, a 0/1 design, an intercept)."""
	nx, ny, n, nc = (CHAIN[k] for k in ('nx', 'ny', 'n', 'nc'))
	row_ptr, cells, _ = design(n, nx, 5, False, False)
	return dict(nx=nx, ny=ny, n=n, nc=nc, row_ptr=row_ptr, cells=cells, C=covariates(nc, n, 5, False, intercept=True), Y=expression(ny, n, F32, 5, False), return_dot=1,
				out_dtype=F32, ldye=(ny + 7) // 8 * 8)
