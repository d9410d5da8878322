"""Extended-precision restatement of K1 (csrc/nrm_residualize.hip), the decoder of its digit planes and the comparators of its outputs -- TEST INFRASTRUCTURE ONLY.

Plain numpy in longdouble (64-bit mantissa on x86: unit roundoff 2^-64), in the style of tests/front_longdouble.py.  The reference takes what the kernel takes:
the rows x, the covariates C, and the pseudo-inverse dci and rank that association._prepare_covariates returned -- the pseudo-inverse is an INPUT of K1, it is
not recomputed here.  Beside every quantity it returns the same expression with every term replaced by its absolute value: that is what the running-error
bound of an fp64 evaluation is made of.

Bounds (u = 2^-53, gamma(c) = c u / (1 - c u); the reference's own error, m 2^-64 for its longest sum of m terms, is added to every gamma).  c is counted from
the kernel's summation order, the longest chain of roundings any output element goes through:
  a = x C^T     k_residualize_v4: one thread adds 4 ceil(n4 / 1024) products by fma (n4 = n & ~3) and at most ONE tail cell; six shuffle steps add the 64 lanes
                of a wave, three adds the four waves:                                    c_a = 4 ceil(n4 / 1024) + [n % 4 != 0] + 6 + 3
                k_residualize: one cell per thread and step:                               c_a = ceil(n / 256) + 6 + 3
                k_residualize_wide: a is an input (ga):                                    c_a = 0
                |da| <= gamma(c_a) |x| |C|^T                                               =: gamma(c_a) a_abs
  b = a dci     nc fmas on top of the error of a:   |db| <= gamma(c_a + nc) a_abs |dci|^T  =: gamma(c_b) b_abs          (this is `coef`)
  res = x - b C nc fmas from the exact x, with b's error times |C|:   |dres| <= gamma(c_b + nc) (|x| + b_abs |C|)  =: gamma(c_r) res_abs        (`out`)
                without active covariates c_r = 0: the rows are copied (fp32 -> fp64 is exact) and `out` must equal x bit for bit.
  ss = sum res^2  v4: 4 ceil(n / 1024) fmas per thread + 6 + 3 =: c_s (padding cells add exact zeros); scalar: ceil(n / 256) + 6 + 3;
                wide: 4 + 6 + 3 in k_residualize_wide, then ceil(blocks / 256) + 6 + 3 in k_rw_sum.  It inherits 2 |res| |dres| + dres^2:
                |dss| <= gamma(c_s) ss + 2 gamma(c_r) sum |res| res_abs + gamma(c_r)^2 sum res_abs^2.
A bound the device exceeds is a finding about the kernel, not a reason to widen the bound.

The fixed-point side is exact integer arithmetic: the decoded digits must equal rint(out 2^-exps) of the SAME call bit for bit (tools/i8_error_model.py is the
one model of quantise / digits / row_stats; there is no second one here)."""
import collections
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import i8_error_model as model  # noqa: E402

LD = np.longdouble
U = 2.0**-53
ULD = 2.0**-64
RES_LOOSE = 12.0  # csrc/nrm_k1.h
EST_SHARE = 1e-8  # the share of |x|^2 the estimate |x|^2 - a.b must keep to be trusted (k_residualize_v4)
CLEAR = 1e-22  # k_rw_sum: |x~|^2 < 1e-22 |x|^2 clears the row
MARGIN = 100.0  # the designated rows of the exponent and clear-rule tests stay this factor away from every threshold, by the reference alone
FIX_STRIDE = 8

Worst = collections.namedtuple('Worst', 'ratio where what')  # ratio of error to bound (<= 1 passes; inf: an exact property is broken)


def ld(a):
	return np.asarray(a, dtype=LD)


def round_up(v, m):
	return (v + m - 1) // m * m


def prepare(C):
	"""(C as fp64, dci, rank) as the library prepares them on the host (association._prepare_covariates: inv_rank of C C^T)."""
	from normalisr_amd.association import _prepare_covariates
	return _prepare_covariates(np.asarray(C, dtype=np.float64))


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------------------
def reference(x, C, dci, rank, a=None):
	"""a = x C^T, b = a dci, res = x - b C, ss = sum res^2 in longdouble, their absolute-value versions, max |res| per row and the estimate est = |x|^2 - a.b
	that K1 accepts its bound with.  a: the products the caller hands to k_residualize_wide (ga), taken as exact input in place of x C^T."""
	x = ld(x)
	rows, n = x.shape
	nc = 0 if C is None else int(np.shape(C)[0])
	active = rank > 0 and nc > 0
	ax = np.abs(x)
	raw = (x * x).sum(axis=1)
	if active:
		C, D = ld(C)[:, :n], ld(dci).reshape(nc, nc)
		aC = np.abs(C)
		if a is None:
			a, a_abs = x @ C.T, ax @ aC.T
		else:
			a = ld(a)
			a_abs = np.abs(a)
		b, b_abs = a @ D.T, a_abs @ np.abs(D).T  # b[q] = sum_e dci[q][e] a[e]
		res, res_abs = x - b @ C, ax + b_abs @ aC
		est, est_abs = raw - (a * b).sum(axis=1), raw + (a_abs * b_abs).sum(axis=1)
	else:
		a = a_abs = b = b_abs = np.zeros((rows, nc), dtype=LD)
		res, res_abs, est, est_abs = x, ax, raw, raw
	ares = np.abs(res)
	return dict(rows=rows, n=n, nc=nc, active=active, a=a, a_abs=a_abs, b=b, b_abs=b_abs, res=res, res_abs=res_abs, ss=(res * res).sum(axis=1),
				ss_abs=(res_abs * res_abs).sum(axis=1), ss_cross=(ares * res_abs).sum(axis=1), max=ares.max(axis=1), xmax=ax.max(axis=1), raw=raw, est=est,
				est_abs=est_abs)


def counts(kind, n, nc, active=True, ldo=None):
	"""The constants c of the module docstring for one launch: kind 'v4' | 'scalar' | 'wide'."""
	if kind == 'v4':
		ca = 4 * math.ceil((n & ~3) / 1024) + (1 if n % 4 else 0) + 6 + 3
		cs = 4 * math.ceil(n / 1024) + 6 + 3
	elif kind == 'scalar':
		ca = math.ceil(n / 256) + 6 + 3
		cs = math.ceil(n / 256) + 6 + 3
	else:
		ca = 0
		cs = 4 + 6 + 3 + math.ceil(math.ceil((ldo or n) / 1024) / 256) + 6 + 3
	cb = ca + nc
	cr = cb + nc
	if not active:
		ca = cb = cr = 0
	return dict(a=ca, b=cb, res=cr, ss=cs, terms=n + 2 * nc)


def gamma(c, terms=0):
	"""c = 0: the value is copied or never formed -- no error at all, the reference's included."""
	return c * U / (1.0 - c * U) + terms * ULD if c else 0.0


def _worst(err, bound, what, rows=None):
	"""Largest err / bound and its index; a non-zero error against a zero bound is infinite."""
	err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
	if err.size == 0:
		return Worst(0.0, None, what)
	with np.errstate(divide='ignore', invalid='ignore'):
		ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
	ratio = np.where(np.isnan(ratio), np.inf, ratio)  # a NaN output
	i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
	return Worst(float(ratio[i]), tuple(int(v) for v in i), what)


def _nonzero(a, what, offset=(0, 0)):
	"""Worst(inf) at the first element of a that is not exactly +-0 (NaN counts), else None."""
	bad = np.argwhere(~(np.asarray(a) == 0))
	if bad.size:
		return Worst(np.inf, tuple(int(v) + o for v, o in zip(bad[0], offset)), what)
	return None


def worst_of(*ws):
	return max(ws, key=lambda w: w.ratio)


# ---- comparators of the fp64 outputs -------------------------------------------------------------------------------------------------------------------------
def compare_coef(coef, ref, cnt):
	"""`coef` (rows, nc) against b."""
	return _worst(np.abs(ld(coef) - ref['b']), gamma(cnt['b'], cnt['terms']) * ref['b_abs'], 'coef')


def compare_out(out, ref, cnt, cleared=None):
	"""`out` on ALL its (rows_pad, ldo) elements: the residuals to their bound, padding rows and padding cells exactly zero.  cleared: rows the wide kernel's
	clear rule must have zeroed."""
	rows, n = ref['rows'], ref['n']
	out = np.asarray(out)
	w = _nonzero(out[rows:], 'out: padding row', (rows, 0)) or _nonzero(out[:rows, n:], 'out: padding cell', (0, n))
	if w:
		return w
	err, bound = np.abs(ld(out[:rows, :n]) - ref['res']), gamma(cnt['res'], cnt['terms']) * ref['res_abs']
	if cleared is not None and cleared.any():
		w = _nonzero(out[:rows][cleared], 'out: row that must be cleared')
		if w:
			return w
		err, bound = err[~cleared], bound[~cleared]
	return _worst(err, bound, 'out')


def ss_bound(ref, cnt):
	g = gamma(cnt['res'], cnt['terms'])
	return gamma(cnt['ss'], cnt['terms']) * ref['ss'] + 2 * g * ref['ss_cross'] + g * g * ref['ss_abs']


def compare_ss(ss, ref, cnt, cleared=None):
	"""`ss` on all rows_pad rows."""
	rows = ref['rows']
	ss = np.asarray(ss)
	w = _nonzero(ss[rows:, None], 'ss: padding row', (rows, 0))
	if w:
		return w
	err, bound = np.abs(ld(ss[:rows]) - ref['ss']), ss_bound(ref, cnt)
	if cleared is not None and cleared.any():
		w = _nonzero(ss[:rows][cleared][:, None], 'ss: row that must be cleared')
		if w:
			return w
		err, bound = err[~cleared], bound[~cleared]
	return _worst(err, bound, 'ss')


def clear_expected(ref, cnt):
	"""k_rw_sum's rule by the reference alone: 1 = the row is cleared, 0 = kept, -1 = within MARGIN of the threshold (not a test case)."""
	hi, lo = ref['ss'] + ss_bound(ref, cnt), ref['ss'] - ss_bound(ref, cnt)
	thr = CLEAR * ref['raw']
	return np.where(hi * MARGIN < thr, 1, np.where(lo > thr * MARGIN, 0, -1))


# ---- the fixed-point side ------------------------------------------------------------------------------------------------------------------------------------
def geometry(n, rows_pad, ns, chunks=0):
	"""Sizes of the digit planes K1 writes for rows of n cells: k-steps of 32 cells, k-steps per chunk, bytes of a dense plane, of a chunk, in all."""
	nks = (round_up(n, 16) + 31) // 32
	cks = nks if chunks <= 0 else (nks + chunks - 1) // chunks
	nchunks = (nks + cks - 1) // cks
	plane = (rows_pad // 32) * cks * 1024
	return dict(nks=nks, cks=cks, nchunks=nchunks, plane_bytes=plane, chunk_bytes=ns * plane, total=nchunks * ns * plane)


def decode_planes(buf, ns, rows_pad, nks, cks=None, plane_pitch=0, offset=0):
	"""Digit planes in the layout of csrc/nrm_gram_i8.hip -> (ns, rows_pad, cells) signed digits.

	A plane is rows_pad / 32 blocks of cks images of 1 KB; an image holds 32 cells of the block's 32 rows, 32 bytes per row as two halves of 16 cells, and the
	halves of the rows with (row >> 3) & 1 are swapped.  Three layouts:
	  whole     cks = nks (None): plane s at offset + s * (rows_pad / 32) nks KB;
	  chunked   cks < nks: chunk c -- a dense operand of cks k-steps, ns planes of (rows_pad / 32) cks KB -- at offset + c * ns * plane; cells = chunks * cks * 32;
	  block     plane_pitch: these rows are a block inside a larger quantised matrix whose planes lie plane_pitch bytes apart; offset: the block's first byte."""
	b = np.asarray(buf).view(np.int8).ravel()  # (int16 out: |-128| must not wrap, and 6 planes of 128 x 65 536 cells stay at 100 MB)
	cks = nks if cks is None else cks
	nchunks = (nks + cks - 1) // cks
	blocks = rows_pad // 32
	dense = blocks * cks * 1024
	stride = plane_pitch if plane_pitch else dense
	assert rows_pad % 32 == 0 and (nchunks == 1 or not plane_pitch)
	swap = ((np.arange(32) >> 3) & 1).astype(bool)
	d = np.empty((ns, rows_pad, nchunks * cks * 32), dtype=np.int16)
	for c in range(nchunks):
		for s in range(ns):
			first = offset + c * ns * dense + s * stride
			img = b[first:first + dense].reshape(blocks, cks, 32, 2, 16).astype(np.int16)
			img[:, :, swap] = img[:, :, swap][:, :, :, ::-1]
			d[s, :, c * cks * 32:(c + 1) * cks * 32] = img.transpose(0, 2, 1, 3, 4).reshape(rows_pad, cks * 32)
	return d


def integers(d):
	"""The integers the digits stand for: sum_s 256^s d_s."""
	return sum(d[s].astype(np.int64) << (8 * s) for s in range(d.shape[0]))


def compare_digits(d, out, exps, rows, n, ns):
	"""Decoded digits against `out` and `exps` of the same call: the integer equals rint(out 2^-exps) bit for bit on every row and cell of the planes, lower
	digits within +-128, the top digit within +-64, padding rows and cells from n on exactly zero (stated on their own: K2 reads them whatever `out` holds)."""
	cells = d.shape[2]
	w = _nonzero(np.abs(d[:, rows:]).max(axis=0), 'digits: padding row', (rows, 0)) or _nonzero(np.abs(d[:, :, n:]).max(axis=0), 'digits: padding cell', (0, n))
	if w:
		return w
	if ns > 1 and np.abs(d[:-1]).max() > 128:
		return Worst(np.inf, tuple(int(v) for v in np.argwhere(np.abs(d[:-1]) > 128)[0]), 'digits: lower digit beyond +-128')
	if np.abs(d[-1]).max() > 64:
		return Worst(np.inf, tuple(int(v) for v in np.argwhere(np.abs(d[-1]) > 64)[0]), 'digits: top digit beyond +-64')
	o = np.zeros((d.shape[1], cells))
	out = np.asarray(out)
	w_ = min(cells, out.shape[1])
	o[:, :w_] = out[:, :w_]
	want, _ = model.quantise(o, ns, sh=np.asarray(exps, dtype=np.int64))
	return _nonzero(integers(d) - want, 'digits: integer != rint(out 2^-exps)') or Worst(0.0, None, 'digits')


def compare_exps(exps, out, ref, cnt, ns):
	"""The two properties of a row's fixed-point exponent, T = 2^(exps + 8 ns - 2):
	  1. T exceeds K1's own largest |out| of the row (every row of `out`, padding included; skipped when the call kept no fp64 output);
	  2. T is never looser than 2 max(RES_LOOSE rms, max) of the reference's residuals.  The kernel either takes the true maximum M' of its own residuals
	     (T <= 2 M', M' <= max + E with E the largest bound of a residual of the row) or accepts the bound m with m^2 n <= RES_LOOSE^2 est, est = |x|^2 - a.b
	     evaluated in fp64 (T <= 2 m; est is held to gamma(c_a + nc + 3) (|x|^2 + a_abs . b_abs) of the reference's, which is added).
	     A row whose reference residuals AND error bound are zero (a zero row) has no scale: its exponent is -(8 ns - 2), as model.quantise gives it."""
	rows, n, B = ref['rows'], ref['n'], 8 * ns - 2
	exps = np.asarray(exps, dtype=np.int64)
	T = np.ldexp(1.0, exps + B)
	ws = []
	if out is not None:
		mx = np.abs(np.asarray(out)).max(axis=1)
		with np.errstate(invalid='ignore'):
			ws.append(_worst(np.where(mx < T, 0.0, 1.0), np.zeros_like(T), 'exps: 2^(exps + 8 NS - 2) does not exceed max |out|'))
	E = (gamma(cnt['res'], cnt['terms']) * ref['res_abs']).max(axis=1)
	M = ref['max'] + E
	est = np.maximum(ref['ss'], ref['est'] + gamma(cnt['a'] + ref['nc'] + 3, cnt['terms']) * ref['est_abs'])
	allowed = 2 * np.maximum(RES_LOOSE * np.sqrt(est / n), M).astype(np.float64)
	zero = np.asarray(M == 0)
	ws.append(_worst(np.where(zero, 0.0, T[:rows]), np.where(zero, 1.0, allowed), 'exps: looser than 2 max(RES_LOOSE rms, max)'))
	ws.append(_worst(np.where(zero, np.abs(exps[:rows] + B), 0), np.zeros(rows), 'exps: zero row'))
	return worst_of(*ws)


def compare_fix(fix, d, exps, ss, n, ns, rows):
	"""The row records (csrc/nrm_fix.h) of ALL rows against model.row_stats of the decoded digits.
	  [0 .. ns-2]  u_s = 2^sh 256^s S_s: integers times powers of two, bit-equal;  [ns-1 .. 4]  zero.
	  [5] c, [6] g, [7] 2^(sh + B) sqrt(n) / |x~|: the device forms them from ss (K1's fp64 sum of squares), the model from the integers q:
	      |sum q^2 - ss 4^-sh| <= sum |q| + n / 4 (each q is within 1/2 of res 2^-sh), so they agree to rel = (sum |q| + n / 4) / (2 sum q^2), plus 8 u for the
	      square roots and products; the device's variance max_s (Q_s - S_s^2 / n) carries one rounding of S^2 / n and one of the difference, 2 u max Q / V.
	  Rows with ss == 0 (zero rows, padding rows) have an all-zero record."""
	fix, ss, exps = np.asarray(fix), np.asarray(ss), np.asarray(exps, dtype=np.int64)
	w = _nonzero(fix[rows:], 'fix: padding row', (rows, 0))
	if w:
		return w
	worst = Worst(0.0, None, 'fix')
	B = 8 * ns - 2
	for i in range(rows):
		dr = [d[s, i, :n].astype(np.int64) for s in range(ns)]
		q = integers(d[:, i, :n])
		st = model.row_stats(dr, q, int(exps[i]), n, ns)
		if not np.array_equal(fix[i, :ns - 1], np.array(st['u'])) or (fix[i, ns - 1:5] != 0).any():
			return Worst(np.inf, (i, ), 'fix: digit sums')
		if not ss[i] > 0:
			if (fix[i] != 0).any():
				return Worst(np.inf, (i, ), 'fix: record of a row with ss == 0')
			continue
		if st['ssq'] == 0:
			return Worst(np.inf, (i, ), 'fix: ss > 0 but every digit is zero')
		rel = (float(np.abs(q).sum()) + n / 4) / (2 * st['ssq']) + 8 * U
		qmax, vmax = max(float((t * t).sum()) for t in dr[:ns - 1]), max(st['V'])
		relc = rel + (2 * U * qmax / vmax if vmax > 0 else 0.0)
		t7 = np.ldexp(2 * st['g'], B)
		for got, want, tol, what in ((fix[i, 5], st['c'], relc, 'c'), (fix[i, 6], st['g'], rel, 'g'), (fix[i, 7], t7, rel, 'max / rms')):
			w = _worst(abs(got - want), tol * want + (np.sqrt(2 * U * qmax / st['ssq']) if what == 'c' and vmax == 0 else 0.0), 'fix: ' + what)
			if w.ratio > worst.ratio:
				worst = Worst(w.ratio, (i, ), w.what)
	return worst


def margins(ref, cmax):
	"""How far the reference alone puts every row from the thresholds of the exponent choice, in the kernel's own terms: loose = m^2 n / (RES_LOOSE^2 est)
	with the bound m = max |x| + sum_c |b_c| max |C_c| (> MARGIN: swept, < 1 / MARGIN: the bound is accepted) and share = est / (EST_SHARE |x|^2)."""
	m = ref['xmax'] + (np.abs(ref['b']) * ld(cmax)[None, :]).sum(axis=1) if ref['active'] else ref['xmax']
	with np.errstate(divide='ignore', invalid='ignore'):
		loose = np.asarray(m * m * ref['n'] / (RES_LOOSE * RES_LOOSE * ref['est']), dtype=np.float64)
		share = np.asarray(ref['est'] / (EST_SHARE * ref['raw']), dtype=np.float64)
	return loose, share


# ---- the cases both test files run (the CPU file on an fp64 emulation of the kernel, the GPU file on the kernel) ----------------------------------------------
def make_rows(rng, rows, n, dtype):
	"""Rows of different scales and means (a wrong row index or a neighbour's coefficients show at once)."""
	x = rng.standard_normal((rows, n)) * np.exp(1.5 * rng.standard_normal((rows, 1))) + 2 * rng.standard_normal((rows, 1))
	return x.astype(dtype)


def make_covariates(rng, cov, n):
	"""cov: a count (an intercept first, standard normal rows after it) | 'inactive' (two all-zero rows: rank 0 with covariates present) |
	'rankdef' (an intercept, two one-hot batches that add up to it, one normal row: rank 3 of 4)."""
	if cov == 'inactive':
		return np.zeros((2, n))
	if cov == 'rankdef':
		batch = (np.arange(n) % 2 == 0).astype(np.float64)
		return np.vstack([np.ones(n), batch, 1 - batch, rng.standard_normal(n)])
	C = rng.standard_normal((cov, n))
	if cov:
		C[0] = 1.0
	return C


CELLS = [1, 3, 4, 5, 1023, 1024, 1025, 1027, 2051]
ROWS = [1, 3, 4, 5, 33, 129]
COVS = [0, 1, 4, 5, 8, 9, 17, 'inactive', 'rankdef']


def grid():
	"""(rows, n, cov, dtype, ns) of the sweep: every cell count, every row count and every covariate set at least once in each type, NS 0 / 5 / 6 in turn.
	Kept small: the cell counts at 5 rows x 5 covariates, the row counts at 1027 cells x 2 covariates, the covariate sets at 5 rows x 1027 cells."""
	cases = []
	for i, n in enumerate(CELLS):
		cases.append((5, n, 5, ('float32', 'float64')[i % 2], (6, 5, 0)[i % 3]))
		cases.append((5, n, 5, ('float64', 'float32')[i % 2], (5, 0, 6)[i % 3]))
	for i, rows in enumerate(ROWS):
		cases.append((rows, 1027, 2, ('float32', 'float64')[i % 2], (6, 5)[i % 2]))
		cases.append((rows, 1027, 2, ('float64', 'float32')[i % 2], (0, 6)[i % 2]))
	for i, cov in enumerate(COVS):
		cases.append((5, 1027, cov, ('float32', 'float64')[i % 2], (6, 5, 0)[i % 3]))
		cases.append((5, 1027, cov, ('float64', 'float32')[i % 2], (5, 0, 6)[i % 3]))
	cases.append((6, 1024, 769, 'float64', 6))  # dynamic LDS beyond 48 KiB: more than 768 covariates
	cases.append((5, 65536, 16, 'float32', 6))  # the non-temporal instantiation: fp32, more than 4 covariates, nc n 8 >= 8 MiB
	cases.append((5, 65536, 16, 'float32', 5))
	cases.append((4, 1024, 1, 'float32', 5))  # (the instantiations the sweep above leaves out: test_every_instantiation_has_a_case)
	cases.append((4, 1024, 1, 'float64', 6))
	return cases


def scalar_cases():
	"""(rows, n, cov, dtype) of the scalar fallback k_residualize<T>: the direct entry with a row pitch that breaks the 16-byte alignment."""
	return [(5, 1027, 5, 'float32'), (5, 1027, 2, 'float64'), (3, 257, 0, 'float32'), (6, 300, 9, 'float64'), (1, 1, 1, 'float64')]


def scalar_inputs(c):
	rng = np.random.default_rng(list(c[:2]))
	return make_rows(rng, c[0], c[1], c[3]), make_covariates(rng, c[2], c[1])


def instantiation(dtype, n, nc, rank, ns, vec=True):
	"""The kernel launch_residualize (csrc/nrm_residualize.hip) picks, restated from its conditions: the scalar kernel when a pitch or a pointer is not
	16-byte aligned; else CB = 4 up to four covariates and 8 beyond, NS as asked, and non-temporal row loads for digit output from fp32 rows against active
	covariates of at least 8 MiB."""
	T = 'float' if dtype == 'float32' else 'double'
	if not vec:
		return 'k_residualize<%s>' % T
	cb = 4 if nc <= 4 else 8
	nt = ns in (5, 6) and cb == 8 and rank > 0 and nc > 0 and T == 'float' and nc * n * 8 >= (8 << 20)
	return 'k_residualize_v4<%s, %d, %d%s>' % (T, cb, ns, ', true' if nt else '')


def all_instantiations():
	"""Every kernel the launcher can reach (the non-temporal loads are asked for fp32 rows only)."""
	names = set()
	for T in ('float', 'double'):
		names.add('k_residualize<%s>' % T)
		for cb in (4, 8):
			for ns in (0, 5, 6):
				names.add('k_residualize_v4<%s, %d, %d>' % (T, cb, ns))
	return names | {'k_residualize_v4<float, 8, 5, true>', 'k_residualize_v4<float, 8, 6, true>'}


def case_id(c):
	return 'r%d-n%d-c%s-%s-ns%d' % (c[0], c[1], c[2], c[3][5:], c[4])


def case_inputs(c):
	"""(x, C) of a grid case, from a seed of its own."""
	rows, n, cov, dtype, ns = c
	rng = np.random.default_rng([rows, n, ns, dtype == 'float64', sum(map(ord, str(cov)))])
	return make_rows(rng, rows, n, dtype), make_covariates(rng, cov, n)


def exponent_rows(n=2051):
	"""The designated rows of the exponent test with their covariates (an intercept and a row uniform in [-1, 1]), every row at least MARGIN from
	RES_LOOSE and from the EST_SHARE rule by the reference alone (tests/test_k1_longdouble_cpu.py verifies it).  Groups of four rows, one decision each:
	  0-3   tight: +-[0.98, 1] (max / rms about 1: the bound is accepted)
	  4-7   1e4 + noise beside the intercept: the bound is 1e4 times too loose, the group is swept
	  8-11  one such row (9) among three tight ones: the group takes ONE decision, so the tight neighbours are swept as well
	  12-15 tight rows, among them one the covariates explain completely (13) and a zero row (14): both fail the share rule, the group is swept
	Returns (x fp64, C, kind per row: 'tight' | 'loose' | 'explained' | 'zero')."""
	rng = np.random.default_rng(2051)
	C = np.vstack([np.ones(n), rng.uniform(-1, 1, (1, n))])
	tight = lambda k: rng.choice([-1.0, 1.0], (k, n)) * rng.uniform(0.98, 1.0, (k, n))
	loose = lambda k: 1e4 + rng.standard_normal((k, n))
	x = np.vstack([tight(4), loose(4), tight(1), loose(1), tight(2), tight(1), 2.5 * C[1:2] + 3.0, np.zeros((1, n)), tight(1)])
	kind = ['tight'] * 4 + ['loose'] * 4 + ['tight', 'loose', 'tight', 'tight'] + ['tight', 'explained', 'zero', 'tight']
	# every tight row is scaled so that 1 lies between its largest |residual| and the bound m (their geometric mean is 1): the bound's exponent is then
	# one above the true maximum's, and the exponent K1 writes tells which of the two it took
	C64, dci, rank = prepare(C)
	ref = reference(x, C64, dci, rank)
	m = ref['xmax'] + (np.abs(ref['b']) * np.abs(C64).max(axis=1)[None, :]).sum(axis=1)
	for i, kd in enumerate(kind):
		if kd == 'tight':
			x[i] *= float(1 / np.sqrt(ref['max'][i] * m[i]))
	return x, C, kind


def wide_rows(rows, n, dtype, const_last):
	"""Design rows and covariates of a k_residualize_wide case: ordinary rows, and -- from 5 rows on, fp64 -- a copy of covariate 1 (row 1), a constant row
	beside the intercept (row 2: both must come back cleared) and covariate 1 plus 1e-9 of noise (row 3: 1e-18 of its norm is left, NOT cleared).
	const_last: the intercept is the LAST covariate and its product sits in column 31 of ga."""
	rng = np.random.default_rng([rows, n, const_last, dtype == 'float64'])
	nc = min(3, n)
	C = rng.standard_normal((nc, n))
	C[nc - 1 if const_last else 0] = 1.0
	x = make_rows(rng, rows, n, 'float64')
	if rows >= 5 and nc == 3 and dtype == 'float64':
		x[1] = C[1]
		x[2] = 3.25
		x[3] = C[1] + 1e-9 * rng.standard_normal(n)
	return x.astype(dtype), C


def wide_products(x, C, const_last):
	"""ga (rows, 32) as nrm_design_products lays it out (fp64 products; the last covariate in column 31 when const_last) and the same products (rows, nc)."""
	a = np.asarray(x, dtype=np.float64) @ np.asarray(C, dtype=np.float64).T
	ga = np.zeros((a.shape[0], 32))
	nc = a.shape[1]
	for q in range(nc):
		ga[:, 31 if (const_last and q == nc - 1) else q] = a[:, q]
	return ga, a
