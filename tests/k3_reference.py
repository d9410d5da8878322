"""Reference of K3 (csrc/nrm_sweep.hip, csrc/nrm_fix.h, csrc/nrm_pvalue.h), its problem builders and the comparators of its outputs -- TEST INFRASTRUCTURE ONLY.

Plain numpy in longdouble (64-bit mantissa on x86: unit roundoff 2^-64), mpmath at 60 digits for P-values (tests/golden/make_pvalue_grid.pval, the function G12
was made with).  K3's inputs are the Gram products `dot`, the sums of squares `ss`, the 8-double row records of nrm_fix.h and the scalars n_cells and dof; the
reference is written from the definitions in nrm_fix.h's header comment and the reference lines nrm_sweep.hip quotes, not from the kernels' loops:

    corr_ij = (1/n) sum_{s+t <= NS-2} u_i[s] u_j[t]          (every term, no prefix sums)          d' = d + corr
    v = ss, 0 -> n                R^2 = d'^2 / (vx vy)         stat = d'/n (kind 0) | d'/vx (kind 1)   r = d' / sqrt(vx vy)
    t = copysign(sqrt(dof min(R^2, 1) / (1 - min(R^2, 1))), d')                  p = I_{fl(1 - R^2)}(dof/2, 1/2)
    symmetric problems read the upper triangle only; their diagonal is exactly 0 in every output.

Running-error bounds of the fp64 evaluation (u = 2^-53, gamma(c) = c u / (1 - c u); 16 2^-64 of every value is added for the reference's own error).  The
count for d' is C_CORR = 11: four additions of the prefix sums V_j[m] = sum_{t<=m} u_j[t], five fmas, the rounding of 1/n, one product with it -- all
of these on terms bounded by corr_abs = (1/n) sum |u_i[s]| |u_j[t]| -- and ONE sum d + corr (u |d'|):
    |dd'|  <= gamma(11) corr_abs + u |d'|                      (no records: d' = d, no error at all)
    stat:     |dd'| / v + u |stat|                              (one division)
    R^2:      (2 |d'| |dd'| + dd'^2) / (vx vy) + 3 u R^2        (two products, one division)
    r:        |dd'| / sqrt(vx vy) + 4 u |r|                      (product, square root counted as TWO roundings -- not assumed correctly rounded --, division)
    t:        1.01 sqrt(dof) (1 - rc)^-3/2 |dd'| / sqrt(vx vy) + u |t| (4 + 2 / (1 - rc)),  rc = min(R^2, 1)      (R^2 and t: plus the fp64 underflow of d'^2)
              (dt/dr = sqrt(dof) (1 - r^2)^-3/2; the three roundings of R^2 are amplified by 1 / (2 (1 - rc)); dof rc, 1 - rc and the quotient are halved by
              the square root, which adds its two)
fp32 outputs add 2^-24 |value| + 2^-150.  A bound the device exceeds is a finding about the kernel, not a reason to widen the bound.

The guard (nrm_fix.h), per pair in longdouble: dr = K c_i c_j + g_i + g_j, num = dr (sqrt(dof) + dof |r|), den = max(1 - R^2, 1e-150)^2.  The kernels take |r|
from a float square root scaled by 1.0000002f: (float)R^2 rounds by 2^-24 (2^-25 after the root), sqrtf by 2^-24, the product by 2^-24 -- 1.5e-7 in all,
below the 2.38e-7 of the factor, so the kernel's |r| lies in [|r|, |r| (1 + 4e-7)].  num_lo takes the true |r|, num_hi takes |r| (1 + 4e-7); a pair is OVER when
num_lo > budget den (1 + 1e-9), UNDER when num_hi < budget den (1 - 1e-9), else UNDECIDED (the guard cases are built so that no pair is; asserted on the CPU).
What the kernels publish depends on how pairs are mapped to threads (a thread counts its zero-P pairs over the budget ONCE, after testing the smallest
(|r| - dr)^2 among them; a thread whose worst combination of c, g and R^2 is within the budget certifies all its pairs at once), so the reference gives intervals:
    hits  in [N_nz + (1 if N_z else 0), N_nz + N_z]     N_nz: over pairs with a non-zero stored P, N_z: over pairs with zero stored P that fail the exemption
    worst in [(1 - 1e-5) max num_lo/den over (under pairs and over pairs with non-zero P),
              (1 + 1e-5) max over (64-row tile x column) of the bound at that tile-column's max c, max g, max R^2 -- the bound is monotone in all three]
The 1e-5: (float)num and (float)den 2^-24 each, __fdividef 2.5 ulp = 3e-7, the 1.0000002 on |r| 4e-7: 8.2e-7 in all."""
import collections
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tools'))
import i8_error_model as model  # noqa: E402

LD = np.longdouble
U = 2.0**-53
ULD = 2.0**-64
TILE = 64
STRIDE = 8
C_CORR = 11  # roundings on the way to corr (module docstring)
UMAX = 1.5  # nrm_pvalue_plan: the series' range in u = -ln(1 - R^2) (plans with dof/2 >= 8)

SCALARS = [(16, 11), (32, 16), (4096, 4093), (8192, 8189), (524288, 524280)]  # no fast path; a = 8; ordinary; R^2 >= 1/4 => P = 0 up front; the workload's cells
SYM_NG = [1, 31, 33, 64, 65, 130, 200]
RECT = [(1, 1), (64, 63), (65, 130)]
MIRROR = [(70, 130, 130, 0), (37, 130, 140, 5)]  # (mx, my, r0, c0)
NSS = [0, 5, 6]
DE = [(0, 1), (1, 31), (3, 5)]  # (nc, nx)
DE_NY = 257

Worst = collections.namedtuple('Worst', 'ratio where what')


def ld(a):
	return np.asarray(a, dtype=LD)


def gamma(c):
	return c * U / (1.0 - c * U)


def worst(err, bound, what):
	"""Largest err / bound and its index; a non-zero (or NaN) error against a zero bound is infinite."""
	err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
	if err.size == 0:
		return Worst(0.0, None, what)
	with np.errstate(divide='ignore', invalid='ignore'):
		ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
	ratio = np.where(np.isnan(ratio), np.inf, ratio)
	i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
	return Worst(float(ratio[i]), tuple(int(v) for v in i), what)


def same_bits(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
	return a.view('u%d' % a.dtype.itemsize) == b.view('u%d' % b.dtype.itemsize)


def bits(got, want, what):
	"""Worst(inf) at the first element whose bit pattern differs, else Worst(0)."""
	bad = np.argwhere(~same_bits(got, want))
	if bad.size:
		return Worst(np.inf, tuple(int(v) for v in bad[0]), what)
	return Worst(0.0, None, what)


# ---- problems ------------------------------------------------------------------------------------------------------------------------------------------------
class Problem:
	"""sym: dot is (ng, ng) and symmetric on the host (the device gets NaN below the diagonal), ssx is ssy, fx is fy.  fx / fy: (rows, 8) records or None."""

	def __init__(self, **k):
		self.__dict__.update(k)

	@property
	def top(self):
		return self.ns - 2

	def pairs(self):
		"""Mask of the pairs of the problem (symmetric: off the diagonal, both triangles)."""
		m = np.ones((self.nx, self.ny), dtype=bool)
		if self.sym:
			m &= ~np.eye(self.nx, dtype=bool)
		return m

	def copy(self):
		"""A private copy (problem() caches its results): sym keeps ssx is ssy and fx is fy."""
		ssx, fx = self.ssx.copy(), None if self.fx is None else self.fx.copy()
		return Problem(sym=self.sym, nx=self.nx, ny=self.ny, n=self.n, dof=self.dof, ns=self.ns, exact=self.exact, dot=self.dot.copy(), ssx=ssx,
					   ssy=ssx if self.sym else self.ssy.copy(), fx=fx, fy=fx if self.sym else (None if self.fy is None else self.fy.copy()), plants=dict(self.plants))

	def set_r(self, i, j, r):
		"""Give the pair (i, j) the Pearson r it would have after the correction."""
		vx, vy = (self.ssx[i] or float(self.n)), (self.ssy[j] or float(self.n))
		c = float(_corr(self.fx[i:i + 1], self.fy[j:j + 1], self.ns, self.n)[0][0, 0]) if self.ns else 0.0
		self.dot[i, j] = r * math.sqrt(vx * vy) - c
		if self.sym:
			self.dot[j, i] = self.dot[i, j]

	def sub(self, r0, r1, c0, c1, sym):
		"""Rows [r0, r1) against columns [c0, c1) of a symmetric problem as a problem of its own (what the pipelined coex hands to the sweeps)."""
		f = self.fx
		return Problem(sym=sym, nx=r1 - r0, ny=c1 - c0, n=self.n, dof=self.dof, ns=self.ns, exact=self.exact, dot=np.ascontiguousarray(self.dot[r0:r1, c0:c1]),
					   ssx=self.ssx[r0:r1].copy(), ssy=self.ssy[c0:c1].copy(), fx=None if f is None else f[r0:r1].copy(), fy=None if f is None else f[c0:c1].copy(),
					   plants={})


def _corr(fx, fy, ns, n, dtype=LD):
	"""(corr, corr_abs): every term of sum_{s+t <= NS-2} u_i[s] u_j[t] / n."""
	nx, ny = fx.shape[0], fy.shape[0]
	c, ca = np.zeros((nx, ny), dtype=dtype), np.zeros((nx, ny), dtype=dtype)
	ux, uy = np.asarray(fx[:, :5], dtype=dtype), np.asarray(fy[:, :5], dtype=dtype)
	for s in range(ns - 1):
		for t in range(ns - 1 - s):
			c += np.outer(ux[:, s], uy[:, t])
			ca += np.outer(np.abs(ux[:, s]), np.abs(uy[:, t]))
	return c / dtype(n), ca / dtype(n)


def _solve_d(target, corr):
	"""The double d with fl(d + corr) == target (consecutive d give consecutive sums while |corr| stays below |target|'s binade)."""
	d = np.float64(target) - np.float64(corr)
	for k in range(17):
		for cand in ((d, ) if k == 0 else (_step(d, k), _step(d, -k))):
			if cand + np.float64(corr) == np.float64(target):
				return cand
	raise AssertionError('no double d with fl(d + %r) == %r' % (corr, target))


def _step(x, k):
	for _ in range(abs(k)):
		x = np.nextafter(x, np.inf if k > 0 else -np.inf)
	return x


def _positions(sym, nx, ny):
	"""name -> (i, j) of the planted pairs, the rows whose ss is the power of two pw, the zero-ss rows, the zero-record column, the duplicate:
	last row and column, both sides of the tile boundary 63 | 64 (of the piece boundary 31 | 32 in smaller problems)."""
	P, pw_x, pw_y = {}, [], []
	info = dict(ss0_x=None, ss0_y=None, zcol=None, dup=None, one=None)
	if ny < 12 or (sym and nx < 12):
		if not sym:
			P['q_eq'] = (0, 0)
			pw_x, pw_y = [0], [0]
		return P, pw_x, pw_y, info
	Ly = ny - 1
	q = 63 if ny >= 66 else (31 if ny >= 34 else ny // 2 - 1)
	if sym:
		dst = q + 7
		P.update(zero=(0, Ly), under=(3, Ly - 1), q_lo=(q, q + 1), q_eq=(q, q + 2), q_hi=(q + 1, q + 2), u_lo=(1, Ly - 1), u_hi=(2, Ly), one=(5, dst),
				 one_plus=(Ly - 1, Ly))
		pw_x = pw_y = [q, q + 1, q + 2]
		info.update(ss0_x=7, ss0_y=7, zcol=3, dup=(5, dst), one=(5, dst))
		spread = [(8 + k, Ly - 3 - k) for k in range(16)]
	else:
		Lx = nx - 1
		x0, x1 = min(63, Lx), min(64, Lx)
		P.update(zero=(0, Ly), under=(Lx, 3), q_lo=(x0, q), q_eq=(x0, q + 1), q_hi=(x1, q + 2), u_lo=(0, 1), u_hi=(Lx, Ly - 1), one=(0, 5), one_plus=(Lx, Ly))
		pw_x, pw_y = sorted({x0, x1}), [q, q + 1, q + 2]
		info.update(ss0_x=2 if (nx >= 5 and 2 not in (x0, x1)) else None, ss0_y=7, zcol=3, dup=(10, 11), one=(0, 5))
		spread = [(k % nx, 12 + k) for k in range(16) if 12 + k < Ly - 2]
	used = set(P.values())
	for k, (i, j) in enumerate(spread):
		if (i, j) in used or (sym and not i < j) or j in pw_y or (sym and i in pw_y) or j == info['ss0_y'] or i == info['ss0_x'] or (sym and (i == 7 or j == 7)):
			continue
		used.add((i, j))
		P['spread%d' % k] = (i, j)
	return P, pw_x, pw_y, info


def _targets(dof):
	"""R^2 of the spread plants: a ln(1 - R^2) evenly spread over [-740, -2] (ln P to first order), capped at 0.999."""
	a = dof / 2.0
	return [min(-math.expm1(-L / a), 0.999) for L in np.linspace(2.0, 740.0, 16)]


@functools.lru_cache(maxsize=None)
def problem(exact, sym, nx, ny, n, dof, ns, seed=0, ones=True):
	"""exact: inputs on which the fp64 result is reproducible on the host bit for bit -- n a power of two, record entries u[s] = S_s 256^s 2^-26 with integer
	|S_s| <= 2^8, so that every partial sum of the correction is an integer multiple of 2^-52 below 2^-1 (53 bits: exact in any order, with or without fma), d and
	ss arbitrary doubles; then d' = fl(d + corr) and R^2 = fl(fl(d' d') / fl(vx vy)) are single IEEE operations.  Otherwise: records with arbitrary real u, c and
	g log-uniform over 1e-9 ... 1e-3, the correction a third of |x||y|.  Both plant the pairs of _positions.  Treat the result as read-only (it is cached)."""
	assert n & (n - 1) == 0
	rng = np.random.default_rng([seed, int(exact), int(sym), nx, ny, n, ns])
	pw = 4.0 / n if exact else float(n)  # the scale of ss, a power of two (exact: |corr| < 0.4 / n stays below the planted d' = pw / 2)
	ssx = pw * rng.uniform(0.5, 2.0, nx)
	ssy = ssx if sym else pw * rng.uniform(0.5, 2.0, ny)

	def records(rows):
		if not ns:
			return None
		f = np.zeros((rows, STRIDE))
		if exact:
			S = rng.integers(-256, 257, (rows, 5)).astype(np.float64)
			f[:, :5] = np.ldexp(S, 8 * np.arange(5) - 26)
		else:
			f[:, :5] = rng.normal(size=(rows, 5)) * math.sqrt(pw * n) * 0.3
		f[:, ns - 1:5] = 0.0
		f[:, 5] = 10.0**rng.uniform(-9, -3, rows)
		f[:, 6] = 10.0**rng.uniform(-9, -3, rows)
		f[:, 7] = 1.0
		return f

	fx = records(nx)
	fy = fx if sym else records(ny)
	P, pw_x, pw_y, info = _positions(sym, nx, ny)
	if not ones:  # (guard cases: an R^2 at 1 makes the estimate of its tile-column, and with it the upper end of `worst`, astronomically large)
		P = {k: v for k, v in P.items() if k not in ('one', 'one_plus', 'spread14', 'spread15')}  # (the last two: P among the subnormals, where zero or not is undecidable)
	# ss first: every d below is solved for the final variances
	ssx[pw_x] = pw
	ssy[pw_y] = pw
	if info['ss0_x'] is not None:
		ssx[info['ss0_x']] = 0.0
	if info['ss0_y'] is not None:
		ssy[info['ss0_y']] = 0.0
	if info['zcol'] is not None and ns:
		fy[info['zcol'], :5] = 0.0
	if info['one'] is not None:
		i, j = info['one']
		if exact and i not in pw_x:  # d' = ss in [1/n, 2/n): the correction, a multiple of 2^-52 / n, is then a multiple of ulp(d) and fl(d + corr) can hit it
			ssx[i] = pw * rng.uniform(0.26, 0.5)
		ssy[j] = ssx[i]
	if info['dup'] is not None:
		a, b = info['dup']
		ssy[b] = ssy[a]
		if ns:
			fy[b] = fy[a]
	vx, vy = np.where(ssx == 0, float(n), ssx), np.where(ssy == 0, float(n), ssy)
	corr = np.zeros((nx, ny)) if not ns else np.asarray(_corr(fx, fy, ns, n)[0], dtype=np.float64)  # (exact problems: exact)
	scale = np.sqrt(np.outer(vx, vy))
	r = rng.normal(size=(nx, ny)) * min(1.5 / math.sqrt(dof + 1), 0.3)
	strong = rng.random((nx, ny)) < 0.1
	r = np.where(strong, rng.uniform(0.3, 0.9, (nx, ny)) * np.sign(r), np.clip(r, -0.95, 0.95))
	if not ones:  # (guard cases: no R^2 whose P-value lies among the subnormals, a ln(1 - R^2) in (-790, -650))
		lo, hi = (-math.expm1(-L / (dof / 2.0)) for L in (650.0, 790.0))
		r = np.where((r * r > lo) & (r * r < hi), np.sign(r) * math.sqrt(min(1.1 * hi, 0.9)), r)
	dot = r * scale - corr
	if info['dup'] is not None:
		a, b = info['dup']
		dot[:, b] = dot[:, a]
	if sym:
		dot = np.triu(dot, 1) + np.triu(dot, 1).T
		if info['dup'] is not None:
			a, b = info['dup']
			dot[b, :] = dot[a, :]
			dot[:, b] = dot[:, a]
			dot = np.triu(dot, 1) + np.triu(dot, 1).T
		dot[np.arange(nx), np.arange(nx)] = ssx  # (what a Gram has there; K3 must not read it into any output)
	thr = -math.expm1(-UMAX)
	tg = _targets(dof)
	for name, (i, j) in P.items():
		s = math.sqrt(vx[i] * vy[j])
		if name == 'zero':
			d = 0.0 - corr[i, j]  # (+0 without records)
		elif name == 'under':
			assert corr[i, j] == 0
			d = 1e-170
		else:
			if name.startswith('q_'):
				assert vx[i] == pw and vy[j] == pw
				want = pw * {'q_lo': 0.5 - 2.0**-54, 'q_eq': 0.5, 'q_hi': 0.5 + 2.0**-52}[name]
			elif name == 'one':
				assert vx[i] == vy[j]
				want = vx[i]
			elif name == 'one_plus':
				want = s * math.sqrt(1 + 5e-9)
			elif name == 'u_lo':
				want = -s * math.sqrt(thr * (1 - 1e-12))
			elif name == 'u_hi':
				want = s * math.sqrt(thr * (1 + 1e-12))
			else:
				k = int(name[6:])
				want = s * math.sqrt(tg[k]) * (-1 if k & 1 else 1)
			solve = exact and (name.startswith('q_') or name == 'one')
			if solve and corr[i, j] < 0:  # (d' takes the correction's sign: |d| < |d'|, so the doubles around d are at least as dense as those around d')
				want = -want
			# (only the R^2 = 1/4 and R^2 = 1 plants need their d' hit exactly; the others are whatever fl(d + corr) makes of them, the host computes the same)
			d = _solve_d(want, corr[i, j]) if solve else want - corr[i, j]
		dot[i, j] = d
		if sym:
			dot[j, i] = d
	return Problem(sym=sym, nx=nx, ny=ny, n=n, dof=float(dof), ns=ns, exact=exact, dot=dot, ssx=ssx, ssy=ssy, fx=fx, fy=fy, plants=P)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------------------
def reference(pb, dot=None):
	"""Every output of the problem in longdouble with its fp64 running-error bound (module docstring); exact problems: the fp64 values as well (d64, r2_64,
	stat64[kind]), computed with single IEEE operations."""
	n, dof = LD(pb.n), LD(pb.dof)
	d = ld(pb.dot if dot is None else dot)
	if pb.sym:
		d = np.triu(d, 1) + np.triu(d, 1).T
	vx, vy = ld(np.where(pb.ssx == 0, float(pb.n), pb.ssx)), ld(np.where(pb.ssy == 0, float(pb.n), pb.ssy))
	vv = np.outer(vx, vy)
	if pb.ns:
		corr, corr_abs = _corr(pb.fx, pb.fy, pb.ns, pb.n)
		d1 = d + corr
		e_d = gamma(C_CORR) * corr_abs + U * np.abs(d1)
	else:
		d1, e_d = d, np.zeros(d.shape, dtype=LD)
	off = pb.pairs()
	if pb.exact:  # d' = fl(d + corr) is known: r and t (and the R^2 the guard reads) follow from IT, with no error on the way in
		d64 = np.asarray(pb.dot if dot is None else dot, dtype=np.float64)
		if pb.sym:
			d64 = np.triu(d64, 1) + np.triu(d64, 1).T
		if pb.ns:
			d64 = d64 + np.asarray(_corr(pb.fx, pb.fy, pb.ns, pb.n, np.float64)[0])  # ONE rounding: the correction is exact
		d64 = np.where(off, d64, 0.0)
		d1, e_d = ld(d64), np.zeros(d.shape, dtype=LD)
	d1, e_d = np.where(off, d1, 0), np.where(off, e_d, 0)
	with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
		r2 = d1 * d1 / vv
		rc = np.minimum(r2, 1)
		om = 1 - rc
		sv = np.sqrt(vv)
		out = dict(stat0=d1 / n, stat1=d1 / vx[:, None], r=d1 / sv, t=np.where(off, np.copysign(np.sqrt(dof * rc / om), d1), 0), r2=r2)
		own = 16 * ULD
		b = dict(stat0=e_d / n + (U + own) * np.abs(out['stat0']), stat1=e_d / vx[:, None] + (U + own) * np.abs(out['stat1']),
				 r2=(2 * np.abs(d1) * e_d + e_d * e_d) / vv + (3 * U + own) * r2, r=e_d / sv + (4 * U + own) * np.abs(out['r']))
		# fp64 underflow (the planted d' = 1e-170): a subnormal d'^2 and a subnormal quotient are each off by up to 2^-1075; |sqrt(a + e) - sqrt(a)| <= sqrt(e)
		tiny = LD(2.0)**-1075 * (1 + 1 / vv)
		b['r2'] = b['r2'] + tiny
		b['t'] = np.where(om > 0, 1.01 * np.sqrt(dof) * om**LD(-1.5) * e_d / sv + np.abs(out['t']) * (U * (4 + 2 / om) + own) + np.sqrt(1.01 * dof * tiny), 0)
	ref = dict(out=out, bound=b, d1=d1, e_d=e_d, off=off)
	if pb.exact:
		v64x, v64y = np.where(pb.ssx == 0, float(pb.n), pb.ssx), np.where(pb.ssy == 0, float(pb.n), pb.ssy)
		with np.errstate(over='ignore', invalid='ignore'):
			ref.update(d64=d64, r2_64=(d64 * d64) / np.outer(v64x, v64y), stat64=[d64 / float(pb.n), d64 / v64x[:, None]])
	return ref


def out_bound(ref, name, dtype):
	b = ref['bound'][name]
	if np.dtype(dtype) == np.float32:
		b = b + 2.0**-24 * np.abs(ref['out'][name]) + 2.0**-150
	return b


def compare(got, ref, name, dtype, mask=None, exact=False):
	"""An output against its longdouble value: error / bound; infinities must agree exactly (t of R^2 >= 1)."""
	want = ref['out'][name]
	g = ld(got)
	inf = np.isinf(want)
	with np.errstate(invalid='ignore'):
		err = np.where(inf, np.where(g == want, 0, np.inf), np.abs(g - want))
	bound = out_bound(ref, name, dtype)
	if name == 't' and not exact:  # t jumps to infinity at R^2 = 1: a pair whose R^2 is within its own bound of 1 may land on either side
		near = np.abs(1 - ref['out']['r2']) <= 4 * ref['bound']['r2']
		err, bound = np.where(near, 0, err), np.where(near, 0, bound)
	if mask is not None:
		err, bound = np.where(mask, err, 0), np.where(mask, bound, 0)
	return worst(err, bound, name)


@functools.lru_cache(maxsize=None)
def _grid():
	"""tests/golden/make_pvalue_grid (needs mpmath), imported once."""
	sys.path.insert(0, os.path.join(HERE, 'golden'))
	try:
		import make_pvalue_grid
	finally:
		sys.path.pop(0)
	return make_pvalue_grid


# ---- P-values ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def p_mp(r2, dof):
	"""mpmath at 60 digits at this R^2 (a double): the function G12 was made with."""
	make_pvalue_grid = _grid()
	# Deep in the tail the 60-digit series takes seconds or gives up (R^2 = 0.1 at 262 140 degrees of freedom: P = 1e-12000).  With x = 1 - R^2,
	# I_x(a, 1/2) = x^a (1-x)^1/2 / (a B(a, 1/2)) 2F1(a + 1/2, 1; a + 1; x) <= x^a / sqrt(1 - x)  (2F1 <= 1 / (1 - x), a B(a, 1/2) >= 1 for a >= 1):
	# below e^-2000 -- 500 orders of magnitude under the smallest subnormal -- the value is 0 to every comparison made here.
	if 0 < r2 < 1 and dof >= 2 and dof / 2 * math.log1p(-r2) - 0.5 * math.log(r2) < -2000:
		return _mp().mpf(0)
	return make_pvalue_grid.pval(float(r2), float(dof))


def subset(pb, r2, limit=200):
	"""At most `limit` pairs (upper triangle of symmetric problems): the planted ones and an even spread of ln P (to first order a ln(1 - R^2)) over the rest."""
	picks = list(dict.fromkeys(pb.plants.values()))
	m = pb.pairs()
	if pb.sym:
		m &= np.triu(np.ones_like(m), 1)
	idx = np.argwhere(m)
	if idx.size:
		w = np.clip(np.asarray(r2, dtype=np.float64)[m], 0, 1 - 1e-16)
		lp = pb.dof / 2 * np.log1p(-w)
		order = np.argsort(lp)
		for L in np.linspace(0, max(-760.0, float(lp.min())), 24):
			k = order[min(np.searchsorted(lp[order], L), order.size - 1)]
			picks.append(tuple(int(v) for v in idx[k]))
	picks = list(dict.fromkeys(picks))[:limit]
	return picks


def p_tolerance(p_ref, dof):
	"""The tolerance of test_gpu_round3.test_pvalue_function_against_mpmath, unchanged: relative for p > 1e-300, else 1e-300 absolute."""
	lp = -float(_mp().log10(p_ref)) if p_ref > 0 else np.inf
	return 2e-14 + 4e-16 * np.log(10) * lp + (3e-12 if dof < 32 else 0)


def _mp():
	import mpmath
	return mpmath


def compare_p_subset(p_got, pb, r2, dtype, d_r2=None):
	"""P of the subset against mpmath at the pair's R^2 (exact problems: the host's fp64 R^2, which is the device's; real problems: the longdouble R^2 rounded
	to double, with (dof/2) |dR^2| / (1 - R^2) added for the counted bound d_r2 on the device's R^2, that rounding and the rounding of 1 - R^2)."""
	errs, bounds, where = [], [], []
	for (i, j) in subset(pb, r2):
		x = float(r2[i, j])
		ref = p_mp(x, pb.dof)
		tol = p_tolerance(ref, pb.dof) if ref > 0 else 0.0
		if d_r2 is not None and x < 1:
			# |dR^2|: the counted bound on the device's R^2, the rounding of the reference's to double, and the subtraction x = fl(1 - R^2) both sides apply first:
			# two R^2 that differ at all can land on neighbouring doubles x (half an ulp of x each)
			tol += pb.dof / 2 * (float(d_r2[i, j]) + U * x + float(np.spacing(1 - x))) / (1 - x)
		got = float(p_got[i, j])
		f32 = np.dtype(dtype) == np.float32
		if d_r2 is not None and x + 2 * float(d_r2[i, j]) >= 1:  # R^2 within its bound of 1: P is monotone, so 0 <= p <= P(R^2 - bound) is all that holds
			errs.append(got if got >= 0 else np.inf)
			bounds.append(float(p_mp(max(x - 2 * float(d_r2[i, j]) - 2 * U, 0.0), pb.dof)) * (1 + 1e-6) + 1e-300)
			where.append((i, j))
			continue
		if ref > 1e-300:
			errs.append(abs(got - float(ref)))
			bounds.append(tol * float(ref) + (2.0**-24 * float(ref) + 2.0**-150 if f32 else 0))
		else:
			errs.append(abs(got - float(ref)))
			bounds.append(1e-300 + (2.0**-149 if f32 else 0))
		where.append((i, j))
	w = worst(np.array(errs), np.array(bounds), 'p (mpmath subset)')
	return Worst(w.ratio, where[w.where[0]] if w.where else None, w.what)


# ---- placement -----------------------------------------------------------------------------------------------------------------------------------------------
def placement(buf, written, what):
	"""buf: a NaN-pre-filled output as it came back (any shape); written: mask of the elements the call must write.  No NaN inside, only NaN outside (callers
	with NaN among the expected results pass the expectation's own mask)."""
	nan = np.isnan(buf)
	bad = np.argwhere(nan == written)
	if bad.size:
		return Worst(np.inf, tuple(int(v) for v in bad[0]), what + (': not written' if written[tuple(bad[0])] else ': written outside'))
	return Worst(0.0, None, what)


def symmetric_zero_diagonal(a, what):
	if not same_bits(a, a.T.copy()).all():
		return Worst(np.inf, tuple(int(v) for v in np.argwhere(~same_bits(a, a.T.copy()))[0]), what + ': not bitwise symmetric')
	dg = np.diagonal(a)
	if not ((dg == 0) & ~np.signbit(dg)).all():
		return Worst(np.inf, None, what + ': diagonal not +0')
	return Worst(0.0, None, what)


# ---- the guard -----------------------------------------------------------------------------------------------------------------------------------------------
def _nonzero_class(r2, dof, dtype):
	"""(+1 | -1 | 0): the P-value at this R^2 is surely non-zero / surely zero as stored in dtype / too close to the smallest subnormal to say (a factor 1000)."""
	mp = _mp()
	try:
		p = p_mp(r2, dof)
	except mp.libmp.libhyper.NoConvergence:  # (the 60-digit series gives up on some P-values of order one at 262 140 degrees of freedom: zero they are not)
		from scipy import special
		p = mp.mpf(float(special.betainc(dof / 2, 0.5, 1.0 - r2)))
		assert p > 1e-100
	lim = mp.mpf(2)**(-1075 if np.dtype(dtype) == np.float64 else -150)
	if p > (mp.mpf(2e-300) if np.dtype(dtype) == np.float64 else lim * 1000):  # (below 1e-300 G12 holds the device's function to 1e-300 absolute only)
		return 1
	if p < lim / 1000:
		return -1
	return 0


def guard_reference(pb, ref, budget, domain, dtype):
	"""domain: 'unordered' (symmetric problem, upper triangle: k_assoc_sweep_sym), 'ordered' (symmetric, both triangles: k_assoc_sweep) or 'rect'.
	dtype: of the stored P whose being zero decides between counting and the exemption test (the generic kernel tests the fp64 P: pass float64).
	Returns the classes, the intervals of hits and worst and the number of undecided pairs (classification or zero-ness)."""
	dof = LD(pb.dof)
	K = LD(model.k_const(pb.ns))
	cx, gx, cy, gy = (ld(v) for v in (pb.fx[:, 5], pb.fx[:, 6], pb.fy[:, 5], pb.fy[:, 6]))
	dr = K * np.outer(cx, cy) + gx[:, None] + gy[None, :]
	r2 = ref['out']['r2']
	ar = np.sqrt(r2)
	den = np.maximum(1 - r2, LD(1e-150))**2
	num_lo = dr * (np.sqrt(dof) + dof * ar)
	num_hi = dr * (np.sqrt(dof) + dof * ar * (1 + LD(4e-7)))
	m = pb.pairs()
	if domain == 'unordered':
		m &= np.triu(np.ones_like(m), 1)
	over = m & (num_lo > budget * den * (1 + LD(1e-9)))
	under = m & (num_hi < budget * den * (1 - LD(1e-9)))
	undecided = int((m & ~over & ~under).sum())
	n_nz = n_z = n_ex = 0
	nz = np.zeros(m.shape, dtype=bool)
	for i, j in np.argwhere(over):
		x = float(r2[i, j])
		c = _nonzero_class(x, pb.dof, dtype)
		if c == 0:
			undecided += 1
		elif c > 0:
			n_nz += 1
			nz[i, j] = True
		else:  # the exemption: P at (|r| - dr)^2, in fp64, for either end of the kernel's |r|
			lo = [max(float(ar[i, j] * f - dr[i, j]), 0.0)**2 for f in (LD(1), 1 + LD(4e-7))]
			cs = {_nonzero_class(v, pb.dof, np.float64) for v in lo}
			if cs == {-1}:
				n_ex += 1
			elif cs == {1}:
				n_z += 1
			else:
				undecided += 1
	counted = under | nz
	with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
		w_lo = float((num_lo / den)[counted].max()) * (1 - 1e-5) if counted.any() else 0.0
		# upper end: per 64-row tile and column, the bound at the maxima of the tile-column's pairs (every thread's pairs are a subset of one)
		w_hi = 0.0
		for t0 in range(0, pb.nx, TILE):
			mm = m[t0:t0 + TILE]
			neg = LD(-1)
			cm = np.where(mm, cx[t0:t0 + TILE, None], neg).max(axis=0)
			gm = np.where(mm, gx[t0:t0 + TILE, None], neg).max(axis=0)
			rm = np.where(mm, r2[t0:t0 + TILE], neg).max(axis=0)
			has = mm.any(axis=0)
			if not has.any():
				continue
			drm = K * cm * cy + gm + gy
			bnd = drm * (np.sqrt(dof) + dof * np.sqrt(np.maximum(rm, 0)) * (1 + LD(4e-7))) / np.maximum(1 - rm, LD(1e-150))**2
			w_hi = max(w_hi, float(bnd[has].max()))
		w_hi *= 1 + 1e-5
	return dict(over=over, under=under, nz=nz, n_nz=n_nz, n_z=n_z, n_exempt=n_ex, undecided=undecided, hits=(n_nz + (1 if n_z else 0), n_nz + n_z), worst=(w_lo, w_hi),
				ratio=num_lo / den, dr=dr)


def choose_budget(pb, ref, want_over=300):
	"""A budget in the widest gap of the sorted per-pair estimates near the want_over-th largest (an input of the case, from the reference alone): no pair is
	within 1e-3 of it."""
	dof = LD(pb.dof)
	K = LD(model.k_const(pb.ns))
	dr = K * np.outer(ld(pb.fx[:, 5]), ld(pb.fy[:, 5])) + ld(pb.fx[:, 6])[:, None] + ld(pb.fy[:, 6])[None, :]
	r2 = ref['out']['r2']
	ratio = dr * (np.sqrt(dof) + dof * np.sqrt(r2)) / np.maximum(1 - r2, LD(1e-150))**2
	v = np.sort(np.asarray(ratio[pb.pairs()], dtype=np.float64))[::-1]
	lo, hi = max(want_over // 2, 1), min(2 * want_over, v.size - 1)
	k = lo + int(np.argmax(v[lo:hi] / v[lo + 1:hi + 1]))
	assert v[k] / v[k + 1] > 1.002
	return float(np.sqrt(v[k] * v[k + 1]))


GUARD_CASES = ['sym6', 'sym5', 'sym6-exact', 'rect6', 'rect5', 'mirror6', 'mirror5', 'exempt', 'large-g']


@functools.lru_cache(maxsize=None)
def guard_case(name):
	"""(problem, budget, entry): the budget sits in a gap of the per-pair estimates, so that under, over with P != 0 and over with P == 0 all occur and no
	pair is undecided (tests/test_k3_reference_cpu.py asserts both).  'exempt': rows 20 and 90 carry g = 1e-4, every other record is 1e-9, their own pair
	has R^2 = 0.6 (P = 0, also at |r| - dr) and is the only one over the budget: hits == 0.  'large-g': row 20 has g = 0.5 instead: every pair of it is over, and
	P of the strong pair is 0 at |r| = 0.775 but not at |r| - dr = 0.27: hits >= 1."""
	if name in ('exempt', 'large-g'):
		pb = problem(False, True, 130, 130, 4096, 4093, 6, ones=False).copy()
		pb.fx[:, 5:7] = 1e-9
		pb.fx[90, 6] = 1e-4
		pb.fx[20, 6] = 1e-4 if name == 'exempt' else 0.5
		rng = np.random.default_rng(5)
		for i in (20, 90):
			for j in range(130):
				if j != i and pb.ssx[j] != 0:
					pb.set_r(min(i, j), max(i, j), 0.01 * rng.uniform(0.5, 1.0))
		pb.set_r(20, 90, math.sqrt(0.6))
		return pb, 0.1, 'sym'
	kind, ns = name.split('-')[0][:-1], int(name.split('-')[0][-1])
	exact = name.endswith('exact')
	n, dof = (524288, 524280) if ns == 5 else (4096, 4093)
	if kind == 'sym':
		pb = problem(exact, True, 200, 200, n, dof, ns, seed=1 if exact else 0, ones=False)
	elif kind == 'rect':
		pb = problem(exact, False, 65, 130, n, dof, ns, ones=False)
	else:
		pb = problem(exact, False, 70, 130, n, dof, ns, ones=False)
	return pb, choose_budget(pb, reference(pb), {'sym5': 1500}.get(name, 300)), kind


def check_guard(flags, prefill, g):
	"""(hits within its interval, worst within its interval) as Worst records."""
	hits = int(flags[2]) - int(prefill)
	worst_f = float(np.asarray(flags[3], dtype=np.int32).view(np.float32))
	lo, hi = g['hits']
	wl, wh = g['worst']
	a = Worst(0.0 if lo <= hits <= hi else np.inf, None, 'hits %d in [%d, %d]' % (hits, lo, hi))
	b = Worst(0.0 if wl <= worst_f <= wh else np.inf, None, 'worst %.9g in [%.9g, %.9g]' % (worst_f, wl, wh))
	return a, b


# ---- the streaming de sweep and alpha --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def de_problem(nc, nx, n, dof, rank, seed=0):
	"""G = [y C^T (nc) | y X~^T (nx) | unused] in covariates-then-design order, ssraw = |y|^2, dci, ssx.  Rows 0-3 have |y|^2 a millionth BELOW a dci a^T (the
	clamp at 0, then the 0 -> n rule), row 4 has ssx-independent d = 0, the last row R^2 = 1/4 exactly when nothing is projected out."""
	rng = np.random.default_rng([seed, nc, nx, n, int(dof), rank])
	ny = DE_NY
	a = rng.normal(size=(ny, nc)) * math.sqrt(n)
	A = rng.normal(size=(nc, nc + 2))
	dci = np.linalg.inv(A @ A.T) / n if nc else np.zeros((0, 0))
	ssx = n * rng.uniform(0.5, 2.0, nx)
	if nx > 2:
		ssx[1] = 0.0
	q = np.einsum('yc,ce,ye->y', a, dci, a) if (nc and rank > 0) else np.zeros(ny)
	sy = n * rng.uniform(0.5, 2.0, ny)
	ssraw = q + sy
	ssraw[:4] = q[:4] * (1 - 1e-6) if (nc and rank > 0) else 0.0
	vy = np.where(np.arange(ny) < 4, float(n), sy)
	vx = np.where(ssx == 0, float(n), ssx)
	r = rng.normal(size=(ny, nx)) * min(1.5 / math.sqrt(dof + 1), 0.3)
	r = np.where(rng.random((ny, nx)) < 0.1, rng.uniform(0.3, 0.9, (ny, nx)) * np.sign(r), np.clip(r, -0.95, 0.95))
	d = r * np.sqrt(np.outer(vy, vx))
	d[4, :] = 0.0
	d[ny - 1, 0] = 0.5 * math.sqrt(vx[0] * vy[ny - 1])
	G = np.full((ny, 32), 7.0)  # (the unused columns hold a sentinel: reading one into a result shows)
	G[:, :nc] = a
	G[:, nc:nc + nx] = d
	return dict(G=G, ssraw=ssraw, dci=dci, ssx=ssx, nc=nc, nx=nx, ny=ny, n=n, dof=float(dof), rank=rank)


def de_raw(G, nc, const_last):
	"""The columns as nrm_gram_skinny leaves them: const_last -- the last covariate in column 31, the design rows one column earlier."""
	if not const_last:
		return G.copy()
	raw = G.copy()
	raw[:, nc - 1:31] = G[:, nc:32]
	raw[:, 31] = G[:, nc - 1]
	return raw


def de_reference(dp):
	"""by = dci a, |y~|^2 = max(|y|^2 - a dci a^T, 0), 0 -> n, then the pair formulas with d = G[y, nc + x]; outputs are (nx, ny).  Bounds: by gamma(nc) |dci||a|;
	the quadratic form gamma(2 nc) |a||dci||a| plus u for the difference; the variance's relative error e_v enters R^2 once, r half, t by 1 / (2 (1 - rc))."""
	nc, nx, n, dof = dp['nc'], dp['nx'], LD(dp['n']), LD(dp['dof'])
	a, D = ld(dp['G'][:, :nc]), ld(dp['dci'])
	active = nc > 0 and dp['rank'] > 0
	if active:
		by, by_abs = a @ D.T, np.abs(a) @ np.abs(D).T
		q, q_abs = (a * by).sum(axis=1), (np.abs(a) * by_abs).sum(axis=1)
	else:
		by = by_abs = np.zeros((dp['ny'], nc), dtype=LD)
		q = q_abs = np.zeros(dp['ny'], dtype=LD)
	raw = ld(dp['ssraw'])
	sy = np.maximum(raw - q, 0)
	e_sy = np.where(sy > 0, gamma(2 * nc + 1) * q_abs + U * sy, 0) if active else np.zeros_like(sy)
	margin = np.where(sy > 0, sy, q - raw) if active else None  # (how far each row is from the clamp, to be compared with e_sy by the CPU test)
	vy = np.where(sy == 0, n, sy)
	vx = ld(np.where(dp['ssx'] == 0, float(dp['n']), dp['ssx']))
	d = ld(dp['G'][:, nc:nc + nx]).T
	vv = np.outer(vx, vy)
	ev = (e_sy / vy)[None, :]
	with np.errstate(divide='ignore', invalid='ignore'):
		r2 = d * d / vv
		rc = np.minimum(r2, 1)
		om = 1 - rc
		out = dict(stat0=d / n, stat1=d / vx[:, None], r=d / np.sqrt(vv), t=np.copysign(np.sqrt(dof * rc / om), d), r2=r2)
		own = 16 * ULD
		b = dict(stat0=(U + own) * np.abs(out['stat0']), stat1=(U + own) * np.abs(out['stat1']), r=np.abs(out['r']) * (ev / 2 + 4 * U + own), r2=r2 * (ev + 3 * U + own))
		b['t'] = np.where(om > 0, np.abs(out['t']) * (1.01 * ev / (2 * om) + U * (4 + 2 / om) + own), 0)
	return dict(out=out, bound=b, by=by, by_bound=gamma(nc) * by_abs + own * np.abs(by), ssy=sy, ssy_bound=e_sy + own * sy, margin=margin, e_sy=e_sy,
				off=np.ones((nx, dp['ny']), dtype=bool))


def alpha_reference(stat, kind, ssx, n, bx, by):
	"""alpha[x, j, c] = by[j, c] - gamma[x, j] bx[x, c], gamma = stat (kind 1) or stat n / vx (kind 0).  Roundings: kind 0 one division and one product on gamma;
	the product with bx and the difference (two, or one fma)."""
	g = ld(stat)
	cnt = 2
	if kind == 0:
		g = g * (LD(n) / ld(np.where(ssx == 0, float(n), ssx)))[:, None]
		cnt += 2
	prod = g[:, :, None] * ld(bx)[:, None, :]
	out = ld(by)[None, :, :] - prod
	return out, U * (cnt * np.abs(prod) + np.abs(out)) + 16 * ULD * (np.abs(prod) + np.abs(out))


# ---- which kernel a call launches (restated from nrm_assoc_sweep_band) --------------------------------------------------------------------------------------------
def instantiation(entry, dtype, symmetric=0, stat_kind=0, want_rt=False):
	t = 'double' if np.dtype(dtype) == np.float64 else 'float'
	if entry == 'mirror':
		return 'k_assoc_sweep_mirror<%s>' % t
	if entry == 'de':
		return 'k_de_small_sweep<%s>' % t
	if entry == 'alpha':
		return 'k_alpha<%s, %s>' % (t, t)
	if symmetric and not want_rt and stat_kind == 0:
		return 'k_assoc_sweep_sym<%s, 32>' % t
	return 'k_assoc_sweep<%s>' % t


def tile_branches(nx, ny, symmetric, row0=0, row1=None):
	"""The tile branches of k_assoc_sweep a call reaches: 'rect', 'upper', 'diagonal', 'mirrored', and 'ragged' when a last tile is partial."""
	row1 = nx if row1 is None else row1
	out = set()
	for bi in range(row0 // TILE, (row1 + TILE - 1) // TILE):
		for bj in range((ny + TILE - 1) // TILE):
			out.add('rect' if not symmetric else ('diagonal' if bi == bj else ('mirrored' if bi > bj else 'upper')))
	if nx % TILE or ny % TILE:
		out.add('ragged')
	return out


# ---- every comparator on the outputs of one sweep ----------------------------------------------------------------------------------------------------------------
def judge(outs, pb, ref, dtype, stat_kind, p_expect=None, mp_subset=True):
	"""outs: name -> the (nx, ny) part of a NaN-pre-filled output as it came back ('p', 'stat', and 'r', 't' when asked for).  p_expect (exact problems): the
	fp64 P-values of nrm_pvalues_from_r2 at the host's R^2 (symmetric: 0 on the diagonal).  Returns name -> Worst."""
	ws = {}
	full = np.ones((pb.nx, pb.ny), dtype=bool)
	for name, a in outs.items():
		ws[name + ' placement'] = placement(a, full, name)
		if pb.sym:
			ws[name + ' symmetry'] = symmetric_zero_diagonal(a, name)
	cast = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
	if pb.exact:
		ws['stat bits'] = bits(outs['stat'], cast(ref['stat64'][stat_kind]), 'stat == numpy fp64')
		if p_expect is not None:
			ws['p bits'] = bits(outs['p'], cast(p_expect), 'p == nrm_pvalues_from_r2(host R^2)')
		if mp_subset:
			ws['p mpmath'] = compare_p_subset(outs['p'], pb, ref['r2_64'], dtype)
	else:
		ws['stat'] = compare(outs['stat'], ref, 'stat%d' % stat_kind, dtype)
		if mp_subset:
			ws['p mpmath'] = compare_p_subset(outs['p'], pb, np.asarray(ref['out']['r2'], dtype=np.float64), dtype, d_r2=ref['bound']['r2'])
	for name in ('r', 't'):
		if name in outs:
			ws[name] = compare(outs[name], ref, name, dtype, exact=pb.exact)
	return ws


def expect_flags01(pb, ref_r2, ssx, ssy, dot):
	"""(flags[0] > 0, flags[1] > 0) as they must come back: an off-diagonal in-range pair with a non-finite d or ss; some R^2 > 1 + 1e-8."""
	m = pb.pairs()
	nf = ~np.isfinite(dot) | ~np.isfinite(ssx)[:, None] | ~np.isfinite(ssy)[None, :]
	if pb.sym:
		nf = np.triu(nf, 1) | np.triu(nf, 1).T
	with np.errstate(invalid='ignore'):
		rng = np.asarray(ref_r2, dtype=np.float64) > 1.0 + 1e-8
	return bool((nf & m).any()), bool((rng & m).any())
