"""Extended-precision restatements of the front half, one function per device stage -- TEST INFRASTRUCTURE ONLY.

Written from the formulas in the header comments of csrc/nrm_lcpm.hip, nrm_lcpm_sparse.hip, nrm_fitvar.hip and nrm_fitvar_plan.hip, in numpy's longdouble
(64-bit mantissa on x86: unit roundoff 2^-64 = 5.4e-20) with mpmath where a special function is needed.  Every stage function takes the arrays the kernel of
that stage reads (fp64 / fp32 / integer) and returns longdouble, so a stage is checked in isolation: its inputs are never another kernel's outputs.  Beside
each sum the function returns the sum of the ABSOLUTE values of its terms, which is what the worst-case rounding bound of an fp64 sum is made of
(tests/test_gpu_front_stages.py).  Pinned to what the reference returned (golden G18) by tests/test_front_longdouble_cpu.py."""
import numpy as np

LD = np.longdouble
U = 2.0**-53  # unit roundoff of fp64
LN1E6 = LD(6) * np.log(LD(10))


def ld(a):
	return np.asarray(a, dtype=LD)


def _mp():
	import mpmath
	mpmath.mp.prec = 100
	return mpmath


def mp_to_ld(v):
	"""An mpmath number as a longdouble: head and tail in fp64, added in longdouble."""
	hi = float(v)
	return LD(hi) + LD(float(v - hi))


def psi_values(xs, t0):
	"""(psi(1 + x) for the integers xs, psi(t0)) by mpmath.digamma, as longdouble."""
	mp = _mp()
	return np.array([mp_to_ld(mp.digamma(mp.mpf(int(x)) + 1)) for x in np.asarray(xs).ravel()], dtype=LD).reshape(np.shape(xs)), mp_to_ld(mp.digamma(mp.mpf(t0)))


def ulp(a):
	"""The spacing of fp64 at |a| (of the longdouble reference value rounded to fp64)."""
	return np.spacing(np.abs(np.asarray(a, dtype=np.float64)))


# ---- lcpm ---------------------------------------------------------------------------------------------------------------------------------------------
def counts(x):
	"""The integer pass: per-cell totals and non-zero counts, per-gene zero counts, grand total, maximum.  Exact (Python integers / int64)."""
	x = np.asarray(x).astype(np.int64)
	return dict(cell_total=x.sum(axis=0), cell_nnz=(x != 0).sum(axis=0), gene_zero=(x == 0).sum(axis=1), total=int(x.sum()), max=int(x.max()))


def colsum(x, etab):
	"""(sum_g E[x_gk], t1[k] = ln(sum) - ln 1e6) from the fp64 table E the kernel reads; the terms are positive, so the sum is its own sum of absolute values."""
	s = ld(etab)[np.asarray(x).astype(np.int64)].sum(axis=0)
	return s, np.log(s) - LN1E6


def write(x, tab, t1=None):
	"""T[x_gk] - t1[k] from the fp64 table T and the fp64 t1 the kernel reads."""
	out = ld(tab)[np.asarray(x).astype(np.int64)]
	return out if t1 is None else out - ld(t1)[None, :]


def lcpm(x, normalize=True, ntot=None):
	"""End to end: (lcpm, t1, info) with psi by mpmath at the counts present; T[x] = psi(1 + x) - psi(sum(x) + 2), t1[k] = ln sum_g exp(T[x_gk]) - ln 1e6.
	info: the distinct counts `vals`, psi(1 + vals), psi(t0), and psi(1 + x) element by element (what the digamma bound of a test is relative to)."""
	x = np.asarray(x).astype(np.int64)
	t0 = int(x.sum()) + 2 if ntot is None else ntot + 2
	vals, inv = np.unique(x, return_inverse=True)
	p, p0 = psi_values(vals, t0)
	tv = p - p0
	t = tv[inv].reshape(x.shape)
	info = dict(vals=vals, psi=p, psi_t0=p0, psi_x=p[inv].reshape(x.shape))
	if not normalize:
		return t, None, info
	t1 = np.log(np.exp(tv)[inv].reshape(x.shape).sum(axis=0)) - LN1E6
	return t - t1[None, :], t1, info


# ---- the three streaming passes of compute_var (csrc/nrm_fitvar.hip) -----------------------------------------------------------------------------------
def moments(y, cw):
	"""a = y cw^T and sum_k |y_gk| |cw_ck|."""
	y, cw = ld(y), ld(cw)
	return y @ cw.T, np.abs(y) @ np.abs(cw).T


def coef(a, mi):
	"""b = a mi^T and sum_d |mi_qd| |a_gd|."""
	a, mi = ld(a), ld(mi)
	return a @ mi.T, np.abs(a) @ np.abs(mi).T


def resid(y, u, c, b):
	"""r = u (y - b C) and |y| + |b| |C| (what the rounding of the fit is relative to)."""
	y, u, c, b = ld(y), ld(u), ld(c), ld(b)
	return u[None, :] * (y - b @ c), np.abs(y) + np.abs(b) @ np.abs(c)


def gene_stats(r):
	"""m_g = mean_k r_gk, sc_g = sqrt(mean_k (r_gk - m_g)^2)."""
	m = r.mean(axis=1)
	return m, np.sqrt(((r - m[:, None])**2).mean(axis=1))


def cell_var(r, m, sc):
	"""v_k = mean_g ((r_gk - m_g) / sc_g)^2 with the m and sc given."""
	d = (r - ld(m)[:, None]) / ld(sc)[:, None]
	return (d**2).mean(axis=0)


# ---- the plan's kernels (csrc/nrm_fitvar_plan.hip) -----------------------------------------------------------------------------------------------------
def design(c, s):
	"""u = 1 / s, cw = C u^2, M = sum_k (u_k C_k)(u_k C_k)^T and sum_k |.| of the same products."""
	c, u = ld(c), 1 / ld(s)
	cu = c * u
	return u, cu * u, cu @ cu.T, np.abs(cu) @ np.abs(cu).T


def logsum(v, c):
	"""l = ln sqrt v, g = [C;1] l and sum_k |[C;1]_rk| |l_k|."""
	l = np.log(np.sqrt(ld(v)))
	c1 = np.vstack([ld(c), np.ones((1, l.size), dtype=LD)])
	return l, c1 @ l, np.abs(c1) @ np.abs(l)


def new_scale(g, m2i, c, s):
	"""coef = M2^+ g, f = coef^T [C;1], new = exp(f) s (before the division by its minimum)."""
	c1 = np.vstack([ld(c), np.ones((1, np.shape(c)[1]), dtype=LD)])
	co = ld(m2i) @ ld(g)
	f = co @ c1
	return co, f, np.exp(f) * ld(s)


def transition(new, s, best, state, eps):
	"""One step of the state machine on fp64 values, as the header of nrm_fitvar_plan.hip states it: (s, best, next record).  new is already divided by its
	minimum.  The record is {bestv, steps, last t1, 0}; once bestv > eps fails nothing changes; a NaN t1 is never the best step."""
	new, s, best, state = (np.asarray(a, dtype=np.float64) for a in (new, s, best, state))
	if not state[0] > eps:
		return s.copy(), best.copy(), state.copy()
	with np.errstate(invalid='ignore', divide='ignore'):
		t1 = np.abs((new - s) / s).max()  # (numpy's max carries a NaN)
	better = bool(t1 < state[0])
	return new.copy(), (new.copy() if better else best.copy()), np.array([t1 if better else state[0], state[1] + 1.0, t1, 0.0])


def weights(best):
	"""w = (1 / best) / min(1 / best)."""
	w = 1 / ld(best)
	return w / w.min()


# ---- compute_var end to end ---------------------------------------------------------------------------------------------------------------------------
def orthonormal(rows):
	"""An orthonormal basis of the span of FULL-RANK rows: Gram-Schmidt applied twice, in longdouble.  No pseudo-inverse and no rank threshold."""
	q = []
	for v in ld(rows):
		for _ in range(2):
			for p in q:
				v = v - (p @ v) * p
		nv = np.sqrt(v @ v)
		assert nv > 0
		q.append(v / nv)
	return np.array(q, dtype=LD)


def compute_var(dt, basis, basis1, stepmax=1, eps=1E-6):
	"""(w, [t1 of every iteration]): reference norm.py:56-128 with both regressions as orthogonal projections.  basis: full-rank rows spanning the covariates'
	row space; basis1: full-rank rows spanning span(covariates, 1) (for one-hot batches plus an intercept, drop one batch row)."""
	dt, basis = ld(dt), ld(basis)
	q1 = orthonormal(basis1)
	s = np.ones(dt.shape[1], dtype=LD)
	best, bestv, n, t1s = None, LD(1E300), 0, []
	while n < stepmax and bestv > eps:
		u = 1 / s
		q = orthonormal(basis * u)
		y = dt * u
		r = y - (y @ q.T) @ q
		m, sc = gene_stats(r)
		l = np.log(np.sqrt(cell_var(r, m, sc)))
		new = np.exp((q1 @ l) @ q1) * s
		new = new / new.min()
		t1 = np.abs((new - s) / s).max()
		t1s.append(t1)
		s = new
		n += 1
		if t1 < bestv:
			bestv, best = t1, s
	return weights(best), t1s


def compute_var_fp64(dt, dc, stepmax=1, eps=1E-6):
	"""What the device computes, in fp64 numpy: both projections through inv_rank on the Gram matrix (normalisr_amd.association).  A second reference: its
	distance from compute_var above is the error of the METHOD at fp64, with no code under test involved."""
	from normalisr_amd.association import inv_rank
	dt, dc = np.asarray(dt, dtype=np.float64), np.asarray(dc, dtype=np.float64)
	ns = dt.shape[1]
	c1 = np.vstack([dc, np.ones((1, ns))])
	d = 1 / np.sqrt((c1**2).sum(axis=1))  # (the second Gram matrix is taken of unit rows: the constant-1 row has no unit to share with the covariates)
	m2i = inv_rank((c1 * d[:, None]) @ (c1 * d[:, None]).T)[0] * d[:, None] * d[None, :]
	s = np.ones(ns)
	best, bestv, n = None, 1E300, 0
	while n < stepmax and bestv > eps:
		u = 1 / s
		cu = dc * u
		mi = inv_rank(cu @ cu.T)[0]
		b = (dt @ (cu * u).T) @ mi.T
		r = u * (dt - b @ dc)
		r = r - r.mean(axis=1)[:, None]
		r = r / np.sqrt((r**2).mean(axis=1))[:, None]
		l = np.log(np.sqrt((r**2).mean(axis=0)))
		new = np.exp((m2i @ (c1 @ l)) @ c1) * s
		new /= new.min()
		t1 = np.abs((new - s) / s).max()
		s = new
		n += 1
		if t1 < bestv:
			bestv, best = t1, s
	w = 1 / best
	return w / w.min()
