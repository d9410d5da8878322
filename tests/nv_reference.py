"""normvar at kernel level (csrc/nrm_normvar.hip) -- TEST INFRASTRUCTURE ONLY, no torch at import.  One plain numpy.longdouble function per C entry, written from the
reference's text (norm.py:131-167, :243-260) and the entries' contracts in include/normalisr_hip.h; comparators with ABSOLUTE, termwise bounds; an fp64 emulation
of every kernel in the kernel's own order (for tests/test_nv_reference_cpu.py: the bounds must hold for it and reject its mutations); the case table and the route
function that restates the launchers' choice of instantiation; exact twins on which every sum is an integer or a dyadic below 2^53 and outputs compare bit for bit.

The bounds, with u = 2^-53, re = the relative error of one e = exp(wt ln w) as the kernels compute it, D = the depth of a sum:
    re    = NV_EXP + u |wt ln w|        nv_exp's own 3.5e-16 (measured by test_normvar_exp_against_numpy) and the rounding of its argument wt * ln w, which moves the
                                        exponent by u |x| and so e by that relative amount; e = 1 exactly where wt == 0: re = 0 there
    sum   : (D + t) u sum |terms|       t roundings inside a term on top of its factors' own relative errors; D = the thread's cells + 6 levels of the wave tree + 3
                                        adds over the waves (an fma counts as one rounding)
    U = e^2: 2 re + u;  V = e^2 y: 2 re + 2u;  s1 term y e: re + u;  s2 term (y e)^2: 2 re + 2u (the square is inside the fma);  pair term (e^2 c) c': 2 re + 2u
    (e^2, the product, the fma counts in D);  a term (e^2 y) c: 2 re + 2u.
    apply : sc * e * (y - fit):  fit is nc fmas ((nc) u sum |b c|), the difference u |y - fit|, two products 2u, e re:  [re + (nc + 3) u] |sc| e (|y| + sum |b c|),
            plus half an fp32 ulp of the result (2^-24 |out|, and 2^-150 for the subnormal grid) when the output is fp32.
    b     : against the longdouble pseudo-inverse of the moments the device itself produced.  The Jacobi iteration applies plane rotations: each changes an element with
            relative error <= 6u (Wilkinson), an element is touched by at most 4 (nc - 1) rotations of a sweep (its row and its column, from both sides), the code
            allows 60 sweeps: a backward error of 1440 (nc - 1) u ||M||.  With ||a|| <= ||M|| ||b|| that is 1440 (nc - 1) u cond ||b||, plus (3 nc + 2) u cond ||b||
            for forming M^+ (three-factor terms) and M^+ a.  For nc = 1 the (nc - 1) is taken as 1 (the division).
    scale : as computed, against the longdouble one-pass formula on the device's own moments AND coefficients: d1 = s2 / n - mean^2 carries 3u s2 / n (the quotient, the
            square, the difference), d2 = s2 - a . b carries u s2 + (nc + 1) u sum |a b|; the scale is (d1 n / d2)^(wt / 2): wt / 2 of both relative errors, plus 8u
            for two roots, two quotients and pow (a few ulp on the device).
"""
import functools

import numpy as np

from k3_reference import LD, U, Worst, ld, worst, same_bits, bits  # noqa: F401

F32, F64 = np.float32, np.float64
NV_EXP = 3.5e-16
NV_R, NV_G, NV_NC, WIDE_NC = 4, 2, 8, 1024
TAU, MARK = 2.0**-20, -1.0  # csrc/nrm_nv_scale.h
SLACK = 1.0
TOL = 1e-8


# ---- the references -----------------------------------------------------------------------------------------------------------------------------------------------
def weight(lnw, wt, dtype=LD):
	"""e (rows, n) = w**wt, exactly 1 where wt == 0 (norm.py:244-246), and its relative error as the kernels compute it."""
	x = np.asarray(wt, dtype)[:, None] * np.asarray(lnw, dtype)[None, :]
	e = np.exp(x)
	e[np.asarray(wt) == 0] = 1
	re = NV_EXP + U * np.abs(np.asarray(x, F64))
	re[np.asarray(wt) == 0] = 0
	return e, re


def depth_weights(ldo):
	return -(-ldo // 256) + 9


def depth_cells(n):
	return 4 * -(-(n & ~3) // 1024) + 1 + 9


def weights(y, lnw, wt, ldo, rows_pad):
	"""nrm_normvar_weights: U = e^2, V = e^2 y (rows_pad, ldo) zero padded, s1 = sum y e, s2 = sum (y e)^2 (rows_pad, zero past rows); with the bounds."""
	rows, n = y.shape
	e, re = weight(lnw, wt)
	yl = ld(y)
	Uo, Vo = np.zeros((rows_pad, ldo), LD), np.zeros((rows_pad, ldo), LD)
	Uo[:rows, :n], Vo[:rows, :n] = e * e, e * e * yl
	bu, bv = np.zeros((rows_pad, ldo)), np.zeros((rows_pad, ldo))
	bu[:rows, :n] = (2 * re + U) * np.asarray(e * e, F64)
	bv[:rows, :n] = (2 * re + 2 * U) * np.asarray(np.abs(e * e * yl), F64)
	s1, s2, b1, b2 = (np.zeros(rows_pad, LD) for _ in range(4))
	yp = yl * e
	D = depth_weights(ldo)
	s1[:rows], s2[:rows] = yp.sum(axis=1), (yp * yp).sum(axis=1)
	b1[:rows] = ((re + (1 + D) * U) * np.abs(yp)).sum(axis=1)
	b2[:rows] = ((2 * re + (2 + D) * U) * yp * yp).sum(axis=1)
	return dict(U=Uo, V=Vo, s1=s1, s2=s2), dict(U=bu, V=bv, s1=np.asarray(b1, F64), s2=np.asarray(b2, F64))


def moments(y, lnw, wt, c):
	"""d_mom (rows, nc (nc + 1) / 2 + nc + 2): M_g's pairs in triu order, then a_g, then s1, s2; and the termwise bound."""
	rows, n = y.shape
	nc = c.shape[0]
	e, re = weight(lnw, wt)
	yl, cl = ld(y), ld(c)
	iu = np.triu_indices(nc)
	e2 = e * e
	D = depth_cells(n)
	cols, bnd = [], []
	r2 = ld(2 * re + (2 + D) * U)
	for q, d in zip(*iu):
		t = e2 * (cl[q] * cl[d])[None, :]
		cols.append(t.sum(axis=1)), bnd.append((r2 * np.abs(t)).sum(axis=1))
	for q in range(nc):
		t = e2 * yl * cl[q][None, :]
		cols.append(t.sum(axis=1)), bnd.append((r2 * np.abs(t)).sum(axis=1))
	yp = yl * e
	cols += [yp.sum(axis=1), (yp * yp).sum(axis=1)]
	bnd += [(ld(re + (1 + D) * U) * np.abs(yp)).sum(axis=1), (r2 * yp * yp).sum(axis=1)]
	return np.stack(cols, axis=1), np.asarray(np.stack(bnd, axis=1), F64)


def jacobi(m):
	"""Eigenvalues and eigenvectors (columns) of a small symmetric longdouble matrix: the cyclic Jacobi iteration, run until the off-diagonal part is below 1e-22 of the diagonal."""
	a = np.array(m, dtype=LD)
	n = a.shape[0]
	v = np.eye(n, dtype=LD)
	for _ in range(100):
		off = (np.triu(a, 1)**2).sum()
		if not off > LD(1e-44) * (np.diag(a)**2).sum():
			break
		for p in range(n - 1):
			for q in range(p + 1, n):
				if a[p, q] == 0:
					continue
				with np.errstate(over='ignore'):
					th = (a[q, q] - a[p, p]) / (2 * a[p, q])
					t = (1 if th >= 0 else -1) / (abs(th) + np.sqrt(th * th + 1))
				cs = 1 / np.sqrt(t * t + 1)
				sn = t * cs
				for x in (a, v):  # columns p, q of a and of v
					xp, xq = x[:, p].copy(), x[:, q].copy()
					x[:, p], x[:, q] = cs * xp - sn * xq, sn * xp + cs * xq
				ap, aq = a[p].copy(), a[q].copy()  # rows p, q of a
				a[p], a[q] = cs * ap - sn * aq, sn * ap + cs * aq
				a[p, q] = a[q, p] = 0
	return np.diag(a).copy(), v


def inv_rank(m, tol=TOL):
	"""(M^+, rank, cond of the kept part, gap) by inv_rank's rule (association.py:77-80): singular values below tol x the largest count as zero; a zero matrix keeps
	everything (nrm_jacobi.h:69).  gap: how far, as a factor, the nearest eigenvalue is from tol x the largest (the cases plant >= 1e3: the rank is then a fact)."""
	w, v = jacobi(m)
	s = np.abs(w)
	smax = s.max()
	keep = s >= LD(tol) * smax
	with np.errstate(divide='ignore', invalid='ignore'):
		iw = np.where(keep, 1 / w, 0)
		inv = (v * iw[None, :]) @ v.T
		cond = float(smax / s[keep].min()) if smax > 0 else np.inf
		r = s / (LD(tol) * smax) if smax > 0 else np.full(len(s), np.inf)
		gap = float(np.min(np.maximum(r, 1 / np.where(r > 0, r, LD(1e-300)))))
	return inv, int(keep.sum()), cond, gap


def unpack(mom_row, nc):
	iu = np.triu_indices(nc)
	npair = len(iu[0])
	M = np.zeros((nc, nc), LD)
	M[iu] = mom_row[:npair]
	M[(iu[1], iu[0])] = mom_row[:npair]
	return M, ld(mom_row[npair:npair + nc]), LD(mom_row[npair + nc]), LD(mom_row[npair + nc + 1])


def one_pass(s1, s2, a, b, n, wt, keepvar):
	"""The scale in the one-pass form, the mark of csrc/nrm_nv_scale.h, how decided the mark is (distance of the nearer difference from tau x its minuend, as a factor)
	and the relative bound of the scale as computed."""
	if not keepvar or wt == 0:
		return LD(1), False, np.inf, 0.0
	n = LD(n)
	q = s2 / n
	d1, d2 = q - (s1 / n)**2, s2 - (a * b).sum()
	with np.errstate(divide='ignore', invalid='ignore'):
		f = [float(d / (LD(TAU) * m)) if m > 0 else np.inf for d, m in ((d1, q), (d2, s2))]
		marked = min(f) < 1
		decided = min(max(x, 1 / x) if x > 0 else np.inf for x in f)
		sc = (np.sqrt(max(d1, LD(0))) / np.sqrt(max(d2, LD(0)) / n))**LD(wt)
		nc = len(a)
		rel = 0.5 * wt * (3 * U * float(q / d1) + U * float((s2 + (nc + 1) * np.abs(a * b).sum()) / d2)) + 8 * U if d1 > 0 and d2 > 0 else np.inf
	return sc, marked, decided, rel


def solve(mom, nc, n, wt, tol, keepvar, b_dev=None):
	"""From moments rows: b = M^+ a, integer rank, cond, gap; the one-pass scale on b_dev (the device's own coefficients) when given, else on b."""
	out = dict(b=[], rank=[], cond=[], gap=[], scale=[], marked=[], decided=[], scale_rel=[], bnorm=[])
	for g in range(mom.shape[0]):
		M, a, s1, s2 = unpack(ld(mom[g]), nc)
		inv, rk, cond, gap = inv_rank(M, tol)
		with np.errstate(invalid='ignore'):
			b = inv @ a
		sc, mk, dec, rel = one_pass(s1, s2, a, ld(b_dev[g]) if b_dev is not None else b, n, float(wt[g]), keepvar)
		for k, v in zip(out, (b, rk, cond, gap, sc, mk, dec, rel, float(np.sqrt((b * b).sum())))):
			out[k].append(v)
	return {k: np.array(v) for k, v in out.items()}


def b_bound(nc, cond, bnorm):
	return SLACK * (1440 * max(nc - 1, 1) + 3 * nc + 2) * U * cond * bnorm


def scale_two_pass(y, lnw, wt, c, b):
	"""The reference's dv and dv2 from the row itself (norm.py:248-249,255-259) and the scale (dv / dv2)^wt; with the relative bound of nrm_normvar_rescale's value:
	d = y e - mean with the mean's own error (re + (1 + D) u) sum |y e| / n, r = e (y - fit) as in apply; a sum of squares moves by 2 sum |t| dt + (D + 1) u sum t^2."""
	rows, n = y.shape
	nc = c.shape[0]
	e, re = weight(lnw, wt)
	yl, cl, bl = ld(y), ld(c), ld(b)
	yp = yl * e
	D = -(-n // 256) + 9
	mean = yp.mean(axis=1)
	dmean = ((re + (1 + D) * U) * np.abs(yp)).sum(axis=1) / n
	d = yp - mean[:, None]
	fit, afit = bl @ cl, np.abs(bl) @ np.abs(cl)
	r = e * (yl - fit)
	v1, v2 = (d * d).sum(axis=1), (r * r).sum(axis=1)
	dd = (re + U) * np.abs(yp) + dmean[:, None] + U * np.abs(d)
	dr = e * ((nc + 1) * U * afit + U * np.abs(yl - fit)) + (re + U) * np.abs(r)
	e1 = 2 * (np.abs(d) * dd).sum(axis=1) + (D + 1) * U * v1
	e2 = 2 * (np.abs(r) * dr).sum(axis=1) + (D + 1) * U * v2
	wtl = ld(wt)
	with np.errstate(divide='ignore', invalid='ignore'):
		dv, dv2 = np.sqrt(v1 / n), np.sqrt(v2 / n)
		sc = (dv / dv2)**wtl
		rel = 0.5 * np.asarray(wtl * (e1 / v1 + e2 / v2), F64) + 8 * U
	sc[np.asarray(wt) == 0] = 1
	return dict(dv=dv, dv2=dv2, scale=sc, rel=rel)


def apply(y, lnw, wt, c, b, scale, out_dtype=F64):
	"""nrm_normvar_apply: scale e (y - b . c), and its bound."""
	e, re = weight(lnw, wt)
	yl, cl, bl, sl = ld(y), ld(c), ld(b), ld(scale)
	nc = c.shape[0]
	with np.errstate(invalid='ignore', over='ignore'):
		out = sl[:, None] * e * (yl - bl @ cl)
		mag = np.abs(sl)[:, None] * e * (np.abs(yl) + np.abs(bl) @ np.abs(cl))
		bound = np.asarray((re + (nc + 3) * U) * mag, F64)
		if np.dtype(out_dtype) == np.dtype(F32):
			bound = bound + 2.0**-24 * np.asarray(np.abs(out), F64) + 2.0**-150
	return out, bound * SLACK


def apply_w2(y, w2, c, b, out_dtype=F64):
	"""nrm_normvar_apply_w2: y - w2 (b . c); nc fmas, a product, a difference: (nc + 2) u (|y| + |w2| sum |b c|)."""
	yl, wl, cl, bl = ld(y), ld(w2), ld(c), ld(b)
	nc = c.shape[0]
	out = yl - wl * (bl @ cl)
	bound = np.asarray((nc + 2) * U * (np.abs(yl) + np.abs(wl) * (np.abs(bl) @ np.abs(cl))), F64)
	if np.dtype(out_dtype) == np.dtype(F32):
		bound = bound + 2.0**-24 * np.asarray(np.abs(out), F64) + 2.0**-150
	return out, bound * SLACK


def judge(got, ref, bound, what, exact=False):
	"""Worst error-to-bound ratio; exact: the bits of the reference rounded once to got's type."""
	got = np.asarray(got)
	if exact:
		return bits(got, np.asarray(ref, got.dtype), what + ' (bits)')
	with np.errstate(invalid='ignore'):
		err = np.abs(ld(got) - ref)
	err = np.where(np.isnan(np.asarray(err, F64)) & ~(np.isnan(np.asarray(ref, F64)) & np.isnan(got)), np.inf, np.nan_to_num(np.asarray(err, F64), nan=0.0, posinf=np.inf))
	both_inf = np.isinf(got) & (np.asarray(ref, F64) == got)
	return worst(np.where(both_inf, 0.0, err), bound, what)


def judge_rel(got, ref, rel, what):
	return worst(np.abs(np.asarray(ld(got) / ref - 1, F64)), rel, what)


# ---- the thread maps and the emulation ------------------------------------------------------------------------------------------------------------------------------
def map_strided(count):
	"""k_nv_weights, k_nv_apply_w2, k_nv_rescale: thread tid takes k = tid, tid + 256, ...  -> (256, S) cell indices, -1 where the thread has none."""
	S = -(-count // 256)
	k = np.arange(256)[:, None] + 256 * np.arange(S)[None, :]
	return np.where(k < count, k, -1)


def map_four(n):
	"""k_nv_moments, k_nv_apply: the four-cell loop k = 4 tid + 1024 it + v below n4 = n & ~3 (it outer, v inner), then the tail k = n4 + tid."""
	n4 = n & ~3
	S = -(-n4 // 1024)
	k = (4 * np.arange(256)[:, None, None] + 1024 * np.arange(S)[None, :, None] + np.arange(4)[None, None, :]).reshape(256, 4 * S)
	k = np.where(k < n4, k, -1)
	tail = n4 + np.arange(256)[:, None]
	return np.concatenate([k, np.where(tail < n, tail, -1)], axis=1)


def thread_of(n):
	"""cell -> (thread, in the tail loop?) of the four-cell map."""
	k = np.arange(n)
	n4 = n & ~3
	return np.where(k < n4, (k % 1024) // 4, k - n4), k >= n4


def bad_waves(nonfinite):
	"""flags[1] of k_nv_apply: the number of (workgroup, wave) pairs with a non-finite stored value; nonfinite (rows, n) bool."""
	rows, n = nonfinite.shape
	th, _ = thread_of(n)
	g, k = np.nonzero(nonfinite)
	return len(set(zip((g // NV_R).tolist(), (th[k] // 64).tolist())))


def fma(a, b, c):
	"""fl(a b + c) through longdouble (the product carries 64 bits, not 106: a double rounding in rare cases; exact on the twins)."""
	return np.asarray(ld(a) * ld(b) + ld(c), F64)


def wave_tree(v):
	"""nrm_wave_sum (csrc/nrm_device.h): v += shfl_down(v, o) for o = 32 .. 1; lane 0's value.  v (..., 64)."""
	v = np.array(v, F64)
	for o in (32, 16, 8, 4, 2, 1):
		v = v[..., :o] + v[..., o:2 * o]
	return v[..., 0]


def block_sum(terms, cellmap, use_fma=None, drop_wave=None, order='tree'):
	"""Per thread in its cells' order (acc += t, or acc = fma(f, f2, acc) with use_fma = (f, f2)), nrm_wave_sum per wave, ((w0 + w1) + w2) + w3.  terms (..., n)."""
	lead = (use_fma[0] if use_fma else terms).shape[:-1]
	acc = np.zeros(lead + (256, ), F64)
	for s in range(cellmap.shape[1]):
		k = cellmap[:, s]
		live = k >= 0
		kk = np.where(live, k, 0)
		if use_fma:
			acc = np.where(live, fma(use_fma[0][..., kk], use_fma[1][..., kk], acc), acc)
		else:
			acc = np.where(live, acc + terms[..., kk], acc)
	w = wave_tree(acc.reshape(lead + (4, 64)))
	if drop_wave is not None:
		w[..., drop_wave] = 0.0
	return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def emu_e(lnw, wt, mut=None):
	"""fp64 e as the kernels form it: exp of the ROUNDED product wt * ln w (numpy's exp stands for nv_exp: both within NV_EXP), 1 for wt == 0."""
	wt = np.asarray(wt, F64)
	if mut == 'wt of the neighbouring row':
		wt = np.roll(wt, 1)
	e = np.exp(wt[:, None] * np.asarray(lnw, F64)[None, :])
	e[wt == 0] = 1.0
	return e


def emu_weights(y, lnw, wt, ldo, rows_pad, mut=None):
	rows, n = y.shape
	e = emu_e(lnw, wt, mut)
	yv = np.asarray(y, F64)
	Uo, Vo = np.zeros((rows_pad, ldo)), np.zeros((rows_pad, ldo))
	u = e if mut == 'e for e^2 in U' else e * e
	Uo[:rows, :n], Vo[:rows, :n] = u, u * yv
	if mut == 'padding columns of U left':
		Uo[:, n:] = 1e-300
	if mut == 'padding rows of V left':
		Vo[rows:] = 1e-300
	yp = np.zeros((rows_pad, ldo))
	yp[:rows, :n] = yv * e
	cm = map_strided(ldo)
	if mut == 'tail cells dropped':
		cm = map_strided(n & ~3)
	dw = 3 if mut == 'one wave left out' else None
	return dict(U=Uo, V=Vo, s1=block_sum(yp, cm, drop_wave=dw), s2=block_sum(None, cm, use_fma=(yp, yp), drop_wave=dw))


def emu_moments(y, lnw, wt, c, mut=None):
	rows, n = y.shape
	nc = c.shape[0]
	e = emu_e(lnw, wt, mut)
	yv, cv = np.asarray(y, F64), np.asarray(c, F64)
	e2 = e * e
	cm = map_four(n)
	if mut == 'tail cells dropped':
		cm = cm[:, :-1]
	dw = 1 if mut == 'one wave left out' else None
	pairs = list(zip(*(np.tril_indices(nc) if mut == 'pairs in tril order' else np.triu_indices(nc))))
	cols = []
	for q, d in pairs:
		cols.append(block_sum(None, cm, use_fma=(e2 * cv[q][None, :], np.broadcast_to(cv[d], e2.shape)), drop_wave=dw))
	ea = e if mut == 'e for e^2 in a' else e2
	for q in range(nc):
		cols.append(block_sum(None, cm, use_fma=(ea * yv, np.broadcast_to(cv[q], e2.shape)), drop_wave=dw))
	yp = yv * e
	cols += [block_sum(yp, cm, drop_wave=dw), block_sum(None, cm, use_fma=(yp, yp), drop_wave=dw)]
	mom = np.stack(cols, axis=1)
	if mut == 'second gene of an odd last pair dropped' and rows % NV_G == 0:
		mom[rows - 1] = np.nan  # (the buffer's pre-fill: nothing stored)
	if mut == 'last gene of an odd count dropped' and rows % NV_G == 1:
		mom[rows - 1] = np.nan
	return mom


def emu_solve(mom, nc, n, wt, tol, keepvar, mut=None, pitch=None):
	"""k_nv_solve in fp64: numpy's eigh stands for the Jacobi iteration (both backward stable), the rule of nrm_jacobi.h:69, b = M^+ a row by row, the one-pass scale
	with the mark."""
	rows = mom.shape[0]
	b, sc, rk = np.zeros((rows, nc)), np.ones(rows), np.zeros(rows, np.int64)
	iu = np.triu_indices(nc)
	npair = len(iu[0])
	for g in range(rows):
		M = np.zeros((nc, nc))
		M[iu] = mom[g, :npair]
		M[(iu[1], iu[0])] = mom[g, :npair]
		a = mom[g, npair:npair + nc].copy()
		if mut == 'last covariate missing from the fit' and nc > 1:
			M, a = M[:-1, :-1], a[:-1]
		w, v = np.linalg.eigh(M)
		keep = np.abs(w) >= tol * np.abs(w).max()
		with np.errstate(divide='ignore', invalid='ignore'):
			inv = (v * np.where(keep, 1 / w, 0.0)[None, :]) @ v.T
			bb = inv @ a
		rk[g] = keep.sum()
		b[g, :len(bb)] = bb
		if keepvar:
			wtg = wt[(g + 1) % rows] if mut == 'wt of the neighbouring row' else wt[g]
			nn = float(pitch if mut == 'mean divided by the pitch' else n)  # (the row's pitch in place of its cell count)
			s1, s2, ab = mom[g, npair + nc], mom[g, npair + nc + 1], float((a * bb).sum())
			mean = s1 / nn
			d1, d2 = s2 / n - mean * mean, s2 - ab
			with np.errstate(divide='ignore', invalid='ignore'):
				sc[g] = MARK if wtg != 0 and (d1 < TAU * (s2 / n) or d2 < TAU * s2) else (np.sqrt(max(d1, 0.0)) / np.sqrt(max(d2, 0.0) / n))**wtg
	return dict(b=b, scale=sc, rank=rk)


def emu_rescale(y, lnw, wt, c, b, scale):
	"""k_nv_rescale in its own order (the strided map, nrm_block_sum) for the genes that hold MARK."""
	rows, n = y.shape
	e = emu_e(lnw, wt)
	yv = np.asarray(y, F64)
	cm = map_strided(n)
	out = np.array(scale, F64)
	for g in np.nonzero(out < 0)[0]:
		yp = yv[g] * e[g]
		mean = block_sum(yp, cm) / n
		fit = np.zeros(n)
		for q in range(c.shape[0]):
			fit = fma(b[g, q], c[q], fit)
		d, r = yp - mean, e[g] * (yv[g] - fit)
		v1, v2 = block_sum(None, cm, use_fma=(d, d)), block_sum(None, cm, use_fma=(r, r))
		with np.errstate(divide='ignore', invalid='ignore'):
			out[g] = (np.sqrt(v1 / n) / np.sqrt(v2 / n))**wt[g]
	return out


def emu_apply(y, lnw, wt, c, b, scale, out_dtype=F64, flags1=0, mut=None):
	rows, n = y.shape
	nc = c.shape[0]
	e = emu_e(lnw, wt, mut)
	yv, cv, bv, sc = np.asarray(y, F64), np.asarray(c, F64), np.asarray(b, F64), np.asarray(scale, F64)
	if mut == 'scale of the neighbouring row':
		sc = np.roll(sc, 1)
	if mut == 'WIDE table read at pitch 64' and nc > 64:  # row r of a workgroup's table starts at 64 r, not nc r: the flat table of the four rows read at the wrong offset
		bw = np.zeros_like(bv)
		for g0 in range(0, rows, NV_R):
			flat = np.zeros(NV_R * nc)
			blk = bv[g0:g0 + NV_R]
			flat[:blk.size] = blk.ravel()
			for r in range(blk.shape[0]):
				seg = flat[64 * r:64 * r + nc]
				bw[g0 + r, :len(seg)] = seg
		bv = bw
	fit = np.zeros((rows, n))
	for q in range(nc - 1 if mut == 'last covariate missing from the fit' else nc):
		fit = fma(bv[:, q][:, None], cv[q][None, :], fit)
	with np.errstate(invalid='ignore', over='ignore'):
		full = sc[:, None] * e * (yv - fit)
		out = full.astype(out_dtype)
		if mut == 'fp32 output truncated, not rounded' and np.dtype(out_dtype) == np.dtype(F32):  # toward zero: up to one ulp, the bound allows half
			out = np.where(np.abs(out.astype(F64)) > np.abs(full), np.nextafter(out, F32(0)), out)
	if mut == 'tail cells dropped':
		out[:, n & ~3:] = np.nan
	cnt = bad_waves(~np.isfinite(out))
	return dict(out=out, flags1=cnt if mut == 'flags[1] set instead of added' else flags1 + cnt)


def emu_apply_w2(y, w2, c, b, out_dtype=F64, mut=None):
	yv, cv, bv = np.asarray(y, F64), np.asarray(c, F64), np.asarray(b, F64)
	fit = np.zeros(yv.shape)
	for q in range(c.shape[0] - (1 if mut == 'last covariate missing from the fit' else 0)):
		fit = fma(bv[:, q][:, None], cv[q][None, :], fit)
	w = np.asarray(w2, F64)
	if mut == 'w2 of the neighbouring row':
		w = np.roll(w, 1, axis=0)
	return (yv - w * fit).astype(out_dtype)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------------
CELLS = [1, 3, 4, 7, 1024, 1029, 2053]
GENES = [1, 2, 3, 5, 9, 65, 130]
APPLY_NC = [1, 8, 9, 64, 65, 130, 1024]
W2_NC = [1, 63, 64]
COVS = ['full', 'repeat', 'onehot', 'zero']
# how the pointers and pitches are laid out: name -> (skip of y, lnw, c, out; pitch parity 'min' | 'odd' | 'even')
LAYOUTS = {'aligned': (0, 0, 0, 0, 'even'), 'minimal': (0, 0, 0, 0, 'min'), 'odd pitch': (0, 0, 0, 0, 'odd'), 'y off': (1, 0, 0, 0, 'even'), 'lnw off': (0, 1, 0, 0, 'even'),
		   'c off': (0, 0, 1, 0, 'even'), 'out off': (0, 0, 0, 1, 'even')}


def _pitch(n, itemsize, parity):
	"""minimal; 'even': the next pitch above n whose rows stay 16-byte aligned; 'odd': an odd pitch above n (never aligned for more than one row)."""
	if parity == 'min':
		return n
	q = 16 // itemsize
	p = (n // q + 2) * q
	return p if parity == 'even' else p + 1


def _case(entry, rows, n, nc, ydt=F64, odt=F64, layout='aligned', cov='full', keepvar=1, seed=0):
	return dict(entry=entry, rows=rows, n=n, nc=nc, ydt=ydt, odt=odt, layout=layout, cov=cov, keepvar=keepvar, seed=seed)


def case_id(c):
	return '%s-g%d-n%d-nc%d-%s-%s-%s-%s-k%d' % (c['entry'], c['rows'], c['n'], c['nc'], np.dtype(c['ydt']).name, np.dtype(c['odt']).name, c['layout'].replace(' ', '_'),
												c['cov'], c['keepvar'])


def cases():
	out = []
	lay = list(LAYOUTS)
	# weights: every cell count and gene count once, both types, the layouts in turn
	for i, (n, g) in enumerate(zip(CELLS, GENES)):
		for ydt in (F32, F64):
			out.append(_case('weights', g, n, 0, ydt, layout=lay[(i + (ydt == F64)) % 3]))
	out += [_case('weights', 5, 1029, 0, F32, layout='y off'), _case('weights', 9, 7, 0, F64, layout='lnw off')]
	# solve: every covariate count x type x (aligned, not); cells, genes, covariate sets and the unaligned layouts in turn
	unal = ['odd pitch', 'y off', 'lnw off', 'c off', 'minimal']
	for nc in range(1, NV_NC + 1):
		for t, ydt in enumerate((F32, F64)):
			for a, al in enumerate((True, False)):
				i = 4 * nc + 2 * t + a
				n = [1024, 1029, 2053, 7][i % 4] if al or i % 5 else [3, 1, 4][i % 3]
				cov = COVS[i % 3] if nc >= 4 else 'full'
				out.append(_case('solve', GENES[i % len(GENES)] if n > 7 or i % 2 else GENES[i % 5], n, nc, ydt, layout='aligned' if al else unal[i % len(unal)], cov=cov, keepvar=(i // 3) % 2 if nc > 1 else 1,
								 seed=i))
	out += [_case('solve', 5, 1029, 3, F64, cov='zero'), _case('solve', 130, 7, 2, F32, layout='minimal'), _case('solve', 1, 1, 1, F64), _case('solve', 3, 3, 2, F32, layout='odd pitch'),
			_case('solve', 2, 3, 5, F64, layout='c off')]  # (fewer cells than covariates: rank 3 of 5 without a planted dependency)
	# apply: every covariate count x the four type pairs x (aligned, not)
	i = 0
	for nc in APPLY_NC:
		for ydt in (F32, F64):
			for odt in (F32, F64):
				for al in (True, False):
					i += 1
					if nc == 1024:
						rows, n = 5, 5
					elif nc >= 64:
						rows, n = [1, 2, 5, 9][i % 4], [1029, 7, 3, 1024][i % 4]
					else:
						rows, n = GENES[i % len(GENES)], CELLS[i % len(CELLS)] if i % 2 else 2053 if i % 4 == 0 else 1029
					if rows * n * max(nc, 8) > 3e6:
						rows = 9
					out.append(_case('apply', rows, n, nc, ydt, odt, 'aligned' if al else (unal + ['out off'])[(i // 2) % 6], seed=i))
	# apply_w2: the four type pairs, the three covariate counts
	i = 0
	for nc in W2_NC:
		for ydt in (F32, F64):
			for odt in (F32, F64):
				i += 1
				out.append(_case('apply_w2', GENES[i % len(GENES)], CELLS[(i + 2) % len(CELLS)], nc, ydt, odt, lay[i % len(lay)], seed=i))
	return out


CASES = cases()


def layout(c):
	"""(skips, pitches) of a case: y, lnw, c, out skips in elements; ldy, ldc, ldo."""
	sy, sl, sc, so, par = LAYOUTS[c['layout']]
	n = c['n']
	return dict(sy=sy, sl=sl, sc=sc, so=so, ldy=_pitch(n, np.dtype(c['ydt']).itemsize, par), ldc=_pitch(n, 8, par), ldo=_pitch(n, np.dtype(c['odt']).itemsize, par))


def route(c, base=256):
	"""The launchers' selection restated (csrc/nrm_normvar.hip: nv_aligned, the nc > 64 switch, the type pairs) -> the set of kernel instantiations a case launches.
	Buffers start on `base`-byte boundaries (the allocator's), moved by their skip."""
	L = layout(c)
	ys, os_ = np.dtype(c['ydt']).itemsize, np.dtype(c['odt']).itemsize
	ty, to = np.dtype(c['ydt']).name, np.dtype(c['odt']).name
	al = (base + L['sy'] * ys) % 16 == 0 and (L['ldy'] * ys) % 16 == 0 and (base + 8 * L['sl']) % 16 == 0 and (base + 8 * L['sc']) % 16 == 0 and L['ldc'] % 2 == 0
	if c['entry'] == 'weights':
		return {('k_nv_weights', ty)}
	if c['entry'] == 'solve':
		return {('k_nv_moments', ty, c['nc'], al), ('k_nv_solve', c['nc'])}
	if c['entry'] == 'apply':
		al = al and (base + L['so'] * os_) % 16 == 0 and (L['ldo'] * os_) % 16 == 0
		return {('k_nv_apply', ty, to, al, c['nc'] > 64)}
	return {('k_nv_apply_w2', ty, to)}


def all_instantiations():
	t = ('float32', 'float64')
	return ({('k_nv_moments', a, nc, al) for a in t for nc in range(1, 9) for al in (True, False)} | {('k_nv_solve', nc) for nc in range(1, 9)}
			| {('k_nv_apply', a, b, al, w) for a in t for b in t for al in (True, False) for w in (True, False)} | {('k_nv_apply_w2', a, b) for a in t for b in t}
			| {('k_nv_weights', a) for a in t})


def covariates(kind, nc, n, rng, exact=False):
	"""full rank; a repeated row; one-hot batches plus an intercept (rank nc - 1); all zero.  The deficient sets are EXACTLY deficient (the planted eigenvalue is 0 up to
	the rounding of the moments, ~1e-16 of the largest: 1e8 below tol) and the full ones well conditioned (checked by the gap in the CPU test)."""
	if exact:
		c = rng.integers(-3, 4, (nc, n)).astype(F64)
	else:
		c = rng.normal(size=(nc, n))
		if nc >= 1:
			c[-1] = 1.0
	if kind == 'repeat' and nc >= 2:
		c[1] = c[0]
	elif kind == 'onehot' and nc >= 3:
		c[:nc - 1] = np.eye(nc - 1)[:, rng.integers(0, nc - 1, n)]
		c[nc - 1] = 1.0
	elif kind == 'zero':
		c[:] = 0.0
	return c


@functools.lru_cache(maxsize=None)
def problem(i, exact=False):
	"""The inputs of CASES[i] (read-only: cached).  exact: small-integer y and c, lnw = 0 wherever wt != 0 (so e = 1), dyadic b, power-of-two scale."""
	c = CASES[i]
	for attempt in range(20):  # (a solve case whose draw leaves an eigenvalue within 1e4 of tol x the largest is drawn again: the integer rank must be a fact)
		pb = _draw(i, exact, attempt)
		if c['entry'] != 'solve':
			return pb
		sv = solve(np.asarray(moments(pb['y'], pb['lnw'], pb['wt'], pb['c'])[0], F64), c['nc'], c['n'], pb['wt'], TOL, 0)
		if (sv['gap'] >= 1e4).all():
			return pb
	raise AssertionError('no decided draw for ' + case_id(c))


def _draw(i, exact, attempt):
	c = CASES[i]
	rng = np.random.default_rng(1000 + 7 * i + c['seed'] + 100000 * attempt)
	rows, n, nc = c['rows'], c['n'], c['nc']
	wt = rng.uniform(0.05, 1.5, rows)
	wt[::3] = 0.0
	if rows > 1:
		wt[1] = 1.5
	if exact:
		y = rng.integers(-9, 10, (rows, n)).astype(c['ydt'])
		lnw = np.zeros(n)
	else:
		y = (rng.normal(size=(rows, n)) * rng.uniform(0.5, 2, (rows, 1)) - rng.choice([0.0, 9.0], (rows, 1))).astype(c['ydt'])
		lnw = rng.uniform(-1.5, 1.5, n)
	pb = dict(c, y=y, lnw=lnw, wt=wt, exact=exact)
	if nc:
		C = covariates(c['cov'], nc, n, rng, exact)
		pb['c'] = C
		if c['entry'] == 'solve' and not exact and rows >= 5 and n >= 1024:  # a gene for the rule of csrc/nrm_nv_scale.h: row 4 (wt != 0) explained by the covariates to 1e-5
			fit = rng.normal(size=nc) @ C + 2.0
			y[4] = (fit + 1e-5 * np.sqrt((fit**2).mean()) * rng.normal(size=n)).astype(c['ydt'])
		if c['entry'] in ('apply', 'apply_w2'):
			if exact:
				pb['b'] = rng.integers(-8, 9, (rows, nc)) / 4.0
				pb['scale'] = 2.0**rng.integers(-3, 4, rows)
			else:
				pb['b'] = rng.normal(size=(rows, nc)) / np.sqrt(nc)
				pb['scale'] = rng.uniform(0.3, 3.0, rows)
			pb['w2'] = rng.integers(1, 5, (rows, n)).astype(F64) if exact else np.exp(rng.uniform(-1.5, 1.5, (rows, n)))
	return pb


# ---- the ladder (part 4 of the issue: the variance-keeping scale under cancellation) ----------------------------------------------------------------------------------
RHOS = [1.0, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7]
LADDER_N, LADDER_WT, LADDER_DRAWS = 2500, (0.7, 1.5), 5
BAR = 1e-6  # normvar's results to 1e-6


def ladder_rows(rho, kind, nc=3, seed=0, n=LADDER_N, dtype=F64):
	"""LADDER_DRAWS x len(LADDER_WT) rows at rho = dv2 / rms(weighted row), about: 'flat' -- y = 3 (1 + rho noise), a nearly flat row, which the intercept explains;
	'explained' -- y = a combination of the covariates + rho x its rms x noise.  nc covariates with an intercept, weights exp(0.25 N(0, 1)).
	-> y (rows, n), lnw, wt, c (nc, n)."""
	rng = np.random.default_rng(100 + seed)
	lnw = 0.25 * rng.normal(size=n)
	c = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	wt = np.repeat(np.asarray(LADDER_WT), LADDER_DRAWS)
	rows = len(wt)
	noise = rng.normal(size=(rows, n))
	if kind == 'flat':
		y = 3.0 * (1.0 + rho * noise)
	else:
		fit = rng.normal(size=(rows, nc)) @ c
		y = fit + rho * noise * np.sqrt((fit**2).mean(axis=1, keepdims=True))
	return y.astype(dtype), lnw, wt, c


def reference_two_pass(y, lnw, wt, c, tol=TOL):
	"""The reference per gene in longdouble, two-pass throughout (norm.py:150-163,244-259): -> out (rows, n), scale, rho = dv2 / rms(y e)."""
	rows, n = y.shape
	e, _ = weight(lnw, wt)
	yl, cl = ld(y), ld(c)
	out, scs, rhos = np.zeros((rows, n), LD), np.zeros(rows, LD), np.zeros(rows)
	for g in range(rows):
		ce = cl * e[g][None, :]
		yp = yl[g] * e[g]
		inv = inv_rank(ce @ ce.T, tol)[0]
		r = yp - (inv @ (ce @ yp)) @ ce
		dv = np.sqrt(((yp - yp.mean())**2).mean())
		dv2 = np.sqrt((r * r).mean())
		scs[g] = (dv / dv2)**LD(wt[g]) if wt[g] != 0 else 1
		out[g] = r * scs[g]
		rhos[g] = float(dv2 / np.sqrt((yp * yp).mean()))
	return out, scs, rhos


def emu_scale(y, lnw, wt, c, form, tol=TOL):
	"""The scale in fp64 by the one-pass sums ('one'), the two-pass form ('two') or the rule of part 4 ('rule': one-pass unless marked, then k_nv_rescale's order)."""
	rows, n = y.shape
	nc = c.shape[0]
	mom = emu_moments(y, lnw, wt, c)
	sv = emu_solve(mom, nc, n, wt, tol, 1)
	if form == 'rule':
		return emu_rescale(y, lnw, wt, c, sv['b'], sv['scale']), sv['scale'] < 0
	if form == 'two':
		return emu_rescale(y, lnw, wt, c, sv['b'], np.full(rows, MARK)), np.ones(rows, bool)
	iu = np.triu_indices(nc)
	npair = len(iu[0])
	a, s1, s2 = mom[:, npair:npair + nc], mom[:, npair + nc], mom[:, npair + nc + 1]
	mean = s1 / n
	with np.errstate(divide='ignore', invalid='ignore'):
		sc = (np.sqrt(np.maximum(s2 / n - mean * mean, 0.0)) / np.sqrt(np.maximum(s2 - (a * sv['b']).sum(axis=1), 0.0) / n))**wt
	return sc, np.zeros(rows, bool)


# ---- the judges: what the CPU file holds the emulation to and the GPU file the device ---------------------------------------------------------------------------------
def rows_pad_of(rows):
	return -(-rows // NV_R) * NV_R + NV_R  # (a whole extra workgroup of padding rows)


@functools.lru_cache(maxsize=None)
def reference(i, exact=False):
	"""The longdouble reference of CASES[i] and its bounds, computed once (read-only)."""
	pb = problem(i, exact)
	e = pb['entry']
	if e == 'weights':
		return weights(pb['y'], pb['lnw'], pb['wt'], layout(pb)['ldc'], rows_pad_of(pb['rows']))  # (U and V at the pitch the case gives its fp64 rows)
	if e == 'solve':
		return moments(pb['y'], pb['lnw'], pb['wt'], pb['c'])
	if e == 'apply':
		return apply(pb['y'], pb['lnw'], pb['wt'], pb['c'], pb['b'], pb['scale'], pb['odt'])
	return apply_w2(pb['y'], pb['w2'], pb['c'], pb['b'], pb['odt'])


def judge_weights(got, i, exact=False):
	ref, bnd = reference(i, exact)
	return {k: judge(got[k], ref[k], bnd[k], k, exact) for k in ('U', 'V', 's1', 's2')}


def judge_solve(mom, b, scale, rank, i, exact=False, tol=TOL):
	"""moments against the reference; b, rank and the scale as computed against the longdouble solve of the moments handed in (the device's own)."""
	pb = problem(i, exact)
	ref, bnd = reference(i, exact)
	ws = {'mom': judge(mom, ref, bnd, 'moments', exact)}
	if not np.isfinite(mom).all():
		return ws, None
	sv = solve(mom, pb['nc'], pb['n'], pb['wt'], tol, pb['keepvar'], b_dev=b)
	ws['rank'] = Worst(0.0 if np.array_equal(rank, sv['rank']) else np.inf, None, 'integer ranks %s against %s' % (rank.tolist(), sv['rank'].tolist()))
	fin = np.isfinite(sv['cond'])  # (a zero matrix keeps its zero eigenvalues and divides by them: nothing to compare but the rank)
	err = np.sqrt(np.asarray(((ld(b) - sv['b'])**2).sum(axis=1), F64))
	ws['b'] = worst(np.where(fin, np.nan_to_num(err, nan=np.inf), 0.0), b_bound(pb['nc'], np.where(fin, sv['cond'], 1.0), sv['bnorm']), 'b')
	one = (pb['wt'] == 0) | (pb['keepvar'] == 0)
	ws['scale is 1'] = Worst(0.0 if (scale[one] == 1.0).all() else np.inf, None, 'scale exactly 1 for wt == 0 or keepvar == 0')
	dec = fin & ~one & (sv['decided'] > 1.001)
	ws['mark'] = Worst(0.0 if np.array_equal(scale[dec] == MARK, sv['marked'][dec]) else np.inf, None, 'the mark where it is decided')
	live = dec & ~sv['marked'] & np.isfinite(sv['scale_rel'])
	with np.errstate(divide='ignore', invalid='ignore'):
		ws['scale'] = worst(np.nan_to_num(np.abs(np.asarray(ld(scale[live]) / sv['scale'][live] - 1, F64)), nan=np.inf), SLACK * sv['scale_rel'][live], 'scale as computed')
	return ws, sv


def judge_rescale(scale, b, i, marked, exact=False):
	"""After nrm_normvar_rescale: the marked genes against the longdouble two-pass scale on the coefficients handed in, where that scale is defined (a row the
	covariates reproduce exactly -- fewer cells than covariates -- has dv2 = 0 up to rounding and no scale to compare)."""
	pb = problem(i, exact)
	tp = scale_two_pass(pb['y'], pb['lnw'], pb['wt'], pb['c'], b)
	ok = marked & np.isfinite(tp['rel']) & np.isfinite(np.asarray(tp['scale'], F64)) & (np.asarray(tp['scale'], F64) > 0) & (tp['rel'] < 1e-3)
	with np.errstate(divide='ignore', invalid='ignore'):
		return worst(np.nan_to_num(np.abs(np.asarray(ld(scale[ok]) / tp['scale'][ok] - 1, F64)), nan=np.inf), SLACK * tp['rel'][ok], 'scale from the row'), ok


def judge_apply(out, i, exact=False):
	ref, bnd = reference(i, exact)
	return {'out': judge(out, ref, bnd, 'out', exact)}


def emulate(i, exact=False, mut=None):
	"""The emulation of CASES[i] -> what the judges take."""
	pb = problem(i, exact)
	e = pb['entry']
	if e == 'weights':
		return emu_weights(pb['y'], pb['lnw'], pb['wt'], reference(i, exact)[0]['U'].shape[1], rows_pad_of(pb['rows']), mut)
	if e == 'solve':
		mom = emu_moments(pb['y'], pb['lnw'], pb['wt'], pb['c'], mut)
		if not np.isfinite(mom).all():
			return dict(mom=mom, b=None, scale=None, rank=None)
		with np.errstate(all='ignore'):
			return dict(mom=mom, **emu_solve(mom, pb['nc'], pb['n'], pb['wt'], TOL, pb['keepvar'], mut, layout(pb)['ldy']))
	if e == 'apply':
		return emu_apply(pb['y'], pb['lnw'], pb['wt'], pb['c'], pb['b'], pb['scale'], pb['odt'], mut=mut)
	return dict(out=emu_apply_w2(pb['y'], pb['w2'], pb['c'], pb['b'], pb['odt'], mut))


def judge_case(got, i, exact=False):
	e = CASES[i]['entry']
	if e == 'weights':
		return judge_weights(got, i, exact)
	if e == 'solve':
		if got['b'] is None:
			return {'mom': judge(got['mom'], *reference(i, exact), 'moments', exact)}
		return judge_solve(got['mom'], got['b'], got['scale'], got['rank'], i, exact)[0]
	return judge_apply(got['out'], i, exact)
