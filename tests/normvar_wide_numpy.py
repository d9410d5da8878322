"""float64 numpy restatement of normvar's basis form for many covariates -- TEST INFRASTRUCTURE ONLY.

Written from the mathematics of DESIGN.md ("normvar with hundreds of covariates"), not from the package: one orthonormal basis B of the covariates' row space
(eigen-decomposition of dc dc^T, the rank by the rule of the reference's inv_rank), then per gene the positive definite system
    M_g b_g = a_g,   M_g = B diag(e_g^2) B^T,   a_g = B (e_g^2 o y_g),   e_gk = w_k^wt_g,
solved by Cholesky, the residual e_g o (y_g - b_g B) and the variance-keeping scale (dv / dv2)^wt_g with dv2^2 = (s2 - a . b) / n.  Pinned against what the
reference returned (tests/golden/G22_wide_covariates.npz, tests/test_wide_covariates_cpu.py); the check of the device path at shapes the fixture does not hold."""
import numpy as np


def basis(dc, tol=1E-8):
	"""(B, r, eigenvalues in descending order): B (r, n) orthonormal rows spanning the rows of dc."""
	dc = np.asarray(dc, dtype=np.float64)
	lam, u = np.linalg.eigh(dc @ dc.T)
	lam, u = lam[::-1], u[:, ::-1]
	r = int((lam >= tol * lam[0]).sum())
	return (u[:, :r] / np.sqrt(lam[:r])).T @ dc, r, lam


def normvar(dt, dc, w, wt, keepvar=True, tol=1E-8):
	"""dtn of the reference's normvar (normmean=False), through the basis and a Cholesky solve per gene."""
	from scipy.linalg import cho_factor, cho_solve
	dt, w, wt = np.asarray(dt, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(wt, dtype=np.float64)
	b, r, _ = basis(dc, tol)
	n = dt.shape[1]
	out = np.empty_like(dt)
	for g in range(dt.shape[0]):
		e = w**wt[g] if wt[g] != 0 else np.ones(n)
		e2 = e * e
		m = (b * e2) @ b.T
		a = b @ (e2 * dt[g])
		coef = cho_solve(cho_factor(m), a)
		res = e * (dt[g] - coef @ b)
		if keepvar:
			yp = dt[g] * e
			s1, s2 = yp.sum(), (yp * yp).sum()
			dv = np.sqrt(max(s2 / n - (s1 / n)**2, 0.0))
			dv2 = np.sqrt(max(s2 - a @ coef, 0.0) / n)
			res = res * (dv / dv2)**wt[g]
		out[g] = res
	return out
