// The host arithmetic of the whole-problem entries (nrm_host_*.hip, nrm_api.hip): whatever decides a route or a rank, and the small dense algebra between two
// kernel launches.  Like nrm_host_logic.h it is kept free of HIP headers, so that g++ can build it with -fsanitize=address,undefined for the CPU test-suite
// (tests/host/entry_math_sanitize.cpp, tests/host/front_entry_math_sanitize.cpp).  Every loop keeps the summation order it had inside the entries: their results are compared bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/normalisr_hip.h"
#include "nrm_jacobi.h"
#include "nrm_jacobi_lanes.h"
#include "nrm_nv_scale.h"

void nrm_set_error(const char* fmt, ...);

static inline void nrm_store_one(int out_dtype, void* h_out, size_t i, double v) {
	if (out_dtype == NRM_F64)
		((double*)h_out)[i] = v;
	else
		((float*)h_out)[i] = (float)v;
}
// a double vector into the caller's array of out_dtype
static inline void nrm_store_as(int out_dtype, void* h_out, const double* v, int64_t count) {
	for (int64_t i = 0; i < count; i++) nrm_store_one(out_dtype, h_out, (size_t)i, v[i]);
}

// a constant covariate row (the intercept): its index and value, or -1
static inline int nrm_constant_row(const double* c64, int64_t nc, int64_t n, double* value) {
	for (int64_t c = 0; c < nc; c++) {
		const double v = c64[c * n];
		if (v == 0.0) continue;
		bool all = true;
		for (int64_t k = 1; k < n && all; k++) all = c64[c * n + k] == v;
		if (all) {
			*value = v;
			return (int)c;
		}
	}
	*value = 0.0;
	return -1;
}

// mcc (nc, nc) = C C^T over n cells, both triangles
static inline void nrm_covariate_gram(const double* c64, int64_t nc, int64_t n, std::vector<double>& mcc) {
	mcc.assign((size_t)nc * nc, 0.0);
	for (int64_t c = 0; c < nc; c++)
		for (int64_t d = c; d < nc; d++) {
			double s = 0.0;
			for (int64_t k = 0; k < n; k++) s += c64[(size_t)(c * n + k)] * c64[(size_t)(d * n + k)];
			mcc[(size_t)(c * nc + d)] = mcc[(size_t)(d * nc + c)] = s;
		}
}

// ---- the covariates' pseudo-inverse for a caller without LAPACK (nrm_covariates_pinv, the resident coex plan) ------------------------------------------------
// covariates of c_dtype as fp64, the conversion every entry makes
static inline void nrm_covariates_to_f64(const void* h_dc, int c_dtype, size_t count, std::vector<double>& c64) {
	c64.resize(count);
	if (c_dtype == NRM_F64) {
		if (count) memcpy(c64.data(), h_dc, count * 8);
	} else
		for (size_t i = 0; i < count; i++) c64[i] = (double)((const float*)h_dc)[i];
}
// dci (nc, nc) = the pseudo-inverse of C C^T and its integer rank by the reference's rule (association.py:77-80: singular values below tol x the largest count as
// zero), for covariates with a non-zero entry; all-zero covariates are rank 0 with a zero dci (association.py:899-903 as normalisr_amd.association._prepare_covariates
// reads it).  C C^T is summed cell by cell in fp64 (nrm_covariate_gram), the eigenvalues come from the Jacobi iteration of nrm_small_pinv.  1 <= nc <= 32.
static inline int nrm_covariates_pinv_f64(const double* c64, int64_t nc, int64_t n, double tol, double* dci, int* rank) {
	bool any = false;
	for (size_t i = 0; i < (size_t)(nc * n) && !any; i++) any = c64[i] != 0.0;
	*rank = 0;
	if (!any) {
		for (int64_t i = 0; i < nc * nc; i++) dci[i] = 0.0;
		return NRM_OK;
	}
	std::vector<double> mcc;
	nrm_covariate_gram(c64, nc, n, mcc);
	for (double v : mcc)
		if (!std::isfinite(v)) {
			nrm_set_error("array must not contain infs or NaNs");
			return NRM_E_ARG;
		}
	int64_t r = 0;
	nrm_small_pinv_one<32>(mcc.data(), (int)nc, tol, dci, &r);
	*rank = (int)r;
	return NRM_OK;
}

// ---- the streaming de: a constant covariate moves to the end of Z ----------------------------------------------------------------------------
// perm[j] = the caller's index of Z's covariate j (ci last; ci < 0: the identity)
static inline std::vector<int64_t> nrm_const_last_perm(int64_t nc, int ci) {
	std::vector<int64_t> perm((size_t)nc);
	int64_t j = 0;
	for (int64_t c = 0; c < nc; c++)
		if (c != ci) perm[(size_t)j++] = c;
	if (ci >= 0) perm[(size_t)j] = ci;
	return perm;
}
// the covariates in Z's order and their pseudo-inverse permuted with them (h_dci == NULL: zeros)
static inline void nrm_permute_covariates(const double* h_c64, const double* h_dci, const std::vector<int64_t>& perm, int64_t n, std::vector<double>& hc, std::vector<double>& hd) {
	const int64_t nc = (int64_t)perm.size();
	hc.resize((size_t)nc * n);
	hd.resize((size_t)nc * nc);
	for (int64_t c = 0; c < nc; c++) memcpy(&hc[(size_t)(c * n)], h_c64 + perm[(size_t)c] * n, (size_t)n * 8);
	for (int64_t a = 0; a < nc; a++)
		for (int64_t b = 0; b < nc; b++) hd[(size_t)(a * nc + b)] = h_dci ? h_dci[perm[(size_t)a] * nc + perm[(size_t)b]] : 0.0;
}
// coefficients (cnt, nc) of es bytes each in Z's covariate order back into the caller's
static inline void nrm_alpha_unpermute(const char* z_order, const std::vector<int64_t>& perm, size_t cnt, size_t es, void* h_alpha) {
	const size_t nc = perm.size();
	for (size_t i = 0; i < cnt; i++)
		for (size_t c = 0; c < nc; c++) memcpy((char*)h_alpha + (i * nc + (size_t)perm[c]) * es, z_order + (i * nc + c) * es, es);
}

// ---- single=1 with more than 8 covariates: the groupings' statistics (association.py:350-374) ---------------------------------------------------
// cells per grouping, ns[i] = n_common + its own; NRM_E_NUMERIC for a grouping with a single value on its cells (:917-918).  hrows (nx, 3): own cells, min, max
static inline int nrm_single1_cell_counts(const double* hrows, int64_t n_common, int64_t nx, std::vector<double>& ns) {
	ns.resize((size_t)nx);
	for (int64_t i = 0; i < nx; i++) {
		ns[(size_t)i] = (double)n_common + hrows[(size_t)i * 3];
		double lo = hrows[(size_t)i * 3 + 1], hi = hrows[(size_t)i * 3 + 2];
		if (n_common > 0) {
			lo = lo < 0.0 ? lo : 0.0;
			hi = hi > 0.0 ? hi : 0.0;
		}
		if (!(hi > lo)) {  // > 1 distinct value among the selected cells (:917-918)
			nrm_set_error("grouping %lld has a single value on the cells selected for it (association.py:917-918)", (long long)i);
			return NRM_E_NUMERIC;
		}
	}
	return NRM_OK;
}
// covariate Gram of the shared cells: the selection kernel's partial sums (8 x 8 blocks on and above the diagonal, gb partials each) added up in a fixed order
static inline void nrm_single1_reduce_gram(const double* hpart, int64_t gb, int64_t nc, std::vector<double>& mcc) {
	const int64_t nb = (nc + 7) / 8;
	mcc.assign((size_t)nc * nc, 0.0);
	int64_t q = 0;
	for (int64_t bi = 0; bi < nb; bi++)
		for (int64_t bj = bi; bj < nb; bj++, q++) {
			double blk[64];
			for (int e = 0; e < 64; e++) blk[e] = 0.0;
			for (int64_t g = 0; g < gb; g++)
				for (int e = 0; e < 64; e++) blk[e] += hpart[(size_t)((q * gb + g) * 64 + e)];
			for (int i = 0; i < 8; i++)
				for (int j = 0; j < 8; j++) {
					const int64_t a = bi * 8 + i, b = bj * 8 + j;
					if (a < nc && b < nc) mcc[(size_t)(a * nc + b)] = mcc[(size_t)(b * nc + a)] = blk[i * 8 + j];
				}
		}
}
// the groupings' own sums over their own cells, gs (nx, nc (nc + 1) / 2 + nc + 1): M_i = C_S C_S^T (upper, packed), C_S x_S, |x_S|^2 (association.py:350-364)
static inline void nrm_single1_group_sums(const int64_t* hseg, const int64_t* hidx, const double* hxe, const double* c64, int64_t n, int64_t nc, int64_t nx, std::vector<double>& gs) {
	const int64_t gsw = nc * (nc + 1) / 2 + nc + 1;
	gs.assign((size_t)nx * gsw, 0.0);
	for (int64_t i = 0; i < nx; i++) {
		double* o = &gs[(size_t)i * gsw];
		for (int64_t e = hseg[(size_t)i]; e < hseg[(size_t)i + 1]; e++) {
			const int64_t k = hidx[(size_t)e];
			const double x = hxe[(size_t)e];
			int64_t w = 0;
			for (int64_t c = 0; c < nc; c++)
				for (int64_t d = c; d < nc; d++) o[w++] += c64[(size_t)(c * n + k)] * c64[(size_t)(d * n + k)];
			for (int64_t c = 0; c < nc; c++) o[w++] += c64[(size_t)(c * n + k)] * x;
			o[w] += x * x;
		}
	}
}
// per grouping: pseudo-inverse of M_i (integer rank), ccx, vx, dof -- rec (nx, pitch = 26 + nc + nc nc): ns, vx, [the P-value plan: the caller], ccx at 26, M_i^+ after it
static inline int nrm_single1_group_records(const std::vector<double>& gs, const std::vector<double>& mcc, const std::vector<double>& ns, int64_t nc, int64_t nx, int dimreduce,
									 std::vector<double>& rec, std::vector<double>& vxx, std::vector<double>& dof) {
	const int64_t pitch = 26 + nc + nc * nc, npair = nc * (nc + 1) / 2, gsw = npair + nc + 1;
	rec.assign((size_t)nx * pitch, 0.0);
	dof.resize((size_t)nx);
	vxx.resize((size_t)nx);
	std::vector<int64_t> rk((size_t)nx, 0);
	std::vector<double> mc((size_t)nx * nc * nc), mi((size_t)nx * nc * nc);
	for (int64_t i = 0; i < nx; i++) {
		const double* o = &gs[(size_t)i * gsw];
		int64_t w = 0;
		for (int64_t c = 0; c < nc; c++)
			for (int64_t d = c; d < nc; d++, w++) mc[(size_t)((i * nc + c) * nc + d)] = mc[(size_t)((i * nc + d) * nc + c)] = o[w] + mcc[(size_t)(c * nc + d)];
	}
	for (size_t e = 0; e < mc.size(); e++)
		if (!std::isfinite(mc[e])) {
			nrm_set_error("array must not contain infs or NaNs");
			return NRM_E_ARG;
		}
	const int rc = nrm_small_pinv(mc.data(), nx, nc, 1e-8, mi.data(), rk.data(), 0);  // association.py:350-351
	if (rc) return rc;
	for (int64_t i = 0; i < nx; i++) {
		double* r = &rec[(size_t)i * pitch];
		const double* o = &gs[(size_t)i * gsw];
		const double* xc = o + npair;
		double* m = &mi[(size_t)i * nc * nc];
		if (rk[(size_t)i] == 0) memset(m, 0, (size_t)nc * nc * 8);
		double xx = o[npair + nc];
		for (int64_t c = 0; c < nc; c++) {
			double t = 0.0;
			for (int64_t d = 0; d < nc; d++) t += m[c * nc + d] * xc[d];
			r[26 + c] = t;  // ccx
		}
		for (int64_t c = 0; c < nc; c++) xx -= xc[c] * r[26 + c];
		memcpy(r + 26 + nc, m, (size_t)nc * nc * 8);
		vxx[(size_t)i] = xx / ns[(size_t)i];
	}
	for (int64_t i = 0; i < nx; i++) {
		if (vxx[(size_t)i] == 0.0) vxx[(size_t)i] = 1.0;  // association.py:362-364
		dof[(size_t)i] = ns[(size_t)i] - 1 - (double)rk[(size_t)i] - dimreduce;
		if (dof[(size_t)i] <= 0) {
			nrm_set_error("Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.");
			return NRM_E_DEVICE;
		}
		rec[(size_t)i * pitch] = ns[(size_t)i];
		rec[(size_t)i * pitch + 1] = vxx[(size_t)i];
	}
	return NRM_OK;
}

// ---- normvar with 9 .. 32 covariates: b_g = M_g^+ a_g and the variance-keeping scale (norm.py:248-259) ---------------------------------------------
// mi (rows, nc, nc); a_g = hga + g lda; s1 / s2: the genes' sums and sums of squares; hscale stays 1 without keepvar
static inline void nrm_normvar_coefficients(const double* mi, const double* hga, int64_t lda, const double* hs1, const double* hs2, const double* h_wt, int64_t rows, int64_t nc, int64_t n,
									 int keepvar, std::vector<double>& hb, std::vector<double>& hscale) {
	hb.resize((size_t)rows * nc);
	hscale.assign((size_t)rows, 1.0);
	for (int64_t g = 0; g < rows; g++) {
		const double* a = &hga[(size_t)(g * lda)];
		double ab = 0.0;
		for (int64_t q = 0; q < nc; q++) {
			double t = 0.0;
			for (int64_t d = 0; d < nc; d++) t += mi[(size_t)((g * nc + q) * nc + d)] * a[d];
			hb[(size_t)(g * nc + q)] = t;
			ab += a[q] * t;
		}
		if (keepvar) hscale[(size_t)g] = nrm_nv_scale(hs1[(size_t)g], hs2[(size_t)g], ab, (double)n, h_wt[g]);  // (NRM_NV_MARK where the sums have cancelled: nrm_normvar_rescale)
	}
}

// ---- single=4's closed form -------------------------------------------------------------------------------------------------------------------
// Inverse of a symmetric positive definite matrix in place: Cholesky factor, triangular inverse, L^-T L^-1; false when the matrix is not positive definite
static inline bool nrm_spd_inverse_host(std::vector<double>& m, int64_t n) {
	std::vector<double> l((size_t)n * n, 0.0);
	for (int64_t j = 0; j < n; j++) {
		double d = m[(size_t)(j * n + j)];
		for (int64_t k = 0; k < j; k++) d -= l[(size_t)(j * n + k)] * l[(size_t)(j * n + k)];
		if (!(d > 0)) return false;
		l[(size_t)(j * n + j)] = std::sqrt(d);
		for (int64_t i = j + 1; i < n; i++) {
			double s = m[(size_t)(i * n + j)];
			for (int64_t k = 0; k < j; k++) s -= l[(size_t)(i * n + k)] * l[(size_t)(j * n + k)];
			l[(size_t)(i * n + j)] = s / l[(size_t)(j * n + j)];
		}
	}
	std::vector<double> li((size_t)n * n, 0.0);  // L^-1, lower triangular
	for (int64_t j = 0; j < n; j++) {
		li[(size_t)(j * n + j)] = 1.0 / l[(size_t)(j * n + j)];
		for (int64_t i = j + 1; i < n; i++) {
			double s = 0.0;
			for (int64_t k = j; k < i; k++) s -= l[(size_t)(i * n + k)] * li[(size_t)(k * n + j)];
			li[(size_t)(i * n + j)] = s / l[(size_t)(i * n + i)];
		}
	}
	for (int64_t i = 0; i < n; i++)
		for (int64_t j = 0; j <= i; j++) {
			double s = 0.0;
			for (int64_t k = i; k < n; k++) s += li[(size_t)(k * n + i)] * li[(size_t)(k * n + j)];
			m[(size_t)(i * n + j)] = m[(size_t)(j * n + i)] = s;
		}
	return true;
}

// N~ = M~^-1 when the device's Newton-Schulz iteration did not converge.  hm: M~ (pitch nxp, upper triangle valid), hss: |x~_i|^2.  Gives *norm_mt = ||M~||_1,
// npad = N~ (nxp, nxp; zero padding) and small (3, nx) = its diagonal / kappa numerators / absolute row sums; false: M~ is not positive definite
static inline bool nrm_spd_inverse_fallback(const double* hm, const double* hss, int64_t nx, int64_t nxp, double* norm_mt, std::vector<double>& npad, std::vector<double>& small) {
	std::vector<double> a((size_t)nx * nx);
	for (int64_t i = 0; i < nx; i++)
		for (int64_t j = 0; j < nx; j++) a[(size_t)(i * nx + j)] = i <= j ? hm[(size_t)(i * nxp + j)] : hm[(size_t)(j * nxp + i)];
	*norm_mt = 0.0;
	for (int64_t j = 0; j < nx; j++) {
		double s = 0.0;
		for (int64_t i = 0; i < nx; i++) s += std::fabs(a[(size_t)(i * nx + j)]);
		*norm_mt = s > *norm_mt ? s : *norm_mt;
	}
	if (!nrm_spd_inverse_host(a, nx)) return false;
	npad.assign((size_t)nxp * nxp, 0.0);
	small.assign((size_t)3 * nx, 0.0);
	for (int64_t i = 0; i < nx; i++) {
		for (int64_t j = 0; j < nx; j++) {
			const double v = a[(size_t)(i * nx + j)];
			npad[(size_t)(i * nxp + j)] = v;
			small[(size_t)(nx + i)] += std::fabs(v) * std::sqrt(hss[(size_t)j]);
			small[(size_t)(2 * nx + i)] += std::fabs(v);
		}
		small[(size_t)i] = a[(size_t)(i * nx + i)];
	}
	return true;
}

// Does the closed form apply to a design with full-rank covariates?  The reference's own rank test on A A^T (singular values >= tol x the largest,
// association.py:77), settled from norms at hand (single4.py: _surely_full_rank): lambda_max <= ||M~||_1 + ||a||_F^2 ||Mcc^-1|| + ||Mcc||,
// 1 / lambda_min <= ||N~||_1 (1 + ||b||_F)^2 + ||Mcc^-1||.  bx (nx, nc), mcc = C C^T (nc <= 32); nc == 0: the norms of M~ alone.
static inline int nrm_full_rank_certified(double norm_mt, double norm_ninv, const double* bx, const double* mcc, int64_t nx, int64_t nc, double tol, bool* certified) {
	double lam_max = norm_mt, inv_norm = norm_ninv;
	*certified = false;
	if (nc) {
		std::vector<double> ev((size_t)nc);
		const int rc = nrm_small_eigvals(mcc, nc, ev.data());
		if (rc) return rc;
		double a2 = 0.0, b2 = 0.0;
		for (int64_t i = 0; i < nx; i++)
			for (int64_t c = 0; c < nc; c++) {
				double a = 0.0;
				for (int64_t d = 0; d < nc; d++) a += bx[(size_t)(i * nc + d)] * mcc[(size_t)(d * nc + c)];
				a2 += a * a;
				b2 += bx[(size_t)(i * nc + c)] * bx[(size_t)(i * nc + c)];
			}
		if (!(ev[0] > 0)) lam_max = NAN;
		else {
			lam_max = norm_mt + a2 / ev[0] + ev[(size_t)nc - 1];
			inv_norm = norm_ninv * (1.0 + std::sqrt(b2)) * (1.0 + std::sqrt(b2)) + 1.0 / ev[0];
		}
	}
	*certified = std::isfinite(lam_max) && std::isfinite(inv_norm) && lam_max > 0 && inv_norm > 0 && 1.0 / (inv_norm * lam_max) >= 2.0 * tol;
	return NRM_OK;
}

// Does the closed form on rows residualised with the pseudo-inverse of C C^T (rank < nc) give the reference's per-grouping results?  Every T_i --
// A A^T without row and column i, which association.py:521-530 pseudo-inverts -- must have the rank nx - 1 + rank at `tol` (association.py:77).
// The certificate of single4.py (pinv_rank_certificate): with Mcc = V diag(w) V^T split into kept and dropped eigenvectors and eps0 the largest
// dropped eigenvalue, eps0 <= tol w_max / 2, and lambda_min(R) - ||E|| - eps0 >= 2 tol (lambda_max(R) + ||E|| + eps0), R the Gram matrix of
// [X; V_r^T C] bounded from ||M~||_1, ||N~||_1 and b V_r, ||E|| <= ||X||_F sqrt(eps0).  mcc is destroyed.
static inline bool nrm_pinv_rank_certified(std::vector<double>& mcc, int64_t nc, int rank, const double* bx, const double* ssx, int64_t nx, double norm_mt, double norm_ninv,
									double tol) {
	std::vector<double> v((size_t)nc * nc), w((size_t)nc);
	nrm_jacobi(mcc.data(), v.data(), w.data(), (int)nc);
	double lam1 = 0.0;
	for (int64_t k = 0; k < nc; k++) lam1 = w[(size_t)k] > lam1 ? w[(size_t)k] : lam1;
	if (!(lam1 > 0) || !std::isfinite(lam1)) return false;
	double eps0 = 0.0, wmin = INFINITY, wmax = 0.0;
	int kept = 0;
	for (int64_t k = 0; k < nc; k++) {
		const double e = w[(size_t)k];
		if (!std::isfinite(e)) return false;
		if (e >= tol * lam1) {
			kept++;
			wmin = e < wmin ? e : wmin;
			wmax = e > wmax ? e : wmax;
		} else if (e > eps0)
			eps0 = e;
	}
	if (kept != rank || !(eps0 <= 0.5 * tol * lam1)) return false;
	double a2 = 0.0, b2 = 0.0, xf2 = 0.0;
	for (int64_t i = 0; i < nx; i++) {
		xf2 += ssx[(size_t)i];
		for (int64_t k = 0; k < nc; k++) {
			const double e = w[(size_t)k];
			if (!(e >= tol * lam1)) continue;
			double br = 0.0;  // (b V_r)_ik
			for (int64_t d = 0; d < nc; d++) br += bx[(size_t)(i * nc + d)] * v[(size_t)(d * nc + k)];
			a2 += br * br * e * e;
			b2 += br * br;
			xf2 += br * br * e;
		}
	}
	const double lam_max = norm_mt + a2 / wmin + wmax;
	const double inv_norm = norm_ninv * (1.0 + std::sqrt(b2)) * (1.0 + std::sqrt(b2)) + 1.0 / wmin;
	const double e = std::sqrt((xf2 > 0 ? xf2 : 0.0) * eps0);
	const double lo = 1.0 / inv_norm - e - eps0, hi = lam_max + e + eps0;
	return std::isfinite(lo) && std::isfinite(hi) && norm_mt > 0 && norm_ninv > 0 && hi > 0 && lo >= 2.0 * tol * hi;
}

// alpha_y = b_y - B_y b_x, the same for every grouping (association.py:551-553 in the closed form): B^T (ny, nx; pitch ldbt) against b_x (nx, nc), written
// to h_alpha (nx, ny, nc) of out_dtype
static inline void nrm_single4_alpha(const double* hbt, int64_t ldbt, const double* hby, const double* hbx, int64_t nx, int64_t ny, int64_t nc, int out_dtype, void* h_alpha) {
	for (int64_t y = 0; y < ny; y++)
		for (int64_t c = 0; c < nc; c++) {
			double s = hby[(size_t)(y * nc + c)];
			for (int64_t i = 0; i < nx; i++) s -= hbt[(size_t)(y * ldbt + i)] * hbx[(size_t)(i * nc + c)];
			for (int64_t i = 0; i < nx; i++) nrm_store_one(out_dtype, h_alpha, (size_t)(i * ny + y) * nc + c, s);
		}
}

// ---- the front half: lcpm, compute_var, qc_reads (nrm_host_front.hip) ---------------------------------------------------------------------------------------
// lcpm's two tables from the digamma values (lcpm.py:107,158): tab[x] = psi(1 + x) - psi(t0), etab[x] = exp(tab[x]) -- exp() once per table entry -- and
// unit = max over x >= 1 of (etab[x] - etab[0]) / x, the bound of one stored entry's term in nrm_lcpm_csr_colsum's fixed-point sum (0 for a table of one entry)
static inline double nrm_lcpm_tables(const double* psi, double psi_t0, int64_t len, std::vector<double>& tab, std::vector<double>& etab) {
	tab.resize((size_t)len);
	etab.resize((size_t)len);
	for (int64_t x = 0; x < len; x++) {
		tab[(size_t)x] = psi[x] - psi_t0;
		etab[(size_t)x] = std::exp(tab[(size_t)x]);
	}
	double unit = 0.0;
	for (int64_t x = 1; x < len; x++) {
		const double u = (etab[(size_t)x] - etab[0]) / (double)x;
		unit = u > unit ? u : unit;
	}
	return unit;
}
// lcpm's three covariate rows from the integer totals (lcpm.py:194-200): cov (3, n) = ln total, genes without a read, ln^2 total.  Returns the first cell
// without a read (lcpm.py:196 raises for it; its column is left unwritten), -1 when every cell has one
static inline int64_t nrm_lcpm_cov_rows(const int64_t* cell_total, const int64_t* cell_nnz, int64_t rows, int64_t n, double* cov) {
	for (int64_t k = 0; k < n; k++) {
		if (cell_total[k] <= 0) return k;
		const double t = std::log((double)cell_total[k]);
		cov[k] = t;
		cov[n + k] = (double)(rows - cell_nnz[k]);
		cov[2 * n + k] = t * t;
	}
	return -1;
}
// (x x^T)^+ for x (r, n), 1 <= r <= 64, on rows scaled to unit length: D pinv(D x x^T D) D with D = diag(1 / |row|), all-zero rows left as they are
// (norm._pinv_gram_unit_rows: the rank rule, relative to the largest eigenvalue, then does not depend on the units of the rows).  The Jacobi routine of
// nrm_fitvar_pinv_host, one lane.  *rank = the eigenvalues kept
static inline void nrm_pinv_gram_unit_rows(const double* x, int64_t r, int64_t n, double tol, double* inv, int64_t* rank) {
	std::vector<double> d((size_t)r), xs((size_t)r * n), a((size_t)(2 * r * r + 3 * r));
	for (int64_t i = 0; i < r; i++) {
		double s = 0.0;
		for (int64_t k = 0; k < n; k++) s += x[i * n + k] * x[i * n + k];
		s = std::sqrt(s);
		d[(size_t)i] = 1.0 / (s > 0 ? s : 1.0);
		for (int64_t k = 0; k < n; k++) xs[(size_t)(i * n + k)] = x[i * n + k] * d[(size_t)i];
	}
	nrm_covariate_gram(xs.data(), r, n, a);
	a.resize((size_t)(2 * r * r + 3 * r));
	nrm_pinv_lanes(NrmSerialLanes(), a.data(), a.data() + r * r, a.data() + 2 * r * r, a.data() + 2 * r * r + r, (int)r, tol, inv, rank);
	for (int64_t i = 0; i < r; i++)
		for (int64_t j = 0; j < r; j++) inv[i * r + j] *= d[(size_t)i] * d[(size_t)j];  // (symmetric to the bit, as the routine's own result)
}
// the six integer thresholds of one qc_reads iteration on nt genes x ns cells still alive (qc.py:56-71): a count is an integer, so `count >= bound` with a
// double bound is `count >= ceil(bound)`; the proportional bounds are taken of the CURRENT numbers.  params = n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell
static inline void nrm_qc_thresholds(const double* params, int64_t nt, int64_t ns, int64_t* thr) {
	thr[0] = (int64_t)std::ceil(params[0]);
	thr[1] = (int64_t)std::ceil(params[1]);
	thr[2] = (int64_t)std::ceil(params[2] * (double)ns);
	thr[3] = (int64_t)std::ceil(params[3]);
	thr[4] = (int64_t)std::ceil(params[4]);
	thr[5] = (int64_t)std::ceil(params[5] * (double)nt);
}
