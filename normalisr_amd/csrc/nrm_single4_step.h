// single=4 in closed form (association.py:421-576,926-980) on the device, written once: the sizes, the buffers and the launch sequences that
// nrm_association_tests_single4_host / _pinv_host (nrm_host_single4.hip) and the resident plan (nrm_single4_plan.hip) both run.  Two halves:
//   the DESIGN side (alloc_design_side), which needs the design and the covariates only -- |x~|^2 and b_x, M~ = X~ X~^T, N~ = M~^-1 by Newton-Schulz iteration on
//   the fp64 Gram kernel (the host's Cholesky factorisation when that does not converge), dxx, varx, ||M~||_1, ||N~||_1 and the rank certificate of nrm_host_math.h;
//   the GENE side (enqueue), which needs the expression matrix -- G = Y~ X~^T, |y~|^2 and b_y on request, B^T = G N~, nrm_single4_sweep.
// Each on one of two routes: the sparse-design kernels on the design's lists (`sparse`), or K1 and the fp64 Gram kernel on the dense design rows.  The caller sets
// the sizes and the non-owning pointers; `take(DevBuf&, bytes)` allocates what the record keeps (the plan's counts pool bytes, the entries pass nrm_take_plain).
// Only the alloc_* members allocate, synchronise or read back -- the design side is one of them; what enqueue queues, a plan captures.
#pragma once
#include "nrm_host_entry.h"
#include "nrm_de_sparse_step.h"

// Inverse of the symmetric positive definite matrix whose upper tiles are in d_m (nxp x nxp) by Newton-Schulz iteration on the fp64 Gram kernel
// (normalisr_amd/single4.py: _spd_inverse_device); d_n (nxp x nxp) receives the inverse (zero padding), small (3, nx) its diagonal / kappa numerators / absolute
// row sums; *norm1 = ||M||_1.  *ok = 0: not converged (the caller takes the host's Cholesky factorisation).
static inline int nrm_spd_inverse_device(const double* d_m, int64_t nx, int64_t nxp, const double* d_ss, double* d_n, std::vector<double>& small, double* norm1, int* ok,
										 void* gwork, hipStream_t st) {
	*ok = 0;
	DevBuf mp, t, tt, xt, x, scal, work, res, dsmall;
	const size_t mb = (size_t)nxp * nxp * 8;
	for (DevBuf* b : {&mp, &t, &tt, &xt, &x}) NRM_TRY(b->alloc(mb));
	NRM_TRY(scal.alloc(16));
	NRM_TRY(work.alloc((size_t)std::max<int64_t>(2 * nxp, (nxp / 32) * (nxp / 32)) * 8));
	NRM_TRY(res.alloc(8));
	NRM_TRY(nrm_spd_prepare(d_m, nxp, nx, nxp, mp.as<double>(), scal.as<double>(), work.as<double>(), st));
	double hs[2];
	NRM_HIP(hipMemcpyAsync(hs, scal.p, 16, hipMemcpyDeviceToHost, st));
	NRM_HIP(hipStreamSynchronize(st));
	*norm1 = hs[0];
	if (!std::isfinite(hs[0]) || hs[0] <= 0) return NRM_OK;
	bool done = false;
	for (int start = 0; start < 2 && !done; start++) {  // diag(1 / M_ii) first (nearly orthogonal rows: five steps), then I / ||M||_1 (always converges)
		NRM_TRY(nrm_spd_start(mp.as<double>(), nxp, start == 0 ? 1 : 0, scal.as<double>(), x.as<double>(), st));
		const int look_from = start == 0 ? 2 : 4;
		bool diverged = false;
		for (int it = 0; it < 60; it++) {
			NRM_TRY(nrm_gram_f64(mp.as<double>(), x.as<double>(), nxp, nxp, nxp, nxp, nxp, t.as<double>(), nxp, 0, 0, 0, gwork, st));  // T = M X
			NRM_TRY(nrm_spd_transpose_residual(t.as<double>(), nxp, tt.as<double>(), res.as<double>(), work.as<double>(), st));
			double r = INFINITY;
			if (it >= look_from) {
				NRM_HIP(hipMemcpyAsync(&r, res.p, 8, hipMemcpyDeviceToHost, st));
				NRM_HIP(hipStreamSynchronize(st));
			}
			if (std::isnan(r) || (start == 0 && it == look_from && !(r < 1.0))) {
				diverged = true;
				break;
			}
			NRM_TRY(nrm_gram_f64(x.as<double>(), tt.as<double>(), nxp, nxp, nxp, nxp, nxp, xt.as<double>(), nxp, 0, 0, 0, gwork, st));  // X T
			NRM_TRY(nrm_spd_update(x.as<double>(), xt.as<double>(), nxp * nxp, st));
			if (r < 1e-7) {
				done = true;
				break;
			}
		}
		if (start == 1 && diverged) return NRM_OK;
	}
	if (!done) return NRM_OK;
	NRM_TRY(dsmall.alloc((size_t)3 * nx * 8));
	NRM_TRY(nrm_spd_finish(x.as<double>(), nx, nxp, d_ss, d_n, dsmall.as<double>(), st));
	NRM_HIP(hipStreamSynchronize(st));  // (st may be a non-blocking stream, which a plain hipMemcpy does not wait for)
	NRM_TRY(download(small, dsmall.p, (size_t)3 * nx));
	*ok = 1;
	return NRM_OK;
}

struct NrmSingle4Step {
	int64_t rows = 0, nx = 0, ny = 0, n = 0, ldx = 0, ldy = 0, nc = 0;  // rows: the design rows the buffers are sized for; nx <= rows: those of the design at hand
	int x_dtype = NRM_F64, y_dtype = NRM_F64, out_dtype = NRM_F64, rank = 0, dimreduce = 0, return_dot = 0, ci = -1;  // ci: the constant covariate, or -1
	bool want_alpha = false, sparse = false;  // sparse: the route
	double cval = 0.0, tol = 1e-8;
	int64_t kp = 0, nxp = 0, nyp = 0, rows_pad = 0;  // kp, nyp, rows_pad: alloc_fixed; nxp = nx rounded up to the row tile: alloc_design_side
	const char* who = "";                            // the caller's name in the certificates' refusals
	const NrmDesignLists* L = nullptr;               // the lists of the nx rows (the sparse route)
	const void* d_x = nullptr;                       // the nx design rows as a matrix (nx, n) of x_dtype, pitch ldx
	const void* d_y = nullptr;                       // the expression matrix (ny, n) of y_dtype, pitch ldy
	const double *d_c = nullptr, *d_dci = nullptr;   // covariates (nc, n) fp64, their pseudo-inverse
	const double* h_c64 = nullptr;                   // the covariates on the host (the certificates' C C^T)
	void *p = nullptr, *stat = nullptr, *vary = nullptr;  // the sweep's outputs (nx, ny) of out_dtype, pitch ny
	// what the design side leaves on the host: the norms, dxx (nx) = 1 / (n N~_ii), b_x (nx, nc)
	double norm_mt = 0.0, norm_ninv = 0.0;
	std::vector<double> dxx, hbx;
	// flags: the counters int32[8] -- [0], [1] nrm_single4_sweep, [2] rows handed back by the sparse-design kernels --, cleared at alloc and by whoever reads them
	DevBuf flags, gwork, ssx, bx, mt, dn, ddxx, dvarx, g, ssy, by, bt, work, rxd, ryd;
	NrmSparseProducts pw;  // the sparse route's workspace for the genes' products

	double dof() const { return (double)(n - nx - rank - dimreduce); }
	int64_t ldb() const { return nc > 0 ? nc : 1; }

	// the derived sizes, and what both routes need, for all `rows` design rows
	template <typename Take>
	int alloc_fixed(Take take, hipStream_t st) {
		kp = nrm_round_up(n, NRM_K_TILE), rows_pad = nrm_round_up(rows, NRM_ROW_TILE), nyp = nrm_round_up(ny, NRM_ROW_TILE);
		NRM_TRY(nrm_take_all(take, {{&flags, 32}, {&gwork, nrm_gram_workspace_bytes()}, {&ssx, rows_pad * 8}, {&bx, rows * ldb() * 8}, {&mt, rows_pad * rows_pad * 8},
									{&dn, rows_pad * rows_pad * 8}, {&ddxx, rows * 8}, {&dvarx, rows * 8}, {&g, nyp * rows_pad * 8}, {&ssy, nyp * 8}, {&bt, nyp * rows_pad * 8},
									{&work, ny * 8}}));
		if (want_alpha) NRM_TRY(take(by, (size_t)ny * nc * 8));
		NRM_HIP(hipMemsetAsync(flags.p, 0, 32, st));
		return NRM_OK;
	}
	template <typename Take>
	int alloc_sparse(Take take, hipStream_t st) {
		return pw.common.p ? NRM_OK : pw.alloc(ny, n, nc, ci, take, st);
	}
	// the dense route's residual rows, in one piece each
	template <typename Take>
	int alloc_dense(Take take) {
		if (rxd.p) return NRM_OK;
		NRM_TRY(take(rxd, (size_t)rows_pad * kp * 8));
		return take(ryd, (size_t)nyp * kp * 8);
	}

	// The design side on the route at hand, eagerly and with its read-backs.  *handed_back > 0 (sparse route only): that many design rows all but inside the span of
	// the covariates -- nothing further was computed; the caller takes the dense route and calls again.  NRM_E_UNSUPPORTED: M~ is not positive definite, or the
	// closed form has no certificate at `tol`.
	int alloc_design_side(hipStream_t st, int64_t* handed_back) {
		*handed_back = 0;
		nxp = nrm_round_up(nx, NRM_ROW_TILE);
		NRM_HIP(hipMemsetAsync(ssx.p, 0, (size_t)nxp * 8, st));
		NRM_HIP(hipMemsetAsync(bx.p, 0, (size_t)nx * ldb() * 8, st));
		NRM_HIP(hipMemsetAsync(g.p, 0, (size_t)nyp * nxp * 8, st));  // (K2 leaves pure-padding sub-blocks unwritten; whatever the other route left there goes)
		if (sparse) {
			int32_t hf[4];
			NRM_TRY(nrm_design_stats(L->row_ptr.as<int64_t>(), L->cells.as<int32_t>(), L->row_vals.as<double>(), d_c, n, nc, d_dci, nx, ssx.as<double>(),
									 nc ? bx.as<double>() : nullptr, flags.as<int32_t>(), st));
			DevBuf ss2;  // (|x~|^2 again, as the product kernel computes it for its rows: not used)
			NRM_TRY(ss2.alloc((size_t)nxp * 8));
			// M~ = X~ X~^T: the genes' product with the design rows in the place of the expression rows
			NRM_TRY(sparse_products(*L, d_x, x_dtype, nx, n, d_c, nc, ci, cval, d_dci, bx.as<double>(), ldb(), mt.as<double>(), nxp, 0, ss2.as<double>(),
									nullptr, flags.as<int32_t>(), st));
			// a design row all but inside the span of the covariates is known HERE: before the inverse and the genes' products, which the dense route would only repeat
			NRM_TRY(nrm_read_flags(flags.p, st, hf));
			if (hf[2] > 0) {
				*handed_back = hf[2];
				NRM_HIP(hipMemsetAsync(flags.p, 0, 32, st));
				return NRM_OK;
			}
		} else {
			NRM_TRY(nrm_residualize(d_x, x_dtype, nx, n, ldx, d_c, nc, n, d_dci, rank, rxd.as<double>(), kp, nxp, ssx.as<double>(), nc ? bx.as<double>() : nullptr, st));
			NRM_TRY(nrm_gram_f64(rxd.as<double>(), rxd.as<double>(), nxp, nxp, kp, kp, kp, mt.as<double>(), nxp, 1, nx, nx, gwork.p, st));
		}
		// N~ = M~^-1
		std::vector<double> small;
		int okdev = 0;
		NRM_TRY(nrm_spd_inverse_device(mt.as<double>(), nx, nxp, ssx.as<double>(), dn.as<double>(), small, &norm_mt, &okdev, gwork.p, st));
		if (!okdev) {  // the host's Cholesky factorisation
			std::vector<double> hm, hss, npad;
			NRM_HIP(hipStreamSynchronize(st));
			NRM_TRY(download(hm, mt.p, (size_t)nxp * nxp));
			NRM_TRY(download(hss, ssx.p, (size_t)nx));
			if (!nrm_spd_inverse_fallback(hm.data(), hss.data(), nx, nxp, &norm_mt, npad, small)) return dependent();
			NRM_HIP(hipMemcpy(dn.p, npad.data(), npad.size() * 8, hipMemcpyHostToDevice));
		}
		norm_ninv = 0.0;
		dxx.assign((size_t)nx, 0.0);
		for (int64_t i = 0; i < nx; i++) {
			const double d = small[(size_t)i];
			if (!std::isfinite(d) || !std::isfinite(small[(size_t)(nx + i)]) || !std::isfinite(small[(size_t)(2 * nx + i)]) || !(d > 0)) return dependent();
			norm_ninv = small[(size_t)(2 * nx + i)] > norm_ninv ? small[(size_t)(2 * nx + i)] : norm_ninv;
			dxx[(size_t)i] = 1.0 / ((double)n * d);
		}
		std::vector<double> varx = dxx;  // (the reference's 0 -> 1, association.py:546-547)
		for (double& v : varx)
			if (v == 0.0) v = 1.0;
		NRM_HIP(hipMemcpyAsync(ddxx.p, dxx.data(), (size_t)nx * 8, hipMemcpyHostToDevice, st));
		NRM_HIP(hipMemcpyAsync(dvarx.p, varx.data(), (size_t)nx * 8, hipMemcpyHostToDevice, st));
		NRM_HIP(hipStreamSynchronize(st));
		// Does the closed form apply?  Every grouping's rank nx - 1 + rank for rank-deficient covariates, else the reference's own rank test on A A^T (nrm_host_math.h)
		std::vector<double> mcc;
		nrm_covariate_gram(h_c64, nc, n, mcc);
		hbx.clear();
		if (nc) NRM_TRY(download(hbx, bx.p, (size_t)nx * nc));
		if (rank < nc) {
			std::vector<double> hss;
			NRM_TRY(download(hss, ssx.p, (size_t)nx));
			if (!nrm_pinv_rank_certified(mcc, nc, rank, hbx.data(), hss.data(), nx, norm_mt, norm_ninv, tol)) {
				nrm_set_error("%s: some grouping may not have the rank nx - 1 + %d at tol = %g (no certificate from the norms ||M~||_1 = %g, ||N~||_1 = %g); the package takes the spectrum of A A^T and, if need be, the per-grouping algorithm",
							  who, rank, tol, norm_mt, norm_ninv);
				return NRM_E_UNSUPPORTED;
			}
		} else {
			bool certified = false;
			NRM_TRY(nrm_full_rank_certified(norm_mt, norm_ninv, hbx.data(), mcc.data(), nx, nc, tol, &certified));
			if (!certified) {
				nrm_set_error("%s: the design may be rank deficient at tol = %g (no certificate from the norms ||M~||_1 = %g, ||N~||_1 = %g); the package takes the spectrum of A A^T and, if need be, the per-grouping algorithm",
							  who, tol, norm_mt, norm_ninv);
				return NRM_E_UNSUPPORTED;
			}
		}
		return NRM_OK;
	}

	// The gene side: the products on the route at hand, B^T = G N~, the sweep into p, stat and vary.  Launches and memset nodes only.
	int enqueue(hipStream_t st) {
		double* coefy = want_alpha ? by.as<double>() : nullptr;
		if (want_alpha) NRM_HIP(hipMemsetAsync(by.p, 0, (size_t)ny * nc * 8, st));
		if (sparse) {
			NRM_TRY(pw.enqueue(*L, d_y, y_dtype, ny, n, ldy, d_c, nc, ci, cval, d_dci, bx.as<double>(), ldb(), g.as<double>(), nxp, 1, ssy.as<double>(), coefy, flags.as<int32_t>(), st));
		} else {
			NRM_TRY(nrm_residualize(d_y, y_dtype, ny, n, ldy, d_c, nc, n, d_dci, rank, ryd.as<double>(), kp, nyp, ssy.as<double>(), coefy, st));
			NRM_TRY(nrm_gram_f64(ryd.as<double>(), rxd.as<double>(), nyp, nxp, kp, kp, kp, g.as<double>(), nxp, 0, ny, nx, gwork.p, st));
		}
		NRM_TRY(nrm_gram_f64(g.as<double>(), dn.as<double>(), nyp, nxp, nxp, nxp, nxp, bt.as<double>(), nxp, 0, ny, nx, gwork.p, st));
		return nrm_single4_sweep(bt.as<double>(), g.as<double>(), nxp, ssy.as<double>(), ddxx.as<double>(), nx, ny, nx, n, dof(), return_dot, p, stat, vary, out_dtype, ny,
								 work.as<double>(), flags.as<int32_t>(), st);
	}

private:
	static int dependent() {
		nrm_set_error("design rows are linearly dependent given the covariates");
		return NRM_E_UNSUPPORTED;
	}
};
