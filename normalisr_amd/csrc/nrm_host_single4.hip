// single=4 behind the C seam (numpy buffers in, numpy buffers out, no torch): nrm_association_tests_single4_host (`normalisr de -m covariate`:
// association.py:421-576,926-980, full-rank designs), nrm_association_tests_single4_pinv_host (the same, covariates of any rank: one-hot batches and an
// intercept), and the two pieces the package needs to follow the reference's per-grouping algorithm where the closed form does not apply, nrm_gram_host and
// nrm_pvalues_host -- the kernels normalisr_amd/single4.py drives through the device-pointer entries, sequenced here in C++ with the library's own scratch pool.
// The arithmetic that decides whether the closed form applies (the two rank certificates, the host's Cholesky inverse) is in nrm_host_math.h.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nrm_host_entry.h"
#include "nrm_design.h"

// ---- the two pieces the package needs to follow the reference's per-grouping algorithm of single=4 WITHOUT torch ------------------------------------------
// (association.py:926-980 forms the Gram matrices of A = [dx; dc] and of dy against A with numpy.matmul and hands them to association_test_4; for designs the closed
// form does not cover -- rank-deficient A A^T, mpc / method / qr, dy=None -- nrm_association_tests_single4_host answers NRM_E_UNSUPPORTED and normalisr_amd/single4.py
// runs that algorithm on these products: the contractions on the fp64 Gram kernel, the small pseudo-inverses in numpy, the P-values by nrm_pvalues_host.)
// h_out (ra, rb) fp64 = A B^T over n cells; h_b == NULL: B = A (rb = ra).  h_ssa (ra) / h_ssb (rb) or NULL: the rows' sums of squares.
extern "C" int nrm_gram_host(const void* h_a, int a_dtype, int64_t ra, const void* h_b, int b_dtype, int64_t rb, int64_t n, double* h_out, double* h_ssa, double* h_ssb) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(h_a && h_out && ra > 0 && n > 0 && (a_dtype == NRM_F32 || a_dtype == NRM_F64) && (!h_b || (rb > 0 && (b_dtype == NRM_F32 || b_dtype == NRM_F64))),
				"nrm_gram_host: bad arguments");
	if (!h_b) rb = ra;
	hipStream_t st = nullptr;
	const int64_t kp = nrm_round_up(n, NRM_K_TILE), rap = nrm_round_up(ra, NRM_ROW_TILE), rbp = nrm_round_up(rb, NRM_ROW_TILE);
	DevBuf raw, a64, b64, ssa, ssb, dot, gwork;
	auto padded = [&](const void* h, int dtype, int64_t rows, int64_t rp, DevBuf& out, DevBuf& ss) -> int {
		NRM_TRY(upload_matrix(h, dtype, rows, n, raw, st));
		NRM_TRY(out.alloc((size_t)rp * kp * 8));
		NRM_TRY(ss.alloc((size_t)rp * 8));
		NRM_TRY(nrm_residualize(raw.p, dtype, rows, n, n, nullptr, 0, 0, nullptr, 0, out.as<double>(), kp, rp, ss.as<double>(), nullptr, st));  // no covariates: the fp64 padded copy + sums of squares
		NRM_HIP(hipStreamSynchronize(st));
		raw.release();
		return NRM_OK;
	};
	NRM_TRY(padded(h_a, a_dtype, ra, rap, a64, ssa));
	if (h_b) NRM_TRY(padded(h_b, b_dtype, rb, rbp, b64, ssb));
	NRM_TRY(dot.alloc_zero((size_t)rap * rbp * 8, st));  // (the kernel leaves pure-padding sub-blocks unwritten)
	NRM_TRY(gwork.alloc((size_t)nrm_gram_workspace_bytes()));
	NRM_TRY(nrm_gram_f64(a64.as<double>(), h_b ? b64.as<double>() : a64.as<double>(), rap, rbp, kp, kp, kp, dot.as<double>(), rbp, 0, ra, rb, gwork.p, st));
	std::vector<double> hd;
	NRM_TRY(download(hd, dot.p, (size_t)rap * rbp));
	for (int64_t i = 0; i < ra; i++) memcpy(h_out + i * rb, &hd[(size_t)(i * rbp)], (size_t)rb * 8);
	if (h_ssa) NRM_HIP(hipMemcpy(h_ssa, ssa.p, (size_t)ra * 8, hipMemcpyDeviceToHost));
	if (h_ssb) NRM_HIP(hipMemcpy(h_ssb, h_b ? ssb.p : ssa.p, (size_t)rb * 8, hipMemcpyDeviceToHost));
	return NRM_OK;
}

// h_p[i] = I_{1 - h_r2[i]}(dof / 2, 1 / 2): scipy.stats.beta.cdf(1 - R2, dof / 2, 0.5) of association.py:563 for host arrays (the device function of nrm_pvalue.h)
extern "C" int nrm_pvalues_host(const double* h_r2, int64_t count, double dof, double* h_p) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(count >= 0 && (count == 0 || (h_r2 && h_p)), "nrm_pvalues_host: bad arguments");
	if (count == 0) return NRM_OK;
	hipStream_t st = nullptr;
	DevBuf r2, p;
	NRM_TRY(r2.alloc((size_t)count * 8));
	NRM_TRY(p.alloc((size_t)count * 8));
	NRM_HIP(hipMemcpy(r2.p, h_r2, (size_t)count * 8, hipMemcpyHostToDevice));
	NRM_TRY(nrm_pvalues_from_r2(r2.as<double>(), count, dof, p.as<double>(), st));
	NRM_HIP(hipMemcpy(h_p, p.p, (size_t)count * 8, hipMemcpyDeviceToHost));
	return NRM_OK;
}

// ---- single=4 (association.py:421-576,926-980) in closed form, for full-rank designs --------------------------------------------------------
namespace {

// Inverse of the symmetric positive definite matrix whose upper tiles are in d_m (nxp x nxp) by Newton-Schulz iteration on the fp64 Gram kernel
// (normalisr_amd/single4.py: _spd_inverse_device); d_n receives the inverse (zero padding), small (3, nx) its diagonal / kappa numerators / absolute
// row sums; *norm1 = ||M||_1.  *ok = 0: not converged (the caller takes the host's Cholesky factorisation).
int spd_inverse_device(const double* d_m, int64_t nx, int64_t nxp, const double* d_ss, DevBuf& d_n, std::vector<double>& small, double* norm1, int* ok, void* gwork,
					   hipStream_t st) {
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
	NRM_TRY(d_n.alloc(mb));
	NRM_TRY(dsmall.alloc((size_t)3 * nx * 8));
	NRM_TRY(nrm_spd_finish(x.as<double>(), nx, nxp, d_ss, d_n.as<double>(), dsmall.as<double>(), st));
	NRM_TRY(download(small, dsmall.p, (size_t)3 * nx));
	*ok = 1;
	return NRM_OK;
}

// single=4's closed form, both entries: rank == nc (full-rank covariates, A A^T certified full rank) or 0 < rank < nc (nrm_pinv_rank_certified)
int single4_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc, int c_dtype, int64_t nc, int64_t n,
				 const double* h_dci, int rank, int dimreduce, int return_dot, double tol, void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary,
				 int out_dtype, bool full_rank_only) {
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(h_dx && h_dy && nx > 0 && ny > 0 && n > 0 && nc >= 0 && (nc == 0 || (h_dc && h_dci)), "Unmatching dx/dy/dc dimensions.");
	NRM_REQUIRE(h_p && h_stat && h_varx && h_vary, "nrm_association_tests_single4_host: null output");
	NRM_REQUIRE((x_dtype == NRM_F32 || x_dtype == NRM_F64) && (y_dtype == NRM_F32 || y_dtype == NRM_F64) && (out_dtype == NRM_F32 || out_dtype == NRM_F64), "bad dtype");
	if (full_rank_only && rank != nc) {  // (the closed form for rank-deficient covariates: nrm_association_tests_single4_pinv_host)
		nrm_set_error("nrm_association_tests_single4_host covers full-rank designs (closed form); rank-deficient covariates follow the per-grouping algorithm of the package");
		return NRM_E_UNSUPPORTED;
	}
	NRM_REQUIRE(rank >= 0 && rank <= nc, "dcr higher than covariate dimension.");
	if (rank < nc && rank == 0) {  // (all-zero covariates)
		nrm_set_error("nrm_association_tests_single4_pinv_host: covariates of rank 0 follow the per-grouping algorithm of the package");
		return NRM_E_UNSUPPORTED;
	}
	if (n <= nx + rank + dimreduce) {  // (rank nx - 1 + rank per grouping: dof = n - nx - rank - dimreduce, association.py:558)
		nrm_set_error("Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.");
		return NRM_E_DEVICE;
	}
	hipStream_t st = nullptr;
	const int64_t kp = nrm_round_up(n, NRM_K_TILE), nxp = nrm_round_up(nx, NRM_ROW_TILE), nyp = nrm_round_up(ny, NRM_ROW_TILE);
	DevBuf dx, dy, dc, dci, gwork, flags;
	std::vector<double> c64;
	NRM_TRY(upload_matrix(h_dx, x_dtype, nx, n, dx, st));
	NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, dy, st));
	NRM_TRY(covariates_f64(h_dc, c_dtype, nc, n, c64, dc));
	if (nc) {
		NRM_TRY(dci.alloc((size_t)nc * nc * 8));
		NRM_HIP(hipMemcpy(dci.p, h_dci, (size_t)nc * nc * 8, hipMemcpyHostToDevice));
	}
	NRM_TRY(gwork.alloc((size_t)nrm_gram_workspace_bytes()));
	NRM_TRY(flags.alloc_zero(16, st));
	double cval = 0.0;
	const int ci = nc ? nrm_constant_row(c64.data(), nc, n, &cval) : -1;
	// the design rows: from their entries when there are few (gRNA incidence), else K1's fp64 residuals
	DevBuf ssx, bx, mt, rxd;
	NRM_TRY(ssx.alloc_zero((size_t)nxp * 8, st));
	NRM_TRY(bx.alloc_zero((size_t)nx * (nc > 0 ? nc : 1) * 8, st));
	NRM_TRY(mt.alloc((size_t)nxp * nxp * 8));
	auto residualize_design = [&]() -> int {  // K1 on the design rows: x~ (nxp, kp), |x~|^2, b_x
		NRM_TRY(rxd.alloc((size_t)nxp * kp * 8));
		return nrm_residualize(dx.p, x_dtype, nx, n, n, dc.as<double>(), nc, n, dci.as<double>(), rank, rxd.as<double>(), kp, nxp, ssx.as<double>(), nc ? bx.as<double>() : nullptr,
							   st);
	};
	NrmDesignLists L;
	bool sparse = false;
	if (nrm_de_sparse_wanted(nx, ny, n, nc)) {
		NRM_TRY(L.build(dx.p, x_dtype, nx, n, true, 1.0 / 16, st));
		sparse = L.ok;
	}
	for (int pass = 0; pass < 2; pass++) {  // (a second pass only when the sparse-design kernels hand rows back: the same on K1 and the fp64 Gram kernel)
		int32_t hf[4];
		if (sparse) {
			NRM_TRY(nrm_design_stats(L.row_ptr.as<int64_t>(), L.cells.as<int32_t>(), L.row_vals.as<double>(), dc.as<double>(), n, nc, dci.as<double>(), nx, ssx.as<double>(),
									 nc ? bx.as<double>() : nullptr, flags.as<int32_t>(), st));
			DevBuf ss2;  // (|x~|^2 again, as the product kernel computes it for its rows: not used)
			NRM_TRY(ss2.alloc((size_t)nxp * 8));
			// M~ = X~ X~^T: the same product with the design rows in the place of the expression rows
			NRM_TRY(sparse_products(L, dx.p, x_dtype, nx, n, dc.as<double>(), nc, ci, cval, dci.as<double>(), bx.as<double>(), nc > 0 ? nc : 1, mt.as<double>(), nxp, 0,
									ss2.as<double>(), nullptr, flags.as<int32_t>(), st));
			// a design row all but inside the span of the covariates is known HERE: looked at before the inverse and the genes' products, which a
			// handed-back call would only repeat (round-5 advisory)
			NRM_TRY(nrm_read_flags(flags.p, st, hf));
			if (hf[2] > 0) {
				sparse = false;
				NRM_HIP(hipMemsetAsync(flags.p, 0, 16, st));
				continue;
			}
		} else {
			NRM_TRY(residualize_design());
			NRM_TRY(nrm_gram_f64(rxd.as<double>(), rxd.as<double>(), nxp, nxp, kp, kp, kp, mt.as<double>(), nxp, 1, nx, nx, gwork.p, st));
		}
		// N~ = M~^-1
		DevBuf dn;
		std::vector<double> small;
		double norm_mt = 0.0;
		int okdev = 0;
		NRM_TRY(spd_inverse_device(mt.as<double>(), nx, nxp, ssx.as<double>(), dn, small, &norm_mt, &okdev, gwork.p, st));
		if (!okdev) {  // the host's Cholesky factorisation
			std::vector<double> hm, hss, npad;
			NRM_TRY(download(hm, mt.p, (size_t)nxp * nxp));
			NRM_TRY(download(hss, ssx.p, (size_t)nx));
			if (!nrm_spd_inverse_fallback(hm.data(), hss.data(), nx, nxp, &norm_mt, npad, small)) {
				nrm_set_error("design rows are linearly dependent given the covariates");
				return NRM_E_UNSUPPORTED;
			}
			NRM_TRY(dn.alloc(npad.size() * 8));
			NRM_HIP(hipMemcpy(dn.p, npad.data(), npad.size() * 8, hipMemcpyHostToDevice));
		}
		double norm_ninv = 0.0;
		std::vector<double> dxx((size_t)nx);
		for (int64_t i = 0; i < nx; i++) {
			const double d = small[(size_t)i];
			if (!std::isfinite(d) || !std::isfinite(small[(size_t)(nx + i)]) || !std::isfinite(small[(size_t)(2 * nx + i)]) || !(d > 0)) {
				nrm_set_error("design rows are linearly dependent given the covariates");
				return NRM_E_UNSUPPORTED;
			}
			norm_ninv = small[(size_t)(2 * nx + i)] > norm_ninv ? small[(size_t)(2 * nx + i)] : norm_ninv;
			dxx[(size_t)i] = 1.0 / ((double)n * d);
		}
		// the genes: Y~ X~^T (as (genes, design rows)), |y~|^2, b_y on request
		const bool want_alpha = h_alpha != nullptr && nc > 0;
		DevBuf g, ssy, by, ryd;
		NRM_TRY(g.alloc_zero((size_t)nyp * nxp * 8, st));
		NRM_TRY(ssy.alloc((size_t)nyp * 8));
		if (want_alpha) NRM_TRY(by.alloc_zero((size_t)ny * nc * 8, st));
		if (sparse) {
			NRM_TRY(sparse_products(L, dy.p, y_dtype, ny, n, dc.as<double>(), nc, ci, cval, dci.as<double>(), bx.as<double>(), nc > 0 ? nc : 1, g.as<double>(), nxp, 1,
									ssy.as<double>(), want_alpha ? by.as<double>() : nullptr, flags.as<int32_t>(), st));
			NRM_TRY(nrm_read_flags(flags.p, st, hf));
			if (hf[2] > 0) {  // rows all but inside the span of the covariates: K1's two sweeps and the fp64 Gram kernel for this call
				sparse = false;
				NRM_HIP(hipMemsetAsync(flags.p, 0, 16, st));
				continue;
			}
		} else {
			if (!rxd.p) NRM_TRY(residualize_design());  // (handed back from the sparse kernels: the design rows' residuals are needed after all)
			NRM_TRY(ryd.alloc((size_t)nyp * kp * 8));
			NRM_TRY(nrm_residualize(dy.p, y_dtype, ny, n, n, dc.as<double>(), nc, n, dci.as<double>(), rank, ryd.as<double>(), kp, nyp, ssy.as<double>(),
									want_alpha ? by.as<double>() : nullptr, st));
			NRM_TRY(nrm_gram_f64(ryd.as<double>(), rxd.as<double>(), nyp, nxp, kp, kp, kp, g.as<double>(), nxp, 0, ny, nx, gwork.p, st));
			ryd.release();
		}
		// B^T = (Y~ X~^T) N~, the sweep
		DevBuf bt, ddxx, op, ostat, ovary, work;
		NRM_TRY(bt.alloc((size_t)nyp * nxp * 8));
		NRM_TRY(nrm_gram_f64(g.as<double>(), dn.as<double>(), nyp, nxp, nxp, nxp, nxp, bt.as<double>(), nxp, 0, ny, nx, gwork.p, st));
		NRM_TRY(ddxx.alloc((size_t)nx * 8));
		NRM_HIP(hipMemcpyAsync(ddxx.p, dxx.data(), (size_t)nx * 8, hipMemcpyHostToDevice, st));
		const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
		NRM_TRY(op.alloc(ob));
		NRM_TRY(ostat.alloc(ob));
		NRM_TRY(ovary.alloc(ob));
		NRM_TRY(work.alloc((size_t)ny * 8));
		NRM_TRY(nrm_single4_sweep(bt.as<double>(), g.as<double>(), nxp, ssy.as<double>(), ddxx.as<double>(), nx, ny, nx, n, (double)(n - nx - rank - dimreduce), return_dot, op.p, ostat.p,
								  ovary.p, out_dtype, ny, work.as<double>(), flags.as<int32_t>(), st));
		// (the reference's assertions on the closed form's results speak only if the closed form applies: a nearly rank-deficient design can fail them
		//  where the per-grouping algorithm -- which the package then takes -- returns results; association.py:421-576.  Round-5 advisory.)
		int32_t hf2[2];
		NRM_TRY(nrm_read_flags(flags.p, st, hf2));
		const int flag_rc = nrm_assoc_assertions(hf2, "");
		// Does the closed form apply?  Every grouping's rank nx - 1 + rank for rank-deficient covariates, else the reference's own rank test on A A^T (nrm_host_math.h)
		std::vector<double> hbx, mcc;
		nrm_covariate_gram(c64.data(), nc, n, mcc);
		if (rank < nc) {
			std::vector<double> hss;
			NRM_TRY(download(hbx, bx.p, (size_t)nx * nc));
			NRM_TRY(download(hss, ssx.p, (size_t)nx));
			if (!nrm_pinv_rank_certified(mcc, nc, rank, hbx.data(), hss.data(), nx, norm_mt, norm_ninv, tol)) {
				nrm_set_error("nrm_association_tests_single4_pinv_host: some grouping may not have the rank nx - 1 + %d at tol = %g (no certificate from the norms); the package takes the spectrum of A A^T and, if need be, the per-grouping algorithm", rank, tol);
				return NRM_E_UNSUPPORTED;
			}
		} else {
			bool certified = false;
			if (nc) NRM_TRY(download(hbx, bx.p, (size_t)nx * nc));
			NRM_TRY(nrm_full_rank_certified(norm_mt, norm_ninv, hbx.data(), mcc.data(), nx, nc, tol, &certified));
			if (!certified) {
				nrm_set_error("nrm_association_tests_single4_host: the design may be rank deficient at tol = %g (no certificate from the norms); the package takes the spectrum of A A^T and, if need be, the per-grouping algorithm", tol);
				return NRM_E_UNSUPPORTED;
			}
		}
		if (flag_rc) {
			nrm_set_error("association results failed the reference's assertions (association.py:557): non-finite values or R^2 > 1+1e-8 in the closed form of a full-rank design");
			return flag_rc;
		}
		NRM_TRY(copy_out(h_p, op.p, ob));
		NRM_TRY(copy_out(h_stat, ostat.p, ob));
		NRM_TRY(copy_out(h_vary, ovary.p, ob));
		for (double& v : dxx)
			if (v == 0.0) v = 1.0;
		nrm_store_as(out_dtype, h_varx, dxx.data(), nx);
		if (want_alpha) {
			std::vector<double> hbt, hby;
			NRM_TRY(download(hbt, bt.p, (size_t)nyp * nxp));
			NRM_TRY(download(hby, by.p, (size_t)ny * nc));
			nrm_single4_alpha(hbt.data(), nxp, hby.data(), hbx.data(), nx, ny, nc, out_dtype, h_alpha);
		}
		return NRM_OK;
	}
	nrm_set_error("nrm_association_tests_single4_host: internal error (no pass completed)");
	return NRM_E_DEVICE;
}

}  // namespace

extern "C" int nrm_association_tests_single4_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc, int c_dtype,
												   int64_t nc, int64_t n, const double* h_dci, int rank, int dimreduce, int return_dot, double tol, void* h_p,
												   void* h_stat, void* h_alpha, void* h_varx, void* h_vary, int out_dtype) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	return single4_host(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, tol, h_p, h_stat, h_alpha, h_varx, h_vary,
						out_dtype, true);
}

extern "C" int nrm_association_tests_single4_pinv_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc,
														int c_dtype, int64_t nc, int64_t n, const double* h_dci, int rank, int dimreduce, int return_dot, double tol,
														void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary, int out_dtype) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	return single4_host(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, tol, h_p, h_stat, h_alpha, h_varx, h_vary,
						out_dtype, false);
}
