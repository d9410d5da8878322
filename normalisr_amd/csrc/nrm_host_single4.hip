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
#include "nrm_single4_step.h"

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

// single=4's closed form, both entries: rank == nc (full-rank covariates, A A^T certified full rank) or 0 < rank < nc (nrm_pinv_rank_certified).  The design side and
// the gene side are NrmSingle4Step's (nrm_single4_step.h: the record the resident plan runs too); alpha and the assertions are taken on the host here.
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
	DevBuf dx, dy, dc, dci, op, ostat, ovary;
	std::vector<double> c64;
	NRM_TRY(upload_matrix(h_dx, x_dtype, nx, n, dx, st));
	NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, dy, st));
	NRM_TRY(covariates_f64(h_dc, c_dtype, nc, n, c64, dc));
	if (nc) {
		NRM_TRY(dci.alloc((size_t)nc * nc * 8));
		NRM_HIP(hipMemcpy(dci.p, h_dci, (size_t)nc * nc * 8, hipMemcpyHostToDevice));
	}
	NrmSingle4Step s;
	s.rows = s.nx = nx, s.ny = ny, s.n = n, s.ldx = s.ldy = n, s.nc = nc;
	s.x_dtype = x_dtype, s.y_dtype = y_dtype, s.out_dtype = out_dtype, s.rank = rank, s.dimreduce = dimreduce, s.return_dot = return_dot, s.tol = tol;
	s.want_alpha = h_alpha != nullptr && nc > 0;
	s.ci = nc ? nrm_constant_row(c64.data(), nc, n, &s.cval) : -1;
	s.who = rank < nc ? "nrm_association_tests_single4_pinv_host" : "nrm_association_tests_single4_host";
	s.d_x = dx.p, s.d_y = dy.p, s.d_c = dc.as<double>(), s.d_dci = dci.as<double>(), s.h_c64 = c64.data();
	NRM_TRY(s.alloc_fixed(nrm_take_plain, st));
	const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
	NRM_TRY(op.alloc(ob));
	NRM_TRY(ostat.alloc(ob));
	NRM_TRY(ovary.alloc(ob));
	s.p = op.p, s.stat = ostat.p, s.vary = ovary.p;
	// the design rows: from their entries when there are few (gRNA incidence), else K1's fp64 residuals
	NrmDesignLists L;
	if (nrm_de_sparse_wanted(nx, ny, n, nc)) {
		NRM_TRY(L.build(dx.p, x_dtype, nx, n, true, 1.0 / 16, st));
		s.sparse = L.ok;
		s.L = &L;
	}
	for (int pass = 0; pass < 2; pass++) {  // (a second pass only when the sparse-design kernels hand rows back: the same on K1 and the fp64 Gram kernel)
		if (s.sparse)
			NRM_TRY(s.alloc_sparse(nrm_take_plain, st));
		else
			NRM_TRY(s.alloc_dense(nrm_take_plain));
		int64_t handed = 0;
		NRM_TRY(s.alloc_design_side(st, &handed));
		if (handed > 0) {
			s.sparse = false;
			continue;
		}
		NRM_TRY(s.enqueue(st));
		int32_t hf[4];
		NRM_TRY(nrm_read_flags(s.flags.p, st, hf));
		if (s.sparse && hf[2] > 0) {  // rows all but inside the span of the covariates: K1's two sweeps and the fp64 Gram kernel for this call
			s.sparse = false;
			NRM_HIP(hipMemsetAsync(s.flags.p, 0, 32, st));
			continue;
		}
		// (the reference's assertions on the closed form's results speak only if the closed form applies -- the design side has certified that by now: a nearly
		//  rank-deficient design can fail them where the per-grouping algorithm, which the package then takes, returns results; association.py:421-576)
		if (nrm_assoc_assertions(hf, "")) {
			nrm_set_error("association results failed the reference's assertions (association.py:557): non-finite values or R^2 > 1+1e-8 in the closed form of a full-rank design");
			return NRM_E_NUMERIC;
		}
		NRM_TRY(copy_out(h_p, op.p, ob));
		NRM_TRY(copy_out(h_stat, ostat.p, ob));
		NRM_TRY(copy_out(h_vary, ovary.p, ob));
		std::vector<double> varx = s.dxx;
		for (double& v : varx)
			if (v == 0.0) v = 1.0;
		nrm_store_as(out_dtype, h_varx, varx.data(), nx);
		if (s.want_alpha) {
			std::vector<double> hbt, hby;
			NRM_TRY(download(hbt, s.bt.p, (size_t)s.nyp * s.nxp));
			NRM_TRY(download(hby, s.by.p, (size_t)ny * nc));
			nrm_single4_alpha(hbt.data(), s.nxp, hby.data(), s.hbx.data(), nx, ny, nc, out_dtype, h_alpha);
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
