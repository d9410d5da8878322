// The expression side of normvar (norm.py:166-289) on a matrix in HBM, written once: the sizes, the buffers and the launches -- nrm_normvar_solve (the genes'
// moments in one pass and a lane per gene solving its small OLS), then nrm_normvar_rescale and nrm_normvar_apply -- that nrm_normvar_host (nrm_host_normvar.hip) and
// the resident front-half plan (nrm_front_plan.hip) both run.  It is the C twin of norm.NormvarPlan._launch, which drives the same entries on torch's tensors.
// The caller sets the sizes and the non-owning pointers; `take(DevBuf&, bytes)` allocates (the plan's counts pool bytes, the entry passes nrm_take_plain).  Only the
// alloc members allocate; what solve and finish queue, a plan captures.
//
// finish is the one place where these two callers write normvar's result: whatever filled b and scale -- solve here, or the entry's Gram-launch route on the host
// for 9 to 32 covariates -- the genes whose one-pass variance sums cancelled (marked in scale, csrc/nrm_nv_scale.h) get their scale from the row itself before the
// pass that writes the result.
#pragma once
#include "nrm_host_entry.h"

struct NrmNormvarStep {
	int64_t rows = 0, n = 0, ldy = 0, nc = 0, ldo = 0;
	double tol = 1e-8;
	int keepvar = 1, y_dtype = NRM_F64, out_dtype = NRM_F64;
	const void* d_y = nullptr;                        // the matrix (rows, n), pitch ldy
	const double *d_lnw = nullptr, *d_wt = nullptr;  // ln w (n); the genes' exponents (rows)
	const double* d_c = nullptr;                      // the scaled covariates (nc, n)
	void* d_out = nullptr;                            // (rows, n) of out_dtype, pitch ldo
	int32_t* flags = nullptr;                         // int32[4], cleared by the caller: [0] += genes of rank 0 (solve), [1] += waves with a non-finite result (apply)
	DevBuf mom, b, scale, rank;

	// what finish reads, for a caller that fills it by other means than solve
	template <typename Take>
	int alloc_coefficients(Take take) {
		return nrm_take_all(take, {{&b, rows * nc * 8}, {&scale, rows * 8}});
	}
	template <typename Take>
	int alloc(Take take) {
		NRM_TRY(take(mom, (size_t)rows * (size_t)(nc * (nc + 1) / 2 + nc + 2) * 8));
		NRM_TRY(alloc_coefficients(take));
		return take(rank, (size_t)rows * 8);
	}
	int solve(hipStream_t st) {
		return nrm_normvar_solve(d_y, y_dtype, rows, n, ldy, d_lnw, d_wt, d_c, nc, n, tol, keepvar ? 1 : 0, mom.as<double>(), b.as<double>(), scale.as<double>(), rank.as<int64_t>(),
								 flags, st);
	}
	int finish(hipStream_t st) {
		NRM_TRY(nrm_normvar_rescale(d_y, y_dtype, rows, n, ldy, d_lnw, d_wt, d_c, nc, n, b.as<double>(), scale.as<double>(), st));
		return nrm_normvar_apply(d_y, y_dtype, rows, n, ldy, d_lnw, d_wt, d_c, nc, n, b.as<double>(), scale.as<double>(), d_out, out_dtype, ldo, flags, st);
	}
};
