// What nrm_single4_plan_create (nrm_single4_plan.hip) decides before any device call: every argument check, the covariates as fp64 and, when the caller has none,
// their pseudo-inverse and rank.  Free of HIP headers, like nrm_de_plan_args.h, whose design record and checks it reuses, so that g++ can build it with
// -fsanitize=address,undefined for the CPU test-suite (tests/host/single4_plan_args_sanitize.cpp).
#pragma once
#include "nrm_de_plan_args.h"

// Every check of create, in the order nrm_de_plan_create_args makes them; then tol.  *rank and *h_dci are the caller's, or -- *h_dci == NULL -- the library's own
// (own_dci keeps them); c64: the covariates as fp64.  max_covariates: nrm_de_sparse_max_covariates().  "Insufficient number of cells" waits for the design: the
// degrees of freedom count the rows kept.
static inline int nrm_single4_plan_create_args(const NrmDePlanDesign& g, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n, int64_t ldt, int dt_on_device,
											   const void* h_dc, int c_dtype, int64_t nc, const double** h_dci, int* rank, int dimreduce, int out_dtype, double tol,
											   int64_t max_covariates, std::vector<double>& c64, std::vector<double>& own_dci) {
	const char* who = "nrm_single4_plan_create";
	NRM_TRY_ARGS(nrm_plan_create_args_open(who, g, ng0, dt, dt_dtype, nt, n, c_dtype, nc, out_dtype));
	NRM_REQUIRE(nc >= 0 && (nc == 0 || h_dc), "Unmatching dx/dy/dc dimensions.");  // (the words of nrm_association_tests_single4_host for covariates that are not there)
	if (nc > max_covariates) {
		nrm_set_error("%s: the sparse-design kernel takes at most %lld covariates", who, (long long)max_covariates);
		return NRM_E_UNSUPPORTED;
	}
	NRM_TRY_ARGS(nrm_plan_create_args_close(who, dimreduce, n, ldt, dt_on_device));
	NRM_REQUIRE(tol > 0 && tol < 1, "%s: tol must be a positive number below 1", who);  // (a NaN fails both)
	nrm_covariates_to_f64(h_dc, c_dtype, (size_t)(nc * n), c64);
	if (!*h_dci && nc > 0) {
		if (nc > 32) {
			nrm_set_error("%s: the library computes the pseudo-inverse of at most 32 covariates (pass h_dci and rank for more)", who);
			return NRM_E_UNSUPPORTED;
		}
		own_dci.resize((size_t)(nc * nc));
		NRM_TRY_ARGS(nrm_covariates_pinv_f64(c64.data(), nc, n, tol, own_dci.data(), rank));
		*h_dci = own_dci.data();
	}
	if (nc == 0) *rank = 0;
	NRM_REQUIRE(*rank >= 0, "Negative dcr detected.");
	NRM_REQUIRE(*rank <= nc, "dcr higher than covariate dimension.");
	if (nc > 0 && *rank == 0) {  // (all-zero covariates)
		nrm_set_error("%s: covariates of rank 0 follow the per-grouping algorithm of the package", who);
		return NRM_E_UNSUPPORTED;
	}
	return NRM_OK;
}
