// What nrm_de_plan_create and nrm_de_plan_design (nrm_de_plan.hip) decide before any device call: the design as they take it and every argument check, the
// covariates' pseudo-inverse included.  Free of HIP headers, like nrm_host_logic.h and nrm_host_math.h, so that g++ can build it with -fsanitize=address,undefined
// for the CPU test-suite (tests/host/de_plan_args_sanitize.cpp).
#pragma once
#include "nrm_host_logic.h"
#include "nrm_host_math.h"

#define NRM_TRY_ARGS(call)   \
	do {                     \
		int rc_ = (call);    \
		if (rc_) return rc_; \
	} while (0)

struct NrmDePlanDesign {
	int form = 0;                  // 0 dense, 1 canonical CSR
	const void* values = nullptr;  // the matrix, or the CSR data (NULL: all ones)
	int dtype = NRM_F64;
	int64_t ld = 0;
	const int64_t* indptr = nullptr;
	const int32_t* indices = nullptr;
	int64_t nnz = 0;
	int on_device = 0;
};

static inline int nrm_de_plan_design_args(const char* who, const NrmDePlanDesign& g, int64_t ng0, int64_t n) {
	NRM_REQUIRE(g.form == 0 || g.form == 1, "%s: the design is dense (0) or canonical CSR (1)", who);
	NRM_REQUIRE(g.dtype == NRM_F32 || g.dtype == NRM_F64, "%s: bad dtype", who);
	NRM_REQUIRE(ng0 > 0 && n > 0, "Incorrect dx/dy/dc size.");
	if (g.form == 0) {
		NRM_REQUIRE(g.values != nullptr, "Incorrect dx/dy/dc size.");
		NRM_REQUIRE(g.on_device ? g.ld >= n : g.ld == n, "%s: row pitch smaller than the row (a host matrix is contiguous)", who);
	} else {
		NRM_REQUIRE(g.indptr != nullptr && g.nnz >= 0 && (g.nnz == 0 || g.indices != nullptr), "Incorrect dx/dy/dc size.");
		NRM_REQUIRE(g.nnz / ng0 <= n, "%s: more stored entries than the matrix has cells", who);  // (ng0 * n may not fit 64 bits)
	}
	return NRM_OK;
}

// the design as the entries take it, one argument each; n: the cells of the plan, the row pitch of a dense design that states none
static inline NrmDePlanDesign nrm_de_plan_design_of(int form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz, int on_device,
													int64_t n) {
	NrmDePlanDesign g;
	g.form = form, g.values = dg, g.dtype = dg_dtype, g.ld = ldg ? ldg : n, g.indptr = indptr, g.indices = indices, g.nnz = nnz, g.on_device = on_device;
	return g;
}

// The checks that open and close nrm_de_plan_create_args and nrm_single1_plan_create_args (nrm_single1_plan_args.h); who: the create entry.
static inline int nrm_plan_create_args_open(const char* who, const NrmDePlanDesign& g, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n, int c_dtype, int64_t nc,
											int out_dtype) {
	NRM_REQUIRE((dt_dtype == NRM_F32 || dt_dtype == NRM_F64) && (out_dtype == NRM_F32 || out_dtype == NRM_F64) && (nc <= 0 || c_dtype == NRM_F32 || c_dtype == NRM_F64),
				"%s: bad dtype", who);
	NRM_REQUIRE(ng0 > 0 && nt > 0 && n > 0 && dt != nullptr, "Incorrect dx/dy/dc size.");
	NRM_REQUIRE(n <= 0x7fffffffLL && ng0 <= 0x7fffffffLL && nt <= 0x7fffffffLL, "%s: more than 2^31 - 1 rows or cells", who);
	return nrm_de_plan_design_args(who, g, ng0, n);
}
static inline int nrm_plan_create_args_close(const char* who, int dimreduce, int64_t n, int64_t ldt, int dt_on_device) {
	NRM_REQUIRE(dimreduce >= 0, "dimreduce must be a non-negative integer.");
	NRM_REQUIRE(dt_on_device ? ldt >= n : ldt == n, "%s: row pitch smaller than the row (a host matrix is contiguous)", who);
	return NRM_OK;
}

// Every check of create, in the order the coex plan makes them.  *rank and *h_dci are the caller's, or -- *h_dci == NULL -- the library's own (own_dci keeps them);
// c64: the covariates as fp64.  max_covariates: nrm_de_sparse_max_covariates().
static inline int nrm_de_plan_create_args(const NrmDePlanDesign& g, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n, int64_t ldt, int dt_on_device,
										  const void* h_dc, int c_dtype, int64_t nc, const double** h_dci, int* rank, int dimreduce, int out_dtype, int64_t max_covariates,
										  std::vector<double>& c64, std::vector<double>& own_dci) {
	NRM_TRY_ARGS(nrm_plan_create_args_open("nrm_de_plan_create", g, ng0, dt, dt_dtype, nt, n, c_dtype, nc, out_dtype));
	NRM_REQUIRE(nc >= 0 && (nc == 0 || h_dc), "Incorrect dx/dy/dc size.");
	if (nc > max_covariates) {
		nrm_set_error("nrm_de_plan_create: the sparse-design kernel takes at most %lld covariates", (long long)max_covariates);
		return NRM_E_UNSUPPORTED;
	}
	nrm_covariates_to_f64(h_dc, c_dtype, (size_t)(nc * n), c64);
	if (!*h_dci && nc > 0) {
		if (nc > 32) {
			nrm_set_error("nrm_de_plan_create: the library computes the pseudo-inverse of at most 32 covariates (pass h_dci and rank for more)");
			return NRM_E_UNSUPPORTED;
		}
		own_dci.resize((size_t)(nc * nc));
		NRM_TRY_ARGS(nrm_covariates_pinv_f64(c64.data(), nc, n, 1e-8, own_dci.data(), rank));
		*h_dci = own_dci.data();
	}
	NRM_TRY_ARGS(nrm_assoc_check_args(g.form == 0 ? g.values : (const void*)g.indptr, ng0, nt, h_dc, nc, n, *rank, dimreduce));
	return nrm_plan_create_args_close("nrm_de_plan_create", dimreduce, n, ldt, dt_on_device);
}
