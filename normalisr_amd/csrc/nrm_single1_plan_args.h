// What nrm_single1_plan_create and nrm_single1_plan_design (nrm_single1_plan.hip) decide before any device call: every argument check, and the covariates as fp64.
// Free of HIP headers, like nrm_de_plan_args.h, whose design record and design checks it reuses, so that g++ can build it with -fsanitize=address,undefined for the
// CPU test-suite (tests/host/single1_plan_args_sanitize.cpp).  There is no pseudo-inverse and no rank here: single=1 takes one per grouping, on the device.
#pragma once
#include "nrm_de_plan_args.h"

#define NRM_SINGLE1_PLAN_MAX_COVARIATES 32  // (S1_NCMAX of csrc/nrm_single1.hip: the wide statistics kernels and the stream kernel)

// Every check of create, in the order nrm_de_plan_create_args makes them.  c64: the covariates as fp64.
static inline int nrm_single1_plan_create_args(const NrmDePlanDesign& g, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n, int64_t ldt, int dt_on_device,
											   const void* h_dc, int c_dtype, int64_t nc, int dimreduce, int out_dtype, std::vector<double>& c64) {
	NRM_TRY_ARGS(nrm_plan_create_args_open("nrm_single1_plan_create", g, ng0, dt, dt_dtype, nt, n, c_dtype, nc, out_dtype));
	NRM_REQUIRE(nc >= 0 && (nc == 0 || h_dc), "Unmatching dx/dy/dc dimensions.");  // (the words of nrm_association_tests_single1_host for covariates that are not there)
	if (nc > NRM_SINGLE1_PLAN_MAX_COVARIATES) {
		nrm_set_error("nrm_single1_plan_create covers up to %d covariates (the package's masked-Gram path takes more)", NRM_SINGLE1_PLAN_MAX_COVARIATES);
		return NRM_E_UNSUPPORTED;
	}
	NRM_TRY_ARGS(nrm_plan_create_args_close("nrm_single1_plan_create", dimreduce, n, ldt, dt_on_device));
	nrm_covariates_to_f64(h_dc, c_dtype, (size_t)(nc * n), c64);
	return NRM_OK;
}

// single=1's counters ([0], [1] nrm_single1_cells; [2], [3], [4] nrm_single1_group_info) as what the reference asserts or raises, in this order: the selection
// (association.py:917-918), the SVD's finiteness check, the cell count, the results (:248,252).  The whole-problem entry and the plan's check both say it through here.
static inline int nrm_single1_status(const int32_t hf[8]) {
	if (hf[2]) {
		nrm_set_error("%d groupings take a single value on the cells selected for them (association.py:917-918)", hf[2]);
		return NRM_E_NUMERIC;
	}
	if (hf[4]) {
		nrm_set_error("array must not contain infs or NaNs");
		return NRM_E_ARG;
	}
	if (hf[3]) {
		nrm_set_error("Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.");
		return NRM_E_DEVICE;
	}
	return nrm_assoc_assertions(hf, "");
}
