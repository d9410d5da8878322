// What the resident plans of de (nrm_de_plan.hip: single=0; nrm_single1_plan.hip: single=1; nrm_single4_plan.hip: single=4) do to a design when it is set, in nrm_de_design.hip: de's row filter
// (de.py:93), the row map, the rows kept compacted on the device, and their lists (csrc/nrm_design_lists.hip, csrc/nrm_design_csr.hip).
#pragma once
#include <memory>
#include "nrm_host_entry.h"
#include "nrm_de_plan_args.h"

struct NrmDeDesign {
	std::unique_ptr<NrmDesignLists> L;  // the lists of the rows kept (L->ok says whether they were filled)
	int64_t ngk = 0, list_bytes = 0;    // rows kept; bytes the lists hold
};

// "Malformed CSR design matrix ...": NRM_E_ARG
int nrm_de_design_malformed();

// The design `in` (ng0, n) of a plan called `who`: d_mask (ng0) one byte per row (1: tested), d_c2f (ng0) int64 the design row of every compact row, d_f2c (ng0)
// the compact row of every design row or -1, and out: the lists of the rows kept, with the ELL form on request; max_density > 0: the lists are filled only while at
// most that share of the rows kept is set (NrmDesignLists::build's rule), 0: always.  Reads the size records back (a few words, three times at the most) and waits
// for the fill; everything it takes besides the lists returns to the pool on the way out.  The caller has synchronised the device.  No row left: NRM_E_ARG.
int nrm_de_design_set(const char* who, const NrmDePlanDesign& in, int64_t ng0, int64_t n, uint8_t* d_mask, int64_t* d_c2f, int32_t* d_f2c, bool want_ell, double max_density,
					  hipStream_t st, NrmDeDesign& out);

// ---- what the entries of these plans do alike around a design.  Plan: nrm_de_plan, nrm_single1_plan or nrm_single4_plan -- L, device, drop_graph() and name, "nrm_de_plan"
// and so on ----------------------------------------------------------------------------------------------------------------------------------------------
template <typename Plan>
int plan_bind(Plan* pl, const char* who) {
	NRM_REQUIRE(pl != nullptr, "%s: null plan", who);
	NRM_REQUIRE(pl->L != nullptr, "%s: the plan has no design (the last %s_design was refused)", who, Plan::name);
	NRM_HIP(hipSetDevice(pl->device));
	return NRM_OK;
}

// *_plan_design once the arguments are checked; set_design(plan, g): the plan's own plan_set_design
template <typename Plan, typename SetDesign>
int nrm_plan_new_design(Plan* plan, const NrmDePlanDesign& g, SetDesign set_design) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_HIP(hipSetDevice(plan->device));
	NRM_HIP(hipDeviceSynchronize());  // (the steps queued on the old lists are through, and so is whatever filled the caller's arrays)
	plan->drop_graph();
	const int rc = set_design(plan, g);
	if (rc != NRM_OK) plan->L.reset();  // (the row map may already be the refused design's: the plan has none until a design is accepted)
	return rc;
}

// *bh_bytes: nrm_bh's workspace for the q-values of count P-values, 0 without want_q; who: the create entry
static inline int nrm_plan_bh_bytes(const char* who, int want_q, int64_t count, int out_dtype, int64_t* bh_bytes) {
	*bh_bytes = want_q ? nrm_bh_workspace_bytes(count, out_dtype) : 0;
	if (*bh_bytes < 0) {
		nrm_set_error("%s: q-values of %lld P-values are not provided (nrm_bh takes at most 2^31 - 1)", who, (long long)count);
		return (int)*bh_bytes;
	}
	return NRM_OK;
}
