// What nrm_front_plan_create and nrm_front_plan_create_csr (nrm_front_plan.hip) decide before any device call: every argument check, for canonical CSR host arrays
// the O(rows) part of the structure, the user covariate rows' finiteness and normcov's constant-row test on them (norm.py:34-37), and the host restatement of
// normcov's row classification (norm.py:39) that the device kernel k_front_cov applies to every row of every step.  Free of HIP headers, like nrm_de_plan_args.h,
// so that g++ can build it with -fsanitize=address,undefined for the CPU test-suite (tests/host/front_plan_args_sanitize.cpp, front_plan_csr_args_sanitize.cpp).
#pragma once
#include "nrm_host_logic.h"

#define NRM_FRONT_LCPM_ROWS 3         // ln total, genes without a read, ln^2 total (lcpm.py:194-200)
#define NRM_FRONT_MAX_ROWS (65535LL * 32)  // the row tiles of nrm_lcpm_* and nrm_fitvar_cells are grid rows: at most 65535 tiles of 32 genes
#define NRM_FRONT_MAX_STEPS 1000000LL  // as nrm_compute_var_host
#define NRM_FRONT_M2_ROWS 16          // rows of [dc;1] the plan's own pseudo-inverse kernel holds in LDS

#define NRM_COV_BINARY 0      // a row holding only 0 and 1: left alone (norm.py:39)
#define NRM_COV_CONTINUOUS 1  // centred and scaled
#define NRM_COV_ONES 2        // the constant-1 row normcov appends (c=True)
#define NRM_COV_CONSTANT -1   // one distinct value: normcov raises (norm.py:34-37)

struct NrmFrontPlanArgs {
	const void* reads = nullptr;
	int dtype = NRM_I32;
	int64_t rows = 0, n = 0, ld = 0;
	int on_device = 0;
	const double* h_cov = nullptr;  // (n_cov, n) raw user covariates
	int64_t n_cov = 0, ntot = -1, stepmax = 1;
	double eps = 1e-6, tol = 1e-8;
	int out_dtype = NRM_F64;
	int64_t count_cap = 0;
	// nrm_front_plan_create_csr: `reads` is the stored values; indptr (rows + 1) int64, indices int32; nnz stored entries in arrays of nnz_cap elements
	int csr = 0;
	const int64_t* indptr = nullptr;
	const int32_t* indices = nullptr;
	int64_t nnz = 0, nnz_cap = 0;
};

// what the eager CSR path says of a malformed matrix (nrm_host_front.hip; normalisr_amd/lcpm.py: MALFORMED_CSR)
#define NRM_MALFORMED_CSR                                                                                                                      \
	"Malformed CSR matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and " \
	"increase strictly (sum duplicates and sort the indices first)."

static inline bool nrm_front_count_dtype(int dtype) { return dtype == NRM_I64 || dtype == NRM_I32 || dtype == NRM_I16 || dtype == NRM_U8; }
static inline int nrm_front_count_bytes(int dtype) { return dtype == NRM_I64 ? 8 : dtype == NRM_I32 ? 4 : dtype == NRM_I16 ? 2 : 1; }

// the O(rows) part of a host CSR matrix's structure: 0 = p[0] <= p[1] <= ... <= p[rows] = nnz (the columns of every entry are the count kernel's to check)
static inline int nrm_front_csr_offsets(const int64_t* indptr, int64_t rows, int64_t nnz) {
	bool ok = indptr[0] == 0 && indptr[rows] == nnz;
	for (int64_t r = 0; r < rows && ok; r++) ok = indptr[r] <= indptr[r + 1];
	NRM_REQUIRE(ok, "%s", NRM_MALFORMED_CSR);
	return NRM_OK;
}

// normcov's view of one covariate row of n cells: NRM_COV_CONSTANT, NRM_COV_BINARY or NRM_COV_CONTINUOUS
static inline int nrm_normcov_row_class(const double* row, int64_t n) {
	bool same = true, cont = false;
	for (int64_t k = 0; k < n; k++) {
		same = same && row[k] == row[0];
		cont = cont || (row[k] != 0.0 && row[k] != 1.0);
	}
	return same ? NRM_COV_CONSTANT : cont ? NRM_COV_CONTINUOUS : NRM_COV_BINARY;
}

// Every check of create (a.csr == 0) and of create_csr, under the entry's name.  max_covariates: nrm_normvar_device_covariates(); table_cap: nrm_lcpm_table_cap().
static inline int nrm_front_plan_args_check(const char* who, const NrmFrontPlanArgs& a, int64_t max_covariates, int64_t table_cap) {
	NRM_REQUIRE(a.reads != nullptr && (!a.csr || (a.indptr != nullptr && a.indices != nullptr)) && a.n_cov >= 0 && (a.n_cov == 0 || a.h_cov != nullptr), "%s: null pointer", who);
	NRM_REQUIRE(a.rows > 0 && a.n > 0, "reads must not be empty.");
	NRM_REQUIRE(nrm_front_count_dtype(a.dtype), "%s: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8", who);
	NRM_REQUIRE(a.out_dtype == NRM_F32 || a.out_dtype == NRM_F64, "%s: out_dtype must be NRM_F32 or NRM_F64", who);
	NRM_REQUIRE(a.rows <= NRM_FRONT_MAX_ROWS && a.n <= 0x7fffffffLL, "%s: at most %lld genes and 2^31 - 1 cells", who, (long long)NRM_FRONT_MAX_ROWS);
	if (a.csr) {
		NRM_REQUIRE(a.nnz_cap >= 1 && a.nnz >= 0 && a.nnz <= a.nnz_cap, "%s: 0 <= nnz <= nnz_cap and nnz_cap >= 1 must hold", who);
		NRM_REQUIRE((uintptr_t)a.indptr % 8 == 0 && (uintptr_t)a.indices % 4 == 0 && (uintptr_t)a.reads % (uintptr_t)nrm_front_count_bytes(a.dtype) == 0, "%s: misaligned CSR arrays", who);
		if (!a.on_device)
			if (const int rc = nrm_front_csr_offsets(a.indptr, a.rows, a.nnz)) return rc;
	} else
		NRM_REQUIRE(a.on_device ? a.ld >= a.n : a.ld == a.n, "%s: row pitch smaller than the row (a host matrix is contiguous)", who);
	const int64_t total = a.n_cov + NRM_FRONT_LCPM_ROWS + 1;
	if (total > max_covariates || total + 1 > NRM_FRONT_M2_ROWS) {
		const int64_t bound = max_covariates < NRM_FRONT_M2_ROWS - 1 ? max_covariates : NRM_FRONT_M2_ROWS - 1;
		nrm_set_error("%s: %lld user covariates + lcpm's %d + the constant row = %lld, beyond the %lld covariates normvar keeps on the device (nrm_normvar_device_covariates)", who,
					  (long long)a.n_cov, NRM_FRONT_LCPM_ROWS, (long long)total, (long long)bound);
		return NRM_E_UNSUPPORTED;
	}
	NRM_REQUIRE(a.eps > 0 && a.stepmax > 0, "eps and stepmax must be positive.");
	NRM_REQUIRE(a.stepmax <= NRM_FRONT_MAX_STEPS, "%s: at most %lld steps", who, (long long)NRM_FRONT_MAX_STEPS);
	NRM_REQUIRE(a.tol > 0 && a.tol < 1, "%s: tol must lie in (0, 1)", who);
	NRM_REQUIRE(a.ntot != 0, "ntot must be positive (t0 = ntot + 2 > 2, lcpm.py:95).");
	NRM_REQUIRE(a.count_cap >= 2 && a.count_cap <= table_cap, "%s: count_cap must lie in [2, %lld]", who, (long long)table_cap);
	for (int64_t r = 0; r < a.n_cov; r++) {
		const double* row = a.h_cov + r * a.n;
		for (int64_t k = 0; k < a.n; k++) NRM_REQUIRE(std::isfinite(row[k]), "array must not contain infs or NaNs");
		NRM_REQUIRE(nrm_normcov_row_class(row, a.n) != NRM_COV_CONSTANT, "Detected constant covariate. Please only provide full-rank covariate without constant covariate.");
	}
	return NRM_OK;
}
static inline int nrm_front_plan_create_args(const NrmFrontPlanArgs& a, int64_t max_covariates, int64_t table_cap) {
	NRM_REQUIRE(!a.csr, "nrm_front_plan_create: a dense matrix (nrm_front_plan_create_csr takes CSR counts)");
	return nrm_front_plan_args_check("nrm_front_plan_create", a, max_covariates, table_cap);
}
static inline int nrm_front_plan_create_csr_args(const NrmFrontPlanArgs& a, int64_t max_covariates, int64_t table_cap) {
	NRM_REQUIRE(a.csr, "nrm_front_plan_create_csr: CSR counts (nrm_front_plan_create takes a dense matrix)");
	return nrm_front_plan_args_check("nrm_front_plan_create_csr", a, max_covariates, table_cap);
}
// Every check of upload_csr, before any copy: the plan holds CSR counts of its own, the new ones fit, and their offsets are a CSR matrix's
static inline int nrm_front_plan_upload_csr_args(bool csr, bool adopted, int64_t rows, int64_t nnz_cap, const int64_t* indptr, const int32_t* indices, const void* data, int64_t nnz) {
	const char* who = "nrm_front_plan_upload_csr";
	NRM_REQUIRE(csr, "%s: the plan holds a dense matrix (nrm_front_plan_upload)", who);
	NRM_REQUIRE(!adopted, "%s: the plan adopted the caller's device matrix (rewrite it in place)", who);
	NRM_REQUIRE(indptr != nullptr && (nnz <= 0 || (indices != nullptr && data != nullptr)), "%s: null pointer", who);
	NRM_REQUIRE(nnz >= 0 && nnz <= nnz_cap, "%s: %lld stored entries, beyond the plan's nnz_cap = %lld", who, (long long)nnz, (long long)nnz_cap);
	return nrm_front_csr_offsets(indptr, rows, nnz);
}

// compute_var's counters ([0] nrm_fitvar_genes, [1] nrm_fitvar_weights) as what the reference raises (norm.py:108,125-127).  nrm_compute_var_host and the plan's
// check both say it through here.
static inline int nrm_compute_var_status(const int32_t f[2]) {
	if (f[0]) {
		nrm_set_error("compute_var: %d genes with a constant residual, whose spread divides (norm.py:108,125)", f[0]);
		return NRM_E_NUMERIC;
	}
	if (f[1]) {
		nrm_set_error("compute_var: %d weights are not finite and positive (norm.py:125-127)", f[1]);
		return NRM_E_NUMERIC;
	}
	return NRM_OK;
}

// normvar's counters ([0] genes of rank 0: nrm_normvar_solve, [1] nrm_normvar_apply) as what the reference raises (norm.py:160,286).  The plan's check says both
// through here; nrm_normvar_host hands the count of [0] to its caller with NRM_OK (*zero_rank) and says [1] through here.
static inline int nrm_normvar_status(const int32_t f[2]) {
	if (f[0]) {
		nrm_set_error("Zero-rank covariates found.");
		return NRM_E_DEVICE;
	}
	if (f[1]) {
		nrm_set_error("normvar: non-finite results (norm.py:286)");
		return NRM_E_NUMERIC;
	}
	return NRM_OK;
}

// The plan's counters as what the reference raises, in the order it would meet them: lcpm (lcpm.py:86, :97, :196), the table cap, normcov (norm.py:34-37),
// compute_var (norm.py:108,125-127), scaling_factor (lcpm.py:278-282), normvar (norm.py:160,286).  f: the sixteen counters; cap and count for the cap's words.
static inline int nrm_front_plan_status(const int32_t f[16], int64_t cap, int64_t count) {
	NRM_REQUIRE(!f[0], "Negative value in d detected.");
	if (f[2]) {
		nrm_set_error("lcpm: the matrix holds no read (t0 = sum + 2 > 2, lcpm.py:95)");
		return NRM_E_NUMERIC;
	}
	NRM_REQUIRE(!f[1], "Found cell with no read at all. Please remove.");
	if (f[3]) {
		nrm_set_error("nrm_front_plan: the plan tabulates psi(1 + count) for counts below count_cap = %lld; the largest count here is %lld.", (long long)cap, (long long)count);
		return NRM_E_UNSUPPORTED;
	}
	NRM_REQUIRE(!f[4], "Detected constant covariate. Please only provide full-rank covariate without constant covariate.");
	if (const int rc = nrm_compute_var_status(f + 8)) return rc;
	if (f[6]) {
		nrm_set_error("scaling_factor: no gene has a zero entry, or a value is not finite (lcpm.py:278-282)");
		return NRM_E_NUMERIC;
	}
	return nrm_normvar_status(f + 12);
}
// The same with the count pass's structure check in front (a CSR plan; a dense plan's word stays 0): malformed is a word of its own beside the sixteen, met
// before anything the malformed matrix's numbers may have set
static inline int nrm_front_plan_status_csr(int64_t malformed, const int32_t f[16], int64_t cap, int64_t count) {
	NRM_REQUIRE(!malformed, "%s", NRM_MALFORMED_CSR);
	return nrm_front_plan_status(f, cap, count);
}
