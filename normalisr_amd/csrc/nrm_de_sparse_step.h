// The sparse-design form of single=0 de (association.py:224-235 for a design with few entries), written once: the workspace of the products and the step --
// nrm_design_stats -> row sums or fused covariate table -> nrm_de_sparse -> nrm_assoc_sweep -> nrm_alpha -- that nrm_host_de_sparse (nrm_host_de.hip) and the
// resident plan (nrm_de_plan.hip) both run.  `take(DevBuf&, bytes)` allocates: the plan counts pool bytes through it, the entries pass nrm_take_plain.  The enqueue
// members launch and queue memset nodes only: a plan captures them.
#pragma once
#include "nrm_host_entry.h"

// What nrm_de_sparse needs beside its operands: `common`, and for the rows' sums with the covariates either the table `ct` the kernel fuses them from (up to
// nrm_de_sparse_fused_covariates() of them) or `code` -- every cell a shared one -- for the stream kernel of single=1, which then takes them.
struct NrmSparseProducts {
	DevBuf common, ct, code;
	template <typename Take>
	int alloc(int64_t ny, int64_t n, int64_t ncu, int ci, Take take, hipStream_t st) {
		NRM_TRY(take(common, (size_t)(ncu + 1) * ny * 8));
		if (ncu - (ci >= 0 ? 1 : 0) <= nrm_de_sparse_fused_covariates()) return take(ct, (size_t)nrm_de_sparse_ct_doubles(n, ncu, ci) * 8);
		NRM_TRY(take(code, (size_t)n * 4));
		return nrm_fill_i32(code.p, NRM_S1_COMMON, n, st);
	}
	// x~ . y~ for every (design row, expression row): d_dot (nxp, nyp) or, by_gene, (nyp, nxp)
	int enqueue(const NrmDesignLists& L, const void* d_y, int y_dtype, int64_t ny, int64_t n, int64_t ldy, const double* d_c, int64_t ncu, int ci, double cval, const double* d_dci,
				const double* d_bx, int64_t ldb, double* d_dot, int64_t ldd, int by_gene, double* d_ssy, double* d_coefy, int32_t* d_flags, hipStream_t st) const {
		if (!ct.p) NRM_TRY(nrm_single1_stream(d_y, y_dtype, ldy, d_c, n, ncu, code.as<int32_t>(), n, ny, common.as<double>(), common.p, nrm_round_up(ny, 8), st));
		return nrm_de_sparse(d_y, y_dtype, ny, n, ldy, common.as<double>(), ncu, d_dci, L.ell.as<int16_t>(), L.ellv.as<double>(), L.base.as<int64_t>(), L.w.as<int32_t>(),
							 L.sig.as<int32_t>(), L.ngroups, L.slot2x.as<int32_t>(), d_bx, ldb, d_dot, ldd, by_gene, d_ssy, d_coefy, d_flags, d_c, n, ci, cval, ct.as<double>(), st);
	}
};

struct NrmDeSparseStep {
	int64_t rows = 0, nx = 0, ny = 0, n = 0, ldy = 0, nc = 0, ncu = 0;  // rows: the design rows the buffers are sized for; nx <= rows: those of the design in L
	int y_dtype = NRM_F64, out_dtype = NRM_F64, ci = -1;                // ncu: the covariates in use (0 when their rank is 0); ci: the constant one, or -1
	bool want_alpha = false;
	double cval = 0.0, dof = 0.0;
	int64_t nxp = 0, nyp = 0;  // rows and ny rounded up to the row tile: alloc()
	const NrmDesignLists* L = nullptr;
	const void* d_y = nullptr;                      // the expression matrix (ny, n), pitch ldy
	const double *d_c = nullptr, *d_dci = nullptr;  // covariates (nc, n) fp64, their pseudo-inverse
	DevBuf ssx, bx, ssy, by, dot, flags;            // flags: the counters int32[8], cleared at alloc and by whoever reads them
	NrmSparseProducts work;

	template <typename Take>
	int alloc(Take take, hipStream_t st) {
		nxp = nrm_round_up(rows, NRM_ROW_TILE), nyp = nrm_round_up(ny, NRM_ROW_TILE);
		NRM_TRY(nrm_take_all(take, {{&flags, 32}, {&ssx, nxp * 8}, {&bx, rows * (nc > 0 ? nc : 1) * 8}, {&ssy, nyp * 8}, {&dot, nxp * nyp * 8}}));
		if (want_alpha) NRM_TRY(take(by, (size_t)ny * nc * 8));
		NRM_HIP(hipMemsetAsync(flags.p, 0, 32, st));
		return work.alloc(ny, n, ncu, ci, take, st);
	}
	// the zeroing a step needs (once, here), the design rows' statistics, the products
	int enqueue_products(hipStream_t st) {
		NRM_HIP(hipMemsetAsync(ssx.p, 0, (size_t)nxp * 8, st));
		NRM_HIP(hipMemsetAsync(bx.p, 0, (size_t)rows * (nc > 0 ? nc : 1) * 8, st));
		NRM_TRY(nrm_design_stats(L->row_ptr.as<int64_t>(), L->cells.as<int32_t>(), L->row_vals.as<double>(), ncu ? d_c : nullptr, n, ncu, ncu ? d_dci : nullptr, nx, ssx.as<double>(),
								 ncu ? bx.as<double>() : nullptr, flags.as<int32_t>(), st));
		if (want_alpha) NRM_HIP(hipMemsetAsync(by.p, 0, (size_t)ny * nc * 8, st));
		return work.enqueue(*L, d_y, y_dtype, ny, n, ldy, d_c, ncu, ci, cval, d_dci, bx.as<double>(), nc > 0 ? nc : 1, dot.as<double>(), nyp, 0, ssy.as<double>(),
							(want_alpha && ncu) ? by.as<double>() : nullptr, flags.as<int32_t>(), st);
	}
	// P-values and the statistic (nx, ny) of out_dtype, r and t on request; alpha (nx, ny, nc) when the step keeps b_y
	// (p_kind 1: ln p in p, nrm_assoc_sweep_pk; the resident plan keeps 0)
	int enqueue_sweep(hipStream_t st, void* p, void* stat, void* r, void* t, void* alpha, int stat_kind, int p_kind = 0) {
		NRM_TRY(nrm_assoc_sweep_pk(dot.as<double>(), nyp, ssx.as<double>(), ssy.as<double>(), nx, ny, n, dof, 0, stat_kind, p, stat, r, t, out_dtype, ny, flags.as<int32_t>(), 0,
								   nullptr, nullptr, 0.0, p_kind, st));
		return want_alpha ? nrm_alpha(stat, out_dtype, ny, stat_kind, ssx.as<double>(), n, bx.as<double>(), by.as<double>(), nx, ny, nc, alpha, out_dtype, st) : NRM_OK;
	}
};
