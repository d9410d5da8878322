// compute_var (norm.py:56-128) on a matrix in HBM, written once: the sizes, the buffers and the launch sequence -- nrm_fitvar_plan_start; `stepmax` times design,
// pinv, moments, genes, cells, update; nrm_fitvar_weights -- that nrm_compute_var_host (nrm_host_front.hip) and the resident front-half plan (nrm_front_plan.hip)
// both run.  It is the C twin of norm.ComputeVarPlan._launch, which drives the same entries on torch's tensors.  The caller sets the sizes and the non-owning
// pointers; `take(DevBuf&, bytes)` allocates (the plan's counts pool bytes, the entry passes nrm_take_plain).  Only alloc allocates; what enqueue queues, a plan
// captures.  Where m2i comes from stays with the caller: nrm_pinv_gram_unit_rows on the host in the entry, a kernel of its own in the plan.
#pragma once
#include "nrm_host_entry.h"

struct NrmFitvarStep {
	int64_t rows = 0, n = 0, ldy = 0, nc = 0, stepmax = 1;
	double eps = 1e-6;
	int y_dtype = NRM_F64;
	const void* d_y = nullptr;      // the matrix (rows, n), pitch ldy
	const double* d_c = nullptr;    // covariates (nc, n)
	const double* d_m2i = nullptr;  // (nc + 1, nc + 1): the pseudo-inverse of [C;1][C;1]^T on unit-length rows (the second regression, norm.py:92,109-110)
	int32_t* flags = nullptr;       // int32[4], cleared by the caller: [0] += genes with a constant residual, [1] += weights that are not finite and positive
	DevBuf a, b, mean, sc, v, part, s, best, u, cw, mi, rank, ws, out;

	template <typename Take>
	int alloc(Take take) {
		const int64_t tiles = (rows + nrm_fitvar_row_tile() - 1) / nrm_fitvar_row_tile();
		return nrm_take_all(take, {{&a, rows * nc * 8}, {&b, rows * nc * 8}, {&mean, rows * 8}, {&sc, rows * 8}, {&v, n * 8}, {&part, tiles * n * 8}, {&s, n * 8}, {&best, n * 8},
								   {&u, n * 8}, {&cw, nc * n * 8}, {&mi, nc * nc * 8}, {&rank, 8}, {&ws, nrm_fitvar_plan_workspace(n, nc) * 8}, {&out, out_doubles() * 8}});
	}
	// out: the state records of four doubles (one per iteration and the first) and, right after the last, the weights: a caller reads both in one copy
	int64_t out_doubles() const { return 4 * (stepmax + 1) + n; }
	double* state() const { return out.as<double>(); }
	double* w() const { return state() + 4 * (stepmax + 1); }

	int enqueue(hipStream_t st) {
		double *S = s.as<double>(), *B = best.as<double>(), *U = u.as<double>(), *CW = cw.as<double>(), *WS = ws.as<double>();
		NRM_TRY(nrm_fitvar_plan_start(n, S, B, state(), st));
		for (int64_t i = 0; i < stepmax; i++) {
			const double* now = state() + 4 * i;
			NRM_TRY(nrm_fitvar_design(d_c, nc, n, n, S, now, eps, U, CW, WS, st));
			NRM_TRY(nrm_fitvar_pinv(n, nc, 1e-8, now, eps, WS, mi.as<double>(), rank.as<int64_t>(), st));
			NRM_TRY(nrm_fitvar_moments(d_y, y_dtype, rows, n, ldy, CW, nc, n, a.as<double>(), st));
			NRM_TRY(nrm_fitvar_genes(d_y, y_dtype, rows, n, ldy, U, d_c, nc, n, a.as<double>(), mi.as<double>(), b.as<double>(), mean.as<double>(), sc.as<double>(), flags, st));
			NRM_TRY(nrm_fitvar_cells(d_y, y_dtype, rows, n, ldy, U, d_c, nc, n, b.as<double>(), mean.as<double>(), sc.as<double>(), part.as<double>(), v.as<double>(), st));
			NRM_TRY(nrm_fitvar_update(v.as<double>(), d_c, nc, n, n, d_m2i, S, B, now, state() + 4 * (i + 1), eps, WS, st));
		}
		return nrm_fitvar_weights(B, n, WS, w(), flags, st);
	}
};
