// Pieces shared by the K1 kernels (nrm_residualize.hip: k_residualize, k_residualize_v4, k_residualize_v8; tools/experiments/nrm_residualize_res.hip: k_residualize_res).
#pragma once
#include "nrm_device.h"
#include "nrm_digits.h"
#include "nrm_fix.h"

#define RES_NC_MAX 2048  // OLS tables a = x C^T and b = a dci live in dynamic LDS: 2 * RES_R * nc doubles (128 KiB at 2048)

// Every lane moves 4 consecutive cells per step (nrm_ld4: 16-byte loads of fp32 input, 32 bytes of fp64 covariates and residuals), so one wave-instruction
// covers 1-2 KiB of a row.  Needs 16-byte aligned rows: ldx % (16/sizeof(T)) == 0, ldc % 2 == 0, ldo % 4 == 0.
// Input rows are streamed (each line is used once per sweep and is gone from L2 long before the next sweep of a long row): their loads
// can be marked non-temporal (NT) so that they do not push the covariates -- re-read by every workgroup -- out of L2.  Measured: with 20
// covariates x 100 000 cells (16 MB of them) K1 20.3 -> 16.9 ms; with 5 x 50 000 (2 MB) 3.27 -> 3.20; but rows of 10 000 cells, whose second
// sweep is served from L2, 0.186 -> 0.225 ms, and fp64 rows of 500 000 cells 10.4 -> 10.9: the launcher asks for it only for fp32 rows
// with at least 8 MB of covariates.

// Fixed-point output for the integer Gram engine (csrc/nrm_gram_i8.hip): digit planes in its tiled layout and one exponent per
// row, written straight from K1 so that the fp64 residuals never make the round trip through HBM (NS = 0: none).
struct QuantOut {
	char* q;              // NS planes of plane_bytes each
	int64_t plane_bytes;
	int64_t nks;          // k-steps of 32 cells
	int64_t cks;          // k-steps per cell chunk (== nks: one chunk); chunk c is an operand of its own at q + c * chunk_bytes
	int64_t chunk_bytes;
	int* exps;            // x = digits * 2^exps[row]
	const double* cmax;   // (nc) largest |C_c| of every covariate row: bounds the residuals without a sweep of their own
	double* fix;          // (rows_pad, NRM_FIX_STRIDE) row records for K3's correction and guard (nrm_fix.h), or nullptr
};

// Loosest fixed-point scale K1 accepts from the bound max|x| + sum_c |b_c| max|C_c| without looking: bound / rms of the residuals
// (the rms estimated from the first sweep as |x|^2 - a.b).  Beyond it -- rows whose mean dwarfs their spread, near-collinear
// covariates with large opposite coefficients -- the residuals are swept for their true maximum, so that no more than log2 of
// this / (true max / rms) of the 8 NS - 2 bits are lost to the overestimate.
#define RES_LOOSE 12.0
