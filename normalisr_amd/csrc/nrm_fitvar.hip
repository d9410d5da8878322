// compute_var (reference norm.py:56-128; `normalisr fitvar`): the per-cell variance-normalisation weights that normvar takes.
// One iteration of the reference, with the cell weights u_k = 1 / s_k of the previous one (all ones in the first):
//     r_gk = u_k (y_gk - sum_c b_gc C_ck)       rows of dt u residualised against dc u   (norm.py:99-103: only FITTED values of the regression are used, so
//                                                b_g = (sum_k u_k^2 C_k C_k^T)^+ (sum_k u_k^2 y_gk C_k): the pseudo-inverse by the package's inv_rank)
//     m_g = mean_k r_gk,  sc_g = sqrt(mean_k (r_gk - m_g)^2)                              (norm.py:106-107)
//     v_k = mean_g ((r_gk - m_g) / sc_g)^2                                                (norm.py:108)
// and the rest (log, the projection onto span(C, 1), exp, the minimum, the best-step rule) is O(cells x covariates) on the host.
// The residual is never stored.  Three reads of the matrix (row-major genes x cells), each with the fit recomputed from b (nc multiply-adds per element, the
// covariates from L2), against one read, one 8-byte write and two 8-byte reads per element if K1 stored an fp64 residual for the two reductions:
//   k_fv_moments  a workgroup per FV_R genes: a_g = sum_k y_gk (u_k^2 C_k), eight covariates at a time in registers
//   k_fv_genes    the same rows: b_g = M^+ a_g, then m_g and -- in a second sweep, about the mean, while the rows are in L2 -- sc_g; flags[0] += genes whose
//                 residual is constant (sc_g = 0: the reference divides by zero there and fails its assertion, norm.py:125)
//   k_fv_cells    a workgroup per FV_TR genes x 1024 cells: per-cell partial sums of ((r - m) / sc)^2, one per row tile,
//   k_fv_finish   added in a fixed order: no floating-point atomics, the same bits every run.
// Covariates: the three passes are loops over them.  Up to FV_NC the workgroup's coefficient table is a static array of 64 columns; beyond, up to NRM_WIDE_NC
// (nrm_wide_covariates()), the WIDE instantiations of k_fv_genes and k_fv_cells keep FV_R x nc coefficients in dynamic LDS (32 KiB at 1024: no opt-in) -- the
// per-cell pass then reloads the table for every FV_R genes of its tile -- and b_g = M^+ a_g reads M^+ by columns (it is symmetric), coalesced over nc x nc.
// The launchers choose by nc; the instantiations for nc <= FV_NC are the ones the library always had.
#include "nrm_device.h"

#define FV_R 4    // genes per workgroup of the per-gene passes, and per step of the per-cell pass: they share the loads of the covariates
#define FV_Q 8    // covariates per sweep of the moments pass
#define FV_TR 32  // genes per partial sum of the per-cell pass
#define FV_NC 63  // the static coefficient tables (64 columns); beyond: the WIDE instantiations, up to NRM_WIDE_NC

extern "C" int64_t nrm_fitvar_row_tile(void) { return FV_TR; }
extern "C" int64_t nrm_wide_covariates(void) { return NRM_WIDE_NC; }

// a (rows, nc): a[g][c] = sum_k y_gk cw_ck, cw = u^2 C
template <typename T, bool ALIGNED>
__global__ void __launch_bounds__(256) k_fv_moments(const T* __restrict__ y, int64_t rows, int64_t n, int64_t ldy, const double* __restrict__ cw, int nc, int64_t ldc,
													 double* __restrict__ a) {
	__shared__ double sm[4][FV_R * FV_Q];
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t row0 = (int64_t)blockIdx.x * FV_R;
	const T* yr[FV_R];
#pragma unroll
	for (int r = 0; r < FV_R; r++) yr[r] = y + (row0 + r < rows ? row0 + r : rows - 1) * ldy;  // (rows past the end repeat the last: nothing of theirs is stored)
	for (int q0 = 0; q0 < nc; q0 += FV_Q) {
		double acc[FV_R][FV_Q];
#pragma unroll
		for (int r = 0; r < FV_R; r++)
#pragma unroll
			for (int q = 0; q < FV_Q; q++) acc[r][q] = 0.0;
		for (int64_t k = (int64_t)tid * 4; k < n; k += 1024) {
			double yv[FV_R][4];
#pragma unroll
			for (int r = 0; r < FV_R; r++) nrm_ld4d<T, ALIGNED>(yr[r], k, n, yv[r]);
#pragma unroll
			for (int q = 0; q < FV_Q; q++) {
				double cv[4] = {0.0, 0.0, 0.0, 0.0};
				if (q0 + q < nc) nrm_ld4d<double, ALIGNED>(cw + (int64_t)(q0 + q) * ldc, k, n, cv);
#pragma unroll
				for (int r = 0; r < FV_R; r++)
#pragma unroll
					for (int j = 0; j < 4; j++) acc[r][q] = fma(yv[r][j], cv[j], acc[r][q]);
			}
		}
#pragma unroll
		for (int r = 0; r < FV_R; r++)
#pragma unroll
			for (int q = 0; q < FV_Q; q++) {
				const double t = nrm_wave_sum(acc[r][q]);
				if (lane == 0) sm[wid][r * FV_Q + q] = t;
			}
		__syncthreads();
		if (tid < FV_R * FV_Q) {
			const int r = tid / FV_Q, q = tid % FV_Q;
			if (row0 + r < rows && q0 + q < nc) a[(row0 + r) * nc + q0 + q] = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
		}
		__syncthreads();
	}
}

// r[i][j] = u_j (y_ij - sum_c b_ic C_cj) for FV_R rows and the lane's four cells (zero at and beyond n: u reads as zero there)
template <typename T, bool ALIGNED>
__device__ __forceinline__ void fv_resid(const T* (&yr)[FV_R], int64_t k, int64_t n, const double* __restrict__ u, const double* __restrict__ c, int nc, int64_t ldc,
										 const double* s_b, const int ldb, double (&res)[FV_R][4]) {
	double uv[4], yv[FV_R][4], fit[FV_R][4];
	nrm_ld4d<double, ALIGNED>(u, k, n, uv);
#pragma unroll
	for (int r = 0; r < FV_R; r++) {
		nrm_ld4d<T, ALIGNED>(yr[r], k, n, yv[r]);
#pragma unroll
		for (int j = 0; j < 4; j++) fit[r][j] = 0.0;
	}
	for (int q = 0; q < nc; q++) {
		double cv[4];
		nrm_ld4d<double, ALIGNED>(c + (int64_t)q * ldc, k, n, cv);
#pragma unroll
		for (int r = 0; r < FV_R; r++)
#pragma unroll
			for (int j = 0; j < 4; j++) fit[r][j] = fma(s_b[r * ldb + q], cv[j], fit[r][j]);
	}
#pragma unroll
	for (int r = 0; r < FV_R; r++)
#pragma unroll
		for (int j = 0; j < 4; j++) res[r][j] = uv[j] * (yv[r][j] - fit[r][j]);
}

extern __shared__ __attribute__((aligned(16))) double fv_wide_b[];  // WIDE: FV_R x nc coefficients

template <typename T, bool ALIGNED, bool WIDE = false>
__global__ void __launch_bounds__(256) k_fv_genes(const T* __restrict__ y, int64_t rows, int64_t n, int64_t ldy, const double* __restrict__ u, const double* __restrict__ c,
												   int nc, int64_t ldc, const double* __restrict__ a, const double* __restrict__ mi, double* __restrict__ b,
												   double* __restrict__ mean, double* __restrict__ sc, int32_t* __restrict__ flags) {
	__shared__ double s_bn[FV_R][64];
	__shared__ double sm[4][FV_R];
	__shared__ double s_mean[FV_R];
	double* const s_b = WIDE ? fv_wide_b : &s_bn[0][0];
	const int ldb = WIDE ? nc : 64;
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t row0 = (int64_t)blockIdx.x * FV_R;
	for (int i = tid; i < FV_R * nc; i += 256) {  // b_g = M^+ a_g
		const int r = i / nc, q = i % nc;
		double t = 0.0;
		if (row0 + r < rows) {
			if constexpr (WIDE) {  // (M^+ is symmetric: column q, consecutive lanes on consecutive addresses)
				for (int d = 0; d < nc; d++) t = fma(mi[(int64_t)d * nc + q], a[(row0 + r) * nc + d], t);
			} else {
				for (int d = 0; d < nc; d++) t = fma(mi[q * nc + d], a[(row0 + r) * nc + d], t);
			}
			b[(row0 + r) * nc + q] = t;
		}
		s_b[r * ldb + q] = t;
	}
	__syncthreads();
	const T* yr[FV_R];
#pragma unroll
	for (int r = 0; r < FV_R; r++) yr[r] = y + (row0 + r < rows ? row0 + r : rows - 1) * ldy;
	double acc[FV_R];
	auto block_sum = [&](double* dst) {  // dst[r] = the workgroup's sum of acc[r], waves added in order
#pragma unroll
		for (int r = 0; r < FV_R; r++) {
			const double t = nrm_wave_sum(acc[r]);
			if (lane == 0) sm[wid][r] = t;
		}
		__syncthreads();
		if (tid < FV_R) dst[tid] = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
		__syncthreads();
	};
#pragma unroll
	for (int r = 0; r < FV_R; r++) acc[r] = 0.0;
	for (int64_t k = (int64_t)tid * 4; k < n; k += 1024) {
		double res[FV_R][4];
		fv_resid<T, ALIGNED>(yr, k, n, u, c, nc, ldc, s_b, ldb, res);
#pragma unroll
		for (int r = 0; r < FV_R; r++) acc[r] += (res[r][0] + res[r][1]) + (res[r][2] + res[r][3]);
	}
	block_sum(s_mean);
	double m[FV_R];
#pragma unroll
	for (int r = 0; r < FV_R; r++) {
		m[r] = s_mean[r] / (double)n;
		acc[r] = 0.0;
	}
	__syncthreads();
	for (int64_t k = (int64_t)tid * 4; k < n; k += 1024) {  // the second sweep: about the mean (the rows come from L2)
		double res[FV_R][4];
		fv_resid<T, ALIGNED>(yr, k, n, u, c, nc, ldc, s_b, ldb, res);
#pragma unroll
		for (int r = 0; r < FV_R; r++)
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const double d = k + j < n ? res[r][j] - m[r] : 0.0;
				acc[r] = fma(d, d, acc[r]);
			}
	}
	block_sum(s_mean);
	if (tid < FV_R && row0 + tid < rows) {
		const double s = sqrt(s_mean[tid] / (double)n);
		mean[row0 + tid] = m[tid];
		sc[row0 + tid] = s;
		if (!(s > 0.0 && s <= 1.7976931348623157e308)) atomicAdd(&flags[0], 1);
	}
}

template <typename T, bool ALIGNED, bool WIDE = false>
__global__ void __launch_bounds__(256) k_fv_cells(const T* __restrict__ y, int64_t rows, int64_t n, int64_t ldy, const double* __restrict__ u, const double* __restrict__ c,
												   int nc, int64_t ldc, const double* __restrict__ b, const double* __restrict__ mean, const double* __restrict__ sc,
												   double* __restrict__ partial) {
	__shared__ double s_bn[WIDE ? 1 : FV_TR][64];
	__shared__ double s_m[FV_TR], s_s[FV_TR];
	const int tid = threadIdx.x;
	const int64_t k = ((int64_t)blockIdx.x * 256 + tid) * 4, row0 = (int64_t)blockIdx.y * FV_TR;
	const int nr = (int)(rows - row0 < FV_TR ? rows - row0 : FV_TR);
	if constexpr (!WIDE) {
		for (int i = tid; i < FV_TR * nc; i += 256) {
			const int r = i / nc, q = i % nc;
			s_bn[r][q] = r < nr ? b[(row0 + r) * nc + q] : 0.0;
		}
	}
	if (tid < FV_TR) {
		s_m[tid] = tid < nr ? mean[row0 + tid] : 0.0;
		s_s[tid] = tid < nr ? sc[row0 + tid] : 1.0;
	}
	__syncthreads();
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
	for (int r0 = 0; r0 < nr; r0 += FV_R) {
		const T* yr[FV_R];
#pragma unroll
		for (int r = 0; r < FV_R; r++) yr[r] = y + (r0 + r < nr ? row0 + r0 + r : rows - 1) * ldy;
		double res[FV_R][4];
		if constexpr (WIDE) {  // the table of these FV_R genes (nr and r0 are the same for every thread of the workgroup: the barriers are uniform)
			__syncthreads();
			for (int i = tid; i < FV_R * nc; i += 256) {
				const int r = i / nc, q = i % nc;
				fv_wide_b[i] = r0 + r < nr ? b[(row0 + r0 + r) * nc + q] : 0.0;
			}
			__syncthreads();
			fv_resid<T, ALIGNED>(yr, k, n, u, c, nc, ldc, fv_wide_b, nc, res);
		} else {
			fv_resid<T, ALIGNED>(yr, k, n, u, c, nc, ldc, &s_bn[r0][0], 64, res);
		}
#pragma unroll
		for (int r = 0; r < FV_R; r++)
			if (r0 + r < nr) {
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const double d = (res[r][j] - s_m[r0 + r]) / s_s[r0 + r];
					acc[j] = fma(d, d, acc[j]);
				}
			}
	}
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (k + j < n) partial[(int64_t)blockIdx.y * n + k + j] = acc[j];
}

// v[k] = the partial sums of cell k added in a fixed order (a wave owns 64 consecutive cells, the workgroup's four waves every fourth tile each) / rows
__global__ void __launch_bounds__(256) k_fv_finish(const double* __restrict__ partial, int64_t tiles, int64_t n, int64_t rows, double* __restrict__ v) {
	__shared__ double sm[4][64];
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int64_t k = (int64_t)blockIdx.x * 64 + lane;
	double s = 0.0;
	if (k < n)
		for (int64_t t = wid; t < tiles; t += 4) s += partial[t * n + k];
	sm[wid][lane] = s;
	__syncthreads();
	if (wid == 0 && k < n) v[k] = (((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane]) / (double)rows;
}

static bool fv_aligned(const void* d_y, int y_dtype, int64_t ldy, const double* d_u, const double* d_c, int64_t ldc) {
	return (uintptr_t)d_y % 16 == 0 && (ldy * (y_dtype == NRM_F64 ? 8 : 4)) % 16 == 0 && (d_u == nullptr || (uintptr_t)d_u % 16 == 0) && (uintptr_t)d_c % 16 == 0 && ldc % 2 == 0;
}

static int fv_check(const char* what, const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_c, int64_t nc, int64_t ldc) {
	NRM_REQUIRE(y_dtype == NRM_F32 || y_dtype == NRM_F64, "%s: bad dtype", what);
	NRM_REQUIRE(d_y && d_c && rows > 0 && n > 0 && ldy >= n && ldc >= n, "%s: bad shape", what);
	NRM_REQUIRE(nc >= 1 && nc <= NRM_WIDE_NC, "%s: 1 to %d covariates", what, NRM_WIDE_NC);
	return NRM_OK;
}

#define FV_LAUNCH(KERNEL, GRID, ...)                                                                          \
	do {                                                                                                      \
		if (y_dtype == NRM_F64) {                                                                             \
			if (al) hipLaunchKernelGGL((KERNEL<double, true>), GRID, dim3(256), 0, st, (const double*)d_y, __VA_ARGS__);  \
			else hipLaunchKernelGGL((KERNEL<double, false>), GRID, dim3(256), 0, st, (const double*)d_y, __VA_ARGS__);    \
		} else {                                                                                              \
			if (al) hipLaunchKernelGGL((KERNEL<float, true>), GRID, dim3(256), 0, st, (const float*)d_y, __VA_ARGS__);    \
			else hipLaunchKernelGGL((KERNEL<float, false>), GRID, dim3(256), 0, st, (const float*)d_y, __VA_ARGS__);      \
		}                                                                                                     \
	} while (0)

// the WIDE instantiations (nc > FV_NC): FV_R x nc doubles of dynamic LDS
#define FV_LAUNCH_WIDE(KERNEL, GRID, ...)                                                                     \
	do {                                                                                                      \
		const size_t lds = (size_t)FV_R * (size_t)nc * sizeof(double);                                        \
		if (y_dtype == NRM_F64) {                                                                             \
			if (al) hipLaunchKernelGGL((KERNEL<double, true, true>), GRID, dim3(256), lds, st, (const double*)d_y, __VA_ARGS__);  \
			else hipLaunchKernelGGL((KERNEL<double, false, true>), GRID, dim3(256), lds, st, (const double*)d_y, __VA_ARGS__);    \
		} else {                                                                                              \
			if (al) hipLaunchKernelGGL((KERNEL<float, true, true>), GRID, dim3(256), lds, st, (const float*)d_y, __VA_ARGS__);    \
			else hipLaunchKernelGGL((KERNEL<float, false, true>), GRID, dim3(256), lds, st, (const float*)d_y, __VA_ARGS__);      \
		}                                                                                                     \
	} while (0)

extern "C" int nrm_fitvar_moments(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_cw, int64_t nc, int64_t ldc, double* d_a, void* stream) {
	NRM_TRY(fv_check("nrm_fitvar_moments", d_y, y_dtype, rows, n, ldy, d_cw, nc, ldc));
	NRM_REQUIRE(d_a, "nrm_fitvar_moments: null pointer");
	hipStream_t st = (hipStream_t)stream;
	const bool al = fv_aligned(d_y, y_dtype, ldy, nullptr, d_cw, ldc);
	FV_LAUNCH(k_fv_moments, dim3((unsigned)((rows + FV_R - 1) / FV_R)), rows, n, ldy, d_cw, (int)nc, ldc, d_a);
	return nrm_check_launch("k_fv_moments");
}

extern "C" int nrm_fitvar_genes(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_u, const double* d_c, int64_t nc, int64_t ldc,
								const double* d_a, const double* d_mi, double* d_b, double* d_mean, double* d_sc, int32_t* d_flags, void* stream) {
	NRM_TRY(fv_check("nrm_fitvar_genes", d_y, y_dtype, rows, n, ldy, d_c, nc, ldc));
	NRM_REQUIRE(d_u && d_a && d_mi && d_b && d_mean && d_sc && d_flags, "nrm_fitvar_genes: null pointer");
	hipStream_t st = (hipStream_t)stream;
	const bool al = fv_aligned(d_y, y_dtype, ldy, d_u, d_c, ldc);
	if (nc > FV_NC) FV_LAUNCH_WIDE(k_fv_genes, dim3((unsigned)((rows + FV_R - 1) / FV_R)), rows, n, ldy, d_u, d_c, (int)nc, ldc, d_a, d_mi, d_b, d_mean, d_sc, d_flags);
	else FV_LAUNCH(k_fv_genes, dim3((unsigned)((rows + FV_R - 1) / FV_R)), rows, n, ldy, d_u, d_c, (int)nc, ldc, d_a, d_mi, d_b, d_mean, d_sc, d_flags);
	return nrm_check_launch("k_fv_genes");
}

extern "C" int nrm_fitvar_cells(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_u, const double* d_c, int64_t nc, int64_t ldc,
								const double* d_b, const double* d_mean, const double* d_sc, double* d_partial, double* d_v, void* stream) {
	NRM_TRY(fv_check("nrm_fitvar_cells", d_y, y_dtype, rows, n, ldy, d_c, nc, ldc));
	NRM_REQUIRE(d_u && d_b && d_mean && d_sc && d_partial && d_v, "nrm_fitvar_cells: null pointer");
	const int64_t tiles = (rows + FV_TR - 1) / FV_TR;
	NRM_REQUIRE(tiles <= 65535, "nrm_fitvar_cells: at most %d rows", 65535 * FV_TR);
	hipStream_t st = (hipStream_t)stream;
	const bool al = fv_aligned(d_y, y_dtype, ldy, d_u, d_c, ldc);
	if (nc > FV_NC) FV_LAUNCH_WIDE(k_fv_cells, dim3((unsigned)((n + 1023) / 1024), (unsigned)tiles), rows, n, ldy, d_u, d_c, (int)nc, ldc, d_b, d_mean, d_sc, d_partial);
	else FV_LAUNCH(k_fv_cells, dim3((unsigned)((n + 1023) / 1024), (unsigned)tiles), rows, n, ldy, d_u, d_c, (int)nc, ldc, d_b, d_mean, d_sc, d_partial);
	NRM_TRY(nrm_check_launch("k_fv_cells"));
	hipLaunchKernelGGL(k_fv_finish, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, d_partial, tiles, n, rows, d_v);
	return nrm_check_launch("k_fv_finish");
}
