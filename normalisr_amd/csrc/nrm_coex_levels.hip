// One more covariate for a co-expression problem that stays in HBM (normalisr_amd/levels.py; reference association.py:224-235 applied to an enlarged dc).
// With q a unit vector orthogonal to the present covariates, the residual Gram matrix G = X (I - P) X^T of the raw rows X becomes G - a a^T, a = X q, and the
// sums of squares ss - a^2 (Frisch-Waugh: q is orthogonal to the covariates, so the raw row serves).
//   k_coex_project    A[k, i] = sum_c X[i, c] Q[k, c]: the one read of the expression matrix.  A workgroup owns R rows and all their cells; products are rounded
//                     to fp64, every sum is carried as an unevaluated pair (two-sum): a lane over its cells in rising order, the lanes of a wave by a shuffle
//                     tree, the four waves in their order.  No floating-point atomics: the same bits on every run.
//   k_coex_downdate   G[i, j] -= A[k, i] A[k, j] for k rising, every product with its rounding error (one fma) and every sum a two-sum, rounded once at the end, on the
//                     64 x 64 tiles with column tile >= row tile; the same for ss, with the two counters.
// Both are bound by memory: X is read once for up to 8 directions, G read and written once.
#include "nrm_common.h"

#define CL_TILE 64  // tile edge of k_coex_downdate

// s + b -> (s, e): Knuth's two-sum, exact for any a, b; the error is added to e.  The file is compiled without contraction where it matters (see below).
__device__ __forceinline__ void cl_add(double& s, double& e, double b) {
#pragma clang fp contract(off)
	const double t = s + b;
	const double bb = t - s;
	e += (s - (t - bb)) + (b - bb);
	s = t;
}

// (s, e) += (s2, e2)
__device__ __forceinline__ void cl_add2(double& s, double& e, double s2, double e2) {
#pragma clang fp contract(off)
	cl_add(s, e, s2);
	e += e2;
}

// (s, e) -= x y: the product rounded once, its rounding error recovered by one fma (exact), both added by two-sum.  Every step gives the same bits for (x, y) and
// (y, x), and s + e at the end is the exact result rounded once, up to terms of second order: a chain of k rounded fmas would carry k roundings.
__device__ __forceinline__ void cl_sub_product(double& s, double& e, double x, double y) {
#pragma clang fp contract(off)
	const double p = x * y;
	const double pe = fma(x, y, -p);
	cl_add(s, e, -p);
	e -= pe;
}

template <typename T, int K, int R>
__global__ void __launch_bounds__(256) k_coex_project(const T* __restrict__ x, int64_t nt, int64_t ns, int64_t ldx, const double* __restrict__ q, int64_t ldq,
													   double* __restrict__ a, int64_t lda) {
#pragma clang fp contract(off)
	__shared__ double sm[4][R * K][2];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t i0 = (int64_t)blockIdx.x * R;
	const T* row[R];
#pragma unroll
	for (int r = 0; r < R; r++) {
		const int64_t i = i0 + r < nt ? i0 + r : nt - 1;  // (rows past the end read the last row again; their sums are not stored)
		row[r] = x + i * ldx;
	}
	double s[R][K], e[R][K];
#pragma unroll
	for (int r = 0; r < R; r++)
#pragma unroll
		for (int k = 0; k < K; k++) s[r][k] = 0, e[r][k] = 0;
	int64_t c = tid;
	for (; c + 256 < ns; c += 512) {  // two cells per lane in flight
		double xv[2][R], qv[2][K];
#pragma unroll
		for (int u = 0; u < 2; u++) {
#pragma unroll
			for (int r = 0; r < R; r++) xv[u][r] = (double)row[r][c + u * 256];
#pragma unroll
			for (int k = 0; k < K; k++) qv[u][k] = q[k * ldq + c + u * 256];
		}
#pragma unroll
		for (int u = 0; u < 2; u++)
#pragma unroll
			for (int r = 0; r < R; r++)
#pragma unroll
				for (int k = 0; k < K; k++) cl_add(s[r][k], e[r][k], xv[u][r] * qv[u][k]);
	}
	for (; c < ns; c += 256) {
#pragma unroll
		for (int r = 0; r < R; r++) {
			const double xv = (double)row[r][c];
#pragma unroll
			for (int k = 0; k < K; k++) cl_add(s[r][k], e[r][k], xv * q[k * ldq + c]);
		}
	}
#pragma unroll
	for (int r = 0; r < R; r++)
#pragma unroll
		for (int k = 0; k < K; k++) {
			double ss = s[r][k], ee = e[r][k];
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				const double s2 = __shfl_down(ss, o, 64), e2 = __shfl_down(ee, o, 64);
				cl_add2(ss, ee, s2, e2);
			}
			if (lane == 0) {
				sm[wave][r * K + k][0] = ss;
				sm[wave][r * K + k][1] = ee;
			}
		}
	__syncthreads();
	if (tid < R * K) {
		const int r = tid / K, k = tid % K;
		double ss = sm[0][tid][0], ee = sm[0][tid][1];
		for (int w = 1; w < 4; w++) cl_add2(ss, ee, sm[w][tid][0], sm[w][tid][1]);
		if (i0 + r < nt) a[(int64_t)k * lda + i0 + r] = ss + ee;
	}
}

__global__ void __launch_bounds__(256) k_coex_downdate(double* __restrict__ g, int64_t nt, int64_t ld, double* __restrict__ ss, const double* __restrict__ ssref,
														const double* __restrict__ a, int64_t k, int64_t lda, int32_t* __restrict__ counters) {
	const int64_t bx = blockIdx.x, by = blockIdx.y;
	if (bx < by) return;  // (tiles below the diagonal are not part of the matrix)
	const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
	const int64_t j = bx * CL_TILE + tx;
	if (j >= nt) return;  // (columns >= nt are padding)
	const int64_t r0 = by * CL_TILE;
	for (int t = 0; t < CL_TILE / 4; t++) {
		const int64_t i = r0 + ty + 4 * t;
		if (i >= nt) break;
		double v = g[i * ld + j], e = 0;
		for (int64_t kk = 0; kk < k; kk++) cl_sub_product(v, e, a[kk * lda + i], a[kk * lda + j]);
		g[i * ld + j] = v + e;
	}
	if (by == 0 && ty == 0) {
		double v = ss[j], e = 0;
		for (int64_t kk = 0; kk < k; kk++) cl_sub_product(v, e, a[kk * lda + j], a[kk * lda + j]);
		v += e;
		ss[j] = v;
		if (!(isfinite(v) && v > 0)) atomicAdd(counters, 1);
		if (v < 0x1p-10 * ssref[j]) atomicAdd(counters + 1, 1);
	}
}

template <typename T, int K>
static void cl_launch_project(const T* x, int64_t nt, int64_t ns, int64_t ldx, const double* q, int64_t ldq, double* a, int64_t lda, hipStream_t st) {
	constexpr int R = K <= 2 ? 8 : (K <= 4 ? 4 : 2);
	hipLaunchKernelGGL((k_coex_project<T, K, R>), dim3((unsigned)((nt + R - 1) / R)), dim3(256), 0, st, x, nt, ns, ldx, q, ldq, a, lda);
}

template <typename T>
static void cl_project(int k, const T* x, int64_t nt, int64_t ns, int64_t ldx, const double* q, int64_t ldq, double* a, int64_t lda, hipStream_t st) {
	switch (k) {
		case 1: cl_launch_project<T, 1>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		case 2: cl_launch_project<T, 2>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		case 3: cl_launch_project<T, 3>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		case 4: cl_launch_project<T, 4>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		case 5: cl_launch_project<T, 5>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		case 6: cl_launch_project<T, 6>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		case 7: cl_launch_project<T, 7>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
		default: cl_launch_project<T, 8>(x, nt, ns, ldx, q, ldq, a, lda, st); break;
	}
}

extern "C" int nrm_coex_project(const void* d_x, int x_dtype, int64_t nt, int64_t ns, int64_t ldx, const double* d_q, int64_t k, int64_t ldq, double* d_a, int64_t lda,
								void* stream) {
	NRM_REQUIRE(x_dtype == NRM_F32 || x_dtype == NRM_F64, "nrm_coex_project: the expression is NRM_F32 or NRM_F64");
	NRM_REQUIRE(d_x && d_q && d_a && nt > 0 && ns > 0 && ldx >= ns && ldq >= ns && lda >= nt, "nrm_coex_project: bad shape");
	NRM_REQUIRE(k >= 1 && k <= 8, "nrm_coex_project: 1 to 8 directions per launch");
	NRM_REQUIRE(nt <= 0x7fffffffLL, "nrm_coex_project: at most 2^31 - 1 rows");
	NRM_REQUIRE((uintptr_t)d_x % (x_dtype == NRM_F64 ? 8 : 4) == 0 && (uintptr_t)d_q % 8 == 0 && (uintptr_t)d_a % 8 == 0, "nrm_coex_project: misaligned");
	if (x_dtype == NRM_F64)
		cl_project<double>((int)k, (const double*)d_x, nt, ns, ldx, d_q, ldq, d_a, lda, (hipStream_t)stream);
	else
		cl_project<float>((int)k, (const float*)d_x, nt, ns, ldx, d_q, ldq, d_a, lda, (hipStream_t)stream);
	return nrm_check_launch("k_coex_project");
}

extern "C" int nrm_coex_downdate(double* d_g, int64_t nt, int64_t ld, double* d_ss, const double* d_ss_ref, const double* d_a, int64_t k, int64_t lda, int32_t* d_counters,
								 void* stream) {
	NRM_REQUIRE(d_g && d_ss && d_ss_ref && d_a && d_counters && nt > 0 && ld >= nt && k >= 1 && lda >= nt, "nrm_coex_downdate: bad shape");
	NRM_REQUIRE((uintptr_t)d_g % 8 == 0 && (uintptr_t)d_ss % 8 == 0 && (uintptr_t)d_ss_ref % 8 == 0 && (uintptr_t)d_a % 8 == 0 && (uintptr_t)d_counters % 4 == 0,
				"nrm_coex_downdate: misaligned");
	const int64_t tiles = (nt + CL_TILE - 1) / CL_TILE;
	NRM_REQUIRE(tiles <= 65535, "nrm_coex_downdate: at most 65535 x 64 rows");
	hipLaunchKernelGGL(k_coex_downdate, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, (hipStream_t)stream, d_g, nt, ld, d_ss, d_ss_ref, d_a, k, lda, d_counters);
	return nrm_check_launch("k_coex_downdate");
}
