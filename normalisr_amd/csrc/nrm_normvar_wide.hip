// normvar (reference norm.py:154-163,232-259) with more covariates than the coefficient tables of csrc/nrm_normvar.hip hold: 64 to NRM_WIDE_NC rows,
// rank-deficient sets (one-hot batches beside the intercept) included.  The reference takes, for every gene, the pseudo-inverse of the (nc, nc) matrix
// dc diag(e_g^2) dc^T, e_gk = w_k^wt_g.  Here the host replaces dc ONCE by an orthonormal basis B (r, n) of its row space (normalisr_amd/norm.py:
// _wide_basis, with the certificate that every gene's reference rank is r); diag(e_g) is invertible, so B diag(e_g) spans what dc diag(e_g) spans and
//     M_g = B diag(e_g^2) B^T   (r x r, symmetric positive definite, condition <= (e_max / e_min)^2)
// gives the same projection by a Cholesky solve  M_g b_g = a_g,  a_g = B (e_g^2 o y_g).  M_g and a_g are rows of U P^T and V B^T on the fp64 matrix
// cores (k_nv_weights writes U = e^2 and V = e^2 y; nrm_gram_f64_whole: the same bits however the genes and pairs are cut into launches), with
//   k_nvw_pairs   P = the r (r + 1) / 2 products B_i o B_j (i <= j, the order of numpy's triu_indices), built a PANEL of rows at a time: at r = 377 and
//                 10 000 cells all of P is 5.7 GB, a panel of 2048 rows 164 MB;
//   k_nvw_chol    a workgroup per gene.  The packed upper triangle of M_g (row i holds j = i .. r - 1) is r (r + 1) / 2 doubles in GLOBAL memory
//                 -- 570 KB at r = 377, 4.2 MB at 1024: far beyond LDS -- so the factorisation M = U^T U is BLOCKED, right-looking, 16 rows at a time, with
//                 LDS as the staging area: the 16 x 16 diagonal block is factored in LDS; the 16 x (r - k) row panel is solved a column per thread
//                 against it; the trailing update streams the panel through LDS in two chunks of 128 columns and each thread updates an 8 x 8
//                 register tile of a 128 x 128 block of the triangle.  Then U^T z = a (a row of U per step), U b = z (a dot product per step), the
//                 variance-keeping scale (dv / dv2)^wt_g with dv2^2 = (s2 - a . b) / n (norm.py:248-259; |y' - P y'|^2 = |y'|^2 - a . b).
//                 A pivot that is not positive, or any value that is not finite, ends that gene: its status is recorded, d_flags counts it, b_g and the
//                 scale are written as zeros -- never a fault, never a NaN handed on silently.  Every sum is in a fixed order: the same bits every run.
#include "nrm_device.h"

#define NVW_NB 16    // rows per block step of the factorisation
#define NVW_CH 128   // columns per LDS chunk of the trailing update

// start of row i in the packed upper triangle of an (r, r) matrix
__device__ __forceinline__ int64_t nvw_row(int64_t i, int64_t r) { return i * r - i * (i - 1) / 2; }

// P[t][k] = B[i][k] * B[j][k] for pair pair0 + t = (i, j) in triu order; rows t >= count and cells k >= n are zero.  One workgroup per row and 1024 cells.
__global__ void __launch_bounds__(256) k_nvw_pairs(const double* __restrict__ B, int r, int64_t n, int64_t ldb, int64_t pair0, int64_t count,
													double* __restrict__ P, int64_t ldp) {
	const int64_t t = blockIdx.x;
	double* dst = P + t * ldp;
	const int64_t kbeg = (int64_t)blockIdx.y * 1024, kend = kbeg + 1024 < ldp ? kbeg + 1024 : ldp;
	if (t >= count) {
		for (int64_t k = kbeg + threadIdx.x; k < kend; k += 256) dst[k] = 0.0;
		return;
	}
	const int64_t p = pair0 + t;
	// row i of the triangle: the largest i with nvw_row(i) <= p (a floating-point guess, then exact steps)
	const double rr = 2.0 * r + 1.0;
	int64_t i = (int64_t)((rr - sqrt(fmax(rr * rr - 8.0 * (double)p, 0.0))) * 0.5);
	if (i < 0) i = 0;
	if (i > r - 1) i = r - 1;
	while (i > 0 && nvw_row(i, r) > p) i--;
	while (i + 1 < r && nvw_row(i + 1, r) <= p) i++;
	const int64_t j = i + (p - nvw_row(i, r));
	const double* bi = B + i * ldb;
	const double* bj = B + j * ldb;
	for (int64_t k = kbeg + threadIdx.x; k < kend; k += 256) dst[k] = k < n ? bi[k] * bj[k] : 0.0;
}

__global__ void __launch_bounds__(256) k_nvw_chol(double* __restrict__ M, int64_t ldm, const double* __restrict__ A, int64_t lda, int r,
												   const double* __restrict__ s1, const double* __restrict__ s2, const double* __restrict__ wt, double n, int keepvar,
												   double* __restrict__ Bout, double* __restrict__ scale, int32_t* __restrict__ status, int32_t* __restrict__ flags) {
	__shared__ double s_d[NVW_NB][NVW_NB + 1];
	__shared__ double s_buf[2 * NVW_NB * NVW_CH];  // factorisation: two panel chunks [16][128]; solves: x | z | diagonal, NRM_WIDE_NC each (3 x 1024 <= 4096)
	__shared__ double s_red[4];
	__shared__ int s_bad;
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t g = blockIdx.x;
	double* m = M + g * ldm;
	const double* a = A + g * lda;
	int fail = 0;  // 1: a pivot that is not positive, 2: a value that is not finite (the same in every thread: taken from LDS)
	if (tid == 0) s_bad = 0;

	for (int k0 = 0; k0 < r && !fail; k0 += NVW_NB) {
		const int nb = r - k0 < NVW_NB ? r - k0 : NVW_NB, k1 = k0 + nb;
		{  // the diagonal block, factored in LDS
			const int ti = tid >> 4, tj = tid & 15;
			s_d[ti][tj] = (ti < nb && tj < nb && tj >= ti) ? m[nvw_row(k0 + ti, r) + (k0 + tj - (k0 + ti))] : 0.0;
			__syncthreads();
			for (int kk = 0; kk < nb; kk++) {
				const double d = s_d[kk][kk];
				if (!(d > 0.0)) fail = d <= 0.0 ? 1 : 2;
				else if (!(d <= 1.7976931348623157e308)) fail = 2;
				if (fail) break;
				const double sq = sqrt(d);
				__syncthreads();
				if (ti == kk && tj >= kk && tj < nb) s_d[kk][tj] = tj == kk ? sq : s_d[kk][tj] / sq;
				__syncthreads();
				if (ti > kk && ti < nb && tj >= ti && tj < nb) s_d[ti][tj] -= s_d[kk][ti] * s_d[kk][tj];
				__syncthreads();
			}
			if (fail) break;
			if (ti < nb && tj < nb && tj >= ti) m[nvw_row(k0 + ti, r) + (tj - ti)] = s_d[ti][tj];
		}
		if (k1 >= r) break;
		// the row panel U12 = U11^-T A12: a column per thread
		for (int j = k1 + tid; j < r; j += 256) {
			double v[NVW_NB];
#pragma unroll
			for (int t = 0; t < NVW_NB; t++) v[t] = t < nb ? m[nvw_row(k0 + t, r) + (j - (k0 + t))] : 0.0;
#pragma unroll
			for (int t = 0; t < NVW_NB; t++) {
				if (t < nb) {
					double x = v[t];
#pragma unroll
					for (int q = 0; q < t; q++) x -= s_d[q][t] * v[q];
					v[t] = x / s_d[t][t];
				}
			}
#pragma unroll
			for (int t = 0; t < NVW_NB; t++)
				if (t < nb) m[nvw_row(k0 + t, r) + (j - (k0 + t))] = v[t];
		}
		__syncthreads();  // (the panel is read back below by other threads of this workgroup)
		// the trailing update A22 -= U12^T U12 on the triangle, 128 x 128 blocks, the panel's columns through LDS
		double* pi = s_buf;
		double* pj = s_buf + NVW_NB * NVW_CH;
		const int ty = tid >> 4, tx = tid & 15;
		for (int i0 = k1; i0 < r; i0 += NVW_CH)
			for (int j0 = i0; j0 < r; j0 += NVW_CH) {
				for (int e = tid; e < NVW_NB * NVW_CH; e += 256) {
					const int t = e / NVW_CH, x = e % NVW_CH;
					pi[e] = (t < nb && i0 + x < r) ? m[nvw_row(k0 + t, r) + (i0 + x - (k0 + t))] : 0.0;
					pj[e] = (t < nb && j0 + x < r) ? m[nvw_row(k0 + t, r) + (j0 + x - (k0 + t))] : 0.0;
				}
				__syncthreads();
				double acc[8][8];
#pragma unroll
				for (int p = 0; p < 8; p++)
#pragma unroll
					for (int q = 0; q < 8; q++) acc[p][q] = 0.0;
				for (int t = 0; t < NVW_NB; t++) {
					double vi[8], vj[8];
#pragma unroll
					for (int p = 0; p < 8; p++) {
						vi[p] = pi[t * NVW_CH + ty + 16 * p];
						vj[p] = pj[t * NVW_CH + tx + 16 * p];
					}
#pragma unroll
					for (int p = 0; p < 8; p++)
#pragma unroll
						for (int q = 0; q < 8; q++) acc[p][q] = fma(vi[p], vj[q], acc[p][q]);
				}
#pragma unroll
				for (int p = 0; p < 8; p++) {
					const int i = i0 + ty + 16 * p;
					if (i < r) {
						double* row = m + nvw_row(i, r) - i;
#pragma unroll
						for (int q = 0; q < 8; q++) {
							const int j = j0 + tx + 16 * q;
							if (j < r && j >= i) row[j] -= acc[p][q];
						}
					}
				}
				__syncthreads();
			}
	}
	__syncthreads();

	double* s_x = s_buf;
	double* s_z = s_buf + NRM_WIDE_NC;
	double* s_dg = s_buf + 2 * NRM_WIDE_NC;
	double ab = 0.0;
	if (!fail) {
		for (int i = tid; i < r; i += 256) {
			s_x[i] = a[i];
			s_dg[i] = m[nvw_row(i, r)];
		}
		__syncthreads();
		for (int t = 0; t < r; t++) {  // U^T z = a: row t of U against what is left of a
			const double zt = s_x[t] / s_dg[t];
			const double* row = m + nvw_row(t, r) - t;
			for (int j = t + 1 + tid; j < r; j += 256) s_x[j] -= row[j] * zt;
			if (tid == 0) s_z[t] = zt;
			__syncthreads();
		}
		for (int i = r - 1; i >= 0; i--) {  // U b = z: b in s_x
			const double* row = m + nvw_row(i, r) - i;
			double part = 0.0;
			for (int j = i + 1 + tid; j < r; j += 256) part = fma(row[j], s_x[j], part);
			part = nrm_wave_sum(part);
			if (lane == 0) s_red[wid] = part;
			__syncthreads();
			if (tid == 0) s_x[i] = (s_z[i] - (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3])) / s_dg[i];
			__syncthreads();
		}
		double part = 0.0;
		bool nf = false;
		for (int i = tid; i < r; i += 256) {
			const double bv = s_x[i];
			nf |= !(fabs(bv) <= 1.7976931348623157e308);
			part = fma(a[i], bv, part);
		}
		part = nrm_wave_sum(part);
		if (lane == 0) s_red[wid] = part;
		if (nf) atomicOr(&s_bad, 1);
		__syncthreads();
		ab = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
		if (s_bad) fail = 2;
	}
	double sc = 1.0;
	if (!fail && keepvar) {
		const double mean = s1[g] / n;
		const double dv = sqrt(fmax(s2[g] / n - mean * mean, 0.0));  // norm.py:248-249
		const double dv2 = sqrt(fmax(s2[g] - ab, 0.0) / n);          // |y' - P y'|^2 = |y'|^2 - a . b
		sc = pow(dv / dv2, wt[g]);                                     // norm.py:259
		if (!(fabs(sc) <= 1.7976931348623157e308)) fail = 2;
	}
	for (int i = tid; i < r; i += 256) Bout[g * r + i] = fail ? 0.0 : s_x[i];
	if (tid == 0) {
		scale[g] = fail ? 0.0 : sc;
		if (status) status[g] = fail;
		if (fail) atomicAdd(&flags[fail == 1 ? 0 : 1], 1);
	}
}

// d_p (rows_pad, ldp) = rows pair0 .. pair0 + count of P, then zero rows; cells n .. ldp zero.  d_b: the basis (r, ldb).
extern "C" int nrm_normvar_pairs(const double* d_b, int64_t r, int64_t n, int64_t ldb, int64_t pair0, int64_t count, double* d_p, int64_t rows_pad, int64_t ldp,
								 void* stream) {
	NRM_REQUIRE(d_b && d_p, "nrm_normvar_pairs: null pointer");
	NRM_REQUIRE(r >= 1 && r <= NRM_WIDE_NC, "nrm_normvar_pairs: 1 to %d basis rows", NRM_WIDE_NC);
	NRM_REQUIRE(n > 0 && ldb >= n && ldp >= n, "nrm_normvar_pairs: bad cell counts");
	NRM_REQUIRE(pair0 >= 0 && count >= 0 && pair0 + count <= r * (r + 1) / 2 && rows_pad >= count && rows_pad > 0 && rows_pad < (1LL << 31),
				"nrm_normvar_pairs: rows [pair0, pair0 + count) must lie in the triangle and in the panel");
	const int64_t kb = (ldp + 1023) / 1024;
	NRM_REQUIRE(kb <= 65535, "nrm_normvar_pairs: too many cells");
	hipLaunchKernelGGL(k_nvw_pairs, dim3((unsigned)rows_pad, (unsigned)kb), dim3(256), 0, (hipStream_t)stream, d_b, (int)r, n, ldb, pair0, count, d_p, ldp);
	return nrm_check_launch("k_nvw_pairs");
}

// d_m (genes, ldm): the packed upper triangles of M_g (overwritten by their Cholesky factors); d_a (genes, lda): a_g; d_s1, d_s2 (genes) from
// nrm_normvar_weights and d_wt (genes), read when keepvar != 0; n cells.  Out: d_b (genes, r), d_scale (genes), d_status (genes, may be null: 0, 1 = a pivot
// that is not positive, 2 = a value that is not finite), d_flags int32[4]: [0] += genes of status 1, [1] += genes of status 2.
extern "C" int nrm_normvar_chol(double* d_m, int64_t ldm, const double* d_a, int64_t lda, int64_t genes, int64_t r, const double* d_s1, const double* d_s2,
								const double* d_wt, int64_t n, int keepvar, double* d_b, double* d_scale, int32_t* d_status, int32_t* d_flags, void* stream) {
	NRM_REQUIRE(d_m && d_a && d_b && d_scale && d_flags, "nrm_normvar_chol: null pointer");
	NRM_REQUIRE(r >= 1 && r <= NRM_WIDE_NC, "nrm_normvar_chol: 1 to %d basis rows", NRM_WIDE_NC);
	NRM_REQUIRE(genes > 0 && genes < (1LL << 31) && ldm >= r * (r + 1) / 2 && lda >= r, "nrm_normvar_chol: bad sizes");
	NRM_REQUIRE(!keepvar || (d_s1 && d_s2 && d_wt && n > 0), "nrm_normvar_chol: keepvar needs the rows' sums, wt and the cell count");
	hipLaunchKernelGGL(k_nvw_chol, dim3((unsigned)genes), dim3(256), 0, (hipStream_t)stream, d_m, ldm, d_a, lda, (int)r, d_s1, d_s2, d_wt, (double)n, keepvar, d_b,
					   d_scale, d_status, d_flags);
	return nrm_check_launch("k_nvw_chol");
}
