// The inverse of ONE symmetric positive definite matrix M (r, r), 1 <= r <= nrm_wide_covariates(), spread over the chip: what norm.ComputeVarPlan needs per
// iteration beyond 63 covariates, where M = (B u)(B u)^T for an orthonormal basis B of the covariates' row space (normalisr_amd/norm.py: _fitvar_bases) replaces the
// reference's pseudo-inverse of the weighted covariates' Gram matrix (norm.py:100 through association.py:4-134).  No eigen-decomposition: blocked right-looking
// Cholesky M = L L^T in block columns of CI_NB = 64, then W = L^-1 block row by block row, then N = W^T W.  Tile products run on v_mfma_f64_16x16x4_f64.
// The launch sequence depends on r only (nb = ceil(r / 64) block columns), on one stream, and a launch boundary is the only dependency between workgroups:
//   k_ci_load                 A = M padded to 64 nb with the identity; a row's count of values that are not finite
//   per block column k:
//     k_ci_diag     (1 wg)    A_kk = L_kk L_kk^T in LDS, column by column, with L_kk^-1 built by the same sweep (forward substitution on the identity) -> W_kk
//     k_ci_panel    (nb-1-k)  L_ik = A_ik L_kk^-T = A_ik W_kk^T                      for i > k
//     k_ci_update   (T(T+1)/2, T = nb-1-k)  A_ij -= L_ik L_jk^T                     for i >= j > k
//   per block row i >= 1:
//     k_ci_invrow   (i)       W_ij = -W_ii sum_{j <= k < i} L_ik W_kj                for j < i
//   k_ci_gram   (nb(nb+1)/2)  N_ij = sum_{k >= j} W_ki^T W_kj for i <= j, written with its mirror image (the same bits on both sides of the diagonal)
// 4 nb - 1 launches: 63 at r = 1024.  Every output element is one workgroup's accumulator, summed over the blocks in ascending order: no floating-point atomics, the
// same bits every run and every replay of a graph that holds the sequence.
// Status: the first failure of a call decides its code (in the workspace) -- 2 for a value of M or a pivot that is not finite, 1 for a pivot that is not positive.
// A failed pivot is replaced by 1 and every launch runs to its end (no loop depends on the data); k_ci_gram then writes zeros and adds 1 to d_status[code - 1].
// nrm_chol_inverse_host: the same blocked algorithm, block boundaries and status rules in plain loops on the host, one thread (tests; not the device's bits).
#include <cmath>
#include <vector>
#include "nrm_common.h"

#define CI_NB 64    // block width
#define CI_KS 32    // cells of a k-slab of the tile products
#define CI_PN 36    // LDS pitch (doubles) of a slab held [row][k]:    16 rows x 4 k of an operand read fall on every bank twice, the minimum for 512 bytes
#define CI_PT 80    // LDS pitch (doubles) of a slab held [k][column]: the four k of an operand read alternate between the two halves of the banks
#define CI_SLAB (CI_KS * CI_PT)  // doubles per operand slab (>= CI_NB * CI_PN)
#define CI_PD 65    // LDS pitch of a 64 x 64 tile held whole

static inline int64_t ci_pad(int64_t r) { return (r + CI_NB - 1) / CI_NB * CI_NB; }

// the workspace in doubles: A (rp, rp) | W (rp, rp) | int32 row counts (rp) and the call's code
struct CiScratch {
	int64_t rp, nb;
	double *a, *w;
	int32_t *rowbad, *code;
	int64_t doubles;
	CiScratch(int64_t r, double* ws) {
		rp = ci_pad(r), nb = rp / CI_NB;
		a = ws, w = ws + rp * rp;
		rowbad = reinterpret_cast<int32_t*>(w + rp * rp);
		code = rowbad + rp;
		doubles = 2 * rp * rp + rp / 2 + 2;
	}
};

__device__ __forceinline__ bool ci_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__global__ void __launch_bounds__(256) k_ci_load(const double* __restrict__ m, int64_t ldm, int r, int rp, double* __restrict__ a, int32_t* __restrict__ rowbad) {
	const int row = blockIdx.x;
	int bad = 0;
	for (int c = threadIdx.x; c < rp; c += 256) {
		double v = row == c ? 1.0 : 0.0;
		if (row < r && c < r) {
			v = m[(int64_t)row * ldm + c];
			bad |= !ci_finite(v);
		}
		a[(int64_t)row * rp + c] = v;
	}
	bad = __syncthreads_or(bad);
	if (threadIdx.x == 0) rowbad[row] = bad;
}

// L(i, c) = s[i][c] for c <= i; X(i, c), the inverse under construction, = s[c][i + 1] for c <= i: both triangles in one 64 x 65 tile
__global__ void __launch_bounds__(256) k_ci_diag(double* __restrict__ a, double* __restrict__ w, int rp, int k, const int32_t* __restrict__ rowbad, int32_t* __restrict__ code) {
	__shared__ double s[CI_NB * CI_PD];
	const int tid = threadIdx.x, i = tid & 63, g = tid >> 6;
	double* const at = a + ((int64_t)k * CI_NB) * rp + k * CI_NB;
	double* const wt = w + ((int64_t)k * CI_NB) * rp + k * CI_NB;
	int mine = 0;
	if (k == 0) {  // the call's code starts here: 2 when k_ci_load met a value that is not finite
		int bad = 0;
		for (int q = tid; q < rp; q += 256) bad |= rowbad[q];
		mine = __syncthreads_or(bad) ? 2 : 0;
	} else
		mine = *code;
	for (int c = g; c < CI_NB; c += 4)
		if (c <= i) s[i * CI_PD + c] = at[(int64_t)i * rp + c];
	__syncthreads();  // (row 0's diagonal is s[0][0], X(0, 0) s[0][1]: the two triangles do not meet)
	for (int c = g; c < CI_NB; c += 4)
		if (c <= i) s[c * CI_PD + i + 1] = c == i ? 1.0 : 0.0;
	__syncthreads();
	for (int j = 0; j < CI_NB; j++) {
		double p = s[j * CI_PD + j];
		if (!(p > 0.0 && ci_finite(p))) {
			if (!mine) mine = ci_finite(p) ? 1 : 2;
			p = 1.0;
		}
		const double d = sqrt(p);
		__syncthreads();  // (every thread has read the pivot)
		if (g == 0) {
			if (i > j) s[i * CI_PD + j] /= d;
			if (i == j) s[j * CI_PD + j] = d;
		} else if (g == 1) {
			if (i <= j) s[i * CI_PD + j + 1] /= d;  // X(j, i)
		}
		__syncthreads();
		if (i > j) {
			const double lij = s[i * CI_PD + j];
			for (int c = g; c < CI_NB; c += 4) {
				if (c > j && c <= i) s[i * CI_PD + c] -= lij * s[c * CI_PD + j];
				if (c <= j) s[c * CI_PD + i + 1] -= lij * s[c * CI_PD + j + 1];  // X(i, c) -= L(i, j) X(j, c)
			}
		}
		__syncthreads();
	}
	for (int c = g; c < CI_NB; c += 4) {
		if (c <= i) at[(int64_t)i * rp + c] = s[i * CI_PD + c];
		wt[(int64_t)i * rp + c] = c <= i ? s[c * CI_PD + i + 1] : 0.0;
	}
	if (tid == 0) *code = mine;
}

// acc += the 64 x 64 product  sum_{c < kk} opA(m, c) opB(n, c)  of one workgroup (256 threads = 4 waves, a 32 x 32 quadrant each: 2 x 2 MFMA tiles).
// opA(m, c) = ag[m * lda + c] (AT: ag[c * lda + m]), opB likewise; kk a multiple of CI_KS.  A slab of 32 c is staged through LDS as it lies in memory; the next
// slab is on its way into registers while the matrix cores work on this one.  MFMA operand maps (f64 16x16x4): lane l supplies A[row = l & 15][k = l >> 4] and
// B[k = l >> 4][column = l & 15] and receives D[row = (l >> 4) + 4 q][column = l & 15] in element q.
template <bool AT, bool BT>
__device__ __forceinline__ void ci_tile_mac(d4_t (&acc)[2][2], const double* __restrict__ ag, int64_t lda, const double* __restrict__ bg, int64_t ldb, int kk, double* lds) {
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, lg = lane >> 4;
	const int m0 = (wid >> 1) * 32, n0 = (wid & 1) * 32;
	double* const la = lds;
	double* const lb = lds + CI_SLAB;
	double ra[8], rb[8];
	auto fetch = [&](int c0) {
#pragma unroll
		for (int q = 0; q < 8; q++) {
			const int e = tid + 256 * q;
			ra[q] = AT ? ag[(int64_t)(c0 + (e >> 6)) * lda + (e & 63)] : ag[(int64_t)(e >> 5) * lda + c0 + (e & 31)];
			rb[q] = BT ? bg[(int64_t)(c0 + (e >> 6)) * ldb + (e & 63)] : bg[(int64_t)(e >> 5) * ldb + c0 + (e & 31)];
		}
	};
	fetch(0);
	for (int c0 = 0; c0 < kk; c0 += CI_KS) {
		__syncthreads();  // (the slab before this one has been read)
#pragma unroll
		for (int q = 0; q < 8; q++) {
			const int e = tid + 256 * q;
			la[AT ? (e >> 6) * CI_PT + (e & 63) : (e >> 5) * CI_PN + (e & 31)] = ra[q];
			lb[BT ? (e >> 6) * CI_PT + (e & 63) : (e >> 5) * CI_PN + (e & 31)] = rb[q];
		}
		__syncthreads();
		if (c0 + CI_KS < kk) fetch(c0 + CI_KS);
#pragma unroll
		for (int ks = 0; ks < CI_KS; ks += 4) {
			double fa[2], fb[2];
#pragma unroll
			for (int t = 0; t < 2; t++) {
				fa[t] = AT ? la[(ks + lg) * CI_PT + m0 + 16 * t + l15] : la[(m0 + 16 * t + l15) * CI_PN + ks + lg];
				fb[t] = BT ? lb[(ks + lg) * CI_PT + n0 + 16 * t + l15] : lb[(n0 + 16 * t + l15) * CI_PN + ks + lg];
			}
#pragma unroll
			for (int t = 0; t < 2; t++)
#pragma unroll
				for (int v = 0; v < 2; v++) acc[t][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fb[v], acc[t][v], 0, 0, 0);
		}
	}
}

__device__ __forceinline__ void ci_zero(d4_t (&acc)[2][2]) {
#pragma unroll
	for (int t = 0; t < 2; t++)
#pragma unroll
		for (int v = 0; v < 2; v++) acc[t][v] = (d4_t){0.0, 0.0, 0.0, 0.0};
}

// f(row, column, value) for every element of the workgroup's 64 x 64 accumulator tile that this lane holds
template <typename F>
__device__ __forceinline__ void ci_for_each(const d4_t (&acc)[2][2], F f) {
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
	const int m0 = (wid >> 1) * 32, n0 = (wid & 1) * 32;
#pragma unroll
	for (int t = 0; t < 2; t++)
#pragma unroll
		for (int v = 0; v < 2; v++)
#pragma unroll
			for (int q = 0; q < 4; q++) f(m0 + 16 * t + lg + 4 * q, n0 + 16 * v + l15, acc[t][v][q]);
}

// tile t of a lower triangle counted row by row: (i, j <= i)
__device__ __forceinline__ void ci_tri(int t, int& i, int& j) {
	i = 0;
	while (t > i) t -= i + 1, i++;
	j = t;
}

__global__ void __launch_bounds__(256) k_ci_panel(double* __restrict__ a, const double* __restrict__ w, int rp, int k) {
	__shared__ double lds[2 * CI_SLAB];
	const int i = k + 1 + blockIdx.x;
	double* const aik = a + ((int64_t)i * CI_NB) * rp + k * CI_NB;
	d4_t acc[2][2];
	ci_zero(acc);
	ci_tile_mac<false, false>(acc, aik, rp, w + ((int64_t)k * CI_NB) * rp + k * CI_NB, rp, CI_NB, lds);  // (every read of A_ik is over before the first write below)
	ci_for_each(acc, [&](int m, int n, double v) { aik[(int64_t)m * rp + n] = v; });
}

__global__ void __launch_bounds__(256) k_ci_update(double* __restrict__ a, int rp, int k) {
	__shared__ double lds[2 * CI_SLAB];
	int i, j;
	ci_tri(blockIdx.x, i, j);
	i += k + 1, j += k + 1;
	d4_t acc[2][2];
	ci_zero(acc);
	ci_tile_mac<false, false>(acc, a + ((int64_t)i * CI_NB) * rp + k * CI_NB, rp, a + ((int64_t)j * CI_NB) * rp + k * CI_NB, rp, CI_NB, lds);
	double* const aij = a + ((int64_t)i * CI_NB) * rp + j * CI_NB;
	ci_for_each(acc, [&](int m, int n, double v) { aij[(int64_t)m * rp + n] -= v; });
}

__global__ void __launch_bounds__(256) k_ci_invrow(const double* __restrict__ a, double* __restrict__ w, int rp, int i) {
	__shared__ double lds[2 * CI_SLAB];
	const int j = blockIdx.x;
	d4_t acc[2][2];
	ci_zero(acc);
	ci_tile_mac<false, true>(acc, a + ((int64_t)i * CI_NB) * rp + j * CI_NB, rp, w + ((int64_t)j * CI_NB) * rp + j * CI_NB, rp, (i - j) * CI_NB, lds);
	__syncthreads();  // the sum S as a whole tile [c][n] over the slabs, then W_ij = -W_ii S with W_ii's elements straight from memory
	ci_for_each(acc, [&](int m, int n, double v) { lds[m * CI_PD + n] = v; });
	__syncthreads();
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, lg = lane >> 4;
	const int m0 = (wid >> 1) * 32, n0 = (wid & 1) * 32;
	const double* const wii = w + ((int64_t)i * CI_NB) * rp + i * CI_NB;
	ci_zero(acc);
#pragma unroll 4
	for (int ks = 0; ks < CI_NB; ks += 4) {
		double fa[2], fb[2];
#pragma unroll
		for (int t = 0; t < 2; t++) {
			fa[t] = wii[(int64_t)(m0 + 16 * t + l15) * rp + ks + lg];
			fb[t] = lds[(ks + lg) * CI_PD + n0 + 16 * t + l15];
		}
#pragma unroll
		for (int t = 0; t < 2; t++)
#pragma unroll
			for (int v = 0; v < 2; v++) acc[t][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fb[v], acc[t][v], 0, 0, 0);
	}
	double* const wij = w + ((int64_t)i * CI_NB) * rp + j * CI_NB;
	ci_for_each(acc, [&](int m, int n, double v) { wij[(int64_t)m * rp + n] = -v; });
}

__global__ void __launch_bounds__(256) k_ci_gram(const double* __restrict__ w, int rp, int r, double* __restrict__ inv, int64_t ldi, const int32_t* __restrict__ code,
												  int32_t* __restrict__ status) {
	__shared__ double lds[2 * CI_SLAB];
	int i, j;
	ci_tri(blockIdx.x, j, i);  // i <= j
	const int failed = *code;
	d4_t acc[2][2];
	ci_zero(acc);
	if (!failed) ci_tile_mac<true, true>(acc, w + ((int64_t)j * CI_NB) * rp + i * CI_NB, rp, w + ((int64_t)j * CI_NB) * rp + j * CI_NB, rp, rp - j * CI_NB, lds);
	ci_for_each(acc, [&](int m, int n, double v) {
		const int row = i * CI_NB + m, col = j * CI_NB + n;
		if (row < r && col < r && row <= col) {  // (a diagonal tile: its upper triangle, mirrored)
			inv[(int64_t)row * ldi + col] = v;
			inv[(int64_t)col * ldi + row] = v;
		}
	});
	if (failed && blockIdx.x == 0 && threadIdx.x == 0) status[failed - 1] += 1;
}

static int ci_check(const char* what, const void* m, int64_t ldm, int64_t r, const void* inv, int64_t ldi, const void* status) {
	NRM_REQUIRE(r >= 1 && r <= NRM_WIDE_NC, "%s: 1 to %d rows", what, NRM_WIDE_NC);
	NRM_REQUIRE(ldm >= r && ldi >= r, "%s: pitch too small", what);
	NRM_REQUIRE(m && inv && status && m != inv, "%s: null pointer", what);
	return NRM_OK;
}

extern "C" int64_t nrm_chol_inverse_workspace(int64_t r) {
	if (r < 1 || r > NRM_WIDE_NC) return 0;
	return CiScratch(r, nullptr).doubles;
}

extern "C" int nrm_chol_inverse(const double* d_m, int64_t ldm, int64_t r, double* d_inv, int64_t ldi, double* d_ws, int32_t* d_status, void* stream) {
	NRM_TRY(ci_check("nrm_chol_inverse", d_m, ldm, r, d_inv, ldi, d_status));
	NRM_REQUIRE(d_ws && (uintptr_t)d_ws % 8 == 0, "nrm_chol_inverse: workspace of nrm_chol_inverse_workspace() doubles required");
	const CiScratch s(r, d_ws);
	const int rp = (int)s.rp, nb = (int)s.nb;
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_ci_load, dim3(rp), dim3(256), 0, st, d_m, ldm, (int)r, rp, s.a, s.rowbad);
	NRM_TRY(nrm_check_launch("k_ci_load"));
	for (int k = 0; k < nb; k++) {
		hipLaunchKernelGGL(k_ci_diag, dim3(1), dim3(256), 0, st, s.a, s.w, rp, k, s.rowbad, s.code);
		const int t = nb - 1 - k;
		if (t > 0) {
			hipLaunchKernelGGL(k_ci_panel, dim3(t), dim3(256), 0, st, s.a, s.w, rp, k);
			hipLaunchKernelGGL(k_ci_update, dim3(t * (t + 1) / 2), dim3(256), 0, st, s.a, rp, k);
		}
		NRM_TRY(nrm_check_launch("k_ci_diag / panel / update"));
	}
	for (int i = 1; i < nb; i++) hipLaunchKernelGGL(k_ci_invrow, dim3(i), dim3(256), 0, st, s.a, s.w, rp, i);
	hipLaunchKernelGGL(k_ci_gram, dim3(nb * (nb + 1) / 2), dim3(256), 0, st, s.w, rp, (int)r, d_inv, ldi, s.code, d_status);
	return nrm_check_launch("k_ci_invrow / gram");
}

extern "C" int nrm_chol_inverse_host(const double* m, int64_t ldm, int64_t r, double* inv, int64_t ldi, int32_t* status) {
	NRM_TRY(ci_check("nrm_chol_inverse_host", m, ldm, r, inv, ldi, status));
	const int64_t rp = ci_pad(r), nb = rp / CI_NB, B = CI_NB;
	std::vector<double> av(rp * rp), wv(rp * rp, 0.0), tv(B * B);
	double *a = av.data(), *w = wv.data(), *t = tv.data();
	int code = 0;
	for (int64_t i = 0; i < rp; i++)
		for (int64_t c = 0; c < rp; c++) {
			double v = i == c ? 1.0 : 0.0;
			if (i < r && c < r) {
				v = m[i * ldm + c];
				if (!std::isfinite(v)) code = 2;
			}
			a[i * rp + c] = v;
		}
	for (int64_t k = 0; k < nb; k++) {
		double* akk = a + k * B * rp + k * B;
		double* wkk = w + k * B * rp + k * B;
		for (int64_t i = 0; i < B; i++)
			for (int64_t c = 0; c < B; c++) wkk[i * rp + c] = i == c ? 1.0 : 0.0;
		for (int64_t j = 0; j < B; j++) {  // the diagonal block and its inverse, column by column
			double p = akk[j * rp + j];
			if (!(p > 0.0 && std::isfinite(p))) {
				if (!code) code = std::isfinite(p) ? 1 : 2;
				p = 1.0;
			}
			const double d = std::sqrt(p);
			akk[j * rp + j] = d;
			for (int64_t i = j + 1; i < B; i++) akk[i * rp + j] /= d;
			for (int64_t c = 0; c <= j; c++) wkk[j * rp + c] /= d;
			for (int64_t i = j + 1; i < B; i++) {
				const double lij = akk[i * rp + j];
				for (int64_t c = j + 1; c <= i; c++) akk[i * rp + c] -= lij * akk[c * rp + j];
				for (int64_t c = 0; c <= j; c++) wkk[i * rp + c] -= lij * wkk[j * rp + c];
			}
		}
		for (int64_t i = k + 1; i < nb; i++) {  // the panel: L_ik = A_ik W_kk^T
			double* aik = a + i * B * rp + k * B;
			for (int64_t x = 0; x < B; x++)
				for (int64_t y = 0; y < B; y++) {
					double sum = 0.0;
					for (int64_t c = 0; c < B; c++) sum += aik[x * rp + c] * wkk[y * rp + c];
					t[x * B + y] = sum;
				}
			for (int64_t x = 0; x < B; x++)
				for (int64_t y = 0; y < B; y++) aik[x * rp + y] = t[x * B + y];
		}
		for (int64_t i = k + 1; i < nb; i++)  // the trailing update
			for (int64_t j = k + 1; j <= i; j++) {
				const double *lik = a + i * B * rp + k * B, *ljk = a + j * B * rp + k * B;
				double* aij = a + i * B * rp + j * B;
				for (int64_t x = 0; x < B; x++)
					for (int64_t y = 0; y < B; y++) {
						double sum = 0.0;
						for (int64_t c = 0; c < B; c++) sum += lik[x * rp + c] * ljk[y * rp + c];
						aij[x * rp + y] -= sum;
					}
			}
	}
	for (int64_t i = 1; i < nb; i++)  // W = L^-1, block row by block row
		for (int64_t j = 0; j < i; j++) {
			const double* wii = w + i * B * rp + i * B;
			for (int64_t x = 0; x < B; x++)
				for (int64_t y = 0; y < B; y++) {
					double sum = 0.0;
					for (int64_t c = j * B; c < i * B; c++) sum += a[(i * B + x) * rp + c] * w[c * rp + j * B + y];
					t[x * B + y] = sum;
				}
			for (int64_t x = 0; x < B; x++)
				for (int64_t y = 0; y < B; y++) {
					double sum = 0.0;
					for (int64_t c = 0; c < B; c++) sum += wii[x * rp + c] * t[c * B + y];
					w[(i * B + x) * rp + j * B + y] = -sum;
				}
		}
	for (int64_t x = 0; x < r; x++)  // N = W^T W
		for (int64_t y = x; y < r; y++) {
			double sum = 0.0;
			if (!code)
				for (int64_t c = y / B * B; c < rp; c++) sum += w[c * rp + x] * w[c * rp + y];
			inv[x * ldi + y] = inv[y * ldi + x] = sum;
		}
	if (code) status[code - 1] += 1;
	return NRM_OK;
}
