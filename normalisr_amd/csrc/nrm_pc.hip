// The covariate of the top principal component of chosen genes (reference gocovt.py: pccovt :271-321 with pc1 :4-25; the row degrees of gotop :258).
// The chosen rows are gathered (nrm_subset_dense), residualised against [covariates; 1] by K1 (nrm_residualize: fp64 residual rows and their sums of squares) and
// contracted by K2 (nrm_gram_f64, symmetric).  This file holds what follows:
//   k_net_degree      row sums of the non-zero bytes of a byte matrix (the degrees of a binary network), integers
//   k_pc_correlation  R = D G D / n with D = diag(1 / (sqrt(ss / n) + 1e-200)), both triangles from the upper one
//   k_pc_matvec       w = R v, a wave per row
//   k_pc_finish       ONE workgroup: lambda = v.w, |w - lambda v|, |w|, v <- w / |w|
//   k_pc_sign         ONE workgroup: the sign rule and the loadings u_g = +-v_g a_g
//   k_pc_score        part[split][j] = sum over the split's genes of u_g Zres[g, j]: the one pass over the m x n residual rows
//   k_pc_fold         out[j] = the splits' partial sums added in their order, rounded once to the output type
// All floating-point sums are taken in an order that depends on the shape alone: lanes stride the terms, a shuffle tree folds the lanes, LDS folds the waves in
// their order.  No floating-point atomics: the same bits on every run.  All four passes are bound by memory.
#include "nrm_device.h"

#define PC_SCORE_CELLS 512   // cells per workgroup of k_pc_score: 256 lanes x 2 adjacent cells (one 16-byte load per lane and gene)
#define PC_SCORE_SHARE 16    // the fewest genes a workgroup of k_pc_score takes
#define PC_SCORE_SPLITS 64   // the most splits of the genes
#define PC_SCORE_TARGET 1024 // workgroups wanted before the genes are left unsplit: four per compute unit

typedef double pc_d2 __attribute__((ext_vector_type(2)));
typedef unsigned int pc_u4 __attribute__((ext_vector_type(4)));

// ---- degrees ------------------------------------------------------------------------------------------------------------------------------------------------------
// non-zero bytes of a 32-bit word: bit 7 of every byte of ((w & 0x7f..) + 0x7f..) | w is set exactly where the byte is non-zero (no carry leaves a byte)
__device__ __forceinline__ unsigned int pc_nzb(unsigned int w) { return (unsigned int)__popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u); }

// a wave owns a row: bytes before the row's first 16-byte boundary and after its last one by one, 16-byte words between them, four in flight
__global__ void __launch_bounds__(256) k_net_degree(const uint8_t* __restrict__ net, int64_t ng, int64_t ld, int64_t* __restrict__ deg) {
	const int lane = threadIdx.x & 63;
	const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (g >= ng) return;  // (wave-uniform)
	const uint8_t* row = net + g * ld;
	int64_t head = (int64_t)((16 - ((uintptr_t)row & 15)) & 15);
	if (head > ng) head = ng;
	const int64_t nvec = (ng - head) / 16, tail0 = head + nvec * 16;
	unsigned int cnt = 0;
	if (lane < head) cnt += row[lane] != 0;
	if (tail0 + lane < ng) cnt += row[tail0 + lane] != 0;  // (fewer than 16 bytes)
	const pc_u4* vec = reinterpret_cast<const pc_u4*>(row + head);
	for (int64_t i0 = 0; i0 < nvec; i0 += 256) {
		pc_u4 t[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t i = i0 + u * 64 + lane;
			t[u] = i < nvec ? vec[i] : pc_u4{0u, 0u, 0u, 0u};
		}
#pragma unroll
		for (int u = 0; u < 4; u++) cnt += pc_nzb(t[u][0]) + pc_nzb(t[u][1]) + pc_nzb(t[u][2]) + pc_nzb(t[u][3]);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
	if (lane == 0) deg[g] = (int64_t)cnt;
}

// ---- correlation matrix -------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pc_scale(double ss, double n) { return 1.0 / (sqrt(ss / n) + 1e-200); }

__global__ void __launch_bounds__(256) k_pc_correlation(const double* __restrict__ gm, int64_t ldg, int64_t m, double n, const double* __restrict__ ss,
														 double* __restrict__ r, int64_t ldr, double* __restrict__ a) {
	const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
	if (h >= m) return;
	const int64_t lo = g < h ? g : h, hi = g < h ? h : g;
	const double alo = pc_scale(ss[lo], n), ahi = pc_scale(ss[hi], n);
	r[g * ldr + h] = ((gm[lo * ldg + hi] * alo) * ahi) / n;  // (in this order: G = 0 beside a = 1e200 stays 0)
	if (g == 0) a[h] = pc_scale(ss[h], n);
}

// ---- power iteration ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pc_matvec(const double* __restrict__ r, int64_t ldr, int64_t m, const double* __restrict__ v, double* __restrict__ w) {
	const int lane = threadIdx.x & 63;
	const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (g >= m) return;
	const double* row = r + g * ldr;
	double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
	int64_t h = lane;
	for (; h + 192 < m; h += 256) {  // four loads in flight, four sums of fixed membership
		const double r0 = row[h], r1 = row[h + 64], r2 = row[h + 128], r3 = row[h + 192];
		s0 = fma(r0, v[h], s0);
		s1 = fma(r1, v[h + 64], s1);
		s2 = fma(r2, v[h + 128], s2);
		s3 = fma(r3, v[h + 192], s3);
	}
	for (; h < m; h += 64) s0 = fma(row[h], v[h], s0);
	const double s = nrm_wave_sum((s0 + s1) + (s2 + s3));
	if (lane == 0) w[g] = s;
}

__global__ void __launch_bounds__(256) k_pc_finish(int64_t m, double* __restrict__ v, const double* __restrict__ w, double* __restrict__ stat) {
	__shared__ double sm[4];
	const int tid = threadIdx.x;
	double s = 0;
	for (int64_t g = tid; g < m; g += 256) s = fma(v[g], w[g], s);
	const double lam = nrm_block_sum<4>(s, sm);
	double e = 0, q = 0;
	for (int64_t g = tid; g < m; g += 256) {
		const double d = w[g] - lam * v[g];
		e = fma(d, d, e);
		q = fma(w[g], w[g], q);
	}
	const double res = sqrt(nrm_block_sum<4>(e, sm)), nw = sqrt(nrm_block_sum<4>(q, sm));
	if (nw > 0)
		for (int64_t g = tid; g < m; g += 256) v[g] = w[g] / nw;
	if (tid == 0) {
		stat[0] = lam;
		stat[1] = res;
		stat[2] = nw;
	}
}

// ---- score --------------------------------------------------------------------------------------------------------------------------------------------------------
// u_g = sign v_g a_g with sign = +1 when the entry of v of largest magnitude (the first of equals) is positive, -1 otherwise; out = {its index, sign}
__global__ void __launch_bounds__(256) k_pc_sign(int64_t m, const double* __restrict__ v, const double* __restrict__ a, double* __restrict__ u, int64_t* __restrict__ out) {
	__shared__ double s_val[256];
	__shared__ int64_t s_idx[256];
	const int tid = threadIdx.x;
	double best = -1.0;
	int64_t at = m;
	for (int64_t g = tid; g < m; g += 256) {  // (rising g: the first of equals stays)
		const double t = fabs(v[g]);
		if (t > best) best = t, at = g;
	}
	s_val[tid] = best;
	s_idx[tid] = at;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) {
		if (tid < o && (s_val[tid + o] > s_val[tid] || (s_val[tid + o] == s_val[tid] && s_idx[tid + o] < s_idx[tid]))) {
			s_val[tid] = s_val[tid + o];
			s_idx[tid] = s_idx[tid + o];
		}
		__syncthreads();
	}
	const int64_t top = s_idx[0] < m ? s_idx[0] : 0;
	const double sign = v[top] < 0 ? -1.0 : 1.0;
	for (int64_t g = tid; g < m; g += 256) u[g] = (sign * v[g]) * a[g];
	if (tid == 0) {
		out[0] = top;
		out[1] = sign < 0 ? -1 : 1;
	}
}

// a lane owns two adjacent cells (one 16-byte load per gene), the workgroup the genes [g0, g1) of its split: four genes' loads are issued before the first is used
__global__ void __launch_bounds__(256) k_pc_score(const double* __restrict__ z, int64_t ldz, int64_t m, int64_t n, int64_t share, const double* __restrict__ u,
												   double* __restrict__ part) {
	const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
	if (j >= n) return;  // (ldz is even and >= n: cell j + 1 is inside the row, padding at worst)
	const int64_t g0 = (int64_t)blockIdx.y * share, g1 = g0 + share < m ? g0 + share : m;
	double s0 = 0, s1 = 0;
	int64_t g = g0;
	for (; g + 4 <= g1; g += 4) {
		pc_d2 t[4];
#pragma unroll
		for (int k = 0; k < 4; k++) t[k] = *reinterpret_cast<const pc_d2*>(z + (g + k) * ldz + j);
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const double c = u[g + k];
			s0 = fma(c, t[k][0], s0);
			s1 = fma(c, t[k][1], s1);
		}
	}
	for (; g < g1; g++) {
		const pc_d2 t = *reinterpret_cast<const pc_d2*>(z + g * ldz + j);
		const double c = u[g];
		s0 = fma(c, t[0], s0);
		s1 = fma(c, t[1], s1);
	}
	double* p = part + (int64_t)blockIdx.y * n;
	p[j] = s0;
	if (j + 1 < n) p[j + 1] = s1;
}

template <typename T>
__global__ void __launch_bounds__(256) k_pc_fold(const double* __restrict__ part, int64_t splits, int64_t n, T* __restrict__ out) {
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	double s = part[j];
	for (int64_t k = 1; k < splits; k++) s += part[k * n + j];
	out[j] = (T)s;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int nrm_net_degree(const uint8_t* d_net, int64_t ng, int64_t ld, int64_t* d_deg, void* stream) {
	NRM_REQUIRE(d_net && d_deg && ng > 0 && ld >= ng, "nrm_net_degree: bad shape");
	NRM_REQUIRE(ng <= 0x7fffffffLL && (uintptr_t)d_deg % 8 == 0, "nrm_net_degree: at most 2^31 - 1 genes, aligned output");
	hipLaunchKernelGGL(k_net_degree, dim3((unsigned)((ng + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_net, ng, ld, d_deg);
	return nrm_check_launch("k_net_degree");
}

extern "C" int nrm_pc_correlation(const double* d_g, int64_t ldg, int64_t m, int64_t n, const double* d_ss, double* d_r, int64_t ldr, double* d_a, void* stream) {
	NRM_REQUIRE(d_g && d_ss && d_r && d_a && m > 0 && n > 0 && ldg >= m && ldr >= m, "nrm_pc_correlation: bad shape");
	NRM_REQUIRE(m <= 65535,"nrm_pc_correlation: at most 65535 rows");
	hipLaunchKernelGGL(k_pc_correlation, dim3((unsigned)((m + 255) / 256), (unsigned)m), dim3(256), 0, (hipStream_t)stream, d_g, ldg, m, (double)n, d_ss, d_r, ldr, d_a);
	return nrm_check_launch("k_pc_correlation");
}

extern "C" int nrm_pc_power(const double* d_r, int64_t ldr, int64_t m, double* d_v, double* d_w, double* d_stat, int iters, void* stream) {
	NRM_REQUIRE(d_r && d_v && d_w && d_stat && m > 0 && ldr >= m && iters > 0, "nrm_pc_power: bad arguments");
	NRM_REQUIRE((m + 3) / 4 <= 0x7fffffffLL, "nrm_pc_power: too many rows");
	hipStream_t st = (hipStream_t)stream;
	for (int i = 0; i < iters; i++) {
		hipLaunchKernelGGL(k_pc_matvec, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, d_r, ldr, m, d_v, d_w);
		hipLaunchKernelGGL(k_pc_finish, dim3(1), dim3(256), 0, st, m, d_v, d_w, d_stat);
	}
	return nrm_check_launch("k_pc_power");
}

// the splits of the genes for m genes x n cells, and the genes of a split (a multiple of 4 but for the last)
static void pc_score_plan(int64_t m, int64_t n, int64_t* splits, int64_t* share) {
	const int64_t blocks = (n + PC_SCORE_CELLS - 1) / PC_SCORE_CELLS;
	int64_t s = (PC_SCORE_TARGET + blocks - 1) / blocks;
	const int64_t most = (m + PC_SCORE_SHARE - 1) / PC_SCORE_SHARE;
	if (s > most) s = most;
	if (s > PC_SCORE_SPLITS) s = PC_SCORE_SPLITS;
	if (s < 1) s = 1;
	int64_t sh = ((m + s - 1) / s + 3) / 4 * 4;
	*share = sh;
	*splits = (m + sh - 1) / sh;
}

extern "C" int64_t nrm_pc_score_workspace(int64_t m, int64_t n) {
	if (m <= 0 || n <= 0) return 0;
	int64_t splits, share;
	pc_score_plan(m, n, &splits, &share);
	return m + splits * n;
}

extern "C" int nrm_pc_score(const double* d_z, int64_t ldz, int64_t m, int64_t n, const double* d_v, const double* d_a, void* d_out, int out_dtype, double* d_work,
							int64_t* d_sign, void* stream) {
	NRM_REQUIRE(out_dtype == NRM_F32 || out_dtype == NRM_F64, "nrm_pc_score: the output is NRM_F32 or NRM_F64");
	NRM_REQUIRE(d_z && d_v && d_a && d_out && d_work && d_sign && m > 0 && n > 0, "nrm_pc_score: bad arguments");
	NRM_REQUIRE(ldz % 2 == 0 && ldz >= n + (n & 1) && (uintptr_t)d_z % 16 == 0, "nrm_pc_score: rows of an even pitch that covers the cells, 16-byte aligned");
	NRM_REQUIRE((uintptr_t)d_work % 8 == 0 && (uintptr_t)d_sign % 8 == 0 && (uintptr_t)d_out % (out_dtype == NRM_F64 ? 8 : 4) == 0, "nrm_pc_score: misaligned");
	int64_t splits, share;
	pc_score_plan(m, n, &splits, &share);
	const int64_t blocks = (n + PC_SCORE_CELLS - 1) / PC_SCORE_CELLS;
	NRM_REQUIRE(blocks <= 0x7fffffffLL, "nrm_pc_score: too many cells");
	hipStream_t st = (hipStream_t)stream;
	double* d_u = d_work;
	double* d_part = d_work + m;
	hipLaunchKernelGGL(k_pc_sign, dim3(1), dim3(256), 0, st, m, d_v, d_a, d_u, d_sign);
	NRM_TRY(nrm_check_launch("k_pc_sign"));
	hipLaunchKernelGGL(k_pc_score, dim3((unsigned)blocks, (unsigned)splits), dim3(256), 0, st, d_z, ldz, m, n, share, d_u, d_part);
	NRM_TRY(nrm_check_launch("k_pc_score"));
	const dim3 fg((unsigned)((n + 255) / 256));
	if (out_dtype == NRM_F64)
		hipLaunchKernelGGL((k_pc_fold<double>), fg, dim3(256), 0, st, d_part, splits, n, (double*)d_out);
	else
		hipLaunchKernelGGL((k_pc_fold<float>), fg, dim3(256), 0, st, d_part, splits, n, (float*)d_out);
	return nrm_check_launch("k_pc_fold");
}
