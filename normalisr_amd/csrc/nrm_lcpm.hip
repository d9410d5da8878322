// lcpm and scaling_factor (reference lcpm.py:21-283): Bayesian logCPM from a read-count matrix -- the first stage of the Normalisr pipeline.
// With the reference's default arguments the result is a table lookup:
//     lcpm[g,k] = T[reads[g,k]] - t1[k],   T[x] = psi(1 + x) - psi(sum(reads) + 2),   t1[k] = ln sum_g exp(T[reads[g,k]]) - ln 1e6 ,
// so the matrix (row-major genes x cells) is streamed three times and nothing else is large:
//   k_lc_count   per-cell read total and non-zero count (a slab per row tile) and each workgroup's total, maximum and minimum, folded by k_lc_count_finish;
//                per-gene zero count (integer atomics: exact)
//   (host)       psi(1 + x) for x = 0 .. max and psi(t0): nrm_lcpm_digamma below; T and E = exp(T) are tables of max + 1 doubles
//   k_lc_colsum  per-cell sum_g E[reads[g,k]] -- exp() is taken once per table entry, not per element -- as one partial sum per tile of LC_TR rows,
//   k_lc_finish  the partial sums added in a fixed order (no floating-point atomics: the same bits every run), t1 = ln(sum) - ln 1e6
//   k_lc_write   T[reads[g,k]] - t1[k], stored as fp64 or fp32 (one rounding, at the store).
// A workgroup owns LC_TR rows x 1024 cells; a lane owns four consecutive cells (one 16-byte load of int32 counts, 16-byte stores), the tables sit in LDS
// when they have at most LC_LDS_TAB entries and are read through L2 otherwise.
#include <cmath>

#include "nrm_device.h"

#define LC_TR 32         // rows per workgroup: one partial sum (and one set of per-cell integer atomics) per LC_TR rows
#define LC_LDS_TAB 4096  // table entries staged in LDS (32 KB: five workgroups per CU)
#define LC_TAB_CAP (1 << 24)

extern "C" int64_t nrm_lcpm_row_tile(void) { return LC_TR; }
extern "C" int64_t nrm_lcpm_table_cap(void) { return LC_TAB_CAP; }
// int64 words of scratch of nrm_lcpm_count: a slab of n words per row tile, and three words per workgroup
extern "C" int64_t nrm_lcpm_count_workspace(int64_t rows, int64_t n) {
	const int64_t tiles = (rows + LC_TR - 1) / LC_TR;
	return tiles * n + 3 * tiles * ((n + 1023) / 1024);
}

// ---- digamma on the host ------------------------------------------------------------------------------------------------------------------------
// psi(z) for z >= 12 by the asymptotic series ln z - 1/(2z) - sum_k B_2k / (2k z^2k), k = 1 .. 7: the first term left out is below 2.4e-18; smaller
// arguments are shifted upward, psi(z) = psi(z + m) - sum_{i<m} 1/(z + i).
static double lc_psi_large(double z) {
	const double w = 1.0 / (z * z);
	double s = 1.0 / 12;  // B_14 / 14
	s = -691.0 / 32760 + w * s;
	s = 1.0 / 132 + w * s;
	s = -1.0 / 240 + w * s;
	s = 1.0 / 252 + w * s;
	s = -1.0 / 120 + w * s;
	s = 1.0 / 12 + w * s;
	return std::log(z) - 0.5 / z - w * s;
}

static double lc_psi(double z) {
	double shift = 0.0;
	while (z < 12.0) {
		shift += 1.0 / z;
		z += 1.0;
	}
	return lc_psi_large(z) - shift;
}

// h_psi[x] = psi(1 + x) for x = 0 .. xmax (lcpm.py:101-107 evaluates scipy's digamma at the counts present), *h_psi_t0 = psi(t0) (lcpm.py:96).
// Integer arguments below 12 are -gamma + H_x by recurrence (eleven additions), the others the series directly: no long sum anywhere.
extern "C" int nrm_lcpm_digamma(int64_t xmax, double t0, double* h_psi, double* h_psi_t0) {
	NRM_REQUIRE(xmax >= 0 && xmax < LC_TAB_CAP, "nrm_lcpm_digamma: the table of psi(1 + count) holds counts below %d; the largest count is %lld", LC_TAB_CAP, (long long)xmax);
	NRM_REQUIRE(h_psi && h_psi_t0 && t0 > 0, "nrm_lcpm_digamma: bad arguments");
	double h = -0.57721566490153286061;  // -gamma = psi(1)
	for (int64_t x = 0; x <= xmax; x++) {
		if (x + 1 < 12) {
			h_psi[x] = h;
			h += 1.0 / (double)(x + 1);
		} else
			h_psi[x] = lc_psi_large((double)(x + 1));
	}
	*h_psi_t0 = lc_psi(t0);
	return NRM_OK;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------------
// stats[workgroup] = {total, maximum, minimum}; partial[tile][k] = 64 * (the tile's total of cell k) + its non-zero count
template <typename T, bool ALIGNED>
__global__ void __launch_bounds__(256) k_lc_count(const T* __restrict__ x, int64_t rows, int64_t n, int64_t ld, int64_t* __restrict__ partial,
												  int64_t* __restrict__ stats, unsigned long long* __restrict__ gene_zero) {
	__shared__ unsigned int s_zero[LC_TR];
	__shared__ int64_t s_stat[4][3];
	const int tid = threadIdx.x;
	if (tid < LC_TR) s_zero[tid] = 0;
	__syncthreads();
	const int64_t k = ((int64_t)blockIdx.x * 256 + tid) * 4, row0 = (int64_t)blockIdx.y * LC_TR;
	const int nr = (int)(rows - row0 < LC_TR ? rows - row0 : LC_TR);
	const int nv = (int)(n - k < 0 ? 0 : n - k > 4 ? 4 : n - k);  // cells of this lane inside the matrix
	int64_t tot[4] = {0, 0, 0, 0}, mx = 0, mn = 0;
	int nz[4] = {0, 0, 0, 0};
	for (int r0 = 0; r0 < nr; r0 += 4) {  // four rows per step: their loads are issued before the first is used
		int64_t v[4][4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t row = row0 + r0 + u < rows ? row0 + r0 + u : rows - 1;  // (rows past the end repeat the last and count for nothing)
			nrm_ld4<T, ALIGNED>(x + row * ld, k, n, v[u]);
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const bool live = r0 + u < nr;
			unsigned int zc = 0;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int64_t t = live ? v[u][j] : 0;
				tot[j] += t;
				nz[j] += t != 0;
				mx = t > mx ? t : mx;
				mn = t < mn ? t : mn;
				zc += (unsigned int)__popcll(__ballot(live && j < nv && t == 0));
			}
			if ((tid & 63) == 0 && zc) atomicAdd(&s_zero[r0 + u], zc);
		}
	}
	// the tile's per-cell total and non-zero count (at most LC_TR: six bits) as one word of the tile's slab, summed by k_lc_count_finish (6.3 million per-cell
	// atomics instead were 0.02 of the pass's 0.21 ms at 5000 x 10 000)
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (j < nv) partial[(int64_t)blockIdx.y * n + k + j] = tot[j] * 64 + nz[j];
	// the workgroup's total, maximum and minimum as one record of its own, folded by k_lc_count_finish: 6280 waves each adding to ONE word for the total and
	// one for the maximum serialised in L2 (the pass: 0.184 ms with those atomics, 0.052 ms with the records, at 5000 x 10 000)
	int64_t t = (tot[0] + tot[1]) + (tot[2] + tot[3]);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		t += __shfl_down(t, o, 64);
		const int64_t m2 = __shfl_down(mx, o, 64), m3 = __shfl_down(mn, o, 64);
		mx = m2 > mx ? m2 : mx;
		mn = m3 < mn ? m3 : mn;
	}
	if ((tid & 63) == 0) {
		s_stat[tid >> 6][0] = t;
		s_stat[tid >> 6][1] = mx;
		s_stat[tid >> 6][2] = mn;
	}
	__syncthreads();
	if (tid < nr && s_zero[tid]) atomicAdd(&gene_zero[row0 + tid], (unsigned long long)s_zero[tid]);
	if (tid == 0) {
		int64_t* st = stats + 3 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
		st[0] = (s_stat[0][0] + s_stat[1][0]) + (s_stat[2][0] + s_stat[3][0]);
		int64_t a = s_stat[0][1], b = s_stat[0][2];
		for (int w = 1; w < 4; w++) {
			a = s_stat[w][1] > a ? s_stat[w][1] : a;
			b = s_stat[w][2] < b ? s_stat[w][2] : b;
		}
		st[1] = a;
		st[2] = b;
	}
}

// info: [0] = grand total, [1] = maximum, [2] = 1 for a negative entry (workgroup 0 folds the nb records of k_lc_count, in order)
__global__ void __launch_bounds__(256) k_lc_count_finish(const int64_t* __restrict__ partial, int64_t tiles, int64_t n, const int64_t* __restrict__ stats, int64_t nb,
														 int64_t* __restrict__ cell_total, int64_t* __restrict__ cell_nnz, int64_t* __restrict__ info) {
	__shared__ int64_t sm[2][4][64];
	__shared__ int64_t s_fold[256][3];
	if (blockIdx.x == 0) {
		int64_t t = 0, mx = 0, mn = 0;
		for (int64_t i = threadIdx.x; i < nb; i += 256) {
			t += stats[3 * i];
			mx = stats[3 * i + 1] > mx ? stats[3 * i + 1] : mx;
			mn = stats[3 * i + 2] < mn ? stats[3 * i + 2] : mn;
		}
		s_fold[threadIdx.x][0] = t;
		s_fold[threadIdx.x][1] = mx;
		s_fold[threadIdx.x][2] = mn;
		__syncthreads();
		if (threadIdx.x == 0) {
			for (int i = 1; i < 256; i++) {
				t += s_fold[i][0];
				mx = s_fold[i][1] > mx ? s_fold[i][1] : mx;
				mn = s_fold[i][2] < mn ? s_fold[i][2] : mn;
			}
			info[0] = t;
			info[1] = mx;
			info[2] = mn < 0;
		}
	}
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int64_t k = (int64_t)blockIdx.x * 64 + lane;
	int64_t tot = 0, nz = 0;
	if (k < n)
		for (int64_t t = wid; t < tiles; t += 4) {
			const int64_t w = partial[t * n + k];
			tot += w >> 6;
			nz += w & 63;
		}
	sm[0][wid][lane] = tot;
	sm[1][wid][lane] = nz;
	__syncthreads();
	if (wid == 0 && k < n) {
		cell_total[k] = sm[0][0][lane] + sm[0][1][lane] + sm[0][2][lane] + sm[0][3][lane];
		cell_nnz[k] = sm[1][0][lane] + sm[1][1][lane] + sm[1][2][lane] + sm[1][3][lane];
	}
}

template <bool LDS>
__device__ __forceinline__ const double* lc_stage(const double* __restrict__ g_tab, int64_t tlen, double* s_tab, int tid) {
	if constexpr (LDS) {
		for (int i = tid; i < (int)tlen; i += 256) s_tab[i] = g_tab[i];
		__syncthreads();
		return s_tab;
	} else
		return g_tab;
}

// partial[tile][k] = sum over the tile's rows of E[x[g,k]], rows added in order
template <typename T, bool ALIGNED, bool LDS>
__global__ void __launch_bounds__(256) k_lc_colsum(const T* __restrict__ x, int64_t rows, int64_t n, int64_t ld, const double* __restrict__ g_tab, int64_t tlen,
													double* __restrict__ partial) {
	extern __shared__ double s_dyn[];
	const int tid = threadIdx.x;
	const double* tab = lc_stage<LDS>(g_tab, tlen, s_dyn, tid);
	const int64_t k = ((int64_t)blockIdx.x * 256 + tid) * 4, row0 = (int64_t)blockIdx.y * LC_TR;
	const int nr = (int)(rows - row0 < LC_TR ? rows - row0 : LC_TR);
	double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
	for (int r = 0; r < nr; r++) {
		int64_t v[4];
		nrm_ld4<T, ALIGNED>(x + (row0 + r) * ld, k, n, v);
#pragma unroll
		for (int j = 0; j < 4; j++) acc[j] += tab[nrm_table_index(v[j], tlen)];
	}
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (k + j < n) partial[(int64_t)blockIdx.y * n + k + j] = acc[j];
}

// sum[k] = the partial sums of cell k added in a fixed order: a wave owns 64 consecutive cells, the workgroup's four waves every fourth tile each
__device__ __forceinline__ double lc_tile_sum(const double* __restrict__ partial, int64_t tiles, int64_t n, double (*sm)[64]) {
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int64_t k = (int64_t)blockIdx.x * 64 + lane;
	double s = 0.0;
	if (k < n)
		for (int64_t t = wid; t < tiles; t += 4) s += partial[t * n + k];
	sm[wid][lane] = s;
	__syncthreads();
	return ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}

__global__ void __launch_bounds__(256) k_lc_finish(const double* __restrict__ partial, int64_t tiles, int64_t n, double* __restrict__ t1) {
	__shared__ double sm[4][64];
	const double s = lc_tile_sum(partial, tiles, n, sm);
	const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
	if (threadIdx.x < 64 && k < n) t1[k] = log(s) - 13.815510557964274;  // ln 1e6 (lcpm.py:158)
}

template <typename T, typename OutT, bool ALIGNED, bool LDS>
__global__ void __launch_bounds__(256) k_lc_write(const T* __restrict__ x, int64_t rows, int64_t n, int64_t ld, const double* __restrict__ g_tab, int64_t tlen,
												   const double* __restrict__ t1, OutT* __restrict__ out, int64_t ldo) {
	extern __shared__ double s_dyn[];
	const int tid = threadIdx.x;
	const double* tab = lc_stage<LDS>(g_tab, tlen, s_dyn, tid);
	const int64_t k = ((int64_t)blockIdx.x * 256 + tid) * 4, row0 = (int64_t)blockIdx.y * LC_TR;
	const int nr = (int)(rows - row0 < LC_TR ? rows - row0 : LC_TR);
	double sub[4];
#pragma unroll
	for (int j = 0; j < 4; j++) sub[j] = t1 && k + j < n ? t1[k + j] : 0.0;
#pragma unroll 4
	for (int r = 0; r < nr; r++) {
		int64_t v[4];
		nrm_ld4<T, ALIGNED>(x + (row0 + r) * ld, k, n, v);
		OutT o[4];
#pragma unroll
		for (int j = 0; j < 4; j++) o[j] = (OutT)(tab[nrm_table_index(v[j], tlen)] - sub[j]);
		OutT* dst = out + (row0 + r) * ldo + k;
		if (ALIGNED && k + 4 <= n) {
			typedef OutT ov_t __attribute__((ext_vector_type(16 / sizeof(OutT))));
#pragma unroll
			for (int h = 0; h < 4; h += 16 / (int)sizeof(OutT)) {
				ov_t t;
#pragma unroll
				for (int j = 0; j < 16 / (int)sizeof(OutT); j++) t[j] = o[h + j];
				*reinterpret_cast<ov_t*>(dst + h) = t;
			}
		} else {
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (k + j < n) dst[j] = o[j];
		}
	}
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
static int lc_check(const char* what, const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld) {
	NRM_REQUIRE(nrm_count_elem(dtype) != 0, "%s: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8", what);
	NRM_REQUIRE(d_x && rows > 0 && n > 0 && ld >= n, "%s: bad shape", what);
	NRM_REQUIRE((rows + LC_TR - 1) / LC_TR <= 65535, "%s: at most %d rows", what, 65535 * LC_TR);
	return NRM_OK;
}

static bool lc_aligned(const void* d_x, int dtype, int64_t ld) { return (uintptr_t)d_x % (4 * nrm_count_elem(dtype)) == 0 && ld % 4 == 0; }

static dim3 lc_grid(int64_t rows, int64_t n) { return dim3((unsigned)((n + 1023) / 1024), (unsigned)((rows + LC_TR - 1) / LC_TR)); }

extern "C" int nrm_lcpm_count(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_gene_zero,
							  int64_t* d_info, int64_t* d_partial, void* stream) {
	NRM_TRY(lc_check("nrm_lcpm_count", d_x, dtype, rows, n, ld));
	NRM_REQUIRE(d_cell_total && d_cell_nnz && d_gene_zero && d_info && d_partial, "nrm_lcpm_count: null pointer");
	const bool al = lc_aligned(d_x, dtype, ld);
	const int64_t tiles = (rows + LC_TR - 1) / LC_TR, nb = tiles * ((n + 1023) / 1024);
	typedef unsigned long long u64;
#define LC_GO2(TY, AL) hipLaunchKernelGGL((k_lc_count<TY, AL>), lc_grid(rows, n), dim3(256), 0, (hipStream_t)stream, (const TY*)d_x, rows, n, ld, d_partial, d_partial + tiles * n, (u64*)d_gene_zero)
#define LC_GO(TY)                \
	do {                         \
		if (al) LC_GO2(TY, true); \
		else LC_GO2(TY, false);  \
	} while (0)
	NRM_BY_COUNT_DTYPE(LC_GO)
#undef LC_GO
#undef LC_GO2
	NRM_TRY(nrm_check_launch("k_lc_count"));
	hipLaunchKernelGGL(k_lc_count_finish, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, (hipStream_t)stream, d_partial, tiles, n, d_partial + tiles * n, nb, d_cell_total, d_cell_nnz, d_info);
	return nrm_check_launch("k_lc_count_finish");
}

extern "C" int nrm_lcpm_colsum(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, const double* d_exp_table, int64_t table_len, double* d_partial,
							   double* d_t1, void* stream) {
	NRM_TRY(lc_check("nrm_lcpm_colsum", d_x, dtype, rows, n, ld));
	NRM_REQUIRE(d_exp_table && table_len > 0 && table_len <= LC_TAB_CAP && d_partial && d_t1, "nrm_lcpm_colsum: bad arguments");
	const bool al = lc_aligned(d_x, dtype, ld), lds = table_len <= LC_LDS_TAB;
	const size_t sh = lds ? (size_t)table_len * 8 : 0;
	hipStream_t st = (hipStream_t)stream;
#define LC_GO3(TY, AL, LD) hipLaunchKernelGGL((k_lc_colsum<TY, AL, LD>), lc_grid(rows, n), dim3(256), sh, st, (const TY*)d_x, rows, n, ld, d_exp_table, table_len, d_partial)
#define LC_GO(TY)                          \
	do {                                   \
		if (al && lds) LC_GO3(TY, true, true);       \
		else if (al) LC_GO3(TY, true, false);        \
		else if (lds) LC_GO3(TY, false, true);       \
		else LC_GO3(TY, false, false);               \
	} while (0)
	NRM_BY_COUNT_DTYPE(LC_GO)
#undef LC_GO
#undef LC_GO3
	NRM_TRY(nrm_check_launch("k_lc_colsum"));
	hipLaunchKernelGGL(k_lc_finish, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, d_partial, (rows + LC_TR - 1) / LC_TR, n, d_t1);
	return nrm_check_launch("k_lc_finish");
}

template <typename T>
static void lc_launch_write(const void* d_x, int64_t rows, int64_t n, int64_t ld, const double* d_table, int64_t table_len, const double* d_t1, void* d_out, int out_dtype,
							int64_t ldo, bool al, hipStream_t st) {
	const bool lds = table_len <= LC_LDS_TAB;
	const size_t sh = lds ? (size_t)table_len * 8 : 0;
#define LC_GO4(TO, AL, LD) hipLaunchKernelGGL((k_lc_write<T, TO, AL, LD>), lc_grid(rows, n), dim3(256), sh, st, (const T*)d_x, rows, n, ld, d_table, table_len, d_t1, (TO*)d_out, ldo)
#define LC_GO(TO)                          \
	do {                                   \
		if (al && lds) LC_GO4(TO, true, true);       \
		else if (al) LC_GO4(TO, true, false);        \
		else if (lds) LC_GO4(TO, false, true);       \
		else LC_GO4(TO, false, false);               \
	} while (0)
	if (out_dtype == NRM_F64) LC_GO(double);
	else LC_GO(float);
#undef LC_GO
#undef LC_GO4
}

extern "C" int nrm_lcpm_write(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, const double* d_table, int64_t table_len, const double* d_t1, void* d_out,
							  int out_dtype, int64_t ldo, void* stream) {
	NRM_TRY(lc_check("nrm_lcpm_write", d_x, dtype, rows, n, ld));
	NRM_REQUIRE(out_dtype == NRM_F32 || out_dtype == NRM_F64, "nrm_lcpm_write: bad dtype");
	NRM_REQUIRE(d_table && table_len > 0 && table_len <= LC_TAB_CAP && d_out && ldo >= n, "nrm_lcpm_write: bad arguments");
	const bool al = lc_aligned(d_x, dtype, ld) && (uintptr_t)d_out % 16 == 0 && (ldo * (out_dtype == NRM_F64 ? 8 : 4)) % 16 == 0 &&
					(d_t1 == nullptr || (uintptr_t)d_t1 % 8 == 0);
#define LC_GO(TY) lc_launch_write<TY>(d_x, rows, n, ld, d_table, table_len, d_t1, d_out, out_dtype, ldo, al, (hipStream_t)stream)
	NRM_BY_COUNT_DTYPE(LC_GO)
#undef LC_GO
	return nrm_check_launch("k_lc_write");
}
