// lcpm and scaling_factor from a SPARSE count matrix (reference lcpm.py:118-137 is its sparse branch): the three passes of nrm_lcpm.hip over canonical CSR
// (genes are rows; indptr int64, indices int32 strictly increasing inside a row, data any of the count dtypes), without the dense counts anywhere.
//     lcpm[g,k] = T[x_gk] - t1[k],   t1[k] = ln( rows * E[0] + sum over the stored entries of cell k of (E[x] - E[0]) ) - ln 1e6 ,   E = exp(T):
// a zero costs nothing in the first two passes, and in the third only the store of T[0] - t1[k].
//   k_lcs_count   a workgroup owns LCS_TR rows.  Flat part: every stored entry once for the structure check, the per-gene count of non-zeros, the tile's total,
//                 maximum and minimum.  Walk: the cells in chunks of LCS_CW, per-cell total and non-zero count of the tile in LDS (integer LDS atomics), one
//                 slab word per (tile, cell); the rows are sorted, so a row's entries of a chunk start where the last chunk's ended: no search.
//   k_lcs_colsum  the same walk with the terms E[x] - E[0] >= 0 as 64-bit FIXED-POINT integers: cell k's terms sum to at most total_k * unit (unit = the
//                 largest (E[x] - E[0]) / x of the table), so they are scaled by the power of two that puts that bound below 2^62 and rounded once each.
//                 Integer sums do not depend on their order: LDS atomics inside a tile, a fixed-order sum over the tiles, the same bits every run, and a
//                 relative error of the per-cell sum below (stored entries of the cell) * 2^-62.  No floating-point atomics.
//   k_lcs_write   a workgroup walks a row in chunks of LCS_CW cells: the chunk's stored counts are scattered into a zeroed LDS image (two images in turn: one
//                 barrier per step), then every lane reads four cells, looks up T only where the count is not zero, and stores 16 bytes: each output
//                 element is stored once.
// Nothing here trusts the structure: indptr is clamped to [0, nnz], a column outside the chunk is skipped, a count outside the table reads its end.
// The two launch arguments that depend on the data -- the number of stored entries and `unit` -- come in two forms.  The entries of the C ABI pass them by value.
// A resident plan (nrm_front_plan.hip), whose captured graph must survive a rewrite of the matrix, pattern included, passes dev = 1 and d_unit: nnz is then the
// CAPACITY of indices and data, the stored entries are indptr[rows] clamped to [0, nnz] (lcs_entries), unit is *d_unit, and no launch argument depends on the
// data.  Whatever the buffers hold, no thread reads outside the rows + 1 offsets and the nnz entries.
#include <cmath>

#include "nrm_device.h"

#define LCS_TR 32       // rows per workgroup of the count and sum passes (a wave owns every eighth)
#define LCS_CW 4096     // cells per chunk: 32 KB of 64-bit accumulators, or two 16 KB images of the write pass
#define LCS_TAB_CAP (1 << 24)

typedef unsigned long long lcs_u64;

// int64 words of scratch of nrm_lcpm_csr_count and nrm_lcpm_csr_colsum: one slab of n words per row tile, four words per tile
extern "C" int64_t nrm_lcpm_csr_workspace(int64_t rows, int64_t n) {
	const int64_t tiles = (rows + LCS_TR - 1) / LCS_TR;
	return tiles * n + 4 * tiles;
}

// binary exponent of cell k's fixed point: total * unit bounds the sum of its terms; 2^shift times that bound is below 2^62
__device__ __forceinline__ int lcs_shift(int64_t total, double unit) {
	const double b = (double)total * unit;
	if (!(total > 0) || !(b > 0.0) || !isfinite(b)) return 0;
	const int e = 61 - ilogb(b);
	return e < -60 ? -60 : e > 900 ? 900 : e;
}

// the stored entries: the argument, or (dev) indptr[rows] clamped to the capacity -- an indptr[rows] outside [0, capacity] then differs from it, which lcs_rows reports
__device__ __forceinline__ int64_t lcs_entries(const int64_t* __restrict__ indptr, int64_t rows, int64_t nnz, int dev) { return dev ? nrm_clamp(indptr[rows], 0, nnz) : nnz; }

// The rows' bounds of a tile into LDS, clamped; returns 1 for an indptr that is not 0 = p[0] <= p[1] <= ... <= p[rows] = nnz (threads below LCS_TR)
__device__ __forceinline__ int lcs_rows(const int64_t* __restrict__ indptr, int64_t rows, int64_t nnz, int64_t row0, int nr, int64_t* s_cur, int64_t* s_end) {
	int bad = 0;
	const int tid = threadIdx.x;
	if (tid < LCS_TR) {
		int64_t s = 0, e = 0;
		if (tid < nr) {
			const int64_t row = row0 + tid, a = indptr[row], b = indptr[row + 1];
			bad = a < 0 || b < a || b > nnz || (row == 0 && a != 0) || (row == rows - 1 && b != nnz);
			s = nrm_clamp(a, 0, nnz);
			e = nrm_clamp(b, s, nnz);
		}
		s_cur[tid] = s;
		s_end[tid] = e;
	}
	return bad;
}

// ---- pass 1: integer totals and the structure check ------------------------------------------------------------------------------------------------------------
// slab[tile][k] = 256 * (the tile's total of cell k) + its count of non-zeros (at most LCS_TR); rec[tile] = {total, maximum, minimum, malformed}
template <typename T>
__global__ void __launch_bounds__(512) k_lcs_count(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t rows, int64_t n,
												   int64_t nnz_arg, int dev, int64_t* __restrict__ slab, int64_t* __restrict__ rec, int64_t* __restrict__ gene_zero) {
	__shared__ lcs_u64 s_acc[LCS_CW];
	__shared__ int64_t s_cur[LCS_TR], s_end[LCS_TR];
	__shared__ int64_t s_stat[8][4];
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t nnz = lcs_entries(indptr, rows, nnz_arg, dev);
	const int64_t row0 = (int64_t)blockIdx.x * LCS_TR;
	const int nr = (int)(rows - row0 < LCS_TR ? rows - row0 : LCS_TR);
	int bad = lcs_rows(indptr, rows, nnz, row0, nr, s_cur, s_end);
	for (int i = tid; i < LCS_CW; i += 512) s_acc[i] = 0;
	__syncthreads();
	// flat part: what needs no cell range
	int64_t tot = 0, mx = 0, mn = 0;
	for (int r = wid; r < nr; r += 8) {
		const int64_t s = s_cur[r], e = s_end[r];
		int64_t nz = 0;
		for (int64_t p0 = s; p0 < e; p0 += 64) {
			const int64_t p = p0 + lane;
			const bool ok = p < e;
			const int64_t col = ok ? (int64_t)idx[p] : 0, prev = ok && p > s ? (int64_t)idx[p - 1] : -1, x = ok ? (int64_t)val[p] : 0;
			bad |= ok && (col < 0 || col >= n || prev >= col);
			tot += x;
			mx = x > mx ? x : mx;
			mn = x < mn ? x : mn;
			nz += __popcll(__ballot(x != 0));
		}
		if (lane == 0) gene_zero[row0 + r] = n - nz;
	}
	// walk: per-cell totals and non-zero counts
	for (int64_t c0 = 0; c0 < n; c0 += LCS_CW) {
		const int64_t cend = c0 + LCS_CW < n ? c0 + LCS_CW : n;
		for (int r = wid; r < nr; r += 8) {
			const int64_t cur = nrm_csr_walk<T>(idx, val, s_cur[r], s_end[r], c0, cend, [&](int c, int64_t x) {
				if (x > 0) atomicAdd(&s_acc[c], ((lcs_u64)x << 8) | 1ull);
			});
			if (lane == 0) s_cur[r] = cur;
		}
		__syncthreads();
		for (int i = tid; i < (int)(cend - c0); i += 512) {
			slab[(int64_t)blockIdx.x * n + c0 + i] = (int64_t)s_acc[i];
			s_acc[i] = 0;
		}
		__syncthreads();
	}
	int64_t b = bad;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		tot += __shfl_down(tot, o, 64);
		const int64_t m2 = __shfl_down(mx, o, 64), m3 = __shfl_down(mn, o, 64);
		mx = m2 > mx ? m2 : mx;
		mn = m3 < mn ? m3 : mn;
		b |= __shfl_down(b, o, 64);
	}
	if (lane == 0) {
		s_stat[wid][0] = tot;
		s_stat[wid][1] = mx;
		s_stat[wid][2] = mn;
		s_stat[wid][3] = b;
	}
	__syncthreads();
	if (tid == 0) {
		for (int w = 1; w < 8; w++) {
			tot += s_stat[w][0];
			mx = s_stat[w][1] > mx ? s_stat[w][1] : mx;
			mn = s_stat[w][2] < mn ? s_stat[w][2] : mn;
			b |= s_stat[w][3];
		}
		int64_t* st = rec + 4 * (int64_t)blockIdx.x;
		st[0] = tot;
		st[1] = mx;
		st[2] = mn;
		st[3] = b;
	}
}

// info: [0] = grand total, [1] = maximum, [2] = 1 for a negative entry, [3] = 1 for a malformed matrix (workgroup 0 folds the tiles' records, in order)
__global__ void __launch_bounds__(256) k_lcs_count_finish(const int64_t* __restrict__ slab, int64_t tiles, int64_t n, const int64_t* __restrict__ rec,
														  int64_t* __restrict__ cell_total, int64_t* __restrict__ cell_nnz, int64_t* __restrict__ info) {
	__shared__ int64_t sm[2][4][64];
	__shared__ int64_t s_fold[256][4];
	if (blockIdx.x == 0) {
		int64_t t = 0, mx = 0, mn = 0, b = 0;
		for (int64_t i = threadIdx.x; i < tiles; i += 256) {
			t += rec[4 * i];
			mx = rec[4 * i + 1] > mx ? rec[4 * i + 1] : mx;
			mn = rec[4 * i + 2] < mn ? rec[4 * i + 2] : mn;
			b |= rec[4 * i + 3];
		}
		s_fold[threadIdx.x][0] = t;
		s_fold[threadIdx.x][1] = mx;
		s_fold[threadIdx.x][2] = mn;
		s_fold[threadIdx.x][3] = b;
		__syncthreads();
		if (threadIdx.x == 0) {
			for (int i = 1; i < 256; i++) {
				t += s_fold[i][0];
				mx = s_fold[i][1] > mx ? s_fold[i][1] : mx;
				mn = s_fold[i][2] < mn ? s_fold[i][2] : mn;
				b |= s_fold[i][3];
			}
			info[0] = t;
			info[1] = mx;
			info[2] = mn < 0;
			info[3] = b != 0;
		}
	}
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int64_t k = (int64_t)blockIdx.x * 64 + lane;
	int64_t tot = 0, nz = 0;
	if (k < n)
		for (int64_t t = wid; t < tiles; t += 4) {
			const int64_t w = slab[t * n + k];
			tot += w >> 8;
			nz += w & 255;
		}
	sm[0][wid][lane] = tot;
	sm[1][wid][lane] = nz;
	__syncthreads();
	if (wid == 0 && k < n) {
		cell_total[k] = sm[0][0][lane] + sm[0][1][lane] + sm[0][2][lane] + sm[0][3][lane];
		cell_nnz[k] = sm[1][0][lane] + sm[1][1][lane] + sm[1][2][lane] + sm[1][3][lane];
	}
}

// ---- pass 2: per-cell sums of E[x] - E[0] in fixed point ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(512) k_lcs_colsum(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t rows, int64_t n,
													int64_t nnz_arg, int dev, const double* __restrict__ tab, int64_t tlen, double unit_arg, const double* __restrict__ d_unit,
													const int64_t* __restrict__ cell_total, int64_t* __restrict__ slab) {
	__shared__ lcs_u64 s_acc[LCS_CW];
	__shared__ short s_shift[LCS_CW];
	__shared__ int64_t s_cur[LCS_TR], s_end[LCS_TR];
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t nnz = lcs_entries(indptr, rows, nnz_arg, dev);
	const double unit = d_unit ? *d_unit : unit_arg;
	const int64_t row0 = (int64_t)blockIdx.x * LCS_TR;
	const int nr = (int)(rows - row0 < LCS_TR ? rows - row0 : LCS_TR);
	(void)lcs_rows(indptr, rows, nnz, row0, nr, s_cur, s_end);
	const double e0 = tab[0];
	for (int64_t c0 = 0; c0 < n; c0 += LCS_CW) {
		const int64_t cend = c0 + LCS_CW < n ? c0 + LCS_CW : n;
		for (int i = tid; i < (int)(cend - c0); i += 512) {
			s_acc[i] = 0;
			s_shift[i] = (short)lcs_shift(cell_total[c0 + i], unit);
		}
		__syncthreads();
		for (int r = wid; r < nr; r += 8) {
			const int64_t cur = nrm_csr_walk<T>(idx, val, s_cur[r], s_end[r], c0, cend, [&](int c, int64_t x) {
				const int64_t xi = nrm_table_index(x, tlen);
				if (xi > 0) {
					const double term = tab[xi] - e0;  // >= 0: psi is increasing
					atomicAdd(&s_acc[c], (lcs_u64)__double2ll_rn(ldexp(term > 0.0 ? term : 0.0, (int)s_shift[c])));
				}
			});
			if (lane == 0) s_cur[r] = cur;
		}
		__syncthreads();
		for (int i = tid; i < (int)(cend - c0); i += 512) slab[(int64_t)blockIdx.x * n + c0 + i] = (int64_t)s_acc[i];
		__syncthreads();
	}
}

// t1[k] = ln(rows * E[0] + 2^-shift_k * (the tiles' integers of cell k, added in a fixed order)) - ln 1e6
__global__ void __launch_bounds__(256) k_lcs_finish(const int64_t* __restrict__ slab, int64_t tiles, int64_t n, int64_t rows, const double* __restrict__ tab, double unit_arg,
													const double* __restrict__ d_unit, const int64_t* __restrict__ cell_total, double* __restrict__ t1) {
	__shared__ lcs_u64 sm[4][64];
	const double unit = d_unit ? *d_unit : unit_arg;
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int64_t k = (int64_t)blockIdx.x * 64 + lane;
	lcs_u64 s = 0;
	if (k < n)
		for (int64_t t = wid; t < tiles; t += 4) s += (lcs_u64)slab[t * n + k];
	sm[wid][lane] = s;
	__syncthreads();
	if (wid == 0 && k < n) {
		const lcs_u64 a = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
		const double sum = (double)rows * tab[0] + ldexp((double)a, -lcs_shift(cell_total[k], unit));
		t1[k] = log(sum) - 13.815510557964274;  // ln 1e6 (lcpm.py:158)
	}
}

// ---- pass 3: the dense result ------------------------------------------------------------------------------------------------------------------------------------
// A lane owns cells c0 + 1024 j + 4 lane .. + 3, j = 0 .. 3, of a chunk.  ALIGNED (the launcher: out, ldo and t1 on 16-byte boundaries): 16-byte stores.
template <typename T, typename OutT, bool ALIGNED>
__global__ void __launch_bounds__(256) k_lcs_write(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t rows, int64_t n,
												   int64_t nnz_arg, int dev, const double* __restrict__ tab, int64_t tlen, const double* __restrict__ t1, OutT* __restrict__ out,
												   int64_t ldo) {
	__shared__ __attribute__((aligned(16))) int s_img[2][LCS_CW];
	typedef int iv_t __attribute__((ext_vector_type(4)));
	typedef double dv_t __attribute__((ext_vector_type(2)));
	const int tid = threadIdx.x;
	const int64_t nnz = lcs_entries(indptr, rows, nnz_arg, dev);
	for (int i = tid; i < 2 * LCS_CW; i += 256) (&s_img[0][0])[i] = 0;
	__syncthreads();
	const double t0 = tab[0];
	int b = 0;
	for (int64_t g = blockIdx.x; g < rows; g += gridDim.x) {
		const int64_t s = nrm_clamp(indptr[g], 0, nnz), e = nrm_clamp(indptr[g + 1], s, nnz);
		int64_t cur = s;
		OutT* orow = out + g * ldo;
		for (int64_t c0 = 0; c0 < n; c0 += LCS_CW, b ^= 1) {
			const int64_t cend = c0 + LCS_CW < n ? c0 + LCS_CW : n;
			double sub[4][4];  // t1 of this lane's cells: asked for before the scatter, used after it
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int64_t k = c0 + j * 1024 + tid * 4;
				if (ALIGNED && t1 && k + 4 <= n) {
					const dv_t a = *reinterpret_cast<const dv_t*>(t1 + k), c = *reinterpret_cast<const dv_t*>(t1 + k + 2);
					sub[j][0] = a[0], sub[j][1] = a[1], sub[j][2] = c[0], sub[j][3] = c[1];
				} else {
#pragma unroll
					for (int i = 0; i < 4; i++) sub[j][i] = t1 && k + i < n ? t1[k + i] : 0.0;
				}
			}
			// scatter: the row's entries from cur on whose column is below cend, 512 per step
			for (;;) {
				int64_t col[2], x[2];
				bool in[2];
#pragma unroll
				for (int u = 0; u < 2; u++) {
					const int64_t p = cur + u * 256 + tid;
					const bool ok = p < e;
					col[u] = ok ? (int64_t)idx[p] : cend;
					x[u] = ok ? (int64_t)val[p] : 0;
					in[u] = ok && col[u] < cend;
				}
				if (in[0] && col[0] >= c0) s_img[b][col[0] - c0] = (int)nrm_table_index(x[0], tlen);
				if (in[1] && col[1] >= c0) s_img[b][col[1] - c0] = (int)nrm_table_index(x[1], tlen);
				const int cnt = __syncthreads_count(in[0]) + __syncthreads_count(in[1]);  // (the barrier between scatter and read as well)
				cur += cnt;
				if (cnt < 512) break;
			}
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int64_t k = c0 + j * 1024 + tid * 4;
				if (k >= cend) continue;
				iv_t* cell = reinterpret_cast<iv_t*>(&s_img[b][j * 1024 + tid * 4]);
				const iv_t xi = *cell;
				*cell = iv_t{0, 0, 0, 0};  // left zeroed for the chunk after the next
				OutT o[4];
#pragma unroll
				for (int i = 0; i < 4; i++) o[i] = (OutT)((xi[i] ? tab[xi[i]] : t0) - sub[j][i]);
				if (ALIGNED && k + 4 <= n) {
					typedef OutT ov_t __attribute__((ext_vector_type(16 / sizeof(OutT))));
#pragma unroll
					for (int h = 0; h < 4; h += 16 / (int)sizeof(OutT)) {
						ov_t t;
#pragma unroll
						for (int i = 0; i < 16 / (int)sizeof(OutT); i++) t[i] = o[h + i];
						*reinterpret_cast<ov_t*>(orow + k + h) = t;
					}
				} else {
#pragma unroll
					for (int i = 0; i < 4; i++)
						if (k + i < n) orow[k + i] = o[i];
				}
			}
		}
	}
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------------------------
// nrm_lcpm_csr_passes_* (nrm_lcpm_step.h) launch both forms; the entries of the C ABI below are their by-value form (dev = 0, d_unit = NULL).
static int lcs_check(const char* what, const void* d_indptr, const void* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz) {
	NRM_REQUIRE(nrm_count_elem(dtype) != 0, "%s: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8", what);
	return nrm_csr_args_check(what, d_indptr, d_indices, d_data, nrm_count_elem(dtype), rows, n, nnz);
}

int nrm_lcpm_csr_passes_count(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int dev,
							  int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_gene_zero, int64_t* d_info, int64_t* d_partial, void* stream) {
	NRM_TRY(lcs_check("nrm_lcpm_csr_count", d_indptr, d_indices, d_data, dtype, rows, n, nnz));
	NRM_REQUIRE(d_cell_total && d_cell_nnz && d_gene_zero && d_info && d_partial, "nrm_lcpm_csr_count: null pointer");
	const int64_t tiles = (rows + LCS_TR - 1) / LCS_TR;
	NRM_REQUIRE(tiles <= 0x7fffffffLL, "nrm_lcpm_csr_count: too many rows");
	hipStream_t st = (hipStream_t)stream;
#define LCS_GO(TY) \
	hipLaunchKernelGGL((k_lcs_count<TY>), dim3((unsigned)tiles), dim3(512), 0, st, d_indptr, d_indices, (const TY*)d_data, rows, n, nnz, dev, d_partial, d_partial + tiles * n, d_gene_zero)
	NRM_BY_COUNT_DTYPE(LCS_GO)
#undef LCS_GO
	NRM_TRY(nrm_check_launch("k_lcs_count"));
	hipLaunchKernelGGL(k_lcs_count_finish, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, d_partial, tiles, n, d_partial + tiles * n, d_cell_total, d_cell_nnz, d_info);
	return nrm_check_launch("k_lcs_count_finish");
}

int nrm_lcpm_csr_passes_colsum(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int dev,
							   const double* d_exp_table, int64_t table_len, double unit, const double* d_unit, const int64_t* d_cell_total, int64_t* d_partial, double* d_t1,
							   void* stream) {
	NRM_TRY(lcs_check("nrm_lcpm_csr_colsum", d_indptr, d_indices, d_data, dtype, rows, n, nnz));
	NRM_REQUIRE(d_exp_table && table_len > 0 && table_len <= LCS_TAB_CAP && d_cell_total && d_partial && d_t1, "nrm_lcpm_csr_colsum: bad arguments");
	NRM_REQUIRE(d_unit || (unit >= 0.0 && std::isfinite(unit)), "nrm_lcpm_csr_colsum: unit must be the largest (E[x] - E[0]) / x of the table");
	const int64_t tiles = (rows + LCS_TR - 1) / LCS_TR;
	hipStream_t st = (hipStream_t)stream;
#define LCS_GO(TY)                                                                                                                                                          \
	hipLaunchKernelGGL((k_lcs_colsum<TY>), dim3((unsigned)tiles), dim3(512), 0, st, d_indptr, d_indices, (const TY*)d_data, rows, n, nnz, dev, d_exp_table, table_len, unit, d_unit, \
					   d_cell_total, d_partial)
	NRM_BY_COUNT_DTYPE(LCS_GO)
#undef LCS_GO
	NRM_TRY(nrm_check_launch("k_lcs_colsum"));
	hipLaunchKernelGGL(k_lcs_finish, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, d_partial, tiles, n, rows, d_exp_table, unit, d_unit, d_cell_total, d_t1);
	return nrm_check_launch("k_lcs_finish");
}

template <typename T>
static void lcs_launch_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int64_t rows, int64_t n, int64_t nnz, int dev, const double* d_table,
							 int64_t table_len, const double* d_t1, void* d_out, int out_dtype, int64_t ldo, bool al, hipStream_t st) {
	const dim3 grid((unsigned)(rows < 16384 ? rows : 16384));
#define LCS_GO4(TO, AL) \
	hipLaunchKernelGGL((k_lcs_write<T, TO, AL>), grid, dim3(256), 0, st, d_indptr, d_indices, (const T*)d_data, rows, n, nnz, dev, d_table, table_len, d_t1, (TO*)d_out, ldo)
#define LCS_GO(TO)              \
	do {                        \
		if (al) LCS_GO4(TO, true); \
		else LCS_GO4(TO, false); \
	} while (0)
	if (out_dtype == NRM_F64) LCS_GO(double);
	else LCS_GO(float);
#undef LCS_GO
#undef LCS_GO4
}

int nrm_lcpm_csr_passes_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int dev,
							  const double* d_table, int64_t table_len, const double* d_t1, void* d_out, int out_dtype, int64_t ldo, void* stream) {
	NRM_TRY(lcs_check("nrm_lcpm_csr_write", d_indptr, d_indices, d_data, dtype, rows, n, nnz));
	NRM_REQUIRE(out_dtype == NRM_F32 || out_dtype == NRM_F64, "nrm_lcpm_csr_write: bad dtype");
	NRM_REQUIRE(d_table && table_len > 0 && table_len <= LCS_TAB_CAP && d_out && ldo >= n, "nrm_lcpm_csr_write: bad arguments");
	const bool al = (uintptr_t)d_out % 16 == 0 && (ldo * (out_dtype == NRM_F64 ? 8 : 4)) % 16 == 0 && (d_t1 == nullptr || (uintptr_t)d_t1 % 16 == 0);
#define LCS_GO(TY) lcs_launch_write<TY>(d_indptr, d_indices, d_data, rows, n, nnz, dev, d_table, table_len, d_t1, d_out, out_dtype, ldo, al, (hipStream_t)stream)
	NRM_BY_COUNT_DTYPE(LCS_GO)
#undef LCS_GO
	return nrm_check_launch("k_lcs_write");
}

extern "C" int nrm_lcpm_csr_count(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
								  int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_gene_zero, int64_t* d_info, int64_t* d_partial, void* stream) {
	return nrm_lcpm_csr_passes_count(d_indptr, d_indices, d_data, dtype, rows, n, nnz, 0, d_cell_total, d_cell_nnz, d_gene_zero, d_info, d_partial, stream);
}

extern "C" int nrm_lcpm_csr_colsum(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
								   const double* d_exp_table, int64_t table_len, double unit, const int64_t* d_cell_total, int64_t* d_partial, double* d_t1,
								   void* stream) {
	return nrm_lcpm_csr_passes_colsum(d_indptr, d_indices, d_data, dtype, rows, n, nnz, 0, d_exp_table, table_len, unit, nullptr, d_cell_total, d_partial, d_t1, stream);
}

extern "C" int nrm_lcpm_csr_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
								  const double* d_table, int64_t table_len, const double* d_t1, void* d_out, int out_dtype, int64_t ldo, void* stream) {
	return nrm_lcpm_csr_passes_write(d_indptr, d_indices, d_data, dtype, rows, n, nnz, 0, d_table, table_len, d_t1, d_out, out_dtype, ldo, stream);
}
