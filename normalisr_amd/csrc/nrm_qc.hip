// Quality control on read counts (reference qc.py:4-85) and the subsetting that follows it, on a count matrix that stays in HBM -- dense or canonical CSR.
// qc_reads removes genes and cells by lower bounds on their totals and on their numbers of expressing cells / expressed genes, again and again until nothing
// changes.  Here the matrix is never rewritten between the iterations: two byte masks (gene_alive, cell_alive) say what is left, and every iteration is
//   k_qc_stats / k_qc_csr_stats   total and number of positive entries of every alive gene over the alive cells and of every alive cell over the alive genes,
//   k_qc_decide                   the six thresholds against those statistics (genes and cells judged on the SAME statistics, qc.py:52-75), the masks cleared
//                                 where a bound is missed, the two alive counts for the host's one read-back,
// and k_subset_dense / k_subset_csr_* then cut the survivors out.  Integer arithmetic only: sums of integers do not depend on their order, so integer atomics
// are used freely and every output is the same bits on every run; there are no floating-point atomics.
// Dense: a workgroup owns QC_TR rows x 1024 cells, a lane four consecutive cells (loads as k_lc_count of nrm_lcpm.hip: 16 bytes where the rows are aligned,
// element by element otherwise and in the ragged last chunk).  The alive rows of the tile are listed in LDS first, so a dead row is never loaded and the
// branch is the same for the whole workgroup.  Per-cell sums stay in registers over the tile's rows and go to the tile's slab (folded in a fixed order by
// k_qc_fold); a row's sum goes through a wave reduction and LDS to one 64-bit atomic per statistic, row and workgroup.
// CSR: as k_lcs_count of nrm_lcpm_sparse.hip -- a workgroup owns QC_TR rows and walks the cells in chunks of QC_CW with the chunk's per-cell accumulators
// and its share of the cell mask in LDS.  Nothing trusts the structure: indptr is clamped to [0, nnz], a column outside its chunk is skipped.
#include "nrm_device.h"

#define QC_TR 32    // rows per workgroup of the statistics passes
#define QC_CW 4096  // cells per chunk of the CSR pass: 32 KB of 64-bit accumulators

typedef unsigned long long qc_u64;

// int64 words of scratch of nrm_qc_stats and nrm_qc_csr_stats: one slab of n words per row tile
extern "C" int64_t nrm_qc_stats_workspace(int64_t rows, int64_t n) { return ((rows + QC_TR - 1) / QC_TR) * n; }

// ---- the masked statistics of a dense matrix ----------------------------------------------------------------------------------------------------------------------
// slab[tile][k] = 256 * (the tile's total of cell k) + its count of positive entries (at most QC_TR); gene_total / gene_nnz are added to (zeroed by the launcher)
template <typename T, bool ALIGNED>
__global__ void __launch_bounds__(256) k_qc_stats(const T* __restrict__ x, int64_t rows, int64_t n, int64_t ld, const uint8_t* __restrict__ gene_alive,
												  const uint8_t* __restrict__ cell_alive, qc_u64* __restrict__ gene_total, qc_u64* __restrict__ gene_nnz,
												  int64_t* __restrict__ slab, qc_u64* __restrict__ info) {
	__shared__ int s_list[QC_TR];
	__shared__ int s_cnt;
	__shared__ qc_u64 s_rtot[QC_TR];
	__shared__ unsigned int s_rnz[QC_TR];
	const int tid = threadIdx.x, lane = tid & 63;
	const int64_t k = ((int64_t)blockIdx.x * 256 + tid) * 4, row0 = (int64_t)blockIdx.y * QC_TR;
	const int nr = (int)(rows - row0 < QC_TR ? rows - row0 : QC_TR);
	if (tid < 64) {  // the tile's alive rows, in order: one list for the whole workgroup
		const bool a = tid < nr && gene_alive[row0 + tid] != 0;
		const qc_u64 m = __ballot(a);
		if (a) s_list[__popcll(m & ((1ull << tid) - 1ull))] = tid;
		if (tid == 0) s_cnt = (int)__popcll(m);
	}
	if (tid < QC_TR) {
		s_rtot[tid] = 0;
		s_rnz[tid] = 0;
	}
	bool live[4];
#pragma unroll
	for (int j = 0; j < 4; j++) live[j] = k + j < n && cell_alive[k + j] != 0;
	const int any = __syncthreads_or(live[0] || live[1] || live[2] || live[3]);  // (the barrier after the list as well)
	const int cnt = any ? s_cnt : 0;  // every cell of the chunk dead: nothing is loaded
	int64_t tot[4] = {0, 0, 0, 0};
	int nz[4] = {0, 0, 0, 0};
	bool neg = false;
	for (int i0 = 0; i0 < cnt; i0 += 4) {  // four rows per step: their loads are issued before the first is used
		int64_t v[4][4];
		int rr[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			rr[u] = s_list[i0 + u < cnt ? i0 + u : cnt - 1];  // (steps past the list repeat its last row and count for nothing)
			nrm_ld4<T, ALIGNED>(x + (row0 + rr[u]) * ld, k, n, v[u]);
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const bool on = i0 + u < cnt;
			int64_t rs = 0;
			int rn = 0;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int64_t t = on && live[j] ? v[u][j] : 0;
				tot[j] += t;
				nz[j] += t > 0;
				rs += t;
				rn += t > 0;
				neg |= t < 0;
			}
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				rs += __shfl_down(rs, o, 64);
				rn += __shfl_down(rn, o, 64);
			}
			if (on && lane == 0 && (rs != 0 || rn != 0)) {
				atomicAdd(&s_rtot[rr[u]], (qc_u64)rs);
				atomicAdd(&s_rnz[rr[u]], (unsigned int)rn);
			}
		}
	}
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (k + j < n) slab[(int64_t)blockIdx.y * n + k + j] = tot[j] * 256 + nz[j];
	const int anyneg = __syncthreads_or(neg);
	if (tid < nr && (s_rtot[tid] != 0 || s_rnz[tid] != 0)) {
		atomicAdd(&gene_total[row0 + tid], s_rtot[tid]);
		atomicAdd(&gene_nnz[row0 + tid], (qc_u64)s_rnz[tid]);
	}
	if (tid == 0 && anyneg) atomicOr(&info[0], 1ull);
}

// cell_total[k], cell_nnz[k]: the tiles' slab words of cell k added in a fixed order (a wave owns 64 consecutive cells, the four waves every fourth tile each)
__global__ void __launch_bounds__(256) k_qc_fold(const int64_t* __restrict__ slab, int64_t tiles, int64_t n, int64_t* __restrict__ cell_total, int64_t* __restrict__ cell_nnz) {
	__shared__ int64_t sm[2][4][64];
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

// ---- the masked statistics of a CSR matrix ------------------------------------------------------------------------------------------------------------------------
// gene_total / gene_nnz of the tile's rows are WRITTEN (a tile owns its rows; 0 for a dead row); slab as k_qc_stats; info[0] |= negative, info[1] |= malformed
template <typename T>
__global__ void __launch_bounds__(256) k_qc_csr_stats(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t rows, int64_t n,
													  int64_t nnz, const uint8_t* __restrict__ gene_alive, const uint8_t* __restrict__ cell_alive,
													  int64_t* __restrict__ gene_total, int64_t* __restrict__ gene_nnz, int64_t* __restrict__ slab, qc_u64* __restrict__ info) {
	__shared__ qc_u64 s_acc[QC_CW];
	__shared__ uint8_t s_live[QC_CW];
	__shared__ int64_t s_cur[QC_TR], s_end[QC_TR];
	__shared__ int s_on[QC_TR];
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t row0 = (int64_t)blockIdx.x * QC_TR;
	const int nr = (int)(rows - row0 < QC_TR ? rows - row0 : QC_TR);
	int bad = 0, on = 0;
	if (tid < QC_TR) {  // the rows' bounds, clamped; a dead row is an empty range
		int64_t s = 0, e = 0;
		if (tid < nr) {
			const int64_t row = row0 + tid, a = indptr[row], b = indptr[row + 1];
			bad = a < 0 || b < a || b > nnz || (row == 0 && a != 0) || (row == rows - 1 && b != nnz);
			on = gene_alive[row] != 0;
			s = nrm_clamp(a, 0, nnz);
			e = on ? nrm_clamp(b, s, nnz) : s;
		}
		s_cur[tid] = s;
		s_end[tid] = e;
		s_on[tid] = on;
	}
	for (int i = tid; i < QC_CW; i += 256) s_acc[i] = 0;
	const int any = __syncthreads_or(on);
	if (!any) {  // every row of the tile dead: nothing is read
		for (int64_t k = tid; k < n; k += 256) slab[(int64_t)blockIdx.x * n + k] = 0;
		if (tid < nr) {
			gene_total[row0 + tid] = 0;
			gene_nnz[row0 + tid] = 0;
		}
		if (bad) atomicOr(&info[1], 1ull);
		return;
	}
	// flat part: every stored entry of the alive rows once, for the structure check
	for (int r = wid; r < nr; r += 4) {
		const int64_t s = s_cur[r], e = s_end[r];
		for (int64_t p0 = s; p0 < e; p0 += 64) {
			const int64_t p = p0 + lane;
			const bool ok = p < e;
			const int64_t col = ok ? (int64_t)idx[p] : 0, prev = ok && p > s ? (int64_t)idx[p - 1] : -1;
			bad |= ok && (col < 0 || col >= n || prev >= col);
		}
	}
	// walk: a wave owns rows wid, wid + 4, ...: their sums stay in its registers over the chunks
	int64_t rs[QC_TR / 4];
	int rn[QC_TR / 4];
#pragma unroll
	for (int i = 0; i < QC_TR / 4; i++) rs[i] = 0, rn[i] = 0;
	bool neg = false;
	for (int64_t c0 = 0; c0 < n; c0 += QC_CW) {
		const int64_t cend = c0 + QC_CW < n ? c0 + QC_CW : n;
		for (int i = tid; i < (int)(cend - c0); i += 256) s_live[i] = cell_alive[c0 + i];
		__syncthreads();
#pragma unroll
		for (int i = 0; i < QC_TR / 4; i++) {
			const int r = wid + 4 * i;
			if (r < nr && s_on[r]) {
				int64_t a = 0;
				int b = 0;
				const int64_t cur = nrm_csr_walk<T>(idx, val, s_cur[r], s_end[r], c0, cend, [&](int c, int64_t x) {
					if (s_live[c]) {
						if (x > 0) atomicAdd(&s_acc[c], ((qc_u64)x << 8) | 1ull);
						a += x;
						b += x > 0;
						neg |= x < 0;
					}
				});
				rs[i] += a;
				rn[i] += b;
				if (lane == 0) s_cur[r] = cur;
			}
		}
		__syncthreads();
		for (int i = tid; i < (int)(cend - c0); i += 256) {
			slab[(int64_t)blockIdx.x * n + c0 + i] = (int64_t)s_acc[i];
			s_acc[i] = 0;
		}
		__syncthreads();
	}
#pragma unroll
	for (int i = 0; i < QC_TR / 4; i++) {
		const int r = wid + 4 * i;
		int64_t a = rs[i];
		int b = rn[i];
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			a += __shfl_down(a, o, 64);
			b += __shfl_down(b, o, 64);
		}
		if (lane == 0 && r < nr) {
			gene_total[row0 + r] = a;
			gene_nnz[row0 + r] = b;
		}
	}
	const int anybad = __syncthreads_or(bad), anyneg = __syncthreads_or(neg);
	if (tid == 0 && anybad) atomicOr(&info[1], 1ull);
	if (tid == 0 && anyneg) atomicOr(&info[0], 1ull);
}

// ---- the decision -------------------------------------------------------------------------------------------------------------------------------------------------
// thr = (n_gene, nc_gene, nc_gene_prop, n_cell, nt_cell, nt_cell_prop), 0 = disabled (every statistic is >= 0); out[0] += alive genes, out[1] += alive cells
struct qc_thr_t {
	int64_t v[6];
};

__global__ void __launch_bounds__(256) k_qc_decide(const int64_t* __restrict__ gene_total, const int64_t* __restrict__ gene_nnz, const int64_t* __restrict__ cell_total,
												   const int64_t* __restrict__ cell_nnz, int64_t rows, int64_t n, qc_thr_t thr, uint8_t* __restrict__ gene_alive,
												   uint8_t* __restrict__ cell_alive, qc_u64* __restrict__ out) {
	__shared__ unsigned int s_g, s_c;
	const int tid = threadIdx.x;
	if (tid == 0) s_g = 0, s_c = 0;
	__syncthreads();
	const int64_t i = (int64_t)blockIdx.x * 256 + tid;
	bool g = false, c = false;
	if (i < rows && gene_alive[i]) {
		g = gene_total[i] >= thr.v[0] && gene_nnz[i] >= thr.v[1] && gene_nnz[i] >= thr.v[2];
		if (!g) gene_alive[i] = 0;
	}
	if (i < n && cell_alive[i]) {
		c = cell_total[i] >= thr.v[3] && cell_nnz[i] >= thr.v[4] && cell_nnz[i] >= thr.v[5];
		if (!c) cell_alive[i] = 0;
	}
	const unsigned int ng = (unsigned int)__popcll(__ballot(g)), nc = (unsigned int)__popcll(__ballot(c));
	if ((tid & 63) == 0) {
		if (ng) atomicAdd(&s_g, ng);
		if (nc) atomicAdd(&s_c, nc);
	}
	__syncthreads();
	if (tid == 0) {
		if (s_g) atomicAdd(&out[0], (qc_u64)s_g);
		if (s_c) atomicAdd(&out[1], (qc_u64)s_c);
	}
}

// ---- subsetting a dense matrix ------------------------------------------------------------------------------------------------------------------------------------
// out[i, j] = x[row_idx[i], col_idx[j]] (NULL: the identity): a lane owns an output column, consecutive lanes consecutive columns -- every store is coalesced and
// every output element is stored once.  An index outside the matrix reads its nearest edge (the caller checks the lists; nothing is read out of bounds).
template <typename U>
__global__ void __launch_bounds__(256) k_subset_dense(const U* __restrict__ x, int64_t rows, int64_t n, int64_t ld, const int64_t* __restrict__ row_idx,
													  const int64_t* __restrict__ col_idx, int64_t ro, int64_t no, U* __restrict__ out, int64_t ldo) {
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= no) return;
	const int64_t c = nrm_clamp(col_idx ? col_idx[j] : j, 0, n - 1);
	for (int64_t i0 = (int64_t)blockIdx.y * 16; i0 < ro; i0 += (int64_t)gridDim.y * 16) {
		const int64_t i1 = i0 + 16 < ro ? i0 + 16 : ro;
#pragma unroll 4
		for (int64_t i = i0; i < i1; i++) {
			const int64_t r = nrm_clamp(row_idx ? row_idx[i] : i, 0, rows - 1);
			out[i * ldo + j] = x[r * ld + c];
		}
	}
}

// ---- subsetting a CSR matrix by masks -----------------------------------------------------------------------------------------------------------------------------
// row_count[g] = the stored entries of row g at kept cells (0 for a dropped row); a wave owns a row.  info[1] |= malformed, over EVERY row.
__global__ void __launch_bounds__(256) k_subset_csr_count(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int64_t rows, int64_t n, int64_t nnz,
														  const uint8_t* __restrict__ gene_alive, const uint8_t* __restrict__ cell_alive, int64_t* __restrict__ row_count,
														  qc_u64* __restrict__ info) {
	const int lane = threadIdx.x & 63;
	const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (g >= rows) return;
	const int64_t a = indptr[g], b = indptr[g + 1];
	bool bad = a < 0 || b < a || b > nnz || (g == 0 && a != 0) || (g == rows - 1 && b != nnz);
	const int64_t s = nrm_clamp(a, 0, nnz), e = nrm_clamp(b, s, nnz);
	const bool on = gene_alive[g] != 0;
	int64_t cnt = 0;
	for (int64_t p0 = s; p0 < e; p0 += 64) {  // (every row is read: the structure of the whole matrix is checked, whatever is kept)
		const int64_t p = p0 + lane;
		const bool ok = p < e;
		const int64_t col = ok ? (int64_t)idx[p] : 0, prev = ok && p > s ? (int64_t)idx[p - 1] : -1;
		const bool inside = ok && col >= 0 && col < n;
		bad |= ok && (!inside || prev >= col);
		cnt += __popcll(__ballot(on && inside && cell_alive[inside ? col : 0] != 0));
	}
	if (lane == 0) row_count[g] = cnt;
	if (__ballot(bad) && lane == 0) atomicOr(&info[1], 1ull);
}

// exclusive prefix of v over the workgroup's 256 threads (in thread order) and the workgroup's total; s_w: four words of LDS
__device__ __forceinline__ int64_t qc_block_scan(int64_t v, int64_t* s_w, int64_t& total) {
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	int64_t inc = v;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int64_t t = __shfl_up(inc, o, 64);
		if (lane >= o) inc += t;
	}
	if (lane == 63) s_w[wid] = inc;
	__syncthreads();
	int64_t off = 0;
	for (int w = 0; w < wid; w++) off += s_w[w];
	total = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
	__syncthreads();
	return off + inc - v;
}

// ONE workgroup: cell_map[k] = kept cells before k (the new column of a kept cell); row_count[g] -> the first output position of row g (an exclusive scan, in
// place); out_indptr = that position for every kept row, then the total; out = {kept rows, kept cells, stored entries kept}.  A thread owns 8 consecutive items.
__global__ void __launch_bounds__(256) k_subset_csr_scan(int64_t* __restrict__ row_count, int64_t rows, const uint8_t* __restrict__ gene_alive,
														 const uint8_t* __restrict__ cell_alive, int64_t n, int64_t* __restrict__ out_indptr, int32_t* __restrict__ cell_map,
														 int64_t* __restrict__ out) {
	__shared__ int64_t s_w[4];
	const int tid = threadIdx.x;
	int64_t kept_cells = 0;
	for (int64_t base = 0; base < n; base += 2048) {
		const int64_t k0 = base + tid * 8;
		int m[8], sum = 0;
#pragma unroll
		for (int j = 0; j < 8; j++) {
			m[j] = k0 + j < n && cell_alive[k0 + j] != 0;
			sum += m[j];
		}
		int64_t total, pos = kept_cells + qc_block_scan(sum, s_w, total);
#pragma unroll
		for (int j = 0; j < 8; j++)
			if (k0 + j < n) {
				cell_map[k0 + j] = (int32_t)pos;
				pos += m[j];
			}
		kept_cells += total;
	}
	int64_t kept_rows = 0, kept_nnz = 0;
	for (int64_t base = 0; base < rows; base += 2048) {
		const int64_t g0 = base + tid * 8;
		int m[8], sum = 0;
		int64_t c[8], csum = 0;
#pragma unroll
		for (int j = 0; j < 8; j++) {
			m[j] = g0 + j < rows && gene_alive[g0 + j] != 0;
			c[j] = m[j] ? row_count[g0 + j] : 0;
			sum += m[j];
			csum += c[j];
		}
		int64_t total, ctotal;
		int64_t r = kept_rows + qc_block_scan(sum, s_w, total), pos = kept_nnz + qc_block_scan(csum, s_w, ctotal);
#pragma unroll
		for (int j = 0; j < 8; j++)
			if (g0 + j < rows) {
				row_count[g0 + j] = pos;
				if (m[j]) out_indptr[r] = pos;
				r += m[j];
				pos += c[j];
			}
		kept_rows += total;
		kept_nnz += ctotal;
	}
	if (tid == 0) {
		out_indptr[kept_rows] = kept_nnz;
		out[0] = kept_rows;
		out[1] = kept_cells;
		out[2] = kept_nnz;
	}
}

// the kept entries of every kept row, in their order, from row_off[g] on: columns through cell_map, values copied (stored zeros stay stored); a wave owns a row
template <typename U>
__global__ void __launch_bounds__(256) k_subset_csr_write(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const U* __restrict__ val, int64_t rows,
														  int64_t n, int64_t nnz, const uint8_t* __restrict__ gene_alive, const uint8_t* __restrict__ cell_alive,
														  const int64_t* __restrict__ row_off, const int32_t* __restrict__ cell_map, int32_t* __restrict__ out_idx,
														  U* __restrict__ out_val, int64_t out_nnz) {
	const int lane = threadIdx.x & 63;
	const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (g >= rows || !gene_alive[g]) return;
	const int64_t s = nrm_clamp(indptr[g], 0, nnz), e = nrm_clamp(indptr[g + 1], s, nnz);
	int64_t pos = row_off[g];
	for (int64_t p0 = s; p0 < e; p0 += 64) {
		const int64_t p = p0 + lane;
		const bool ok = p < e;
		const int64_t col = ok ? (int64_t)idx[p] : 0;
		const bool keep = ok && col >= 0 && col < n && cell_alive[col] != 0;
		const qc_u64 m = __ballot(keep);
		const int64_t w = pos + __popcll(m & ((1ull << lane) - 1ull));
		if (keep && w >= 0 && w < out_nnz) {  // (the bound: the masks or the matrix changed since the count)
			out_idx[w] = cell_map[col];
			out_val[w] = val[p];
		}
		pos += __popcll(m);
	}
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------------------------
static int qc_csr_check(const char* what, const void* d_indptr, const void* d_indices, const void* d_data, int elem, int64_t rows, int64_t n, int64_t nnz) {
	NRM_TRY(nrm_csr_args_check(what, d_indptr, d_indices, d_data, elem, rows, n, nnz));
	NRM_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, "%s: too many rows", what);
	return NRM_OK;
}

#define QC_BY_SIZE(GO)               \
	switch (elem) {                  \
		case 8: GO(uint64_t); break; \
		case 4: GO(uint32_t); break; \
		case 2: GO(uint16_t); break; \
		default: GO(uint8_t); break; \
	}

extern "C" int nrm_qc_stats(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, const uint8_t* d_gene_alive, const uint8_t* d_cell_alive,
							int64_t* d_gene_total, int64_t* d_gene_nnz, int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_info, int64_t* d_work, void* stream) {
	NRM_REQUIRE(nrm_count_elem(dtype) != 0, "nrm_qc_stats: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8");
	NRM_REQUIRE(d_x && rows > 0 && n > 0 && ld >= n, "nrm_qc_stats: bad shape");
	const int64_t tiles = (rows + QC_TR - 1) / QC_TR;
	NRM_REQUIRE(tiles <= 65535, "nrm_qc_stats: at most %d rows", 65535 * QC_TR);
	NRM_REQUIRE(d_gene_alive && d_cell_alive && d_gene_total && d_gene_nnz && d_cell_total && d_cell_nnz && d_info && d_work, "nrm_qc_stats: null pointer");
	NRM_REQUIRE((uintptr_t)d_x % nrm_count_elem(dtype) == 0, "nrm_qc_stats: misaligned matrix");
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_gene_total, 0, (size_t)rows * 8, st));
	NRM_HIP(hipMemsetAsync(d_gene_nnz, 0, (size_t)rows * 8, st));
	NRM_HIP(hipMemsetAsync(d_info, 0, 16, st));
	const bool al = (uintptr_t)d_x % (4 * nrm_count_elem(dtype)) == 0 && ld % 4 == 0;
	const dim3 grid((unsigned)((n + 1023) / 1024), (unsigned)tiles);
#define QC_GO2(TY, AL)                                                                                                                                                \
	hipLaunchKernelGGL((k_qc_stats<TY, AL>), grid, dim3(256), 0, st, (const TY*)d_x, rows, n, ld, d_gene_alive, d_cell_alive, (qc_u64*)d_gene_total, (qc_u64*)d_gene_nnz, \
					   d_work, (qc_u64*)d_info)
#define QC_GO(TY)                \
	do {                         \
		if (al) QC_GO2(TY, true); \
		else QC_GO2(TY, false);  \
	} while (0)
	NRM_BY_COUNT_DTYPE(QC_GO)
#undef QC_GO
#undef QC_GO2
	NRM_TRY(nrm_check_launch("k_qc_stats"));
	hipLaunchKernelGGL(k_qc_fold, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, d_work, tiles, n, d_cell_total, d_cell_nnz);
	return nrm_check_launch("k_qc_fold");
}

extern "C" int nrm_qc_csr_stats(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
								const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, int64_t* d_gene_total, int64_t* d_gene_nnz, int64_t* d_cell_total,
								int64_t* d_cell_nnz, int64_t* d_info, int64_t* d_work, void* stream) {
	NRM_REQUIRE(nrm_count_elem(dtype) != 0, "nrm_qc_csr_stats: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8");
	NRM_TRY(qc_csr_check("nrm_qc_csr_stats", d_indptr, d_indices, d_data, nrm_count_elem(dtype), rows, n, nnz));
	NRM_REQUIRE(d_gene_alive && d_cell_alive && d_gene_total && d_gene_nnz && d_cell_total && d_cell_nnz && d_info && d_work, "nrm_qc_csr_stats: null pointer");
	const int64_t tiles = (rows + QC_TR - 1) / QC_TR;
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_info, 0, 16, st));
#define QC_GO(TY)                                                                                                                                                    \
	hipLaunchKernelGGL((k_qc_csr_stats<TY>), dim3((unsigned)tiles), dim3(256), 0, st, d_indptr, d_indices, (const TY*)d_data, rows, n, nnz, d_gene_alive, d_cell_alive, \
					   d_gene_total, d_gene_nnz, d_work, (qc_u64*)d_info)
	NRM_BY_COUNT_DTYPE(QC_GO)
#undef QC_GO
	NRM_TRY(nrm_check_launch("k_qc_csr_stats"));
	hipLaunchKernelGGL(k_qc_fold, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, d_work, tiles, n, d_cell_total, d_cell_nnz);
	return nrm_check_launch("k_qc_fold");
}

extern "C" int nrm_qc_decide(const int64_t* d_gene_total, const int64_t* d_gene_nnz, const int64_t* d_cell_total, const int64_t* d_cell_nnz, int64_t rows, int64_t n,
							 const int64_t* h_thresholds, uint8_t* d_gene_alive, uint8_t* d_cell_alive, int64_t* d_out, void* stream) {
	NRM_REQUIRE(rows > 0 && n > 0 && h_thresholds, "nrm_qc_decide: bad arguments");
	NRM_REQUIRE(d_gene_total && d_gene_nnz && d_cell_total && d_cell_nnz && d_gene_alive && d_cell_alive && d_out, "nrm_qc_decide: null pointer");
	qc_thr_t thr;
	for (int i = 0; i < 6; i++) {
		NRM_REQUIRE(h_thresholds[i] >= 0, "nrm_qc_decide: thresholds are non-negative");
		thr.v[i] = h_thresholds[i];
	}
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_out, 0, 16, st));
	const int64_t m = rows > n ? rows : n;
	hipLaunchKernelGGL(k_qc_decide, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_gene_total, d_gene_nnz, d_cell_total, d_cell_nnz, rows, n, thr, d_gene_alive,
					   d_cell_alive, (qc_u64*)d_out);
	return nrm_check_launch("k_qc_decide");
}

extern "C" int nrm_subset_dense(const void* d_x, int elem, int64_t rows, int64_t n, int64_t ld, const int64_t* d_row_idx, int64_t rows_out, const int64_t* d_col_idx,
								int64_t n_out, void* d_out, int64_t ldo, void* stream) {
	NRM_REQUIRE(elem == 1 || elem == 2 || elem == 4 || elem == 8, "nrm_subset_dense: elements of 1, 2, 4 or 8 bytes");
	NRM_REQUIRE(d_x && d_out && rows > 0 && n > 0 && ld >= n && rows_out > 0 && n_out > 0 && ldo >= n_out, "nrm_subset_dense: bad shape");
	NRM_REQUIRE((d_row_idx || rows_out == rows) && (d_col_idx || n_out == n), "nrm_subset_dense: without an index list the axis keeps its length");
	NRM_REQUIRE((uintptr_t)d_x % elem == 0 && (uintptr_t)d_out % elem == 0 && (uintptr_t)d_row_idx % 8 == 0 && (uintptr_t)d_col_idx % 8 == 0, "nrm_subset_dense: misaligned");
	const int64_t rt = (rows_out + 15) / 16;
	const dim3 grid((unsigned)((n_out + 255) / 256), (unsigned)(rt < 65535 ? rt : 65535));
	NRM_REQUIRE((n_out + 255) / 256 <= 0x7fffffffLL, "nrm_subset_dense: too many columns");
#define QC_GO(TY) \
	hipLaunchKernelGGL((k_subset_dense<TY>), grid, dim3(256), 0, (hipStream_t)stream, (const TY*)d_x, rows, n, ld, d_row_idx, d_col_idx, rows_out, n_out, (TY*)d_out, ldo)
	QC_BY_SIZE(QC_GO)
#undef QC_GO
	return nrm_check_launch("k_subset_dense");
}

extern "C" int nrm_subset_csr_count(const int64_t* d_indptr, const int32_t* d_indices, int64_t rows, int64_t n, int64_t nnz, const uint8_t* d_gene_alive,
									const uint8_t* d_cell_alive, int64_t* d_row_count, int64_t* d_info, void* stream) {
	NRM_TRY(qc_csr_check("nrm_subset_csr_count", d_indptr, d_indices, d_indices, 1, rows, n, nnz));
	NRM_REQUIRE(d_gene_alive && d_cell_alive && d_row_count && d_info, "nrm_subset_csr_count: null pointer");
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_info, 0, 16, st));
	hipLaunchKernelGGL(k_subset_csr_count, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, d_indptr, d_indices, rows, n, nnz, d_gene_alive, d_cell_alive, d_row_count,
					   (qc_u64*)d_info);
	return nrm_check_launch("k_subset_csr_count");
}

extern "C" int nrm_subset_csr_scan(int64_t* d_row_count, int64_t rows, const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, int64_t n, int64_t* d_out_indptr,
								   int32_t* d_cell_map, int64_t* d_out, void* stream) {
	NRM_REQUIRE(rows > 0 && n > 0 && n <= 0x7fffffffLL, "nrm_subset_csr_scan: bad shape");
	NRM_REQUIRE(d_row_count && d_gene_alive && d_cell_alive && d_out_indptr && d_cell_map && d_out, "nrm_subset_csr_scan: null pointer");
	hipLaunchKernelGGL(k_subset_csr_scan, dim3(1), dim3(256), 0, (hipStream_t)stream, d_row_count, rows, d_gene_alive, d_cell_alive, n, d_out_indptr, d_cell_map, d_out);
	return nrm_check_launch("k_subset_csr_scan");
}

extern "C" int nrm_subset_csr_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int elem, int64_t rows, int64_t n, int64_t nnz,
									const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, const int64_t* d_row_off, const int32_t* d_cell_map, int32_t* d_out_indices,
									void* d_out_data, int64_t out_nnz, void* stream) {
	NRM_REQUIRE(elem == 1 || elem == 2 || elem == 4 || elem == 8, "nrm_subset_csr_write: elements of 1, 2, 4 or 8 bytes");
	NRM_TRY(qc_csr_check("nrm_subset_csr_write", d_indptr, d_indices, d_data, elem, rows, n, nnz));
	NRM_REQUIRE(d_gene_alive && d_cell_alive && d_row_off && d_cell_map && out_nnz >= 0, "nrm_subset_csr_write: bad arguments");
	NRM_REQUIRE(out_nnz == 0 || (d_out_indices && d_out_data && (uintptr_t)d_out_indices % 4 == 0 && (uintptr_t)d_out_data % elem == 0), "nrm_subset_csr_write: bad output");
	if (out_nnz == 0) return NRM_OK;
#define QC_GO(TY)                                                                                                                                                     \
	hipLaunchKernelGGL((k_subset_csr_write<TY>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_indptr, d_indices, (const TY*)d_data, rows, n, nnz, \
					   d_gene_alive, d_cell_alive, d_row_off, d_cell_map, d_out_indices, (TY*)d_out_data, out_nnz)
	QC_BY_SIZE(QC_GO)
#undef QC_GO
	return nrm_check_launch("k_subset_csr_write");
}
