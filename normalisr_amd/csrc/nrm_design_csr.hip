// The lists of csrc/nrm_design_lists.hip from a design that arrives SPARSE: canonical CSR over the design rows (indptr int64, indices int32 strictly increasing
// inside a row, data fp32 / fp64 or none at all: every stored entry 1), in HBM.  The dense kernels sweep the (groupings x cells) matrix twice to recover the
// entry list a gRNA incidence matrix usually started as (association.py:224-235 multiplies it densely, association.py:914-918 selects cells from it); here
//
//   nrm_design_csr_count   a wave per design row walks the row's stored entries: entries per (chunk of DS_CH cells, row) and what they are like, in the format
//                          of nrm_design_count -- cells ascend, so an entry's chunk is cell / DS_CH and a chunk's entries are consecutive: counts from ballots --,
//                          and the structure check (d_info[NRM_DESIGN_CSR_BAD])
//   nrm_design_plan        unchanged: it reads the counts only
//   nrm_design_csr_fill    the second walk writes the library's own CSR arrays (stored zeros dropped) and the ELL blocks, padding included; ranks from
//                          ballots and running counts, no atomics: the same bits run to run, and the bits nrm_design_fill writes for the densified matrix
//   nrm_design_csr_dense   the matrix itself, for the routes that read one: a zero fill and a scatter
// A stored zero is not an entry; a NaN is (value != 0, as the dense kernels count).  Integer work and byte moves bound by launch latency.
// The count kernel trusts nothing: indptr is clamped to [0, nnz] and a column outside [0, n) is flagged and not used.  Fill and dense take a matrix the count
// accepted; they still check every column and every position they write against the sizes the plan allotted.
#include "nrm_device.h"
#include "nrm_design.h"

#define DL_FLAG_SHIFT 16

namespace {

// what an entry is like (the bits of k_dl_count)
template <typename T>
__device__ __forceinline__ unsigned dc_bits(T x) {
	unsigned fl = 0;
	if (x != (T)1) fl |= DL_NOTONE;
	if (x < (T)0) fl |= DL_NEG;
	if (x > (T)1) fl |= DL_GT1;
	if (x == (T)1) fl |= DL_HAS1;
	if (x != x) fl |= DL_NAN;
	return fl;
}

// ---- pass 1: entries per (chunk, design row), the structure check ----------------------------------------------------------------------------------------------
// grid ceil(nslots / 4), 256 threads: a wave per slot (cnt was zeroed: only the chunks a row has entries in are written).  64 stored entries per step; the lanes
// of a step whose entries share a chunk are found by ballot, chunk by chunk (ascending cells: one or a few chunks per step); cur / run / fl (the chunk being
// counted) are the same in every lane.
template <typename T>
__global__ void __launch_bounds__(256) k_dc_count(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t nx, int64_t n,
													  int64_t nnz, int64_t nslots, int32_t* __restrict__ cnt, int64_t* __restrict__ info) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
	if (slot >= nx) return;
	const int64_t a = indptr[slot], b = indptr[slot + 1];
	bool bad = a < 0 || b < a || b > nnz || (slot == 0 && a != 0) || (slot == nx - 1 && b != nnz);
	const int64_t s = nrm_clamp(a, 0, nnz), e = nrm_clamp(b, s, nnz);
	int cur = -1, run = 0;
	unsigned fl = 0;
	for (int64_t p0 = s; p0 < e; p0 += 64) {
		const int64_t p = p0 + lane;
		const bool ok = p < e;
		const int64_t col = ok ? (int64_t)idx[p] : 0, prev = ok && p > s ? (int64_t)idx[p - 1] : -1;
		const bool inr = ok && col >= 0 && col < n;
		bad |= ok && (!inr || prev >= col);
		const T x = inr ? (val ? val[p] : (T)1) : (T)0;
		const bool use = inr && x != (T)0;  // (NaN counts as an entry, as it does for the dense kernels)
		const unsigned f = use ? dc_bits<T>(x) : 0u;
		const int ch = (int)(col / DS_CH);
		uint64_t todo = __ballot(use);
		while (todo) {
			const int c = __shfl(ch, __ffsll((long long)todo) - 1, 64);
			const bool mine = use && ch == c;
			const uint64_t m = __ballot(mine);
			unsigned wfl = 0;
#pragma unroll
			for (int q = 0; q < 5; q++)
				if (__ballot(mine && ((f >> q) & 1))) wfl |= 1u << q;
			if (c != cur) {
				if (cur >= 0 && lane == 0) cnt[(int64_t)cur * nslots + slot] = (run < 0xffff ? run : 0xffff) | (int32_t)(fl << DL_FLAG_SHIFT);
				cur = c, run = 0, fl = 0;
			}
			run += __popcll(m);
			fl |= wfl;
			todo &= ~m;
		}
	}
	if (cur >= 0 && lane == 0) cnt[(int64_t)cur * nslots + slot] = (run < 0xffff ? run : 0xffff) | (int32_t)(fl << DL_FLAG_SHIFT);
	if (__ballot(bad) && lane == 0) atomicOr(reinterpret_cast<unsigned*>(info + NRM_DESIGN_CSR_BAD), 1u);  // (malformed rows only)
}

// ---- pass 2: the entries into their places ---------------------------------------------------------------------------------------------------------------------
// A wave per slot again.  Entry j of the row's list in chunk c goes where k_dl_fill puts it: cells / row_vals [row_ptr[row] + (entries of the row before it)],
// ell / ellv [base[c][p / 64] + ((j / 8) * 64 + p % 64) * 8 + j % 8], p = pos[c][slot]; a chunk's padding (offset DS_CH, value 0) up to the width of its block
// of 64 follows when the walk leaves the chunk, and the chunks the row has no entry in are padded a lane each.
struct DcEll {
	int64_t eb;
	int wd, pl;
};
__device__ __forceinline__ DcEll dc_ell(const int32_t* __restrict__ pos, const int32_t* __restrict__ w, const int64_t* __restrict__ base, int64_t nslots, int ngroups, int64_t slot,
										int c) {
	const int p = pos[(int64_t)c * nslots + slot];
	const int64_t g = (int64_t)c * ngroups + p / 64;
	return DcEll{base[g], w[g], p & 63};
}
__device__ __forceinline__ int64_t dc_at(const DcEll& L, int j) { return L.eb + ((int64_t)(j >> 3) * 64 + L.pl) * 8 + (j & 7); }

template <typename T, bool BINARY>
__global__ void __launch_bounds__(256) k_dc_fill(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t nx, int64_t n,
													 int64_t nslots, int ngroups, int nch, const int32_t* __restrict__ pos, const int32_t* __restrict__ w,
													 const int64_t* __restrict__ base, const int64_t* __restrict__ row_ptr, int16_t* __restrict__ ell, double* __restrict__ ellv,
													 int32_t* __restrict__ cells, double* __restrict__ row_vals) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
	if (slot >= nslots) return;
	const uint64_t below = (1ull << lane) - 1;
	int cur = -1, r = 0;  // the chunk being written, its entries so far (the same in every lane)
	DcEll L{0, 0, 0};
	// the padding of chunk cur's list from entry r on; the lists of the chunks c0 .. c1 - 1, all padding
	auto finish = [&]() {
		if (cur < 0) return;
		for (int j = r + lane; j < L.wd; j += 64) {
			const int64_t q = dc_at(L, j);
			ell[q] = (int16_t)DS_CH;
			if constexpr (!BINARY) ellv[q] = 0.0;
		}
	};
	auto gap = [&](int c0, int c1) {
		for (int c = c0 + lane; c < c1; c += 64) {
			const DcEll G = dc_ell(pos, w, base, nslots, ngroups, slot, c);
			for (int j = 0; j < G.wd; j++) {
				const int64_t q = dc_at(G, j);
				ell[q] = (int16_t)DS_CH;
				if constexpr (!BINARY) ellv[q] = 0.0;
			}
		}
	};
	if (slot < nx) {
		const int64_t a = indptr[slot], b = indptr[slot + 1];
		const int64_t s = a < 0 ? 0 : a, e = b < s ? s : b;
		const int64_t e0 = cells ? row_ptr[slot] : 0, room = cells ? row_ptr[slot + 1] - e0 : 0;
		int64_t tot = 0;  // entries of the row so far
		for (int64_t p0 = s; p0 < e; p0 += 64) {
			const int64_t p = p0 + lane;
			const bool ok = p < e;
			const int64_t col = ok ? (int64_t)idx[p] : 0;
			const bool inr = ok && col >= 0 && col < n;
			const T x = inr ? (val ? val[p] : (T)1) : (T)0;
			const bool use = inr && x != (T)0;
			const int ch = (int)(col / DS_CH), off = (int)(col % DS_CH);
			uint64_t todo = __ballot(use);
			while (todo) {
				const int c = __shfl(ch, __ffsll((long long)todo) - 1, 64);
				const bool mine = use && ch == c;
				const uint64_t m = __ballot(mine);
				if (c != cur) {
					if (ell) {
						finish();
						gap(cur + 1, c);
						L = dc_ell(pos, w, base, nslots, ngroups, slot, c);
					}
					cur = c, r = 0;
				}
				if (mine) {
					const int before = __popcll(m & below);
					if (cells && tot + before < room) {
						cells[e0 + tot + before] = (int32_t)col;
						if constexpr (!BINARY) row_vals[e0 + tot + before] = (double)x;
					}
					const int j = r + before;
					if (ell && j < L.wd) {
						const int64_t q = dc_at(L, j);
						ell[q] = (int16_t)off;
						if constexpr (!BINARY) ellv[q] = (double)x;
					}
				}
				r += __popcll(m);
				tot += __popcll(m);
				todo &= ~m;
			}
		}
	}
	if (ell) {
		finish();
		gap(cur + 1, nch);
	}
}

// ---- the matrix itself -----------------------------------------------------------------------------------------------------------------------------------------
// out was zeroed; a wave per design row stores the row's entries (a stored zero stores a zero).
template <typename T, typename O>
__global__ void __launch_bounds__(256) k_dc_dense(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t nx, int64_t n,
													  O* __restrict__ out, int64_t ldo) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t row = (int64_t)blockIdx.x * 4 + wave;
	if (row >= nx) return;
	const int64_t a = indptr[row], b = indptr[row + 1];
	const int64_t s = a < 0 ? 0 : a, e = b < s ? s : b;
	for (int64_t p = s + lane; p < e; p += 64) {
		const int64_t col = idx[p];
		if (col >= 0 && col < n) out[row * ldo + col] = val ? (O)val[p] : (O)1;
	}
}

}  // namespace

extern "C" int nrm_design_csr_count(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int data_dtype, int64_t nx, int64_t n, int64_t nnz,
									 int32_t* d_cnt, int64_t nslots, int64_t* d_info, void* stream) {
	NRM_REQUIRE(d_indptr && (d_indices || nnz == 0) && d_cnt && d_info && nx > 0 && n > 0 && nnz >= 0 && nslots >= nx && nslots % 64 == 0, "nrm_design_csr_count: bad arguments");
	NRM_REQUIRE(data_dtype == NRM_F32 || data_dtype == NRM_F64, "nrm_design_csr_count: bad dtype");
	const int64_t nch = (n + DS_CH - 1) / DS_CH;
	NRM_REQUIRE(nch <= 65535 && n < (1ll << 31) && nslots < (1ll << 31), "nrm_design_csr_count: matrix too large");
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_info, 0, 8 * sizeof(int64_t), st));
	NRM_HIP(hipMemsetAsync(d_cnt, 0, (size_t)nch * (size_t)nslots * sizeof(int32_t), st));
	const dim3 grid((unsigned)((nx + 3) / 4));
	if (data_dtype == NRM_F64)
		hipLaunchKernelGGL(k_dc_count<double>, grid, dim3(256), 0, st, d_indptr, d_indices, (const double*)d_data, nx, n, nnz, nslots, d_cnt, d_info);
	else
		hipLaunchKernelGGL(k_dc_count<float>, grid, dim3(256), 0, st, d_indptr, d_indices, (const float*)d_data, nx, n, nnz, nslots, d_cnt, d_info);
	return nrm_check_launch("k_dc_count");
}

extern "C" int nrm_design_csr_fill(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int data_dtype, int64_t nx, int64_t n, int64_t nslots,
									const int32_t* d_pos, const int32_t* d_w, const int64_t* d_base, const int64_t* d_row_ptr, const int32_t* d_coff, int16_t* d_ell,
									double* d_ellv, int32_t* d_cells, double* d_row_vals, int binary, void* stream) {
	NRM_REQUIRE(d_indptr && nx > 0 && n > 0 && nslots >= nx && nslots % 64 == 0 && (d_ell || d_cells), "nrm_design_csr_fill: bad arguments");
	NRM_REQUIRE(data_dtype == NRM_F32 || data_dtype == NRM_F64, "nrm_design_csr_fill: bad dtype");
	NRM_REQUIRE(!d_ell || (d_pos && d_w && d_base && (binary || d_ellv)), "nrm_design_csr_fill: the ELL form needs d_pos, d_w, d_base (and d_ellv for valued entries)");
	NRM_REQUIRE(!d_cells || (d_row_ptr && (binary || d_row_vals)), "nrm_design_csr_fill: the CSR form needs d_row_ptr (and d_row_vals for valued entries)");
	(void)d_coff;  // (nrm_design_fill's argument list: a row is walked whole here, so its entries before a chunk are a running count)
	const int64_t nch = (n + DS_CH - 1) / DS_CH, ngroups = nslots / 64;
	NRM_REQUIRE(nch <= 65535 && n < (1ll << 31) && nslots < (1ll << 31), "nrm_design_csr_fill: matrix too large");
	hipStream_t st = (hipStream_t)stream;
	// (without the ELL form the slots past the last design row have nothing to write)
	const dim3 grid((unsigned)(((d_ell ? nslots : nx) + 3) / 4));
#define DC_FILL(T, BIN)                                                                                                                                             \
	hipLaunchKernelGGL((k_dc_fill<T, BIN>), grid, dim3(256), 0, st, d_indptr, d_indices, (const T*)d_data, nx, n, nslots, (int)ngroups, (int)nch, d_pos, d_w, d_base, \
					   d_row_ptr, d_ell, d_ellv, d_cells, d_row_vals)
	if (data_dtype == NRM_F64) {
		if (binary) DC_FILL(double, true); else DC_FILL(double, false);
	} else {
		if (binary) DC_FILL(float, true); else DC_FILL(float, false);
	}
#undef DC_FILL
	return nrm_check_launch("k_dc_fill");
}

extern "C" int nrm_design_csr_dense(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int data_dtype, int64_t nx, int64_t n, void* d_out,
									 int out_dtype, int64_t ldo, void* stream) {
	NRM_REQUIRE(d_indptr && d_out && nx > 0 && n > 0 && ldo >= n && n < (1ll << 31), "nrm_design_csr_dense: bad arguments");
	NRM_REQUIRE((data_dtype == NRM_F32 || data_dtype == NRM_F64) && (out_dtype == NRM_F32 || out_dtype == NRM_F64), "nrm_design_csr_dense: bad dtype");
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_out, 0, (size_t)nx * (size_t)ldo * (out_dtype == NRM_F64 ? 8 : 4), st));
	const dim3 grid((unsigned)((nx + 3) / 4));
#define DC_DENSE(T, O) hipLaunchKernelGGL((k_dc_dense<T, O>), grid, dim3(256), 0, st, d_indptr, d_indices, (const T*)d_data, nx, n, (O*)d_out, ldo)
	if (data_dtype == NRM_F64) {
		if (out_dtype == NRM_F64) DC_DENSE(double, double); else DC_DENSE(double, float);
	} else {
		if (out_dtype == NRM_F64) DC_DENSE(float, double); else DC_DENSE(float, float);
	}
#undef DC_DENSE
	return nrm_check_launch("k_dc_dense");
}
