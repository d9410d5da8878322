// Device-side primitives every kernel file shares: wave and workgroup reductions, the 16-byte loads, the CSR chunk walk, the result stores.
// Device code only: the files the CPU tests build with g++ (nrm_host_logic.h, nrm_small_pinv.hip, nrm_tsv.hip, nrm_fisher.h, nrm_jacobi.h) must not include it.
// Kernels are pinned bit for bit, and a reduction's order or a load's tail rule is part of their result: a function here changes only together with a comparison of
// the device assembly of every file that includes this header ("Source layout of the kernels").
#pragma once
#include <type_traits>
#include "nrm_common.h"

// ---- reductions -------------------------------------------------------------------------------------------------------------------------------------------------
// The 64 lanes' sum by the shuffle-down tree: valid in lane 0 only.
template <typename T>
__device__ __forceinline__ T nrm_wave_sum(T v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	return v;
}

// The workgroup's sum of v in every thread: lanes by the shuffle tree, the NW waves in their order; sm: NW doubles of LDS (the first barrier: sm may still be
// read from the sum before).  FROM_ZERO: the waves' sums are added to 0.0, not to the first of them -- the same order, but +0.0 where every term is -0.0.
// (The tree is written out: with a call of nrm_wave_sum in its place the binnet kernels come out in another instruction order.)
template <int NW, bool FROM_ZERO = false>
__device__ __forceinline__ double nrm_block_sum(double v, double* sm) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	__syncthreads();
	if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
	__syncthreads();
	double t = FROM_ZERO ? 0.0 + sm[0] : sm[0];
#pragma unroll
	for (int w = 1; w < NW; w++) t += sm[w];
	return t;
}

// ---- loads ------------------------------------------------------------------------------------------------------------------------------------------------------
// Four consecutive elements at p, converted to O.  ALIGNED (the launcher: fp32 / fp64 rows on 16-byte boundaries, count rows on 4-element boundaries): one load,
// two of 16 bytes for doubles; otherwise element loads -- a template switch, not a branch, and either way independent loads issued before the first use.  NT marks
// the loads non-temporal (rows streamed once that would push re-read operands out of L2).
template <typename T, bool ALIGNED, bool NT = false, typename O>
__device__ __forceinline__ void nrm_ld4(const T* __restrict__ p, O (&v)[4]) {
	if constexpr (ALIGNED) {
		constexpr int W = std::is_same<T, double>::value ? 2 : 4;
		typedef T vt __attribute__((ext_vector_type(W)));
#pragma unroll
		for (int h = 0; h < 4; h += W) {
			const vt t = NT ? __builtin_nontemporal_load(reinterpret_cast<const vt*>(p + h)) : *reinterpret_cast<const vt*>(p + h);
#pragma unroll
			for (int j = 0; j < W; j++) v[h + j] = (O)t[j];
		}
	} else {
#pragma unroll
		for (int j = 0; j < 4; j++) v[j] = (O)p[j];
	}
}
// Cells k .. k + 3 of a row of n; cells at and beyond n read as 0 (the ragged last group is loaded element by element).
template <typename T, bool ALIGNED, typename O>
__device__ __forceinline__ void nrm_ld4(const T* __restrict__ row, int64_t k, int64_t n, O (&v)[4]) {
	if (ALIGNED && k + 4 <= n)
		nrm_ld4<T, true>(row + k, v);
	else {
#pragma unroll
		for (int j = 0; j < 4; j++) v[j] = k + j < n ? (O)row[k + j] : (O)0;
	}
}

// Four consecutive fp32 / fp64 values as doubles: nrm_ld4 spelled with HIP's float4 / double2.  The bytes loaded are the same, but the compiler tags loads of its
// own vector types for alias analysis and loads of those structs not, and schedules the kernel around them differently: a kernel keeps the form it was pinned with.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void nrm_ld4d(const T* p, double (&v)[4]) {
	if constexpr (ALIGNED && sizeof(T) == 4) {
		const float4 t = *reinterpret_cast<const float4*>(p);
		v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
	} else if constexpr (ALIGNED) {
		const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
		v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
	} else {
#pragma unroll
		for (int j = 0; j < 4; j++) v[j] = (double)p[j];
	}
}
template <typename T, bool ALIGNED>
__device__ __forceinline__ void nrm_ld4d(const T* __restrict__ row, int64_t k, int64_t n, double (&v)[4]) {  // zero at and beyond n
	if (ALIGNED && k + 4 <= n)
		nrm_ld4d<T, true>(row + k, v);
	else {
#pragma unroll
		for (int j = 0; j < 4; j++) v[j] = k + j < n ? (double)row[k + j] : 0.0;
	}
}

template <typename T>
__device__ __forceinline__ void nrm_store_out(void* base, int64_t idx, double v) {  // a result into an fp32 or fp64 output
	reinterpret_cast<T*>(base)[idx] = (T)v;
}

// ---- tables and CSR ---------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t nrm_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int64_t nrm_table_index(int64_t v, int64_t tlen) {  // (a count outside the table -- the matrix changed since the count pass -- reads its end)
	return v < 0 ? 0 : v >= tlen ? tlen - 1 : v;
}

// One wave, one row, one chunk [c0, cend) of cells: the stored entries from cur on whose column is below cend, 128 per step (both loads of a step are issued
// before the first is used); go(column - c0, count) for those inside the chunk.  Returns the position of the first entry left for the next chunk.
template <typename T, typename F>
__device__ __forceinline__ int64_t nrm_csr_walk(const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t cur, int64_t e, int64_t c0, int64_t cend, F go) {
	const int lane = threadIdx.x & 63;
	for (;;) {
		int64_t col[2], x[2];
		bool in[2];
#pragma unroll
		for (int u = 0; u < 2; u++) {
			const int64_t p = cur + u * 64 + lane;
			const bool ok = p < e;
			col[u] = ok ? (int64_t)idx[p] : cend;
			x[u] = ok ? (int64_t)val[p] : 0;
			in[u] = ok && col[u] < cend;
		}
		int cnt = 0;
#pragma unroll
		for (int u = 0; u < 2; u++) {
			if (in[u] && col[u] >= c0) go((int)(col[u] - c0), x[u]);
			cnt += (int)__popcll(__ballot(in[u]));
		}
		cur += cnt;
		if (cnt < 128) return cur;
	}
}
