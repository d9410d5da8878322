// The design of a resident de plan when it is set (nrm_de_design.h): de's row filter (de.py:93), the row map, the rows kept compacted, their lists -- for the
// single=0 plan (nrm_de_plan.hip) and the single=1 plan (nrm_single1_plan.hip) alike, so that a row de drops reaches neither plan's kernels.
#include "nrm_device.h"
#include "nrm_de_design.h"
#include "nrm_design.h"

namespace {

// ---- de's row filter (de.py:93): a design row is tested when it has more than one distinct value, NaNs counting as equal ---------------------------------------
// A wave per row, four rows per workgroup.  The row is read 256 cells at a time (four loads in flight per lane) until a value differs from its first cell: an
// incidence row is settled by its first entry.
template <typename T>
__global__ __launch_bounds__(256) void k_de_vary_dense(const T* __restrict__ x, int64_t rows, int64_t n, int64_t ld, uint8_t* __restrict__ mask) {
	const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (r >= rows) return;  // (whole waves leave: no barrier follows)
	const T* row = x + r * ld;
	const T first = row[0];
	const bool fnan = first != first;
	bool varies = false;
	for (int64_t k0 = 0; k0 < n && !varies; k0 += 256) {
		bool d = false;
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t k = k0 + u * 64 + lane;
			if (k < n) {
				const T v = row[k];
				d |= (v != first) && !(fnan && v != v);
			}
		}
		varies = __ballot(d) != 0ull;
	}
	if (lane == 0) mask[r] = varies ? 1 : 0;
}

// The same from canonical CSR (a stored zero is not an entry, a NaN is one): k entries among n cells -- 0 < k < n: the row holds zero and something else; k == 0: all
// zeros; k == n: every cell is set and the values decide.  The row bounds are clamped to [0, nnz]; no column is used as an address.  data == NULL: every entry is 1.
template <typename T>
__global__ __launch_bounds__(256) void k_de_vary_csr(const int64_t* __restrict__ indptr, const T* __restrict__ data, int64_t rows, int64_t n, int64_t nnz,
													 uint8_t* __restrict__ mask) {
	const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (r >= rows) return;
	const int64_t a = nrm_clamp(indptr[r], 0, nnz), e = nrm_clamp(indptr[r + 1], a, nnz);
	int64_t k = e - a;
	bool differ = false;
	if (data != nullptr && k > 0) {
		const T first = data[a];
		const bool fnan = first != first;
		int cnt = 0;
		bool d = false;
		for (int64_t p = a + lane; p < e; p += 64) {
			const T v = data[p];
			cnt += v != (T)0 ? 1 : 0;
			d |= (v != first) && !(fnan && v != v);
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
		k = cnt;
		differ = __ballot(d) != 0ull;
	}
	const bool varies = (k > 0 && k < n) || (k == n && n > 1 && differ);
	if (lane == 0) mask[r] = varies ? 1 : 0;
}

// The row map from the mask, by one workgroup in row order: c2f[c] = the design row of compact row c (int64: the index list nrm_subset_dense reads), f2c[i] = the
// compact row of design row i or -1, *kept = the rows tested.
__global__ __launch_bounds__(256) void k_de_row_map(const uint8_t* __restrict__ mask, int64_t rows, int64_t* __restrict__ c2f, int32_t* __restrict__ f2c, int64_t* __restrict__ kept) {
	__shared__ int wsum[4];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	int64_t base = 0;
	for (int64_t i0 = 0; i0 < rows; i0 += 256) {
		const int64_t i = i0 + threadIdx.x;
		const bool m = i < rows && mask[i] != 0;
		const unsigned long long b = __ballot(m);
		if (lane == 0) wsum[w] = (int)__popcll(b);
		__syncthreads();
		int before = 0, total = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			before += j < w ? wsum[j] : 0;
			total += wsum[j];
		}
		const int64_t c = base + before + (int64_t)__popcll(b & ((1ull << lane) - 1ull));
		if (m) c2f[c] = i;
		if (i < rows) f2c[i] = m ? (int32_t)c : -1;
		base += total;
		__syncthreads();
	}
	if (threadIdx.x == 0) *kept = base;
}

// NrmDesignLists::build (nrm_host_de.hip) with the two passes over the design handed in, so that a CSR design builds the same fields: count(cnt, nslots, info),
// fill(nslots, pos, w, base, row_ptr, coff, ell, ellv, cells, row_vals, binary).  *bad: the count pass found the CSR arrays malformed.
template <typename Count, typename Fill>
int build_lists(NrmDesignLists& L, int64_t nx, int64_t n, bool want_ell, double max_density, Count count, Fill fill, hipStream_t st, bool* bad, int64_t* bytes) {
	L.nslots = nrm_round_up(nx, 64);
	L.ngroups = L.nslots / 64;
	L.nch = (n + DS_CH - 1) / DS_CH;
	const size_t cs = (size_t)L.nch * L.nslots * 4;
	NRM_TRY(L.cnt.alloc(cs));
	NRM_TRY(L.coff.alloc(cs));
	NRM_TRY(L.info.alloc(8 * sizeof(int64_t)));
	NRM_TRY(L.row_ptr.alloc((size_t)(nx + 1) * 8));
	NRM_TRY(L.slot2x.alloc((size_t)L.nslots * 4));
	if (want_ell) {
		NRM_TRY(L.sig.alloc(cs));
		NRM_TRY(L.pos.alloc(cs));
		NRM_TRY(L.w.alloc((size_t)L.nch * L.ngroups * 4));
		NRM_TRY(L.base.alloc((size_t)L.nch * L.ngroups * 8));
	}
	NRM_TRY(count(L.cnt.as<int32_t>(), L.nslots, L.info.as<int64_t>()));
	NRM_TRY(nrm_design_plan(L.cnt.as<int32_t>(), nx, n, L.nslots, L.sig.as<int32_t>(), L.pos.as<int32_t>(), L.w.as<int32_t>(), L.base.as<int64_t>(), L.row_ptr.as<int64_t>(),
							L.coff.as<int32_t>(), L.slot2x.as<int32_t>(), L.info.as<int64_t>(), st));
	int64_t h[8];
	NRM_HIP(hipMemcpyAsync(h, L.info.p, sizeof(h), hipMemcpyDeviceToHost, st));
	NRM_HIP(hipStreamSynchronize(st));
	*bad = h[NRM_DESIGN_CSR_BAD] != 0;
	if (*bad) return NRM_OK;
	L.nnz = h[0];
	L.padded = h[1];
	L.bits = (int)h[2];
	L.binary = !(L.bits & NRM_DESIGN_NOTONE);
	L.ok = L.nnz > 0 && (max_density <= 0.0 || (double)L.nnz <= max_density * (double)nx * (double)n);
	if (!L.ok) return NRM_OK;
	const size_t pad = (size_t)(L.padded > 8 ? L.padded : 8);
	NRM_TRY(L.cells.alloc((size_t)L.nnz * 4));
	if (!L.binary) NRM_TRY(L.row_vals.alloc((size_t)L.nnz * 8));
	if (want_ell) {
		NRM_TRY(L.ell.alloc(pad * 2));
		if (!L.binary) NRM_TRY(L.ellv.alloc(pad * 8));
	}
	const size_t ell_bytes = want_ell ? 2 * cs + (size_t)L.nch * L.ngroups * 12 + pad * (L.binary ? 2 : 10) : 0;
	*bytes = (int64_t)(2 * cs + ell_bytes + (size_t)(nx + 1) * 8 + (size_t)L.nslots * 4 + (size_t)L.nnz * (L.binary ? 4 : 12) + 64);
	return fill(L.nslots, L.pos.as<int32_t>(), L.w.as<int32_t>(), L.base.as<int64_t>(), L.row_ptr.as<int64_t>(), L.coff.as<int32_t>(), L.ell.as<int16_t>(), L.ellv.as<double>(),
				L.cells.as<int32_t>(), L.row_vals.as<double>(), L.binary ? 1 : 0);
}

int upload_to(const void* h, DevBuf& d, size_t bytes, hipStream_t st) {
	NRM_TRY(d.alloc(bytes));
	if (bytes) NRM_TRY(nrm_upload(h, d.p, (int64_t)bytes, 0, (void*)st));
	return NRM_OK;
}

}  // namespace

int nrm_de_design_malformed() {
	nrm_set_error("Malformed CSR design matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and increase "
				  "strictly (sum duplicates and sort the indices first).");
	return NRM_E_ARG;
}

int nrm_de_design_set(const char* who, const NrmDePlanDesign& in, int64_t ng0, int64_t n, uint8_t* d_mask, int64_t* d_c2f, int32_t* d_f2c, bool want_ell, double max_density,
					  hipStream_t st, NrmDeDesign& out) {
	const size_t es = nrm_esize(in.dtype);
	DevBuf up_v, up_p, up_i, kept, cnt0, info0;
	NRM_TRY(kept.alloc(8));
	const void* values = in.values;
	const int64_t* indptr = in.indptr;
	const int32_t* indices = in.indices;
	int64_t ld = in.ld;
	if (in.form == 0) {
		if (!in.on_device) {
			NRM_TRY(upload_to(in.values, up_v, (size_t)ng0 * n * es, st));
			values = up_v.p, ld = n;
		}
		const dim3 grid((unsigned)((ng0 + 3) / 4));
		if (in.dtype == NRM_F64)
			hipLaunchKernelGGL(k_de_vary_dense<double>, grid, dim3(256), 0, st, (const double*)values, ng0, n, ld, d_mask);
		else
			hipLaunchKernelGGL(k_de_vary_dense<float>, grid, dim3(256), 0, st, (const float*)values, ng0, n, ld, d_mask);
		NRM_TRY(nrm_check_launch("k_de_vary_dense"));
	} else {
		if (!in.on_device) {
			NRM_TRY(upload_to(in.indptr, up_p, (size_t)(ng0 + 1) * 8, st));
			NRM_TRY(upload_to(in.indices, up_i, (size_t)in.nnz * 4, st));
			if (in.values) NRM_TRY(upload_to(in.values, up_v, (size_t)in.nnz * es, st));
			indptr = up_p.as<int64_t>(), indices = in.nnz ? up_i.as<int32_t>() : nullptr, values = in.values ? up_v.p : nullptr;
		}
		// the structure check of nrm_design_csr_count over all ng0 rows, before anything else reads the arrays
		const int64_t nslots0 = nrm_round_up(ng0, 64), nch = (n + DS_CH - 1) / DS_CH;
		NRM_TRY(cnt0.alloc((size_t)nch * nslots0 * 4));
		NRM_TRY(info0.alloc(8 * sizeof(int64_t)));
		NRM_TRY(nrm_design_csr_count(indptr, indices, values, in.dtype, ng0, n, in.nnz, cnt0.as<int32_t>(), nslots0, info0.as<int64_t>(), st));
		int64_t h[8];
		NRM_HIP(hipMemcpyAsync(h, info0.p, sizeof(h), hipMemcpyDeviceToHost, st));
		NRM_HIP(hipStreamSynchronize(st));
		if (h[NRM_DESIGN_CSR_BAD]) return nrm_de_design_malformed();
		cnt0.release();
		const dim3 grid((unsigned)((ng0 + 3) / 4));
		if (in.dtype == NRM_F64)
			hipLaunchKernelGGL(k_de_vary_csr<double>, grid, dim3(256), 0, st, indptr, (const double*)values, ng0, n, in.nnz, d_mask);
		else
			hipLaunchKernelGGL(k_de_vary_csr<float>, grid, dim3(256), 0, st, indptr, (const float*)values, ng0, n, in.nnz, d_mask);
		NRM_TRY(nrm_check_launch("k_de_vary_csr"));
	}
	hipLaunchKernelGGL(k_de_row_map, dim3(1), dim3(256), 0, st, d_mask, ng0, d_c2f, d_f2c, kept.as<int64_t>());
	NRM_TRY(nrm_check_launch("k_de_row_map"));
	int64_t ngk = 0;
	NRM_HIP(hipMemcpyAsync(&ngk, kept.p, 8, hipMemcpyDeviceToHost, st));
	NRM_HIP(hipStreamSynchronize(st));
	NRM_REQUIRE(ngk > 0 && ngk <= ng0, "%s: no design row has more than one distinct value (de.py:93 leaves nothing to test)", who);
	const bool all = ngk == ng0;
	std::unique_ptr<NrmDesignLists> L(new NrmDesignLists);
	bool bad = false;
	int64_t lb = 0;
	DevBuf sub_v, sub_p, sub_i, alive, rcount, cmap, out3, info2;
	if (in.form == 0) {
		// the rows kept, gathered into a matrix of their own (nrm_qc.hip): a dropped row never reaches the lists, nrm_design_stats, the guard or single=1's selection
		const void* src = values;
		int64_t lds = ld;
		if (!all) {
			NRM_TRY(sub_v.alloc((size_t)ngk * n * es));
			NRM_TRY(nrm_subset_dense(values, (int)es, ng0, n, ld, d_c2f, ngk, nullptr, n, sub_v.p, n, st));
			src = sub_v.p, lds = n;
		}
		const int dtype = in.dtype;
		NRM_TRY(build_lists(
			*L, ngk, n, want_ell, max_density, [&](int32_t* c, int64_t nslots, int64_t* info) { return nrm_design_count(src, dtype, ngk, n, lds, c, nslots, info, st); },
			[&](int64_t nslots, const int32_t* pos, const int32_t* w, const int64_t* base, const int64_t* row_ptr, const int32_t* coff, int16_t* ell, double* ellv, int32_t* cells,
				double* row_vals, int binary) { return nrm_design_fill(src, dtype, ngk, n, lds, nslots, pos, w, base, row_ptr, coff, ell, ellv, cells, row_vals, binary, st); },
			st, &bad, &lb));
	} else {
		const int64_t* ip = indptr;
		const int32_t* ix = indices;
		const void* dv = values;
		int64_t nnzk = in.nnz;
		if (!all) {
			// count / scan / write of nrm_qc.hip with every cell alive: the rows kept as canonical CSR again
			NRM_TRY(alive.alloc((size_t)n));
			NRM_HIP(hipMemsetAsync(alive.p, 1, (size_t)n, st));
			NRM_TRY(rcount.alloc((size_t)ng0 * 8));
			NRM_TRY(info2.alloc(16));
			NRM_TRY(sub_p.alloc((size_t)(ng0 + 1) * 8));
			NRM_TRY(cmap.alloc((size_t)n * 4));
			NRM_TRY(out3.alloc(24));
			NRM_TRY(nrm_subset_csr_count(indptr, indices, ng0, n, in.nnz, d_mask, alive.as<uint8_t>(), rcount.as<int64_t>(), info2.as<int64_t>(), st));
			NRM_TRY(nrm_subset_csr_scan(rcount.as<int64_t>(), ng0, d_mask, alive.as<uint8_t>(), n, sub_p.as<int64_t>(), cmap.as<int32_t>(), out3.as<int64_t>(), st));
			int64_t h3[3];
			NRM_HIP(hipMemcpyAsync(h3, out3.p, sizeof(h3), hipMemcpyDeviceToHost, st));
			NRM_HIP(hipStreamSynchronize(st));
			NRM_REQUIRE(h3[0] == ngk && h3[2] >= 0 && h3[2] <= in.nnz, "%s: the compacted design does not match its row map", who);
			nnzk = h3[2];
			NRM_TRY(sub_i.alloc((size_t)nnzk * 4));
			NRM_TRY(sub_v.alloc((size_t)nnzk * (values ? es : 4)));
			// (an all-ones design has no values to move: its columns stand in for them)
			NRM_TRY(nrm_subset_csr_write(indptr, indices, values ? values : (const void*)indices, values ? (int)es : 4, ng0, n, in.nnz, d_mask, alive.as<uint8_t>(),
										 rcount.as<int64_t>(), cmap.as<int32_t>(), sub_i.as<int32_t>(), sub_v.p, nnzk, st));
			ip = sub_p.as<int64_t>(), ix = sub_i.as<int32_t>(), dv = values ? sub_v.p : nullptr;
		}
		const int dtype = in.dtype;
		NRM_TRY(build_lists(
			*L, ngk, n, want_ell, max_density, [&](int32_t* c, int64_t nslots, int64_t* info) { return nrm_design_csr_count(ip, ix, dv, dtype, ngk, n, nnzk, c, nslots, info, st); },
			[&](int64_t nslots, const int32_t* pos, const int32_t* w, const int64_t* base, const int64_t* row_ptr, const int32_t* coff, int16_t* ell, double* ellv, int32_t* cells,
				double* row_vals, int binary) { return nrm_design_csr_fill(ip, ix, dv, dtype, ngk, n, nslots, pos, w, base, row_ptr, coff, ell, ellv, cells, row_vals, binary, st); },
			st, &bad, &lb));
	}
	if (bad) return nrm_de_design_malformed();
	NRM_HIP(hipStreamSynchronize(st));  // (the fill read buffers that leave with this scope)
	out.L = std::move(L);
	out.ngk = ngk;
	out.list_bytes = lb;
	return NRM_OK;
}
