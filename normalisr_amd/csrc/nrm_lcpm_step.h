// The three passes of lcpm (lcpm.py:21-208) over counts in HBM, written once: the view of the counts (dense with a pitch, or canonical CSR), the integer block
// the count pass fills, the partial sums' scratch, and the launches -- nrm_lcpm_count / colsum / write or their _csr_ forms -- that the whole-problem entries
// (lcpm_run, nrm_host_front.hip) and the resident plan (nrm_front_plan.hip) both run.  The caller sets the shape and the view; `take(DevBuf&, bytes)` allocates (the
// plan's counts pool bytes, the entry passes nrm_take_plain).  Only alloc allocates; what the others queue, a plan captures.  What lies between the passes -- t0, the
// table length and the tables themselves -- stays with the caller: on the host after one read-back in the entry, in small kernels in the plan.
#pragma once
#include "nrm_host_entry.h"

// The CSR passes in both forms of their data-dependent scalars (nrm_lcpm_sparse.hip).  dev = 0: nnz stored entries and `unit` by value, as nrm_lcpm_csr_count /
// colsum / write take them.  dev = 1: nnz is the capacity of d_indices and d_data, the stored entries are indptr[rows] read on the device and clamped to it, and
// unit is *d_unit -- what a captured step needs.
int nrm_lcpm_csr_passes_count(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int dev,
							  int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_gene_zero, int64_t* d_info, int64_t* d_partial, void* stream);
int nrm_lcpm_csr_passes_colsum(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int dev,
							   const double* d_exp_table, int64_t table_len, double unit, const double* d_unit, const int64_t* d_cell_total, int64_t* d_partial, double* d_t1,
							   void* stream);
int nrm_lcpm_csr_passes_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int dev,
							  const double* d_table, int64_t table_len, const double* d_t1, void* d_out, int out_dtype, int64_t ldo, void* stream);

struct NrmLcpmPasses {
	int64_t rows = 0, n = 0;
	int dtype = NRM_I32;
	bool csr = false;
	const void* d_x = nullptr;  // dense (rows, n) with pitch ld; CSR: the stored values
	int64_t ld = 0;
	const int64_t* d_indptr = nullptr;  // CSR: rows + 1 offsets, `stored` columns and values
	const int32_t* d_indices = nullptr;
	int64_t stored = 0;
	const double* d_unit = nullptr;  // CSR in a plan: `stored` is the arrays' capacity, the count is indptr[rows] on the device, and colsum reads its unit here
	DevBuf ibuf, part;  // cell totals (n), cells' non-zero counts (n), genes' zero counts (rows), info (4) as one block; the count pass's slabs, then colsum's partials

	int64_t block_words() const { return 2 * n + rows + 4; }
	int64_t* total() const { return ibuf.as<int64_t>(); }
	int64_t* nnz() const { return total() + n; }
	int64_t* zero() const { return total() + 2 * n; }
	int64_t* info() const { return total() + 2 * n + rows; }  // sum, max, negative entries, malformed CSR

	template <typename Take>
	int alloc(Take take) {
		const int64_t cwords = csr ? nrm_lcpm_csr_workspace(rows, n) : nrm_lcpm_count_workspace(rows, n);
		const int64_t tiles = (rows + nrm_lcpm_row_tile() - 1) / nrm_lcpm_row_tile();
		return nrm_take_all(take, {{&ibuf, block_words() * 8}, {&part, std::max(cwords, tiles * n) * 8}});
	}
	// the block is all sums and integer atomics: cleared before every count pass
	int clear(hipStream_t st) {
		NRM_HIP(hipMemsetAsync(ibuf.p, 0, (size_t)block_words() * 8, st));
		return NRM_OK;
	}
	int count(hipStream_t st) {
		if (csr) return nrm_lcpm_csr_passes_count(d_indptr, d_indices, d_x, dtype, rows, n, stored, d_unit != nullptr, total(), nnz(), zero(), info(), part.as<int64_t>(), st);
		return nrm_lcpm_count(d_x, dtype, rows, n, ld, total(), nnz(), zero(), info(), part.as<int64_t>(), st);
	}
	// d_t1 (n): the column sums of exp_table[x]; unit: what nrm_lcpm_tables returned with the table, read by the CSR form only (and by a plan's from d_unit instead)
	int colsum(const double* d_exp_table, int64_t len, double unit, double* d_t1, hipStream_t st) {
		if (csr) return nrm_lcpm_csr_passes_colsum(d_indptr, d_indices, d_x, dtype, rows, n, stored, d_unit != nullptr, d_exp_table, len, unit, d_unit, total(), part.as<int64_t>(), d_t1, st);
		return nrm_lcpm_colsum(d_x, dtype, rows, n, ld, d_exp_table, len, part.as<double>(), d_t1, st);
	}
	int write(const double* d_table, int64_t len, const double* d_t1, void* d_out, int out_dtype, int64_t ldo, hipStream_t st) {
		if (csr) return nrm_lcpm_csr_passes_write(d_indptr, d_indices, d_x, dtype, rows, n, stored, d_unit != nullptr, d_table, len, d_t1, d_out, out_dtype, ldo, st);
		return nrm_lcpm_write(d_x, dtype, rows, n, ld, d_table, len, d_t1, d_out, out_dtype, ldo, st);
	}
};
