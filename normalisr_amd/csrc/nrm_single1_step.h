// One step of single=1 (association.py:263-390, 911-925) on a design's lists, written once: the sizes, the buffers and the launch sequence -- nrm_single1_select;
// nrm_single1_common_gram and the groupings' statistics; nrm_single1_stream; nrm_single1_cells -- that nrm_association_tests_single1_host (nrm_host_single1.hip) and
// the resident plan (nrm_single1_plan.hip) both run.  The caller sets the sizes and the non-owning pointers; `take(DevBuf&, bytes)` allocates (the plan's counts pool
// bytes, the entry passes nrm_take_plain).  Only the alloc_* members allocate, and alloc_kept synchronises and reads back; what the others queue, a plan captures.
#pragma once
#include "nrm_host_entry.h"

struct NrmSingle1Step {
	int64_t rows = 0, nx = 0, ny = 0, n = 0, ldy = 0, nc = 0;  // rows: the design rows the buffers are sized for; nx <= rows: those of the design in L
	int y_dtype = NRM_F64, out_dtype = NRM_F64, dimreduce = 0, return_dot = 0;
	int64_t pitch = 0, gsw = 0, ldye = 0, gpart_doubles = 0;  // derived: alloc_fixed
	int64_t nnz = 0, n_common = 0, n_kept = 0;               // the design's entries; the cells no grouping touches and those with exactly one: alloc_kept
	const NrmDesignLists* L = nullptr;
	const double* d_c = nullptr;  // covariates (nc, n) fp64
	const void* d_y = nullptr;    // the expression matrix (ny, n), pitch ldy
	void *p = nullptr, *stat = nullptr, *vary = nullptr, *alpha = nullptr;  // (nx, ny) of out_dtype; alpha (nx, ny, nc) or NULL
	DevBuf cnt, code, seg, idx, xe, ce, rowinfo, sel_info, gpart, gs, common, info, varx, ye, flags;

	// the derived sizes, and what the shape sizes, for all `rows` design rows; the counters int32[8], cleared
	template <typename Take>
	int alloc_fixed(Take take, hipStream_t st) {
		const int64_t nb = (nc + 7) / 8;  // (an 8 x 8 block of covariates per pair bi <= bj: nrm_single1_common_gram)
		pitch = 26 + nc + nc * nc, gsw = nc * (nc + 1) / 2 + nc + 1, ldye = nrm_round_up(ny, 8);
		gpart_doubles = nb * (nb + 1) / 2 * nrm_single1_select_gram_blocks() * 64;
		NRM_TRY(nrm_take_all(take, {{&cnt, n * 4}, {&code, n * 4}, {&seg, (rows + 1) * 8}, {&rowinfo, rows * 3 * 8}, {&sel_info, 64}, {&gs, rows * gsw * 8},
									{&common, (nc + 1) * ny * 8}, {&info, rows * pitch * 8}, {&varx, rows * 8}, {&flags, 32}}));
		if (nc) NRM_TRY(take(gpart, (size_t)gpart_doubles * 8));
		NRM_HIP(hipMemsetAsync(flags.p, 0, 32, st));
		return NRM_OK;
	}
	// what the design's entries size: the selection's lists
	template <typename Take>
	int alloc_design(int64_t nnz_, Take take) {
		nnz = nnz_;
		if (nc) NRM_TRY(take(ce, (size_t)nnz * nc * 8));
		return nrm_take_all(take, {{&idx, nnz * 8}, {&xe, nnz * 8}});
	}
	// the cell selection (association.py:914-918); the shared cells' Gram matrix is left to common_gram
	int select(hipStream_t st) {
		return nrm_single1_select(L->row_ptr.as<int64_t>(), L->cells.as<int32_t>(), L->row_vals.as<double>(), nx, n, nnz, d_c, n, nc, cnt.as<int32_t>(), code.as<int32_t>(),
								  seg.as<int64_t>(), idx.as<int64_t>(), xe.as<double>(), ce.as<double>(), rowinfo.as<double>(), nullptr, sel_info.as<int64_t>(), st);
	}
	// the selection once for its counts -- the one read-back of sizes -- and the stream kernel's transposed output, sized by the cells that carry exactly one grouping
	template <typename Take>
	int alloc_kept(const char* who, Take take, hipStream_t st) {
		NRM_TRY(select(st));
		int64_t h[8];
		NRM_HIP(hipMemcpyAsync(h, sel_info.p, sizeof(h), hipMemcpyDeviceToHost, st));
		NRM_HIP(hipStreamSynchronize(st));
		NRM_REQUIRE(h[4] >= 0 && h[4] <= nnz, "%s: the selection does not match the design's lists", who);
		n_common = h[3], n_kept = h[4];
		return take(ye, (size_t)(n_kept > 0 ? n_kept : 1) * ldye * nrm_esize(y_dtype) + 64);
	}
	int common_gram(hipStream_t st) { return nc ? nrm_single1_common_gram(cnt.as<int32_t>(), n, d_c, n, nc, gpart.as<double>(), st) : NRM_OK; }
	// The groupings' statistics -- M_i = C_S C_S^T, its pseudo-inverse and integer rank, ccx, vx, dof, the P-value plan (association.py:350-374) -- on the device: a
	// lane per grouping up to 8 covariates, a wave per grouping from 9.  They need the selection only.
	int group_side(hipStream_t st) {
		NRM_TRY(common_gram(st));
		if (nc > 8) {
			NRM_TRY(nrm_single1_group_stats_wide(seg.as<int64_t>(), xe.as<double>(), ce.as<double>(), nc, nx, gs.as<double>(), st));
			return nrm_single1_group_info_wide(gs.as<double>(), gpart.as<double>(), rowinfo.as<double>(), sel_info.as<int64_t>(), nc, nx, dimreduce, info.as<double>(), pitch,
											   varx.as<double>(), flags.as<int32_t>(), st);
		}
		NRM_TRY(nrm_single1_group_stats(seg.as<int64_t>(), idx.as<int64_t>(), xe.as<double>(), d_c, n, nc, nx, gs.as<double>(), st));
		return nrm_single1_group_info(gs.as<double>(), gpart.as<double>(), rowinfo.as<double>(), sel_info.as<int64_t>(), nc, nx, dimreduce, info.as<double>(), pitch,
									  varx.as<double>(), flags.as<int32_t>(), st);
	}
	// The expression matrix read once where it lies (sums over the shared cells, the values at the groupings' own cells transposed), which needs the cell codes only;
	// then, behind `joined` when the groupings' statistics ran on another stream, the results.
	int stream_and_cells(hipStream_t st, hipEvent_t joined) {
		NRM_TRY(nrm_single1_stream(d_y, y_dtype, ldy, d_c, n, nc, code.as<int32_t>(), n, ny, common.as<double>(), ye.p, ldye, st));
		if (joined) NRM_HIP(hipStreamWaitEvent(st, joined, 0));
		return nrm_single1_cells(ye.p, y_dtype, ldye, ce.as<double>(), xe.as<double>(), seg.as<int64_t>(), common.as<double>(), info.as<double>(), pitch, nc, nx, ny, return_dot, p,
								 stat, vary, alpha, out_dtype, ny, flags.as<int32_t>(), st);
	}
	// What follows the selection.  side: the groupings' statistics run there beside the stream kernel -- a fork and a join by the two events, which a capture of `st`
	// records as two branches; side == NULL: everything on `st` in the same order, no events.
	int enqueue_selected(hipStream_t st, hipStream_t side, hipEvent_t forked, hipEvent_t joined) {
		if (side) {
			NRM_HIP(hipEventRecord(forked, st));
			NRM_HIP(hipStreamWaitEvent(side, forked, 0));
		}
		NRM_TRY(group_side(side ? side : st));
		if (side) NRM_HIP(hipEventRecord(joined, side));
		return stream_and_cells(st, side ? joined : nullptr);
	}
	int enqueue(hipStream_t st, hipStream_t side, hipEvent_t forked, hipEvent_t joined) {
		NRM_TRY(select(st));
		return enqueue_selected(st, side, forked, joined);
	}
};
