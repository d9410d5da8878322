// nrm_association_tests_single1_host (`normalisr de -m single`: association.py:263-390,911-925), numpy buffers in, numpy buffers out, no torch: the kernels
// normalisr_amd/single1.py drives through the device-pointer entries, sequenced here in C++ with the library's own scratch pool.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nrm_host_entry.h"
#include "nrm_design.h"

// ---- single=1 (association.py:263-390,911-925) for a design with entries >= 0 ----------------------------------------------------------------
extern "C" int nrm_association_tests_single1_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc, int c_dtype,
												   int64_t nc, int64_t n, int dimreduce, int return_dot, void* h_p, void* h_stat, void* h_alpha, void* h_varx,
												   void* h_vary, int out_dtype) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(h_dx && h_dy && nx > 0 && ny > 0 && n > 0 && nc >= 0 && (nc == 0 || h_dc), "Unmatching dx/dy/dc dimensions.");
	NRM_REQUIRE(h_p && h_stat && h_varx && h_vary, "nrm_association_tests_single1_host: null output");
	NRM_REQUIRE((x_dtype == NRM_F32 || x_dtype == NRM_F64) && (y_dtype == NRM_F32 || y_dtype == NRM_F64) && (out_dtype == NRM_F32 || out_dtype == NRM_F64), "bad dtype");
	if (nc > 32) {
		nrm_set_error("nrm_association_tests_single1_host covers up to 32 covariates (the package's masked-Gram path takes more)");
		return NRM_E_UNSUPPORTED;
	}
	hipStream_t st = nullptr;
	DevBuf dx, dy, dc;
	std::vector<double> c64;
	NRM_TRY(upload_matrix(h_dx, x_dtype, nx, n, dx, st));
	NRM_TRY(covariates_f64(h_dc, c_dtype, nc, n, c64, dc));
	// the design's entries (CSR) and what they are like: dx.max() == 1 (association.py:914)
	NrmDesignLists L;
	NRM_TRY(L.build(dx.p, x_dtype, nx, n, false, 0.25, st));
	if (!(L.bits & NRM_DESIGN_HAS1) || (L.bits & (NRM_DESIGN_GT1 | NRM_DESIGN_NAN))) {
		nrm_set_error("the largest entry of dx must be 1 (association.py:914)");
		return NRM_E_NUMERIC;
	}
	if (!L.ok || (L.bits & NRM_DESIGN_NEG)) {
		nrm_set_error("nrm_association_tests_single1_host covers designs with entries >= 0 of which at most a quarter are set (the package's masked-Gram path takes the others)");
		return NRM_E_UNSUPPORTED;
	}
	// cell selection (association.py:915-918)
	const int64_t nnz = L.nnz;
	const int64_t gb = nrm_single1_select_gram_blocks(), nb = (nc + 7) / 8, npairs = nb * (nb + 1) / 2;
	DevBuf cnt, code, seg, idx, xe, ce, rowinfo, gpart, info;
	NRM_TRY(cnt.alloc((size_t)n * 4));
	NRM_TRY(code.alloc((size_t)n * 4));
	NRM_TRY(seg.alloc((size_t)(nx + 1) * 8));
	NRM_TRY(idx.alloc((size_t)nnz * 8));
	NRM_TRY(xe.alloc((size_t)nnz * 8));
	if (nc) NRM_TRY(ce.alloc((size_t)nnz * nc * 8));
	NRM_TRY(rowinfo.alloc((size_t)nx * 3 * 8));
	if (nc) NRM_TRY(gpart.alloc((size_t)npairs * gb * 64 * 8));
	NRM_TRY(info.alloc(64));
	NRM_TRY(nrm_single1_select(L.row_ptr.as<int64_t>(), L.cells.as<int32_t>(), L.row_vals.as<double>(), nx, n, nnz, dc.as<double>(), n, nc, cnt.as<int32_t>(),
							   code.as<int32_t>(), seg.as<int64_t>(), idx.as<int64_t>(), xe.as<double>(), ce.as<double>(), rowinfo.as<double>(), gpart.as<double>(),
							   info.as<int64_t>(), st));
	std::vector<int64_t> hinfo;
	NRM_TRY(download(hinfo, info.p, 8));  // (the one read-back in front of the stream kernel: the size of its transposed output)
	const int64_t n_common = hinfo[3], n_e = hinfo[4];
	const int64_t pitch = 26 + nc + nc * nc, gsw = nc * (nc + 1) / 2 + nc + 1;
	const int64_t ldye = nrm_round_up(ny, 8);
	const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
	DevBuf ye, common, drec, dvarx, op, ostat, ovary, oalpha, flags;
	NRM_TRY(drec.alloc((size_t)nx * pitch * 8));
	NRM_TRY(dvarx.alloc((size_t)nx * 8));
	NRM_TRY(flags.alloc_zero(32, st));
	std::vector<double> vxx((size_t)nx);
	if (nc <= 8) {
		// Round 6: the groupings' statistics -- M_i = C_S C_S^T, its pseudo-inverse and integer rank, ccx, vx, dof, the P-value plan (association.py:350-374) --
		// stay on the device (nrm_single1_group_stats + nrm_single1_group_info, the launches of single1.Single1Plan): nothing comes back but the counters and varx
		DevBuf gsd;
		NRM_TRY(gsd.alloc((size_t)nx * gsw * 8));
		NRM_TRY(nrm_single1_group_stats(seg.as<int64_t>(), idx.as<int64_t>(), xe.as<double>(), dc.as<double>(), n, nc, nx, gsd.as<double>(), st));
		NRM_TRY(nrm_single1_group_info(gsd.as<double>(), gpart.as<double>(), rowinfo.as<double>(), info.as<int64_t>(), nc, nx, dimreduce, drec.as<double>(), pitch,
									   dvarx.as<double>(), flags.as<int32_t>(), st));
		NRM_HIP(hipStreamSynchronize(st));  // (gsd is released at the end of this block)
	} else if (!nrm_debug_is("single1_stats", "host")) {
		// 9 .. 32 covariates: the same two steps with a wave per grouping (nrm_single1_group_stats_wide + nrm_single1_group_info_wide)
		if (nrm_debug_is("s1_trace", "1")) fprintf(stderr, "single=1: the groupings' statistics on the device (wide), %lld covariates\n", (long long)nc);
		DevBuf gsd;
		NRM_TRY(gsd.alloc((size_t)nx * gsw * 8));
		NRM_TRY(nrm_single1_group_stats_wide(seg.as<int64_t>(), xe.as<double>(), ce.as<double>(), nc, nx, gsd.as<double>(), st));
		NRM_TRY(nrm_single1_group_info_wide(gsd.as<double>(), gpart.as<double>(), rowinfo.as<double>(), info.as<int64_t>(), nc, nx, dimreduce, drec.as<double>(), pitch,
											dvarx.as<double>(), flags.as<int32_t>(), st));
		NRM_HIP(hipStreamSynchronize(st));
	} else {
		// NRM_DEBUG=single1_stats=host: the statistics on the host, as in rounds 4-5 (nrm_host_math.h)
		if (nrm_debug_is("s1_trace", "1")) fprintf(stderr, "single=1: the groupings' statistics on the host, %lld covariates\n", (long long)nc);
		std::vector<double> hrows, hpart, ns, mcc, gs, rec, dof, hxe;
		std::vector<int64_t> hseg, hidx;
		NRM_TRY(download(hrows, rowinfo.p, (size_t)nx * 3));
		NRM_TRY(nrm_single1_cell_counts(hrows.data(), n_common, nx, ns));
		NRM_TRY(download(hpart, gpart.p, (size_t)npairs * gb * 64));
		nrm_single1_reduce_gram(hpart.data(), gb, nc, mcc);
		NRM_TRY(download(hseg, seg.p, (size_t)nx + 1));
		NRM_TRY(download(hidx, idx.p, (size_t)n_e));
		NRM_TRY(download(hxe, xe.p, (size_t)n_e));
		nrm_single1_group_sums(hseg.data(), hidx.data(), hxe.data(), c64.data(), n, nc, nx, gs);
		NRM_TRY(nrm_single1_group_records(gs, mcc, ns, nc, nx, dimreduce, rec, vxx, dof));
		NRM_TRY(nrm_pvalue_plan_init_many(dof.data(), nx, rec.data() + 2, pitch));
		NRM_HIP(hipMemcpy(drec.p, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
		NRM_HIP(hipMemcpy(dvarx.p, vxx.data(), vxx.size() * 8, hipMemcpyHostToDevice));
	}
	// the expression matrix, read once where it lies: sums over the shared cells, the values at the groupings' own cells transposed
	NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, dy, st));
	NRM_TRY(ye.alloc((size_t)(n_e > 0 ? n_e : 1) * ldye * nrm_esize(y_dtype) + 64));
	NRM_TRY(common.alloc((size_t)(nc + 1) * ny * 8));
	NRM_TRY(nrm_single1_stream(dy.p, y_dtype, n, dc.as<double>(), n, nc, code.as<int32_t>(), n, ny, common.as<double>(), ye.p, ldye, st));
	NRM_TRY(op.alloc(ob));
	NRM_TRY(ostat.alloc(ob));
	NRM_TRY(ovary.alloc(ob));
	if (h_alpha && nc) NRM_TRY(oalpha.alloc_zero(ob * nc, st));
	NRM_TRY(nrm_single1_cells(ye.p, y_dtype, ldye, ce.as<double>(), xe.as<double>(), seg.as<int64_t>(), common.as<double>(), drec.as<double>(), pitch, nc, nx, ny, return_dot,
							  op.p, ostat.p, ovary.p, (h_alpha && nc) ? oalpha.p : nullptr, out_dtype, ny, flags.as<int32_t>(), st));
	{  // what the reference asserts or raises, in its order: the selection (:917-918), the SVD's finiteness check, the cell count, the results (:248,252)
		int32_t hf[8];
		NRM_TRY(nrm_read_flags(flags.p, st, hf));
		if (hf[2]) {
			nrm_set_error("%d groupings take a single value on the cells selected for them (association.py:917-918)", hf[2]);
			return NRM_E_NUMERIC;
		}
		if (hf[4]) {
			nrm_set_error("array must not contain infs or NaNs");
			return NRM_E_ARG;
		}
		if (hf[3]) {
			nrm_set_error("Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.");
			return NRM_E_DEVICE;
		}
		NRM_TRY(nrm_assoc_assertions(hf, ""));
	}
	NRM_TRY(copy_out(h_p, op.p, ob));
	NRM_TRY(copy_out(h_stat, ostat.p, ob));
	NRM_TRY(copy_out(h_vary, ovary.p, ob));
	if (h_alpha && nc) NRM_TRY(copy_out(h_alpha, oalpha.p, ob * nc));
	NRM_TRY(download(vxx, dvarx.p, (size_t)nx));
	nrm_store_as(out_dtype, h_varx, vxx.data(), nx);
	return NRM_OK;
}
