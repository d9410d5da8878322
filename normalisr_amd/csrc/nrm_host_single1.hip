// nrm_association_tests_single1_host (`normalisr de -m single`: association.py:263-390,911-925), numpy buffers in, numpy buffers out, no torch: the kernels
// normalisr_amd/single1.py drives through the device-pointer entries, here through NrmSingle1Step (nrm_single1_step.h: the sizes, buffers and launch sequence the
// resident plan runs too) on one stream with the library's own scratch pool; what the counters mean is nrm_single1_status (nrm_single1_plan_args.h).
#include <cstdio>
#include "nrm_host_entry.h"
#include "nrm_design.h"
#include "nrm_single1_plan_args.h"
#include "nrm_single1_step.h"

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
	// the step record (nrm_single1_step.h): sizes, buffers and launches, shared with the resident plan
	NrmSingle1Step s;
	s.rows = s.nx = nx, s.ny = ny, s.n = s.ldy = n, s.nc = nc, s.y_dtype = y_dtype, s.out_dtype = out_dtype, s.dimreduce = dimreduce, s.return_dot = return_dot;
	s.L = &L, s.d_c = dc.as<double>();
	NRM_TRY(s.alloc_fixed(nrm_take_plain, st));
	NRM_TRY(s.alloc_design(L.nnz, nrm_take_plain));
	NRM_TRY(s.alloc_kept("nrm_association_tests_single1_host", nrm_take_plain, st));  // cell selection (association.py:915-918)
	NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, dy, st));
	const bool want_alpha = h_alpha && nc;
	const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
	DevBuf op, ostat, ovary, oalpha;
	NRM_TRY(nrm_take_all(nrm_take_plain, {{&op, ob}, {&ostat, ob}, {&ovary, ob}}));
	if (want_alpha) NRM_TRY(oalpha.alloc_zero(ob * nc, st));
	s.d_y = dy.p, s.p = op.p, s.stat = ostat.p, s.vary = ovary.p, s.alpha = want_alpha ? oalpha.p : nullptr;
	std::vector<double> vxx((size_t)nx);
	const bool host_stats = nc > 8 && nrm_debug_is("single1_stats", "host");
	if (nc > 8 && nrm_debug_is("s1_trace", "1"))
		fprintf(stderr, "single=1: the groupings' statistics on the %s, %lld covariates\n", host_stats ? "host" : "device (wide)", (long long)nc);
	if (!host_stats) {
		// the groupings' statistics stay on the device at every covariate count: nothing comes back but the counters and varx
		NRM_TRY(s.enqueue_selected(st, nullptr, nullptr, nullptr));
	} else {
		// NRM_DEBUG=single1_stats=host from 9 covariates: the statistics on the host, as in rounds 4-5 (nrm_host_math.h), uploaded as the records the device writes
		NRM_TRY(s.common_gram(st));
		std::vector<double> hrows, hpart, ns, mcc, gs, rec, dof, hxe;
		std::vector<int64_t> hseg, hidx;
		NRM_TRY(download(hrows, s.rowinfo.p, (size_t)nx * 3));
		NRM_TRY(nrm_single1_cell_counts(hrows.data(), s.n_common, nx, ns));
		NRM_TRY(download(hpart, s.gpart.p, (size_t)s.gpart_doubles));
		nrm_single1_reduce_gram(hpart.data(), nrm_single1_select_gram_blocks(), nc, mcc);
		NRM_TRY(download(hseg, s.seg.p, (size_t)nx + 1));
		NRM_TRY(download(hidx, s.idx.p, (size_t)s.n_kept));
		NRM_TRY(download(hxe, s.xe.p, (size_t)s.n_kept));
		nrm_single1_group_sums(hseg.data(), hidx.data(), hxe.data(), c64.data(), n, nc, nx, gs);
		NRM_TRY(nrm_single1_group_records(gs, mcc, ns, nc, nx, dimreduce, rec, vxx, dof));
		NRM_TRY(nrm_pvalue_plan_init_many(dof.data(), nx, rec.data() + 2, s.pitch));
		NRM_HIP(hipMemcpy(s.info.p, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
		NRM_HIP(hipMemcpy(s.varx.p, vxx.data(), vxx.size() * 8, hipMemcpyHostToDevice));
		NRM_TRY(s.stream_and_cells(st, nullptr));
	}
	int32_t hf[8];
	NRM_TRY(nrm_read_flags(s.flags.p, st, hf));
	NRM_TRY(nrm_single1_status(hf));
	NRM_TRY(copy_out(h_p, op.p, ob));
	NRM_TRY(copy_out(h_stat, ostat.p, ob));
	NRM_TRY(copy_out(h_vary, ovary.p, ob));
	if (want_alpha) NRM_TRY(copy_out(h_alpha, oalpha.p, ob * nc));
	NRM_TRY(download(vxx, s.varx.p, (size_t)nx));
	nrm_store_as(out_dtype, h_varx, vxx.data(), nx);
	return NRM_OK;
}
