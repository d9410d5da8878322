// single=0 de beyond the dense path, inside nrm_association_tests_host (numpy buffers in, numpy buffers out, no torch): the sparse-design form
// (association.py:224-235 for a design with few entries: a CRISPR screen's gRNA incidence, BASELINE configs[3]) and the streaming form for few design
// rows (case-control DE, BASELINE configs[2]) -- the same kernels the Python host (normalisr_amd/de_sparse.py, engine.association_de_streaming) drives
// through the device-pointer entries, sequenced here in C++ with the library's own scratch pool.  The sparse-design sequence itself is NrmDeSparseStep
// (nrm_de_sparse_step.h), which the resident de plan runs too.
#include "nrm_host_entry.h"
#include "nrm_design.h"
#include "nrm_de_sparse_step.h"

int NrmDesignLists::build(const void* d_x, int x_dtype, int64_t nx, int64_t n, bool want_ell, double max_density, hipStream_t st) {
	nslots = nrm_round_up(nx, 64);
	ngroups = nslots / 64;
	nch = (n + DS_CH - 1) / DS_CH;
	NRM_TRY(cnt.alloc((size_t)nch * nslots * 4));
	NRM_TRY(coff.alloc((size_t)nch * nslots * 4));
	NRM_TRY(info.alloc(8 * sizeof(int64_t)));
	NRM_TRY(row_ptr.alloc((size_t)(nx + 1) * 8));
	NRM_TRY(slot2x.alloc((size_t)nslots * 4));
	if (want_ell) {
		NRM_TRY(sig.alloc((size_t)nch * nslots * 4));
		NRM_TRY(pos.alloc((size_t)nch * nslots * 4));
		NRM_TRY(w.alloc((size_t)nch * ngroups * 4));
		NRM_TRY(base.alloc((size_t)nch * ngroups * 8));
	}
	NRM_TRY(nrm_design_count(d_x, x_dtype, nx, n, n, cnt.as<int32_t>(), nslots, info.as<int64_t>(), st));
	NRM_TRY(nrm_design_plan(cnt.as<int32_t>(), nx, n, nslots, sig.as<int32_t>(), pos.as<int32_t>(), w.as<int32_t>(), base.as<int64_t>(), row_ptr.as<int64_t>(),
							coff.as<int32_t>(), slot2x.as<int32_t>(), info.as<int64_t>(), st));
	int64_t h[8];
	NRM_HIP(hipMemcpyAsync(h, info.p, sizeof(h), hipMemcpyDeviceToHost, st));
	NRM_HIP(hipStreamSynchronize(st));
	nnz = h[0];
	padded = h[1];
	bits = (int)h[2];
	binary = !(bits & NRM_DESIGN_NOTONE);
	ok = nnz > 0 && (double)nnz <= max_density * (double)nx * (double)n;
	if (!ok) return NRM_OK;
	NRM_TRY(cells.alloc((size_t)nnz * 4));
	if (!binary) NRM_TRY(row_vals.alloc((size_t)nnz * 8));
	if (want_ell) {
		NRM_TRY(ell.alloc((size_t)(padded > 8 ? padded : 8) * 2));
		if (!binary) NRM_TRY(ellv.alloc((size_t)(padded > 8 ? padded : 8) * 8));
	}
	return nrm_design_fill(d_x, x_dtype, nx, n, n, nslots, pos.as<int32_t>(), w.as<int32_t>(), base.as<int64_t>(), row_ptr.as<int64_t>(), coff.as<int32_t>(),
						   ell.as<int16_t>(), ellv.as<double>(), cells.as<int32_t>(), row_vals.as<double>(), binary ? 1 : 0, st);
}

// (a temporary workspace per call; the scratch returns to the pool with this scope, hence the synchronise)
int sparse_products(const NrmDesignLists& L, const void* d_y, int y_dtype, int64_t ny, int64_t n, const double* d_c, int64_t ncu, int ci, double cval, const double* d_dci,
					const double* d_bx, int64_t ldb, double* d_dot, int64_t ldd, int by_gene, double* d_ssy, double* d_coefy, int32_t* d_flags, hipStream_t st) {
	NrmSparseProducts work;
	NRM_TRY(work.alloc(ny, n, ncu, ci, nrm_take_plain, st));
	NRM_TRY(work.enqueue(L, d_y, y_dtype, ny, n, n, d_c, ncu, ci, cval, d_dci, d_bx, ldb, d_dot, ldd, by_gene, d_ssy, d_coefy, d_flags, st));
	NRM_HIP(hipStreamSynchronize(st));
	return NRM_OK;
}

int nrm_host_de_sparse(const void* d_x, int x_dtype, int64_t nx, const void* d_y, int y_dtype, int64_t ny, const double* d_c, const double* h_c64, int64_t nc, int64_t n,
					   const double* d_dci, int rank, double dof, int stat_kind, void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary, void* h_r, void* h_t,
					   int out_dtype, int* taken, int64_t* handed_back, int p_kind) {
	hipStream_t st = nullptr;
	*taken = 0;
	*handed_back = 0;
	NrmDesignLists L;
	NRM_TRY(L.build(d_x, x_dtype, nx, n, true, 1.0 / 16, st));
	if (!L.ok) return NRM_OK;
	*taken = 1;
	// the step record (nrm_de_sparse_step.h): sizes, buffers and launches, shared with the resident plan
	NrmDeSparseStep s;
	s.rows = s.nx = nx, s.ny = ny, s.n = s.ldy = n, s.nc = nc, s.y_dtype = y_dtype, s.out_dtype = out_dtype, s.dof = dof;
	s.ncu = (rank > 0 && nc > 0) ? nc : 0;  // (covariates of rank 0 -- all zero -- leave the rows as they are: association.py:899-903)
	s.ci = s.ncu ? nrm_constant_row(h_c64, nc, n, &s.cval) : -1;
	s.want_alpha = h_alpha != nullptr && nc > 0;
	s.L = &L, s.d_y = d_y, s.d_c = d_c, s.d_dci = d_dci;
	NRM_TRY(s.alloc(nrm_take_plain, st));
	NRM_TRY(s.enqueue_products(st));
	const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
	// the caller's result arrays are page-locked in place by a helper thread while the kernels run
	NrmHostPin pin_p, pin_s, pin_r, pin_t;
	std::thread pinner([&] {
		pin_p.try_pin(h_p, (int64_t)ob);
		pin_s.try_pin(h_stat, (int64_t)ob);
		pin_r.try_pin(h_r, (int64_t)ob);
		pin_t.try_pin(h_t, (int64_t)ob);
	});
	NrmJoiner join{pinner};
	NrmAssocOut out;
	DevBuf oalpha;
	NRM_TRY(out.alloc(ob, h_r != nullptr, h_t != nullptr));
	if (s.want_alpha) NRM_TRY(oalpha.alloc(ob * nc));
	NRM_TRY(s.enqueue_sweep(st, out.p.p, out.stat.p, out.r.p, out.t.p, oalpha.p, stat_kind, p_kind));
	int32_t hf[4];
	NRM_TRY(nrm_read_flags(s.flags.p, st, hf));
	NRM_TRY(nrm_assoc_assertions(hf, " tiles"));
	if (hf[2] > 0) {  // rows all but inside the span of the covariates: the caller redoes the call on K1 and the fp64 Gram kernel
		*handed_back = hf[2];
		return NRM_OK;
	}
	pinner.join();
	NRM_TRY(out.copy_to(h_p, h_stat, h_r, h_t, ob));
	if (s.want_alpha) NRM_HIP(hipMemcpy(h_alpha, oalpha.p, ob * nc, hipMemcpyDeviceToHost));
	NRM_TRY(emit_var(s.ssy.as<double>(), ny, n, h_vary, out_dtype));
	if (h_varx) NRM_TRY(emit_var(s.ssx.as<double>(), nx, n, h_varx, out_dtype));
	return NRM_OK;
}

// ---- de with nx + nc <= 32 (case-control DE: BASELINE configs[2]) -------------------------------------------------------------------------------------
// The raw expression rows streamed once against Z = [C; X~] on the fp64 matrix cores (csrc/nrm_gram_skinny.hip), never residualised, never
// quantised: what engine.association_de_streaming does for the Python host, kernel for kernel.  A constant covariate (the intercept) leaves Z -- its
// product with a row is a plain sum the kernel takes on the vector ALU -- by moving to the end of the covariates; dci is permuted with it (no rank
// assumption) and alpha is put back in the caller's order.  d_x: the design rows already in HBM (pitch n); h_dy: uploaded here, into rows zero padded
// to 16 cells when n is not a multiple of 16 (the kernel streams 16-cell slabs without bounds checks).
int nrm_host_de_streaming(const void* d_x, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const double* h_c64, int64_t nc, int64_t n,
						  const double* h_dci, int rank, double dof, int stat_kind, void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary, void* h_r, void* h_t,
						  int out_dtype, int p_kind) {
	hipStream_t st = nullptr;
	NRM_REQUIRE(nx + nc <= 32 && nx > 0 && ny > 0, "nrm_host_de_streaming: needs nx + nc <= 32");
	double cval = 0.0;
	int ci = nc ? nrm_constant_row(h_c64, nc, n, &cval) : -1;
	if (nc + nx > 31 + (ci >= 0 ? 1 : 0)) {
		ci = -1;
		cval = 0.0;
	}
	const int const_last = ci >= 0 ? 1 : 0;
	const int64_t ncz = nc - const_last;  // covariate rows that stay in Z
	const std::vector<int64_t> perm = nrm_const_last_perm(nc, ci);
	DevBuf cz, dciz, z, xpad, gx, xwork, rwork, ssx, coefx, ypad, yraw, g, ssraw, swork, ssy, by, flags, oalpha;
	NrmAssocOut out;
	if (nc) {  // the covariates in Z's order (the constant one last) and their pseudo-inverse permuted with them
		std::vector<double> hc, hd;
		nrm_permute_covariates(h_c64, h_dci, perm, n, hc, hd);
		NRM_TRY(cz.alloc(hc.size() * 8));
		NRM_HIP(hipMemcpy(cz.p, hc.data(), hc.size() * 8, hipMemcpyHostToDevice));
		NRM_TRY(dciz.alloc(hd.size() * 8));
		NRM_HIP(hipMemcpy(dciz.p, hd.data(), hd.size() * 8, hipMemcpyHostToDevice));
	}
	const int64_t k32 = nrm_round_up(n, 128), n16 = nrm_round_up(n, 16);
	NRM_TRY(z.alloc_zero((size_t)32 * k32 * 8, st));
	if (ncz) NRM_TRY(nrm_copy_rows(z.p, k32 * 8, cz.p, n * 8, n * 8, ncz, st));
	// the design rows: readable up to a multiple of 16 cells
	const size_t xe = nrm_esize(x_dtype), ye = nrm_esize(y_dtype);
	const void* xd = d_x;
	int64_t ldx = n;
	if (n16 != n) {
		NRM_TRY(xpad.alloc_zero((size_t)nx * n16 * xe, st));
		NRM_TRY(nrm_copy_rows(xpad.p, n16 * xe, d_x, n * xe, n * xe, nx, st));
		xd = xpad.p;
		ldx = n16;
	}
	NRM_TRY(gx.alloc_zero((size_t)256 * 32 * 8, st));
	const bool active = rank > 0 && nc > 0;
	if (active) {  // a = x C^T against the covariates in Z's order (the constant one: column 31)
		NRM_TRY(xwork.alloc((size_t)nrm_design_products_workspace_doubles(nx, n) * 8));
		NRM_TRY(nrm_design_products(xd, x_dtype, nx, n, ldx, cz.as<double>(), nc, n, gx.as<double>(), xwork.as<double>(), const_last, st));
	}
	const bool want_alpha = h_alpha != nullptr && nc > 0;
	NRM_TRY(rwork.alloc((size_t)64 * ((k32 + 1023) / 1024) * 8));
	NRM_TRY(ssx.alloc_zero((size_t)NRM_ROW_TILE * 8, st));
	if (want_alpha) NRM_TRY(coefx.alloc_zero((size_t)nx * nc * 8, st));
	double* xt = z.as<double>() + ncz * k32;  // the residualised design rows go straight into their rows of Z
	NRM_TRY(nrm_residualize_wide(xd, x_dtype, nx, n, ldx, nc ? cz.as<double>() : nullptr, nc, n, gx.as<double>(), nc ? dciz.as<double>() : nullptr, rank, xt, k32, ssx.as<double>(),
								 want_alpha ? coefx.as<double>() : nullptr, rwork.as<double>(), const_last, st));
	// the expression rows
	const void* yd;
	int64_t ldy = n;
	if (n16 == n) {
		NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, ypad, st));
		yd = ypad.p;
	} else {
		NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, yraw, st));
		NRM_TRY(ypad.alloc_zero((size_t)ny * n16 * ye, st));
		NRM_TRY(nrm_copy_rows(ypad.p, n16 * ye, yraw.p, n * ye, n * ye, ny, st));
		yraw.release();
		yd = ypad.p;
		ldy = n16;
	}
	const int64_t nyp = nrm_round_up(ny, 256);
	NRM_TRY(g.alloc((size_t)nyp * 32 * 8));
	NRM_TRY(ssraw.alloc((size_t)nyp * 8));
	NRM_TRY(swork.alloc((size_t)nrm_gram_skinny_workspace_bytes()));
	NRM_TRY(nrm_gram_skinny(yd, y_dtype, ny, n, ldy, z.as<double>(), k32, k32, g.as<double>(), ssraw.as<double>(), nyp, ncz + nx, cval, swork.p, st));
	const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
	NRM_TRY(out.alloc(ob, h_r != nullptr, h_t != nullptr));
	NRM_TRY(ssy.alloc((size_t)nyp * 8));
	if (want_alpha) NRM_TRY(by.alloc_zero((size_t)ny * nc * 8, st));
	NRM_TRY(flags.alloc_zero(16, st));
	NRM_TRY(nrm_de_small_sweep_pk(g.as<double>(), ssraw.as<double>(), nc ? dciz.as<double>() : nullptr, nc, rank, ssx.as<double>(), nx, ny, n, dof, stat_kind, out.p.p, out.stat.p,
							   out.r.p, out.t.p, out_dtype, ny, ssy.as<double>(), want_alpha ? by.as<double>() : nullptr, flags.as<int32_t>(), const_last, p_kind, st));
	if (want_alpha) {
		NRM_TRY(oalpha.alloc(ob * nc));
		NRM_TRY(nrm_alpha(out.stat.p, out_dtype, ny, stat_kind, ssx.as<double>(), n, coefx.as<double>(), by.as<double>(), nx, ny, nc, oalpha.p, out_dtype, st));
	}
	int32_t hf[4];
	NRM_TRY(nrm_read_flags(flags.p, st, hf));
	NRM_TRY(nrm_assoc_assertions(hf, " tiles"));
	NRM_TRY(out.copy_to(h_p, h_stat, h_r, h_t, ob));
	if (want_alpha) {  // the coefficients came out in Z's covariate order: back to the caller's
		std::vector<char> tmp;
		NRM_TRY(download(tmp, oalpha.p, ob * nc));
		nrm_alpha_unpermute(tmp.data(), perm, (size_t)nx * ny, nrm_esize(out_dtype), h_alpha);
	}
	NRM_TRY(emit_var(ssy.as<double>(), ny, n, h_vary, out_dtype));
	if (h_varx) NRM_TRY(emit_var(ssx.as<double>(), nx, n, h_varx, out_dtype));
	return NRM_OK;
}
