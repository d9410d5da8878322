// The front half of the pipeline as whole-problem entries, numpy buffers in, numpy buffers out, no torch: nrm_lcpm_host / nrm_lcpm_csr_host (lcpm.py:21-208 and
// the zero counts of lcpm.py:258), nrm_compute_var_host (norm.py:56-128) and nrm_qc_reads_host / nrm_qc_reads_csr_host (qc.py:4-85).  The kernels are those of
// csrc/nrm_lcpm.hip, nrm_lcpm_sparse.hip, nrm_fitvar.hip, nrm_fitvar_plan.hip and nrm_qc.hip, unchanged, on the library's own scratch pool.  lcpm's passes and
// compute_var's sequence are the step records NrmLcpmPasses (nrm_lcpm_step.h) and NrmFitvarStep (nrm_fitvar_step.h), which the resident plan of nrm_front_plan.hip
// runs too: an entry uploads, fills a record per call, and does on the host what lies around it -- the read-back and the tables between lcpm's passes, the
// pseudo-inverse before compute_var, the counters' words after it (nrm_front_plan_args.h).  qc_reads is sequenced here as normalisr_amd/qc.py sequences it.  The
// arithmetic between two launches is in nrm_host_math.h.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nrm_fitvar_step.h"
#include "nrm_front_plan_args.h"
#include "nrm_host_entry.h"
#include "nrm_lcpm_step.h"

static const char* const MALFORMED_CSR = NRM_MALFORMED_CSR;  // (nrm_front_plan_args.h: the resident plan says the same)

// a host array of any element size in HBM (upload_matrix knows fp32 / fp64 only); nothing is copied for an empty array
static int upload_bytes(const void* h, int64_t bytes, DevBuf& d, hipStream_t st) {
	NRM_TRY(d.alloc((size_t)bytes));
	if (bytes <= 0) return NRM_OK;
	return nrm_upload(h, d.p, bytes, 0, (void*)st);
}

// a count matrix in HBM, dense or canonical CSR: what the three passes of lcpm and the statistics pass of qc_reads read
struct FrontCounts {
	DevBuf x, indptr, indices;
	int dtype = 0;
	int64_t rows = 0, n = 0, nnz = 0;
	bool csr = false;
	int dense(const void* h_x, int dt, int64_t r, int64_t c, hipStream_t st) {
		dtype = dt, rows = r, n = c, csr = false;
		return upload_bytes(h_x, r * c * nrm_count_elem(dt), x, st);
	}
	int sparse(const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int dt, int64_t r, int64_t c, int64_t z, hipStream_t st) {
		dtype = dt, rows = r, n = c, nnz = z, csr = true;
		NRM_TRY(upload_bytes(h_indptr, (r + 1) * 8, indptr, st));
		NRM_TRY(upload_bytes(h_indices, z * 4, indices, st));
		return upload_bytes(h_data, z * nrm_count_elem(dt), x, st);
	}
	// what lcpm's passes read of it (nrm_lcpm_step.h); a dense matrix uploaded here is contiguous
	void view(NrmLcpmPasses& p) const {
		p.rows = rows, p.n = n, p.dtype = dtype, p.csr = csr, p.d_x = x.p, p.ld = n;
		p.d_indptr = indptr.as<int64_t>(), p.d_indices = indices.as<int32_t>(), p.stored = nnz;
	}
};

static int front_check_dense(const char* what, const void* h_x, int dtype, int64_t rows, int64_t n) {
	NRM_REQUIRE(h_x != nullptr, "%s: null pointer", what);
	NRM_REQUIRE(rows > 0 && n > 0, "reads must not be empty.");
	NRM_REQUIRE(nrm_count_elem(dtype) != 0, "%s: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8", what);
	return NRM_OK;
}
static int front_check_csr(const char* what, const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int dtype, int64_t rows, int64_t n, int64_t nnz) {
	NRM_REQUIRE(h_indptr != nullptr && (nnz <= 0 || (h_indices && h_data)), "%s: null pointer", what);
	NRM_REQUIRE(rows > 0 && n > 0, "reads must not be empty.");
	NRM_REQUIRE(nnz >= 0 && n <= 0x7fffffffLL, "%s: bad shape", what);
	NRM_REQUIRE(nrm_count_elem(dtype) != 0, "%s: counts are NRM_I64, NRM_I32, NRM_I16 or NRM_U8", what);
	NRM_REQUIRE(h_indptr[0] == 0 && h_indptr[rows] == nnz, "%s", MALFORMED_CSR);  // (the device checks the rest; these two bound the uploads)
	return NRM_OK;
}

// ---- lcpm (lcpm.py:21-208) -----------------------------------------------------------------------------------------------------------------------------------
static int lcpm_check(const char* what, bool have_out, void* h_gene_zero, int64_t* h_info, int64_t ntot, int out_dtype) {
	NRM_REQUIRE(h_info != nullptr && (have_out || h_gene_zero), "%s: null pointer", what);
	NRM_REQUIRE(!have_out || out_dtype == NRM_F32 || out_dtype == NRM_F64, "%s: out_dtype must be NRM_F32 or NRM_F64", what);
	NRM_REQUIRE(ntot != 0, "ntot must be positive (t0 = ntot + 2 > 2, lcpm.py:95).");
	return NRM_OK;
}

// the three passes on a matrix already in HBM (nrm_lcpm_step.h): count, one read-back, the tables on the host, colsum, write, copy out
static int lcpm_run(const FrontCounts& m, int normalize, int64_t ntot, void* h_out, int out_dtype, double* h_cov, int64_t* h_gene_zero, int64_t* h_info, hipStream_t st) {
	const int64_t rows = m.rows, n = m.n;
	NrmLcpmPasses lc;
	m.view(lc);
	NRM_TRY(lc.alloc(nrm_take_plain));
	NRM_TRY(lc.clear(st));
	NRM_TRY(lc.count(st));
	std::vector<int64_t> h;
	NRM_TRY(download(h, lc.ibuf.p, (size_t)lc.block_words()));  // (one small read-back: 2 n_cell + n_gene + 4 integers)
	const int64_t* info = &h[(size_t)(lc.info() - lc.total())];
	NRM_REQUIRE(!info[3], "%s", MALFORMED_CSR);
	NRM_REQUIRE(!info[2] || (!h_out && !h_cov), "Negative value in d detected.");  // (the zero counts alone, lcpm.py:258, do not depend on it)
	h_info[0] = info[0];
	h_info[1] = info[1];
	if (h_gene_zero) memcpy(h_gene_zero, &h[(size_t)(lc.zero() - lc.total())], (size_t)rows * 8);
	if (h_cov) NRM_REQUIRE(nrm_lcpm_cov_rows(h.data(), h.data() + n, rows, n, h_cov) < 0, "Found cell with no read at all. Please remove.");
	if (!h_out) return NRM_OK;
	const double t0 = ntot < 0 ? (double)(info[0] + 2) : (double)ntot + 2.0;
	if (!(t0 > 2)) {
		nrm_set_error("lcpm: the matrix holds no read (t0 = sum + 2 > 2, lcpm.py:95)");
		return NRM_E_NUMERIC;
	}
	if (info[1] >= nrm_lcpm_table_cap()) {
		nrm_set_error("lcpm on the device tabulates psi(1 + count) for counts below %lld; the largest count here is %lld.", (long long)nrm_lcpm_table_cap(), (long long)info[1]);
		return NRM_E_UNSUPPORTED;
	}
	const int64_t len = info[1] + 1;
	std::vector<double> psi((size_t)len), tab, etab;
	double psi_t0 = 0.0;
	NRM_TRY(nrm_lcpm_digamma(len - 1, t0, psi.data(), &psi_t0));
	const double unit = nrm_lcpm_tables(psi.data(), psi_t0, len, tab, etab);
	DevBuf d_tab, d_exp, d_t1, out;
	NRM_TRY(d_tab.alloc((size_t)len * 8));
	NRM_HIP(hipMemcpy(d_tab.p, tab.data(), (size_t)len * 8, hipMemcpyHostToDevice));
	if (normalize) {
		NRM_TRY(d_exp.alloc((size_t)len * 8));
		NRM_HIP(hipMemcpy(d_exp.p, etab.data(), (size_t)len * 8, hipMemcpyHostToDevice));
		NRM_TRY(d_t1.alloc((size_t)n * 8));
		NRM_TRY(lc.colsum(d_exp.as<double>(), len, unit, d_t1.as<double>(), st));
	}
	const size_t ob = (size_t)rows * n * nrm_esize(out_dtype);
	NRM_TRY(out.alloc(ob));
	NRM_TRY(lc.write(d_tab.as<double>(), len, d_t1.as<double>(), out.p, out_dtype, n, st));
	return copy_out(h_out, out.p, ob);
}

extern "C" int nrm_lcpm_host(const void* h_x, int dtype, int64_t rows, int64_t n, int normalize, int64_t ntot, void* h_out, int out_dtype, double* h_cov, int64_t* h_gene_zero,
							 int64_t* h_info) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(front_check_dense("nrm_lcpm_host", h_x, dtype, rows, n));
	NRM_TRY(lcpm_check("nrm_lcpm_host", h_out != nullptr, h_gene_zero, h_info, ntot, out_dtype));
	NRM_TRY(nrm_bind_device());
	hipStream_t st = nullptr;
	FrontCounts m;
	NRM_TRY(m.dense(h_x, dtype, rows, n, st));
	return lcpm_run(m, normalize, ntot, h_out, out_dtype, h_cov, h_gene_zero, h_info, st);
}

extern "C" int nrm_lcpm_csr_host(const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int normalize,
								 int64_t ntot, void* h_out, int out_dtype, double* h_cov, int64_t* h_gene_zero, int64_t* h_info) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(front_check_csr("nrm_lcpm_csr_host", h_indptr, h_indices, h_data, dtype, rows, n, nnz));
	NRM_TRY(lcpm_check("nrm_lcpm_csr_host", h_out != nullptr, h_gene_zero, h_info, ntot, out_dtype));
	NRM_TRY(nrm_bind_device());
	hipStream_t st = nullptr;
	FrontCounts m;
	NRM_TRY(m.sparse(h_indptr, h_indices, h_data, dtype, rows, n, nnz, st));
	return lcpm_run(m, normalize, ntot, h_out, out_dtype, h_cov, h_gene_zero, h_info, st);
}

// ---- compute_var (norm.py:56-128) ------------------------------------------------------------------------------------------------------------------------------
extern "C" int nrm_compute_var_host(const void* h_y, int y_dtype, int64_t rows, int64_t n, const double* h_c, int64_t nc, int64_t stepmax, double eps, double* h_w,
									double* h_state) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_REQUIRE(h_y && h_c && h_w && h_state, "nrm_compute_var_host: null pointer");
	NRM_REQUIRE(rows > 0 && n > 0, "dt must not be empty.");
	NRM_REQUIRE(y_dtype == NRM_F32 || y_dtype == NRM_F64, "nrm_compute_var_host: bad dtype");
	NRM_REQUIRE(eps > 0 && stepmax > 0, "eps and stepmax must be positive.");
	NRM_REQUIRE(stepmax <= 1000000, "nrm_compute_var_host: at most 1000000 steps");
	if (nc < 1 || nc > 63) {
		nrm_set_error("nrm_compute_var_host takes 1 to 63 covariates (the pseudo-inverse of [C;1][C;1]^T comes from the library's Jacobi routine of at most 64 rows)");
		return NRM_E_UNSUPPORTED;
	}
	for (int64_t i = 0; i < nc * n; i++) NRM_REQUIRE(std::isfinite(h_c[i]), "array must not contain infs or NaNs");
	// the one matrix the device sequence takes from the host: the pseudo-inverse of [C;1][C;1]^T on unit-length rows (the second regression has an
	// intercept, norm.py:92,109-110; it does not depend on dt)
	std::vector<double> c1((size_t)(nc + 1) * n), m2i((size_t)(nc + 1) * (nc + 1));
	memcpy(c1.data(), h_c, (size_t)nc * n * 8);
	for (int64_t k = 0; k < n; k++) c1[(size_t)(nc * n + k)] = 1.0;
	int64_t rank2 = 0;
	nrm_pinv_gram_unit_rows(c1.data(), nc + 1, n, 1e-8, m2i.data(), &rank2);
	NRM_TRY(nrm_bind_device());
	hipStream_t st = nullptr;
	DevBuf y, c, dm2i, flags;
	NRM_TRY(upload_matrix(h_y, y_dtype, rows, n, y, st));
	NRM_TRY(upload_matrix(h_c, NRM_F64, nc, n, c, st));
	NRM_TRY(dm2i.alloc(m2i.size() * 8));
	NRM_HIP(hipMemcpy(dm2i.p, m2i.data(), m2i.size() * 8, hipMemcpyHostToDevice));
	NrmFitvarStep fit;
	fit.rows = rows, fit.n = n, fit.ldy = n, fit.nc = nc, fit.stepmax = stepmax, fit.eps = eps, fit.y_dtype = y_dtype;
	fit.d_y = y.p, fit.d_c = c.as<double>(), fit.d_m2i = dm2i.as<double>();
	NRM_TRY(fit.alloc(nrm_take_plain));
	NRM_TRY(flags.alloc_zero(16, st));
	fit.flags = flags.as<int32_t>();
	NRM_TRY(fit.enqueue(st));
	int32_t hf[4];
	NRM_TRY(nrm_read_flags(flags.p, st, hf));
	std::vector<double> ho;
	NRM_TRY(download(ho, fit.state() + 4 * stepmax, (size_t)(4 + n)));  // (the last state record and the weights behind it, in one copy)
	h_state[0] = ho[0];  // best change (the reference's bestv)
	h_state[1] = ho[1];  // steps taken
	NRM_TRY(nrm_compute_var_status(hf));
	memcpy(h_w, ho.data() + 4, (size_t)n * 8);
	return NRM_OK;
}

// ---- qc_reads (qc.py:4-85) ------------------------------------------------------------------------------------------------------------------------------------
static int qc_check(const char* what, const double* p, uint8_t* h_gene_alive, uint8_t* h_cell_alive, int64_t* h_info) {
	NRM_REQUIRE(h_gene_alive && h_cell_alive && h_info, "%s: null pointer", what);
	for (int i = 0; i < 6; i++) NRM_REQUIRE(p[i] >= 0, "All parameters must be non-negative.");  // (a NaN fails it too)
	NRM_REQUIRE(p[2] <= 1 && p[5] <= 1, "Proportional parameters must be no greater than 1.");
	for (int i = 0; i < 6; i++) NRM_REQUIRE(p[i] < 9.0e18, "%s: parameters beyond the range of counts", what);
	return NRM_OK;
}

// the reference's loop (qc.py:49-81) on a matrix already in HBM: a masked statistics pass, the thresholds of the current counts against the statistics, one
// read-back of four integers, until neither count changes.  h_info = iterations, genes left, cells left; it stops where no gene or no cell is left
static int qc_run(const FrontCounts& m, const double* params, uint8_t* h_gene_alive, uint8_t* h_cell_alive, int64_t* h_info, hipStream_t st) {
	const int64_t rows = m.rows, n = m.n;
	DevBuf galive, calive, buf, work;
	NRM_TRY(nrm_take_all(nrm_take_plain, {{&galive, rows}, {&calive, n}, {&buf, (2 * rows + 2 * n + 4) * 8}, {&work, nrm_qc_stats_workspace(rows, n) * 8}}));
	NRM_HIP(hipMemsetAsync(galive.p, 1, (size_t)rows, st));
	NRM_HIP(hipMemsetAsync(calive.p, 1, (size_t)n, st));
	int64_t *gt = buf.as<int64_t>(), *gn = gt + rows, *ct = gt + 2 * rows, *cn = ct + n, *tail = cn + n;  // tail: alive genes, alive cells, negative entry, malformed matrix
	int64_t nt = rows, ns = n, nt0 = 0, ns0 = 0, it = 0;
	while (nt0 != nt || ns0 != ns) {
		nt0 = nt, ns0 = ns, it++;
		if (m.csr)
			NRM_TRY(nrm_qc_csr_stats(m.indptr.as<int64_t>(), m.indices.as<int32_t>(), m.x.p, m.dtype, rows, n, m.nnz, galive.as<uint8_t>(), calive.as<uint8_t>(), gt, gn, ct, cn,
									 tail + 2, work.as<int64_t>(), st));
		else
			NRM_TRY(nrm_qc_stats(m.x.p, m.dtype, rows, n, n, galive.as<uint8_t>(), calive.as<uint8_t>(), gt, gn, ct, cn, tail + 2, work.as<int64_t>(), st));
		int64_t thr[6], h[4];
		nrm_qc_thresholds(params, nt, ns, thr);
		NRM_TRY(nrm_qc_decide(gt, gn, ct, cn, rows, n, thr, galive.as<uint8_t>(), calive.as<uint8_t>(), tail, st));
		NRM_HIP(hipMemcpyAsync(h, tail, sizeof(h), hipMemcpyDeviceToHost, st));  // (the one read-back of an iteration)
		NRM_HIP(hipStreamSynchronize(st));
		NRM_REQUIRE(!h[3], "%s", MALFORMED_CSR);
		NRM_REQUIRE(!h[2], "Negative value in reads detected.");
		nt = h[0], ns = h[1];
		if (nt == 0 || ns == 0) break;  // (qc.py:78-81: the caller raises, genes first)
	}
	h_info[0] = it, h_info[1] = nt, h_info[2] = ns;
	NRM_HIP(hipMemcpy(h_gene_alive, galive.p, (size_t)rows, hipMemcpyDeviceToHost));
	NRM_HIP(hipMemcpy(h_cell_alive, calive.p, (size_t)n, hipMemcpyDeviceToHost));
	return NRM_OK;
}

extern "C" int nrm_qc_reads_host(const void* h_x, int dtype, int64_t rows, int64_t n, double n_gene, double nc_gene, double ncp_gene, double n_cell, double nt_cell,
								 double ntp_cell, uint8_t* h_gene_alive, uint8_t* h_cell_alive, int64_t* h_info) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	const double params[6] = {n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell};
	NRM_TRY(front_check_dense("nrm_qc_reads_host", h_x, dtype, rows, n));
	NRM_TRY(qc_check("nrm_qc_reads_host", params, h_gene_alive, h_cell_alive, h_info));
	NRM_TRY(nrm_bind_device());
	hipStream_t st = nullptr;
	FrontCounts m;
	NRM_TRY(m.dense(h_x, dtype, rows, n, st));
	return qc_run(m, params, h_gene_alive, h_cell_alive, h_info, st);
}

extern "C" int nrm_qc_reads_csr_host(const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int dtype, int64_t rows, int64_t n, int64_t nnz, double n_gene,
									 double nc_gene, double ncp_gene, double n_cell, double nt_cell, double ntp_cell, uint8_t* h_gene_alive, uint8_t* h_cell_alive,
									 int64_t* h_info) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	const double params[6] = {n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell};
	NRM_TRY(front_check_csr("nrm_qc_reads_csr_host", h_indptr, h_indices, h_data, dtype, rows, n, nnz));
	NRM_TRY(qc_check("nrm_qc_reads_csr_host", params, h_gene_alive, h_cell_alive, h_info));
	NRM_TRY(nrm_bind_device());
	hipStream_t st = nullptr;
	FrontCounts m;
	NRM_TRY(m.sparse(h_indptr, h_indices, h_data, dtype, rows, n, nnz, st));
	return qc_run(m, params, h_gene_alive, h_cell_alive, h_info, st);
}
