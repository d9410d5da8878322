// What the whole-problem host entries (numpy buffers in, numpy buffers out; no torch) share: the device scratch pool kept between calls, the
// lock that serialises them per process, a scoped device buffer, the uploads, read-backs and result copies every entry makes.  nrm_api.hip owns the pool
// and the lock and holds the dense single=0 entry; the others are in nrm_host_de.hip (sparse-design and streaming de), nrm_host_single1.hip,
// nrm_host_single4.hip (with nrm_gram_host / nrm_pvalues_host), nrm_host_normvar.hip (with nrm_binnet_host) and nrm_host_front.hip (lcpm, compute_var, qc_reads).
// Their arithmetic is in nrm_host_math.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "nrm_common.h"
#include "nrm_host_logic.h"
#include "nrm_host_math.h"

struct NrmHipAlloc {
	void* alloc(size_t bytes) {
		void* p = nullptr;
		if (hipMalloc(&p, bytes) != hipSuccess) {
			(void)hipGetLastError();
			return nullptr;
		}
		return p;
	}
	void free(void* p) { (void)hipFree(p); }
};
typedef DevPoolT<NrmHipAlloc> NrmDevPool;
NrmDevPool& nrm_host_pool();     // (nrm_api.hip)
std::mutex& nrm_host_entry_mutex();  // one whole-problem call at a time per process (the pool and the default stream are shared)
int nrm_bind_device(void);              // the calling thread onto the device nrm_set_device chose for the process (nrm_api.hip); nothing when none was chosen

struct DevBuf {
	void* p = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { release(); }
	void release() {
		if (p) {
			(void)hipDeviceSynchronize();
			nrm_host_pool().give(p);
			p = nullptr;
		}
	}
	int alloc(size_t bytes) {
		release();
		p = nrm_host_pool().take(bytes ? bytes : 16);
		if (!p) {
			nrm_set_error("hipMalloc of %zu bytes failed", bytes);
			return NRM_E_DEVICE;
		}
		return NRM_OK;
	}
	int alloc_zero(size_t bytes, hipStream_t st) {
		NRM_TRY(alloc(bytes));
		NRM_HIP(hipMemsetAsync(p, 0, bytes, st));
		return NRM_OK;
	}
	template <typename T>
	T* as() const {
		return reinterpret_cast<T*>(p);
	}
};
// the `take` of a step record (nrm_single1_step.h, nrm_de_sparse_step.h, nrm_lcpm_step.h, nrm_fitvar_step.h, nrm_normvar_step.h) for a caller that keeps no count of its pool bytes; a table of buffers through a `take`
static inline int nrm_take_plain(DevBuf& b, size_t bytes) { return b.alloc(bytes); }
template <typename Take>
int nrm_take_all(Take take, std::initializer_list<std::pair<DevBuf*, int64_t>> table) {
	for (const auto& e : table) NRM_TRY(take(*e.first, (size_t)e.second));
	return NRM_OK;
}

// Page-lock of a caller-owned result array for the duration of one call (a pageable device-to-host copy runs at a tenth of the PCIe rate); a
// range that cannot be locked (already registered by the caller, locked-memory limit) is simply copied to at the pageable rate.
struct NrmHostPin {
	void* p = nullptr;
	void try_pin(void* q, int64_t bytes) {
		if (q && bytes >= (1 << 20) && nrm_host_pin(q, bytes, 0) == NRM_OK) p = q;
	}
	~NrmHostPin() {
		if (p) {
			(void)hipDeviceSynchronize();
			(void)hipHostUnregister(p);
		}
	}
};
// joins a helper thread on every way out of the scope
struct NrmJoiner {
	std::thread& t;
	~NrmJoiner() {
		if (t.joinable()) t.join();
	}
};

static inline int64_t nrm_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
static inline size_t nrm_esize(int dtype) { return dtype == NRM_F64 ? 8 : 4; }

// host covariates as fp64 (nc, n), on the host and on the device
static inline int covariates_f64(const void* h_dc, int c_dtype, int64_t nc, int64_t n, std::vector<double>& c64, DevBuf& dc) {
	if (nc <= 0) return NRM_OK;
	nrm_covariates_to_f64(h_dc, c_dtype, (size_t)nc * n, c64);
	NRM_TRY(dc.alloc(c64.size() * 8));
	NRM_HIP(hipMemcpy(dc.p, c64.data(), c64.size() * 8, hipMemcpyHostToDevice));
	return NRM_OK;
}

// (from half a GB up: host threads fill page-locked blocks beside the DMA, nrm_upload.hip)
static inline int upload_matrix(const void* h, int dtype, int64_t rows, int64_t n, DevBuf& d, hipStream_t st) {
	NRM_TRY(d.alloc((size_t)rows * n * nrm_esize(dtype)));
	return nrm_upload(h, d.p, rows * n * (int64_t)nrm_esize(dtype), 0, (void*)st);
}

template <typename T>
static inline int download(std::vector<T>& h, const void* d, size_t count) {
	h.resize(count);
	NRM_HIP(hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost));
	return NRM_OK;
}

// results (rows x cols of out_dtype) device -> the caller's array, page-locked for the copy when it is large
static inline int copy_out(void* h, const void* d, size_t bytes) {
	if (!h || !bytes) return NRM_OK;
	NrmHostPin pin;
	pin.try_pin(h, (int64_t)bytes);
	NRM_HIP(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
	return NRM_OK;
}

// the first N words of an entry's result counters, once everything queued on st is done
template <int N>
static inline int nrm_read_flags(const void* d_flags, hipStream_t st, int32_t (&hf)[N]) {
	NRM_HIP(hipMemcpyAsync(hf, d_flags, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
	NRM_HIP(hipStreamSynchronize(st));
	return NRM_OK;
}

// variances = ss / n with the 0 -> 1 rule (association.py:230-233), cast to the output dtype
static inline int emit_var(const double* d_ss, int64_t cnt, int64_t n, void* h_out, int out_dtype) {
	std::vector<double> hs;
	NRM_TRY(download(hs, d_ss, (size_t)cnt));
	for (double& v : hs) {
		v /= (double)n;
		if (v == 0.0) v = 1.0;
	}
	nrm_store_as(out_dtype, h_out, hs.data(), cnt);
	return NRM_OK;
}

// the same for results that stay in HBM (the resident plans: nrm_coex_plan.hip, nrm_de_plan.hip): stored once as the output dtype
template <typename T>
__global__ void k_plan_var(const double* __restrict__ ss, int64_t cnt, double n, void* __restrict__ out) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= cnt) return;
	double v = ss[i] / n;
	if (v == 0.0) v = 1.0;
	reinterpret_cast<T*>(out)[i] = (T)v;
}

// single=0's result matrices (nx, ny) of out_dtype on the device: P-values and the statistic, r and t on request
struct NrmAssocOut {
	DevBuf p, stat, r, t;
	int alloc(size_t bytes, bool want_r, bool want_t) {
		NRM_TRY(p.alloc(bytes));
		NRM_TRY(stat.alloc(bytes));
		if (want_r) NRM_TRY(r.alloc(bytes));
		if (want_t) NRM_TRY(t.alloc(bytes));
		return NRM_OK;
	}
	int copy_to(void* h_p, void* h_stat, void* h_r, void* h_t, size_t bytes) const {
		NRM_HIP(hipMemcpy(h_p, p.p, bytes, hipMemcpyDeviceToHost));
		NRM_HIP(hipMemcpy(h_stat, stat.p, bytes, hipMemcpyDeviceToHost));
		if (h_r) NRM_HIP(hipMemcpy(h_r, r.p, bytes, hipMemcpyDeviceToHost));
		if (h_t) NRM_HIP(hipMemcpy(h_t, t.p, bytes, hipMemcpyDeviceToHost));
		return NRM_OK;
	}
};

// ---- the launch sequence of dense single=0, shared by nrm_association_tests_host (nrm_api.hip) and the resident coex plan (nrm_coex_plan.hip) ----------------
// K1 of one operand: the integer engine's digit planes, exponents and row records (nslices 5 or 6; the fp64 residuals never stored), or fp64 residual rows
static inline int nrm_assoc_k1(const void* d_x, int x_dtype, int64_t rows, int64_t n, int64_t ldx, const double* d_c, int64_t nc, const double* d_dci, int rank, int64_t kp,
							   int64_t rows_pad, double* d_ss, double* d_coef, int nslices, void* d_q, int32_t* d_exp, const double* d_cmax, double* d_fix, double* d_rows,
							   hipStream_t st) {
	if (nslices)
		return nrm_residualize_q(d_x, x_dtype, rows, n, ldx, d_c, nc, n, d_dci, rank, nullptr, kp, rows_pad, d_ss, d_coef, nslices, d_q, d_exp, 0, nc ? d_cmax : nullptr, d_fix, st);
	return nrm_residualize(d_x, x_dtype, rows, n, ldx, d_c, nc, n, d_dci, rank, d_rows, kp, rows_pad, d_ss, d_coef, st);
}
// what K2 and K3 read and write (samexy: the y side is the x side)
struct NrmAssocOperands {
	const void *qx = nullptr, *qy = nullptr;        // digit planes
	const int32_t *ex = nullptr, *ey = nullptr;     // row exponents
	const double *fx = nullptr, *fy = nullptr;      // row records (csrc/nrm_fix.h)
	const double *rx = nullptr, *ry = nullptr;      // fp64 residual rows (nslices == 0)
	const double *ssx = nullptr, *ssy = nullptr;
	int64_t nx = 0, ny = 0, n = 0, mp = 0, np_ = 0, kp = 0;
	int nslices = 0, samexy = 0, stat_kind = 0, out_dtype = NRM_F64;
	int p_kind = 0;  // the form of p: 0 = P-values, 1 = their logarithms (nrm_assoc_sweep_pk)
	double dof = 0.0, guard_tol = 0.0;
	double* dot = nullptr;
	void* gwork = nullptr;
	int32_t* flags = nullptr;
	void *p = nullptr, *stat = nullptr, *r = nullptr, *t = nullptr;
};
static constexpr int64_t NRM_ASSOC_BAND = 8 * NRM_ROW_TILE;
// K2 -> K3 for the output rows [a, b), a a multiple of NRM_ASSOC_BAND
static inline int nrm_assoc_band(const NrmAssocOperands& o, int64_t a, int64_t b, hipStream_t st) {
	if (o.nslices)
		NRM_TRY(nrm_gram_i8_band(o.qx, o.ex, 0, o.qy, o.ey, 0, o.mp, o.np_, o.kp, o.nslices, o.dot, o.np_, o.samexy, o.nx, o.ny, a, b == o.nx ? o.mp : b, o.gwork, st));
	else
		NRM_TRY(nrm_gram_f64_band(o.rx, o.ry, o.mp, o.np_, o.kp, o.kp, o.kp, o.dot, o.np_, o.samexy, o.nx, o.ny, a, b == o.nx ? o.mp : b, o.gwork, st));
	return nrm_assoc_sweep_band_pk(o.dot, o.np_, o.ssx, o.ssy, o.nx, o.ny, o.n, o.dof, o.samexy, o.stat_kind, o.p, o.stat, o.r, o.t, o.out_dtype, o.ny, o.flags, a, b, o.nslices,
								   o.nslices ? o.fx : nullptr, o.nslices ? o.fy : nullptr, o.guard_tol, o.p_kind, st);
}
// the K2 engine of a dense single=0 problem of n cells: 6 digit planes from 2048 cells (the integer engine's error in r grows as 1 / sqrt(n)) when the rows are
// 16-byte aligned (K1's fused quantiser), NRM_GRAM = i8 | i8x5 | f64 overriding, 0 = the fp64 kernel
static inline int nrm_assoc_engine(int64_t n, bool aligned_rows, int* nslices) {
	*nslices = 6;
	if (n < 2048 || n >= (1 << 22)) *nslices = 0;
	else if (const char* g = getenv("NRM_GRAM")) {
		if (!strcmp(g, "f64")) *nslices = 0;
		else if (!strcmp(g, "i8x5")) *nslices = 5;
		else NRM_REQUIRE(!strcmp(g, "i8"), "NRM_GRAM must be i8, i8x5 or f64");
	}
	if (*nslices && !aligned_rows) *nslices = 0;
	return NRM_OK;
}
static inline double nrm_guard_tolerance() {
	const char* t = getenv("NRM_I8_GUARD_TOL");  // largest relative change of a P-value the integer engine may cause (0: no guard)
	return t ? atof(t) : 2.5e-7;
}
// (the checks of association.py:199-216 on a dense single=0 call: nrm_assoc_check_args, nrm_host_logic.h)
// max |C_c| per covariate row (K1's bound on the residuals it quantises) and the pseudo-inverse, uploaded
static inline int covariate_bounds(const std::vector<double>& c64, int64_t nc, int64_t n, const double* h_dci, int rank, DevBuf& cmax, DevBuf& dci) {
	if (nc <= 0) return NRM_OK;
	std::vector<double> cm((size_t)nc, 0.0);
	for (int64_t c = 0; c < nc; c++)
		for (int64_t k = 0; k < n; k++) cm[(size_t)c] = std::max(cm[(size_t)c], std::fabs(c64[(size_t)(c * n + k)]));
	NRM_TRY(cmax.alloc((size_t)nc * 8));
	NRM_HIP(hipMemcpy(cmax.p, cm.data(), (size_t)nc * 8, hipMemcpyHostToDevice));
	NRM_TRY(dci.alloc((size_t)nc * nc * 8));
	NRM_REQUIRE(h_dci != nullptr || rank == 0, "Unmatching dci dimensions.");
	if (h_dci) NRM_HIP(hipMemcpy(dci.p, h_dci, (size_t)nc * nc * 8, hipMemcpyHostToDevice));
	return NRM_OK;
}

// Does a call of this size take the sparse-design kernels, if its design then turns out to have few entries (a CRISPR screen's gRNA incidence)?  Same size
// rule as normalisr_amd.engine; NRM_DE_SPARSE=0 switches it off, =force takes it whatever the size.
static inline bool nrm_de_sparse_wanted(int64_t nx, int64_t ny, int64_t n, int64_t nc) {
	const char* mode = getenv("NRM_DE_SPARSE");
	const bool off = mode && !strcmp(mode, "0"), force = mode && !strcmp(mode, "force");
	return !off && nc <= nrm_de_sparse_max_covariates() && (force || (nx >= 32 && ny >= 64 && n >= 2048 && nx * n >= (1ll << 22)));
}

// The design matrix (already in HBM) as the lists of csrc/nrm_design_lists.hip: CSR always, ELL on request.  ok: 0 < entries <= max_density nx n.
struct NrmDesignLists {
	DevBuf cnt, coff, info, row_ptr, slot2x, sig, pos, w, base, cells, row_vals, ell, ellv;
	int64_t nnz = 0, padded = 0, nslots = 0, ngroups = 0, nch = 0;
	int bits = 0;
	bool binary = true, ok = false;
	int build(const void* d_x, int x_dtype, int64_t nx, int64_t n, bool want_ell, double max_density, hipStream_t st);
};

// x~ . y~ for every (design row, expression row) through the sparse-design kernels (nrm_host_de.hip): d_dot (nxp, nyp) or, by_gene, (nyp, nxp); the rows' sums
// with the covariates inside the kernel for up to nrm_de_sparse_fused_covariates() of them, by the stream kernel of single=1 otherwise
int sparse_products(const NrmDesignLists& L, const void* d_y, int y_dtype, int64_t ny, int64_t n, const double* d_c, int64_t ncu, int ci, double cval, const double* d_dci,
					const double* d_bx, int64_t ldb, double* d_dot, int64_t ldd, int by_gene, double* d_ssy, double* d_coefy, int32_t* d_flags, hipStream_t st);
// the sparse-design form of single=0 de inside nrm_association_tests_host (nrm_host_de.hip); *taken = 0: the design does not qualify
// (dense, or empty) and nothing was written; *handed_back = rows too close to the span of the covariates (the caller runs the dense fp64 path)
int nrm_host_de_sparse(const void* d_x, int x_dtype, int64_t nx, const void* d_y, int y_dtype, int64_t ny, const double* d_c, const double* h_c64, int64_t nc, int64_t n,
					   const double* d_dci, int rank, double dof, int stat_kind, void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary, void* h_r, void* h_t,
					   int out_dtype, int* taken, int64_t* handed_back, int p_kind = 0);
// de with nx + nc <= 32: the streaming kernel (nrm_host_de.hip); d_x in HBM, h_dy uploaded inside
int nrm_host_de_streaming(const void* d_x, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const double* h_c64, int64_t nc, int64_t n,
						  const double* h_dci, int rank, double dof, int stat_kind, void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary, void* h_r, void* h_t,
						  int out_dtype, int p_kind = 0);
