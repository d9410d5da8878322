// Resident front-half plan behind the C ABI (include/normalisr_hip.h: nrm_front_plan_*): read counts resident in HBM in, (dtn, dcn) in HBM out -- the chain
// lcpm -> normcov -> compute_var -> scaling_factor -> normvar of the reference (lcpm.py:21-283, norm.py:4-128,166-289) with its default options, as ONE enqueue on
// ONE stream, and from the second step on one hipGraphLaunch (nrm_plan_core.h).  numpy and the library are all a caller needs: no torch.
//
// The large passes are the step records that the whole-problem entries fill per call and the plan keeps as members: NrmLcpmPasses (nrm_lcpm_step.h: count / colsum /
// write), NrmFitvarStep (nrm_fitvar_step.h: compute_var's whole sequence) and NrmNormvarStep (nrm_normvar_step.h: solve, then rescale and apply).  Each holds its
// sizes, its buffers and its launches once, for nrm_lcpm_host, nrm_compute_var_host, nrm_normvar_host and this plan alike.  What the host does between them in the
// entries is here as small kernels that read their operands from device memory, so that no launch argument of a step depends on the data and a captured graph stays
// valid when the counts are rewritten:
//   k_front_scalars  ONE workgroup: t0 = sum + 2 (or ntot + 2), len = max + 1 (clamped to the cap), the counters of lcpm's refusals
//   k_front_tables   tab[x] = psi(1 + x) - psi(t0), etab[x] = exp(tab[x]) for x < len; a thread per entry of the cap, every entry on its own (nrm_digamma.h)
//   k_front_unit     CSR counts only: the largest (etab[x] - etab[0]) / x of the table just written, the bound of the CSR column sum's fixed point
//   k_front_cov      a workgroup per covariate row: lcpm's three rows from the integer totals, then normcov on [user rows; those three], the ones row appended
//   k_front_m2i      ONE workgroup: ([dc;1][dc;1]^T)^+ on unit-length rows by the lane Jacobi of nrm_jacobi_lanes.h (nrm_pinv_gram_unit_rows of the host entries)
//   k_front_scale    ln w, and wt = (zeros / cells) / max_g (zeros / cells): scaling_factor's default variable rescaled with v0 = 0, v1 = 'max'
//   k_front_dcn      normvar's scaled covariates: continuous rows and the ones row times w (norm.py:261-273 with cat = 1)
// Sums over cells are per-thread partial sums in a fixed stride, added by the shuffle tree and the waves in their order: no floating-point atomics, the same bits
// every run, eager or replayed.  Counters are integers.
// On CSR counts (nrm_front_plan_create_csr) the step is the same with the CSR form of lcpm's three passes: their two data-dependent scalars -- the number of stored
// entries and the unit -- are read on the device (nrm_lcpm_step.h: d_unit), so the graph survives a rewrite of the matrix, its pattern included.
#include <memory>
#include "nrm_device.h"
#include "nrm_digamma.h"
#include "nrm_fitvar_step.h"
#include "nrm_front_plan_args.h"
#include "nrm_host_entry.h"
#include "nrm_jacobi_lanes.h"
#include "nrm_lcpm_step.h"
#include "nrm_normvar_step.h"
#include "nrm_plan_core.h"

#define FP_M2_THREADS 1024
#define FP_FLAGS 16  // [0] negative entry, [1] a cell without a read, [2] no read at all, [3] max >= cap, [4] constant covariate rows, [5] near-constant rows,
					 // [6] scaling_factor, [7] 0, [8..11] compute_var's counters, [12..15] normvar's

static_assert(NRM_FRONT_M2_ROWS * NRM_FRONT_M2_ROWS * 8 * 3 < 32768, "k_front_m2i keeps three square matrices in LDS");

// fs[0] = t0, fs[1] = len (as a double: below 2^24), fs[2] = 0: the unit, cleared for k_front_unit; big[0] = the largest count of a step whose maximum reached
// the cap, big[1] = steps whose CSR matrix was malformed (the count pass's info[3]), big[2] = this step's largest count
__global__ void __launch_bounds__(256) k_front_scalars(const int64_t* __restrict__ info, const int64_t* __restrict__ cell_total, int64_t n, int64_t ntot, int64_t cap,
														double* __restrict__ fs, int32_t* __restrict__ flags, int64_t* __restrict__ big) {
	__shared__ int sm[4];
	int empty = 0;
	for (int64_t k = threadIdx.x; k < n; k += 256) empty += cell_total[k] <= 0;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) empty += __shfl_down(empty, o, 64);
	if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = empty;
	__syncthreads();
	if (threadIdx.x != 0) return;
	empty = (sm[0] + sm[1]) + (sm[2] + sm[3]);
	const int64_t sum = info[0], mx = info[1];
	const double t0 = ntot < 0 ? (double)(sum + 2) : (double)ntot + 2.0;
	const bool over = mx >= cap;
	fs[0] = t0;
	fs[1] = (double)(over ? cap : mx + 1);
	fs[2] = 0.0;
	// (one thread of one workgroup on one stream: nobody else writes these words while a step runs)
	if (info[3]) big[1] += 1;
	if (info[2]) flags[0] += 1;
	if (empty) flags[1] += 1;
	if (!(t0 > 2.0)) flags[2] += 1;
	if (over) {
		flags[3] += 1;
		if (mx > big[0]) big[0] = mx;
	}
	big[2] = mx;
}

__global__ void __launch_bounds__(256) k_front_tables(const double* __restrict__ fs, int64_t cap, double* __restrict__ tab, double* __restrict__ etab) {
	const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x, len = (int64_t)fs[1];
	if (x >= len || x >= cap) return;
	const double t = nrm_digamma(1.0 + (double)x) - nrm_digamma(fs[0]);  // (a t0 that is not positive -- negative entries -- gives NaN; the step is refused by its counter)
	tab[x] = t;
	etab[x] = exp(t);
}

// unit = max over 1 <= x < len of (etab[x] - etab[0]) / x (nrm_lcpm_tables, nrm_host_math.h), from the device's own table: total_k * unit bounds the terms
// etab[x] - etab[0] that nrm_lcpm_csr_colsum adds for cell k.  Non-negative doubles order as their bit patterns: an integer maximum, whatever the order of the
// workgroups.  A quotient that is not a positive number (a NaN table: negative entries, refused by their counter) is left out.  k_front_scalars cleared the word.
__global__ void __launch_bounds__(256) k_front_unit(const double* fs, int64_t cap, const double* __restrict__ etab, unsigned long long* unit_bits) {
	const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x, len = (int64_t)fs[1];
	double u = 0.0;
	if (x >= 1 && x < len && x < cap) {
		const double q = (etab[x] - etab[0]) / (double)x;
		u = q > 0.0 ? q : 0.0;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const double t = __shfl_xor(u, o, 64);
		u = t > u ? t : u;
	}
	if ((threadIdx.x & 63) == 0 && u > 0.0) atomicMax(unit_bits, (unsigned long long)__double_as_longlong(u));
}

// dc (nct, n): row r < n_cov the user's, the next three lcpm's, the last all ones.  cls[r] = the row's class (nrm_front_plan_args.h).
__global__ void __launch_bounds__(256) k_front_cov(const double* __restrict__ user, int n_cov, const int64_t* __restrict__ cell_total, const int64_t* __restrict__ cell_nnz,
													int64_t genes, int64_t n, int nct, double* __restrict__ dc, int32_t* __restrict__ cls, int32_t* __restrict__ flags) {
	__shared__ double sm[4];
	const int r = blockIdx.x, tid = threadIdx.x;
	double* __restrict__ out = dc + (int64_t)r * n;
	if (r == nct - 1) {
		for (int64_t k = tid; k < n; k += 256) out[k] = 1.0;
		if (tid == 0) cls[r] = NRM_COV_ONES;
		return;
	}
	// the raw row, kept in `out`: every thread reads back only what it wrote itself
	const int j = r - n_cov;
	double first = 0.0;
	{
		if (j < 0) first = user[(int64_t)r * n];
		else {
			const double t = log((double)cell_total[0]);  // lcpm.py:194-200 (a cell without a read: -inf or NaN, and the step is refused by its counter)
			first = j == 0 ? t : j == 1 ? (double)(genes - cell_nnz[0]) : t * t;
		}
	}
	int cont = 0, differs = 0;
	double s = 0.0;
	for (int64_t k = tid; k < n; k += 256) {
		double v;
		if (j < 0) v = user[(int64_t)r * n + k];
		else {
			const double t = log((double)cell_total[k]);
			v = j == 0 ? t : j == 1 ? (double)(genes - cell_nnz[k]) : t * t;
		}
		out[k] = v;
		cont |= v != 0.0 && v != 1.0;
		differs |= !(v == first);
		s += v;
	}
	cont = __syncthreads_or(cont);
	differs = __syncthreads_or(differs);
	if (!differs && tid == 0) atomicAdd(&flags[4], 1);  // norm.py:34-37 (the values are still written: nothing downstream reads past a buffer for them)
	if (!cont) {
		if (tid == 0) cls[r] = NRM_COV_BINARY;
		return;
	}
	const double mean = nrm_block_sum<4>(s, sm) / (double)n;  // norm.py:41
	double q = 0.0;
	for (int64_t k = tid; k < n; k += 256) {
		const double d = out[k] - mean;
		q += d * d;
	}
	const double sd = sqrt(nrm_block_sum<4>(q, sm) / (double)n);  // norm.py:43
	if (tid == 0) {
		cls[r] = NRM_COV_CONTINUOUS;
		if (sd < 1e-50 || fabs(sd / mean) < 1e-6) atomicAdd(&flags[5], 1);  // norm.py:44-47: a warning
	}
	for (int64_t k = tid; k < n; k += 256) out[k] = (out[k] - mean) / sd;  // norm.py:42,48
}

struct FrontWorkgroup {
	__device__ int lane() const { return threadIdx.x; }
	__device__ int lanes() const { return blockDim.x; }
	__device__ void sync() const { __syncthreads(); }
};

// m2i (r, r), r = nc + 1: the pseudo-inverse of x x^T for x = [dc; 1] on rows scaled to unit length, D pinv(D x x^T D) D (nrm_pinv_gram_unit_rows, nrm_host_math.h).
// A wave owns a row's norm, then a pair's product: lanes stride the cells, the shuffle tree adds them -- a fixed order.
__global__ void __launch_bounds__(FP_M2_THREADS) k_front_m2i(const double* __restrict__ dc, int nc, int64_t n, double tol, double* __restrict__ m2i) {
	__shared__ double a[NRM_FRONT_M2_ROWS * NRM_FRONT_M2_ROWS], v[NRM_FRONT_M2_ROWS * NRM_FRONT_M2_ROWS], inv[NRM_FRONT_M2_ROWS * NRM_FRONT_M2_ROWS];
	__shared__ double w[NRM_FRONT_M2_ROWS], red[2 * NRM_FRONT_M2_ROWS], d[NRM_FRONT_M2_ROWS];
	__shared__ int64_t rank;
	const int r = nc + 1, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = FP_M2_THREADS / 64;
	for (int i = wid; i < r; i += nw) {
		double s = 0.0;
		for (int64_t k = lane; k < n; k += 64) {
			const double x = i < nc ? dc[(int64_t)i * n + k] : 1.0;
			s = fma(x, x, s);
		}
		s = nrm_wave_sum(s);
		if (lane == 0) {
			s = sqrt(s);
			d[i] = 1.0 / (s > 0 ? s : 1.0);
		}
	}
	__syncthreads();
	const int npair = r * (r + 1) / 2;
	for (int p = wid; p < npair; p += nw) {
		int i = 0, q = p;
		while (q >= r - i) q -= r - i, i++;  // pair p of the upper triangle, row by row: (i, j >= i)
		const int j = i + q;
		const double di = d[i], dj = d[j];
		double s = 0.0;
		for (int64_t k = lane; k < n; k += 64) {
			const double xi = i < nc ? dc[(int64_t)i * n + k] : 1.0, xj = j < nc ? dc[(int64_t)j * n + k] : 1.0;
			s = fma(xi * di, xj * dj, s);
		}
		s = nrm_wave_sum(s);
		if (lane == 0) a[i * r + j] = a[j * r + i] = s;
	}
	__syncthreads();
	nrm_pinv_lanes(FrontWorkgroup(), a, v, w, red, r, tol, inv, &rank);
	__syncthreads();
	for (int e = threadIdx.x; e < r * r; e += FP_M2_THREADS) m2i[e] = inv[e] * (d[e / r] * d[e % r]);
}

// lnw = ln w (normvar's operand); wt = (zeros / cells - 0) / (max_g - 0) (lcpm.py:258,268-283 with v0 = 0, v1 = 'max').  Every workgroup takes the maximum of
// the integer zero counts for itself: exact, whatever the order.
__global__ void __launch_bounds__(256) k_front_scale(const double* __restrict__ w, int64_t n, const int64_t* __restrict__ gene_zero, int64_t genes, double* __restrict__ lnw,
													  double* __restrict__ wt, int32_t* __restrict__ flags) {
	__shared__ int64_t sm[4];
	int64_t mx = 0;
	for (int64_t g = threadIdx.x; g < genes; g += 256) mx = gene_zero[g] > mx ? gene_zero[g] : mx;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const int64_t t = __shfl_xor(mx, o, 64);
		mx = t > mx ? t : mx;
	}
	if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
	__syncthreads();
	for (int i = 0; i < 4; i++) mx = sm[i] > mx ? sm[i] : mx;
	const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
	int bad = 0;
	if (k < n) {
		const double l = log(w[k]);
		lnw[k] = l;
		bad += !(fabs(l) <= 1.7976931348623157e308);
	}
	if (k < genes) {
		const double t = ((double)gene_zero[k] / (double)n - 0.0) / ((double)mx / (double)n - 0.0);
		wt[k] = t;
		bad += !(fabs(t) <= 1.7976931348623157e308);
	}
	if (blockIdx.x == 0 && threadIdx.x == 0 && mx == 0) bad++;  // lcpm.py:278: v1 != v0
	if (bad) atomicAdd(&flags[6], bad);
}

__global__ void __launch_bounds__(256) k_front_dcn(const double* __restrict__ dc, const int32_t* __restrict__ cls, const double* __restrict__ w, int64_t n,
													double* __restrict__ dcn) {
	const int r = blockIdx.y;
	const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const double v = dc[(int64_t)r * n + k];
	dcn[(int64_t)r * n + k] = cls[r] != NRM_COV_BINARY ? v * w[k] : v;  // norm.py:261-273, cat = 1
}

struct nrm_front_plan : NrmPlanCore {
	int64_t rows = 0, n = 0, n_cov = 0, nct = 0, ntot = -1, cap = 0;
	int out_dtype = NRM_F64;
	bool adopted = false, csr = false;
	int64_t nnz_cap = 0;  // CSR: elements the indices and values hold (the plan's own, or the adopted arrays')
	// the three stages that the whole-problem entries run too, as their step records; around them what is the plan's own:
	// the counts and lcpm's scalars, tables and result | the covariates | scaling_factor's operands and normvar's result
	NrmLcpmPasses lc;
	NrmFitvarStep fit;
	NrmNormvarStep nv;
	DevBuf own_x, own_indptr, own_indices, fs, big, flags, tab, etab, t1, lcpm;  // own_x: the dense matrix, or the CSR values
	DevBuf user, dc, dcn, cls, m2i;
	DevBuf lnw, wt, dtn;
	int64_t cv_steps = 0, max_count = 0, warned = 0;
	~nrm_front_plan() { shutdown(); }  // (its body runs before the DevBuf members go back to the pool: NrmPlanCore::shutdown)
};

namespace {

int plan_enqueue(nrm_front_plan* pl, hipStream_t st) {
	const int64_t rows = pl->rows, n = pl->n, nc = pl->nct;
	int32_t* flags = pl->flags.as<int32_t>();
	NrmLcpmPasses& lc = pl->lc;
	// lcpm: count, the scalars and the tables on the device, colsum, write
	NRM_TRY(lc.clear(st));  // (the gene zero counts are integer atomics)
	NRM_TRY(lc.count(st));
	hipLaunchKernelGGL(k_front_scalars, dim3(1), dim3(256), 0, st, lc.info(), lc.total(), n, pl->ntot, pl->cap, pl->fs.as<double>(), flags, pl->big.as<int64_t>());
	NRM_TRY(nrm_check_launch("k_front_scalars"));
	hipLaunchKernelGGL(k_front_tables, dim3((unsigned)((pl->cap + 255) / 256)), dim3(256), 0, st, pl->fs.as<double>(), pl->cap, pl->tab.as<double>(), pl->etab.as<double>());
	NRM_TRY(nrm_check_launch("k_front_tables"));
	if (pl->csr) {
		hipLaunchKernelGGL(k_front_unit, dim3((unsigned)((pl->cap + 255) / 256)), dim3(256), 0, st, pl->fs.as<double>(), pl->cap, pl->etab.as<double>(), pl->fs.as<unsigned long long>() + 2);
		NRM_TRY(nrm_check_launch("k_front_unit"));
	}
	NRM_TRY(lc.colsum(pl->etab.as<double>(), pl->cap, 0.0, pl->t1.as<double>(), st));  // (the unit by value is not read: the CSR form takes lc.d_unit = fs + 2)
	NRM_TRY(lc.write(pl->tab.as<double>(), pl->cap, pl->t1.as<double>(), pl->lcpm.p, pl->out_dtype, n, st));
	// lcpm's covariate rows, normcov, the pseudo-inverse of the second regression
	double* c = pl->dc.as<double>();
	hipLaunchKernelGGL(k_front_cov, dim3((unsigned)nc), dim3(256), 0, st, pl->user.as<double>(), (int)pl->n_cov, lc.total(), lc.nnz(), rows, n, (int)nc, c, pl->cls.as<int32_t>(), flags);
	NRM_TRY(nrm_check_launch("k_front_cov"));
	hipLaunchKernelGGL(k_front_m2i, dim3(1), dim3(FP_M2_THREADS), 0, st, c, (int)nc, n, 1e-8, pl->m2i.as<double>());
	NRM_TRY(nrm_check_launch("k_front_m2i"));
	// compute_var on lcpm in HBM
	NRM_TRY(pl->fit.enqueue(st));
	// scaling_factor's rescale, ln w, the scaled covariates
	const unsigned blocks = (unsigned)((std::max(n, rows) + 255) / 256);
	hipLaunchKernelGGL(k_front_scale, dim3(blocks), dim3(256), 0, st, pl->fit.w(), n, lc.zero(), rows, pl->lnw.as<double>(), pl->wt.as<double>(), flags);
	NRM_TRY(nrm_check_launch("k_front_scale"));
	hipLaunchKernelGGL(k_front_dcn, dim3((unsigned)((n + 255) / 256), (unsigned)nc), dim3(256), 0, st, c, pl->cls.as<int32_t>(), pl->fit.w(), n, pl->dcn.as<double>());
	NRM_TRY(nrm_check_launch("k_front_dcn"));
	// normvar: lcpm, ln w and the genes' exponents in, dtn out
	NRM_TRY(pl->nv.solve(st));
	return pl->nv.finish(st);
}

int plan_bind(nrm_front_plan* pl, const char* who) {
	NRM_REQUIRE(pl != nullptr, "%s: null plan", who);
	NRM_HIP(hipSetDevice(pl->device));
	return NRM_OK;
}

int plan_upload(nrm_front_plan* pl, const char* who, const void* h_reads) {
	NRM_REQUIRE(!pl->csr, "%s: the plan holds CSR counts (nrm_front_plan_upload_csr)", who);
	return nrm_plan_upload(*pl, who, pl->adopted, h_reads, pl->own_x.p, pl->rows * pl->n * (int64_t)nrm_count_elem(pl->lc.dtype));
}

// the three arrays into the plan's own; entries past nnz keep what they held, and no step reads them (the count is indptr[rows])
int plan_upload_csr(nrm_front_plan* pl, const char* who, const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int64_t nnz) {
	NRM_TRY(nrm_front_plan_upload_csr_args(pl->csr, pl->adopted, pl->rows, pl->nnz_cap, h_indptr, h_indices, h_data, nnz));  // every check: before any copy
	NRM_TRY(nrm_plan_upload(*pl, who, false, h_indptr, pl->own_indptr.p, (pl->rows + 1) * 8));
	if (nnz == 0) return NRM_OK;
	NRM_TRY(nrm_plan_upload(*pl, who, false, h_indices, pl->own_indices.p, nnz * 4));
	return nrm_plan_upload(*pl, who, false, h_data, pl->own_x.p, nnz * (int64_t)nrm_count_elem(pl->lc.dtype));
}

// waits, reads every counter once, clears them; caller holds nrm_host_entry_mutex
int plan_check(nrm_front_plan* pl, int64_t* near_constant) {
	hipStream_t st = pl->last ? pl->last : pl->own;
	if (near_constant) *near_constant = 0;
	int32_t hf[FP_FLAGS];
	int64_t hb[3] = {0, 0, 0};
	double hs[4] = {0, 0, 0, 0};
	NRM_HIP(hipDeviceSynchronize());  // (steps may have gone to several streams since the last check)
	NRM_TRY(nrm_read_flags(pl->flags.p, st, hf));
	NRM_HIP(hipMemcpyAsync(hb, pl->big.p, sizeof(hb), hipMemcpyDeviceToHost, st));
	NRM_HIP(hipMemcpyAsync(hs, pl->fit.state() + 4 * pl->fit.stepmax, sizeof(hs), hipMemcpyDeviceToHost, st));
	NRM_TRY(nrm_fill_zero(pl->flags.p, FP_FLAGS * 4, (void*)st));
	NRM_TRY(nrm_fill_zero(pl->big.p, 16, (void*)st));  // (big[2], the last step's maximum, stays: a second check reports it again)
	NRM_HIP(hipStreamSynchronize(st));
	if (pl->steps > 0) pl->cv_steps = (int64_t)hs[1], pl->max_count = hb[2];
	pl->warned = hf[5];
	if (near_constant) *near_constant = hf[5];
	return nrm_front_plan_status_csr(hb[1], hf, pl->cap, hb[0]);
}

}  // namespace

// the plan of checked arguments: the buffers, the three step records, the covariates and -- for counts of its own -- the first upload
static int plan_build(nrm_front_plan** plan, const NrmFrontPlanArgs& a, const char* who) {
	NRM_REQUIRE(nrm_lcpm_row_tile() == 32 && nrm_fitvar_row_tile() == 32, "%s: the row tiles have changed (NRM_FRONT_MAX_ROWS)", who);
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	std::unique_ptr<nrm_front_plan> pl(new nrm_front_plan);
	NRM_HIP(hipGetDevice(&pl->device));
	const int64_t rows = a.rows, n = a.n, n_cov = a.n_cov, nc = n_cov + NRM_FRONT_LCPM_ROWS + 1, es = (int64_t)nrm_esize(a.out_dtype), count_cap = a.count_cap;
	nrm_front_plan* p = pl.get();
	p->rows = rows, p->n = n, p->n_cov = n_cov, p->nct = nc, p->ntot = a.ntot < 0 ? -1 : a.ntot, p->cap = count_cap, p->out_dtype = a.out_dtype, p->adopted = a.on_device != 0;
	p->csr = a.csr != 0, p->nnz_cap = a.nnz_cap;
	NRM_HIP(hipStreamCreateWithFlags(&p->own, hipStreamNonBlocking));
	auto take = [p](DevBuf& b, size_t bytes) { return p->take(b, bytes); };
	// the counts: a dense matrix, or three arrays of the capacity -- never a (rows, n) matrix for CSR counts
	if (!p->adopted && !p->csr) NRM_TRY(take(p->own_x, (size_t)(rows * n) * nrm_count_elem(a.dtype)));
	if (!p->adopted && p->csr)
		NRM_TRY(nrm_take_all(take, {{&p->own_indptr, (rows + 1) * 8}, {&p->own_indices, a.nnz_cap * 4}, {&p->own_x, a.nnz_cap * (int64_t)nrm_count_elem(a.dtype)}}));
	NRM_TRY(take(p->fs, 32));  // (in front of lc.alloc: the CSR passes read their unit from fs + 2)
	// lcpm | the covariates | compute_var | normvar: each record sizes its own buffers, the plan what lies between them
	NrmLcpmPasses& lc = p->lc;
	lc.rows = rows, lc.n = n, lc.dtype = a.dtype, lc.d_x = p->adopted ? a.reads : p->own_x.p, lc.ld = a.ld;
	if (p->csr) {
		lc.csr = true, lc.stored = a.nnz_cap, lc.d_unit = p->fs.as<double>() + 2;
		lc.d_indptr = p->adopted ? a.indptr : p->own_indptr.as<int64_t>(), lc.d_indices = p->adopted ? a.indices : p->own_indices.as<int32_t>();
	}
	NRM_TRY(lc.alloc(take));
	NRM_TRY(nrm_take_all(take, {{&p->big, 24}, {&p->flags, FP_FLAGS * 4}, {&p->tab, count_cap * 8}, {&p->etab, count_cap * 8}, {&p->t1, n * 8}, {&p->lcpm, rows * n * es},
								{&p->user, std::max<int64_t>(n_cov * n, 1) * 8}, {&p->dc, nc * n * 8}, {&p->dcn, nc * n * 8}, {&p->cls, nc * 4}, {&p->m2i, (nc + 1) * (nc + 1) * 8}}));
	NrmFitvarStep& fit = p->fit;
	fit.rows = rows, fit.n = n, fit.ldy = n, fit.nc = nc, fit.stepmax = a.stepmax, fit.eps = a.eps, fit.y_dtype = a.out_dtype;
	fit.d_y = p->lcpm.p, fit.d_c = p->dc.as<double>(), fit.d_m2i = p->m2i.as<double>(), fit.flags = p->flags.as<int32_t>() + 8;
	NRM_TRY(fit.alloc(take));
	NRM_TRY(nrm_take_all(take, {{&p->lnw, n * 8}, {&p->wt, rows * 8}}));
	NrmNormvarStep& nv = p->nv;
	nv.rows = rows, nv.n = n, nv.ldy = n, nv.nc = nc, nv.ldo = n, nv.tol = a.tol, nv.keepvar = 1, nv.y_dtype = nv.out_dtype = a.out_dtype;
	nv.d_y = p->lcpm.p, nv.d_lnw = p->lnw.as<double>(), nv.d_wt = p->wt.as<double>(), nv.d_c = p->dc.as<double>(), nv.flags = p->flags.as<int32_t>() + 12;
	NRM_TRY(nv.alloc(take));
	NRM_TRY(take(p->dtn, (size_t)(rows * n * es)));
	nv.d_out = p->dtn.p;
	NRM_TRY(nrm_fill_zero(p->flags.p, FP_FLAGS * 4, (void*)p->own));
	NRM_TRY(nrm_fill_zero(p->big.p, 24, (void*)p->own));
	NRM_TRY(nrm_fill_zero(p->fs.p, 32, (void*)p->own));
	NRM_TRY(nrm_fill_zero(p->tab.p, count_cap * 8, (void*)p->own));  // (entries past the largest count are never indexed; they are zero, not whatever the pool held)
	NRM_TRY(nrm_fill_zero(p->etab.p, count_cap * 8, (void*)p->own));
	NRM_TRY(nrm_fill_zero(fit.out.p, fit.out_doubles() * 8, (void*)p->own));
	if (n_cov > 0) NRM_HIP(hipMemcpyAsync(p->user.p, a.h_cov, (size_t)(n_cov * n) * 8, hipMemcpyHostToDevice, p->own));
	NRM_HIP(hipStreamSynchronize(p->own));
	if (p->adopted)
		NRM_HIP(hipDeviceSynchronize());  // (whatever the caller queued to fill its matrix is through before the first step reads it)
	else if (p->csr)
		NRM_TRY(plan_upload_csr(p, who, a.indptr, a.indices, a.reads, a.nnz));
	else
		NRM_TRY(plan_upload(p, who, a.reads));
	*plan = pl.release();
	return NRM_OK;
}

static void plan_options(NrmFrontPlanArgs& a, const double* h_cov, int64_t n_cov, int64_t ntot, int64_t stepmax, double eps, double tol, int out_dtype, int64_t count_cap) {
	a.h_cov = h_cov, a.n_cov = n_cov, a.ntot = ntot, a.stepmax = stepmax, a.eps = eps, a.tol = tol, a.out_dtype = out_dtype, a.count_cap = count_cap;
}

extern "C" int nrm_front_plan_create(nrm_front_plan** plan, const void* reads, int dtype, int64_t genes, int64_t n_cells, int64_t ld, int reads_on_device, const double* h_cov,
									 int64_t n_cov, int64_t ntot, int64_t stepmax, double eps, double tol, int out_dtype, int64_t count_cap) {
	NRM_REQUIRE(plan != nullptr, "nrm_front_plan_create: null plan pointer");
	*plan = nullptr;
	NrmFrontPlanArgs a;
	a.reads = reads, a.dtype = dtype, a.rows = genes, a.n = n_cells, a.ld = ld ? ld : n_cells, a.on_device = reads_on_device;
	plan_options(a, h_cov, n_cov, ntot, stepmax, eps, tol, out_dtype, count_cap);
	NRM_TRY(nrm_front_plan_create_args(a, nrm_normvar_device_covariates(), nrm_lcpm_table_cap()));  // every check: before any device call
	return plan_build(plan, a, "nrm_front_plan_create");
}

extern "C" int nrm_front_plan_create_csr(nrm_front_plan** plan, const int64_t* indptr, const int32_t* indices, const void* data, int dtype, int64_t genes, int64_t n_cells,
										 int64_t nnz, int64_t nnz_cap, int on_device, const double* h_cov, int64_t n_cov, int64_t ntot, int64_t stepmax, double eps, double tol,
										 int out_dtype, int64_t count_cap) {
	NRM_REQUIRE(plan != nullptr, "nrm_front_plan_create_csr: null plan pointer");
	*plan = nullptr;
	NrmFrontPlanArgs a;
	a.csr = 1, a.indptr = indptr, a.indices = indices, a.reads = data, a.nnz = nnz, a.nnz_cap = nnz_cap;
	a.dtype = dtype, a.rows = genes, a.n = n_cells, a.ld = n_cells, a.on_device = on_device;
	plan_options(a, h_cov, n_cov, ntot, stepmax, eps, tol, out_dtype, count_cap);
	NRM_TRY(nrm_front_plan_create_csr_args(a, nrm_normvar_device_covariates(), nrm_lcpm_table_cap()));  // every check: before any device call
	return plan_build(plan, a, "nrm_front_plan_create_csr");
}

extern "C" int nrm_front_plan_upload(nrm_front_plan* plan, const void* h_reads) {
	NRM_TRY(plan_bind(plan, "nrm_front_plan_upload"));
	return plan_upload(plan, "nrm_front_plan_upload", h_reads);
}

extern "C" int nrm_front_plan_upload_csr(nrm_front_plan* plan, const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int64_t nnz) {
	NRM_TRY(plan_bind(plan, "nrm_front_plan_upload_csr"));
	return plan_upload_csr(plan, "nrm_front_plan_upload_csr", h_indptr, h_indices, h_data, nnz);
}

extern "C" int nrm_front_plan_step(nrm_front_plan* plan, void* stream) {
	NRM_TRY(plan_bind(plan, "nrm_front_plan_step"));
	return nrm_plan_step(*plan, "nrm_front_plan_step", stream, [plan](hipStream_t st) { return plan_enqueue(plan, st); });
}

extern "C" int nrm_front_plan_check(nrm_front_plan* plan, int64_t* near_constant) {
	NRM_REQUIRE(plan != nullptr, "nrm_front_plan_check: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_front_plan_check"));
	return plan_check(plan, near_constant);
}

extern "C" int nrm_front_plan_results(nrm_front_plan* plan, void* h_dtn, double* h_dcn, double* h_w, double* h_wt, void* h_lcpm, double* h_cov) {
	NRM_REQUIRE(plan != nullptr, "nrm_front_plan_results: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_front_plan_results"));
	NRM_REQUIRE(plan->steps > 0, "nrm_front_plan_results: no step has run");
	NRM_TRY(plan_check(plan, nullptr));
	const size_t mb = (size_t)(plan->rows * plan->n) * nrm_esize(plan->out_dtype), cb = (size_t)(plan->nct * plan->n) * 8;
	NRM_TRY(copy_out(h_dtn, plan->dtn.p, mb));
	NRM_TRY(copy_out(h_dcn, plan->dcn.p, cb));
	NRM_TRY(copy_out(h_w, plan->fit.w(), (size_t)plan->n * 8));
	NRM_TRY(copy_out(h_wt, plan->wt.p, (size_t)plan->rows * 8));
	NRM_TRY(copy_out(h_lcpm, plan->lcpm.p, mb));
	return copy_out(h_cov, plan->dc.p, cb);
}

extern "C" int nrm_front_plan_device_results(nrm_front_plan* plan, void** d_dtn, void** d_dcn, void** d_lcpm, int64_t* ld, void** stream) {
	NRM_REQUIRE(plan != nullptr, "nrm_front_plan_device_results: null plan");
	if (d_dtn) *d_dtn = plan->dtn.p;
	if (d_dcn) *d_dcn = plan->dcn.p;
	if (d_lcpm) *d_lcpm = plan->lcpm.p;
	if (ld) *ld = plan->n;
	if (stream) *stream = (void*)plan->own;
	return NRM_OK;
}

extern "C" int nrm_front_plan_stream(nrm_front_plan* plan, void** stream) { return nrm_plan_stream(plan, "nrm_front_plan_stream", stream); }

extern "C" int nrm_front_plan_info(nrm_front_plan* plan, int64_t info[8]) {
	NRM_REQUIRE(plan != nullptr && info != nullptr, "nrm_front_plan_info: null pointer");
	info[0] = plan->exec ? 1 : 0, info[1] = plan->steps, info[2] = plan->cv_steps, info[3] = plan->max_count, info[4] = plan->cap, info[5] = plan->nct, info[6] = plan->bytes;
	info[7] = plan->warned;
	return NRM_OK;
}

extern "C" int nrm_front_plan_time(nrm_front_plan* plan, int64_t steps, double* ms_per_step) {
	NRM_TRY(plan_bind(plan, "nrm_front_plan_time"));
	return nrm_plan_time(*plan, "nrm_front_plan_time", steps, ms_per_step, [plan] { return nrm_front_plan_step(plan, nullptr); });
}

extern "C" int nrm_front_plan_destroy(nrm_front_plan* plan) { return nrm_plan_destroy(plan); }
