// compute_var with nothing on the host (norm.ComputeVarPlan): what norm.compute_var does in numpy between the three streaming passes of nrm_fitvar.hip, as
// kernels that take device pointers only, so that all stepmax iterations of reference norm.py:98-121 and the weights of norm.py:123-127 are one enqueue.
// Per iteration, for the current scale s (n cells, nc covariates, all fp64):
//   k_fvp_design   u = 1 / s, cw = C u^2 (what k_fv_moments reads) and, per chunk of FVP_CH cells, the upper triangle of sum_k (u_k C_k)(u_k C_k)^T
//   k_fvp_pinv     ONE workgroup: the chunks added in order, then M^+ by nrm_jacobi_lanes.h with a and v in LDS (the rank rule of inv_rank)
//   (nrm_fitvar_moments / genes / cells, unchanged: v)
//   k_fvp_logsum   l = log sqrt v, per chunk of FVP_LCH cells the partial sums of [C;1] l
//   k_fvp_new      coef = M2^+ ([C;1] l) (chunks added in order, by every workgroup for itself), new = exp(coef^T [C_k;1]) s_k, the workgroup's minimum
//   k_fvp_apply    new /= min(new), the workgroup's maximum of |new - s| / s
//   k_fvp_state    t1 = the maximum; s = new; best = new if t1 < bestv; workgroup 0 writes the NEXT state record
// and once, k_fvp_wmin and k_fvp_w: w = 1 / best, w /= min(w), flags[1] += weights that are not finite and positive.
// The state record of an iteration is four doubles {bestv, steps taken, the last t1, 0}; iteration i reads record i and writes record i + 1, so no workgroup
// reads what another is writing.  `bestv > eps` is the reference's loop test (n < stepmax holds for every iteration enqueued): once it fails, the kernels
// of this file return at once and k_fvp_state copies the record, so best, bestv, n and the scale stay as they are; the three streaming passes are not
// ours to change, they run on the unchanged u, cw and M^+ and their v is ignored.
// Minimum and maximum carry a NaN as numpy's do (a NaN t1 is never the best step, norm.py:118).  Sums over cells are partial sums per fixed chunk added
// in a fixed order: no floating-point atomics, the same bits every run.
#include "nrm_common.h"
#include "nrm_jacobi_lanes.h"

#define FVP_NC 63     // as nrm_fitvar.hip
#define FVP_CH 256    // cells per workgroup of the design pass and of the element-wise kernels
#define FVP_TILE 64   // cells of the design pass in LDS at a time
#define FVP_PAIRS 8   // pairs of covariates per thread of the design pass: 63 * 64 / 2 = 2016 <= 8 * 256
#define FVP_LCH 1024  // cells per partial sum of [C;1] l
#define FVP_STATE 4   // doubles per state record

__device__ __forceinline__ bool fvp_stopped(const double* __restrict__ state, double eps) { return !(state[0] > eps); }
__device__ __forceinline__ double fvp_nanmin(double a, double b) { return a != a ? a : b != b ? b : b < a ? b : a; }
__device__ __forceinline__ double fvp_nanmax(double a, double b) { return a != a ? a : b != b ? b : b > a ? b : a; }

// the workgroup's (256 threads) minimum (MAX: maximum) of v, in every thread
template <bool MAX>
__device__ __forceinline__ double fvp_block_ext(double v, double* sm /* 4 */) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const double t = __shfl_xor(v, o, 64);
		v = MAX ? fvp_nanmax(v, t) : fvp_nanmin(v, t);
	}
	__syncthreads();  // (sm may still be read from a previous call)
	if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
	__syncthreads();
	v = sm[0];
#pragma unroll
	for (int i = 1; i < 4; i++) v = MAX ? fvp_nanmax(v, sm[i]) : fvp_nanmin(v, sm[i]);
	return v;
}

// the extreme of part[0 .. m), in every thread
template <bool MAX>
__device__ __forceinline__ double fvp_all_ext(const double* __restrict__ part, int64_t m, double* sm) {
	double v = part[0];
	for (int64_t i = threadIdx.x; i < m; i += 256) v = MAX ? fvp_nanmax(v, part[i]) : fvp_nanmin(v, part[i]);
	return fvp_block_ext<MAX>(v, sm);
}

__global__ void __launch_bounds__(256) k_fvp_start(int64_t n, double* __restrict__ s, double* __restrict__ best, double* __restrict__ state) {
	const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (k < n) {
		s[k] = 1.0;
		best[k] = __longlong_as_double(0x7ff8000000000000LL);  // (the reference's `best is None`: no step was the best, norm.py:122 fails; here the weights are not finite)
	}
	if (k < FVP_STATE) state[k] = k == 0 ? 1e300 : k == 2 ? __longlong_as_double(0x7ff8000000000000LL) : 0.0;
}

__global__ void __launch_bounds__(256) k_fvp_design(const double* __restrict__ c, int nc, int64_t ldc, int64_t n, const double* __restrict__ s, const double* __restrict__ state,
													 double eps, double* __restrict__ u, double* __restrict__ cw, double* __restrict__ mpart) {
	__shared__ double cu[FVP_NC][FVP_TILE + 1];
	if (fvp_stopped(state, eps)) return;
	const int tid = threadIdx.x, npair = nc * (nc + 1) / 2;
	int pi[FVP_PAIRS], pj[FVP_PAIRS];
	double acc[FVP_PAIRS];
#pragma unroll
	for (int e = 0; e < FVP_PAIRS; e++) {  // pair p of the upper triangle, row by row: (i, j >= i)
		int p = tid + e * 256, i = 0;
		while (i < nc - 1 && p >= nc - i) p -= nc - i, i++;
		pi[e] = i, pj[e] = i + p;
		acc[e] = 0.0;
	}
	const int64_t k0 = (int64_t)blockIdx.x * FVP_CH;
	for (int t = 0; t < FVP_CH / FVP_TILE; t++) {
		for (int idx = tid; idx < nc * FVP_TILE; idx += 256) {
			const int r = idx / FVP_TILE, kk = idx % FVP_TILE;
			const int64_t k = k0 + t * FVP_TILE + kk;
			double v = 0.0;
			if (k < n) {
				const double uk = 1.0 / s[k];
				v = c[(int64_t)r * ldc + k] * uk;
				cw[(int64_t)r * n + k] = v * uk;
				if (r == 0) u[k] = uk;
			}
			cu[r][kk] = v;
		}
		__syncthreads();
#pragma unroll
		for (int e = 0; e < FVP_PAIRS; e++)
			if (tid + e * 256 < npair) {
				double a = acc[e];
				for (int kk = 0; kk < FVP_TILE; kk++) a = fma(cu[pi[e]][kk], cu[pj[e]][kk], a);
				acc[e] = a;
			}
		__syncthreads();
	}
#pragma unroll
	for (int e = 0; e < FVP_PAIRS; e++)
		if (tid + e * 256 < npair) mpart[(int64_t)blockIdx.x * npair + tid + e * 256] = acc[e];
}

struct FvpWorkgroup {
	__device__ int lane() const { return threadIdx.x; }
	__device__ int lanes() const { return blockDim.x; }
	__device__ void sync() const { __syncthreads(); }
};

__global__ void __launch_bounds__(64) k_fvp_pinv(const double* __restrict__ mpart, int64_t chunks, int nc, double tol, const double* __restrict__ state, double eps,
												  double* __restrict__ mi, int64_t* __restrict__ rank) {
	__shared__ double a[FVP_NC * FVP_NC], v[FVP_NC * FVP_NC], w[FVP_NC], red[2 * FVP_NC];
	if (fvp_stopped(state, eps)) return;
	const int npair = nc * (nc + 1) / 2;
	for (int e = threadIdx.x; e < nc * nc; e += 64) {
		const int i = e / nc, j = e % nc;
		if (j < i) continue;
		const int p = i * nc - i * (i - 1) / 2 + (j - i);
		double t = 0.0;
		for (int64_t b = 0; b < chunks; b++) t += mpart[b * npair + p];
		a[i * nc + j] = a[j * nc + i] = t;
	}
	__syncthreads();
	nrm_pinv_lanes(FvpWorkgroup(), a, v, w, red, nc, tol, mi, rank);
}

__global__ void __launch_bounds__(256) k_fvp_logsum(const double* __restrict__ v, const double* __restrict__ c, int nc, int64_t ldc, int64_t n, const double* __restrict__ state,
													 double eps, double* __restrict__ gpart) {
	__shared__ double sl[FVP_LCH];
	if (fvp_stopped(state, eps)) return;
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t k0 = (int64_t)blockIdx.x * FVP_LCH;
	for (int j = tid; j < FVP_LCH; j += 256) sl[j] = k0 + j < n ? log(sqrt(v[k0 + j])) : 0.0;
	__syncthreads();
	for (int r = wid; r <= nc; r += 4) {  // (row nc: the intercept)
		double t = 0.0;
		for (int j = lane; j < FVP_LCH; j += 64)
			if (k0 + j < n) t = fma(r < nc ? c[(int64_t)r * ldc + k0 + j] : 1.0, sl[j], t);
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
		if (lane == 0) gpart[(int64_t)blockIdx.x * (nc + 1) + r] = t;
	}
}

__global__ void __launch_bounds__(256) k_fvp_new(const double* __restrict__ gpart, int64_t lchunks, const double* __restrict__ m2i, const double* __restrict__ c, int nc, int64_t ldc,
												  int64_t n, const double* __restrict__ s, const double* __restrict__ state, double eps, double* __restrict__ snew,
												  double* __restrict__ minpart) {
	__shared__ double g[FVP_NC + 1], coef[FVP_NC + 1], sm[4];
	if (fvp_stopped(state, eps)) return;
	const int tid = threadIdx.x, m = nc + 1;
	if (tid < m) {
		double t = 0.0;
		for (int64_t b = 0; b < lchunks; b++) t += gpart[b * m + tid];
		g[tid] = t;
	}
	__syncthreads();
	if (tid < m) {
		double t = 0.0;
		for (int d = 0; d < m; d++) t = fma(m2i[tid * m + d], g[d], t);
		coef[tid] = t;
	}
	__syncthreads();
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + tid;
	double nv = __longlong_as_double(0x7ff0000000000000LL);  // (+inf: cells beyond n do not count in the minimum)
	if (k < n) {
		double f = coef[nc];
		for (int r = 0; r < nc; r++) f = fma(coef[r], c[(int64_t)r * ldc + k], f);
		nv = exp(f) * s[k];
		snew[k] = nv;
	}
	nv = fvp_block_ext<false>(nv, sm);
	if (tid == 0) minpart[blockIdx.x] = nv;
}

__global__ void __launch_bounds__(256) k_fvp_apply(int64_t n, int64_t blocks, const double* __restrict__ s, const double* __restrict__ state, double eps, double* __restrict__ snew,
													const double* __restrict__ minpart, double* __restrict__ maxpart) {
	__shared__ double sm[4];
	if (fvp_stopped(state, eps)) return;
	const double mn = fvp_all_ext<false>(minpart, blocks, sm);
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + threadIdx.x;
	double t = 0.0;
	if (k < n) {
		const double nv = snew[k] / mn, sk = s[k];
		snew[k] = nv;
		t = fabs((nv - sk) / sk);
	}
	t = fvp_block_ext<true>(t, sm);
	if (threadIdx.x == 0) maxpart[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) k_fvp_state(int64_t n, int64_t blocks, const double* __restrict__ snew, const double* __restrict__ maxpart, const double* __restrict__ state,
													double eps, double* __restrict__ s, double* __restrict__ best, double* __restrict__ next) {
	__shared__ double sm[4];
	if (fvp_stopped(state, eps)) {
		if (blockIdx.x == 0 && threadIdx.x < FVP_STATE) next[threadIdx.x] = state[threadIdx.x];
		return;
	}
	const double t1 = fvp_all_ext<true>(maxpart, blocks, sm), bestv = state[0];
	const bool better = t1 < bestv;  // norm.py:118
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + threadIdx.x;
	if (k < n) {
		const double nv = snew[k];
		s[k] = nv;
		if (better) best[k] = nv;
	}
	if (blockIdx.x == 0 && threadIdx.x < FVP_STATE) next[threadIdx.x] = threadIdx.x == 0 ? (better ? t1 : bestv) : threadIdx.x == 1 ? state[1] + 1.0 : threadIdx.x == 2 ? t1 : 0.0;
}

__global__ void __launch_bounds__(256) k_fvp_wmin(int64_t n, const double* __restrict__ best, double* __restrict__ minpart) {
	__shared__ double sm[4];
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + threadIdx.x;
	const double v = fvp_block_ext<false>(k < n ? 1.0 / best[k] : __longlong_as_double(0x7ff0000000000000LL), sm);
	if (threadIdx.x == 0) minpart[blockIdx.x] = v;
}

__global__ void __launch_bounds__(256) k_fvp_w(int64_t n, int64_t blocks, const double* __restrict__ best, const double* __restrict__ minpart, double* __restrict__ w,
												int32_t* __restrict__ flags) {
	__shared__ double sm[4];
	const double mn = fvp_all_ext<false>(minpart, blocks, sm);
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + threadIdx.x;
	if (k < n) {
		const double v = (1.0 / best[k]) / mn;
		w[k] = v;
		if (!(v > 0.0 && v <= 1.7976931348623157e308)) atomicAdd(&flags[1], 1);  // norm.py:126-127
	}
}

// the scratch of one plan, in doubles: the chunks' triangles | the chunks' [C;1] l | a minimum and a maximum per workgroup | the new scale
struct FvpScratch {
	int64_t dchunks, lchunks, blocks, npair;
	double *mpart, *gpart, *minpart, *maxpart, *snew;
	int64_t doubles;
	FvpScratch(int64_t n, int64_t nc, double* ws) {
		dchunks = blocks = (n + FVP_CH - 1) / FVP_CH;
		lchunks = (n + FVP_LCH - 1) / FVP_LCH;
		npair = nc * (nc + 1) / 2;
		mpart = ws;
		gpart = mpart + dchunks * npair;
		minpart = gpart + lchunks * (nc + 1);
		maxpart = minpart + blocks;
		snew = maxpart + blocks;
		doubles = (snew + n) - ws;
	}
};

static int fvp_check(const char* what, int64_t n, int64_t nc) {
	NRM_REQUIRE(n > 0 && n <= (int64_t)FVP_CH * 0x7fffffff, "%s: bad cell count", what);
	NRM_REQUIRE(nc >= 1 && nc <= FVP_NC, "%s: 1 to %d covariates", what, FVP_NC);
	return NRM_OK;
}

extern "C" int64_t nrm_fitvar_plan_workspace(int64_t n, int64_t nc) {
	if (n <= 0 || nc < 1 || nc > FVP_NC) return 0;
	return FvpScratch(n, nc, nullptr).doubles;
}

extern "C" int nrm_fitvar_plan_start(int64_t n, double* d_s, double* d_best, double* d_state, void* stream) {
	NRM_TRY(fvp_check("nrm_fitvar_plan_start", n, 1));
	NRM_REQUIRE(d_s && d_best && d_state, "nrm_fitvar_plan_start: null pointer");
	hipLaunchKernelGGL(k_fvp_start, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, d_s, d_best, d_state);
	return nrm_check_launch("k_fvp_start");
}

extern "C" int nrm_fitvar_design(const double* d_c, int64_t nc, int64_t ldc, int64_t n, const double* d_s, const double* d_state, double eps, double* d_u, double* d_cw,
								 double* d_ws, void* stream) {
	NRM_TRY(fvp_check("nrm_fitvar_design", n, nc));
	NRM_REQUIRE(d_c && d_s && d_state && d_u && d_cw && d_ws && ldc >= n, "nrm_fitvar_design: bad argument");
	const FvpScratch w(n, nc, d_ws);
	hipLaunchKernelGGL(k_fvp_design, dim3((unsigned)w.dchunks), dim3(256), 0, (hipStream_t)stream, d_c, (int)nc, ldc, n, d_s, d_state, eps, d_u, d_cw, w.mpart);
	return nrm_check_launch("k_fvp_design");
}

extern "C" int nrm_fitvar_pinv(int64_t n, int64_t nc, double tol, const double* d_state, double eps, const double* d_ws, double* d_mi, int64_t* d_rank, void* stream) {
	NRM_TRY(fvp_check("nrm_fitvar_pinv", n, nc));
	NRM_REQUIRE(d_state && d_ws && d_mi && d_rank && tol > 0, "nrm_fitvar_pinv: bad argument");
	const FvpScratch w(n, nc, const_cast<double*>(d_ws));
	hipLaunchKernelGGL(k_fvp_pinv, dim3(1), dim3(64), 0, (hipStream_t)stream, w.mpart, w.dchunks, (int)nc, tol, d_state, eps, d_mi, d_rank);
	return nrm_check_launch("k_fvp_pinv");
}

extern "C" int nrm_fitvar_update(const double* d_v, const double* d_c, int64_t nc, int64_t ldc, int64_t n, const double* d_m2i, double* d_s, double* d_best,
								 const double* d_state, double* d_state_next, double eps, double* d_ws, void* stream) {
	NRM_TRY(fvp_check("nrm_fitvar_update", n, nc));
	NRM_REQUIRE(d_v && d_c && d_m2i && d_s && d_best && d_state && d_state_next && d_state != d_state_next && d_ws && ldc >= n, "nrm_fitvar_update: bad argument");
	const FvpScratch w(n, nc, d_ws);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_fvp_logsum, dim3((unsigned)w.lchunks), dim3(256), 0, st, d_v, d_c, (int)nc, ldc, n, d_state, eps, w.gpart);
	NRM_TRY(nrm_check_launch("k_fvp_logsum"));
	hipLaunchKernelGGL(k_fvp_new, dim3((unsigned)w.blocks), dim3(256), 0, st, w.gpart, w.lchunks, d_m2i, d_c, (int)nc, ldc, n, d_s, d_state, eps, w.snew, w.minpart);
	NRM_TRY(nrm_check_launch("k_fvp_new"));
	hipLaunchKernelGGL(k_fvp_apply, dim3((unsigned)w.blocks), dim3(256), 0, st, n, w.blocks, d_s, d_state, eps, w.snew, w.minpart, w.maxpart);
	NRM_TRY(nrm_check_launch("k_fvp_apply"));
	hipLaunchKernelGGL(k_fvp_state, dim3((unsigned)w.blocks), dim3(256), 0, st, n, w.blocks, w.snew, w.maxpart, d_state, eps, d_s, d_best, d_state_next);
	return nrm_check_launch("k_fvp_state");
}

extern "C" int nrm_fitvar_weights(const double* d_best, int64_t n, double* d_ws, double* d_w, int32_t* d_flags, void* stream) {
	NRM_TRY(fvp_check("nrm_fitvar_weights", n, 1));
	NRM_REQUIRE(d_best && d_ws && d_w && d_flags, "nrm_fitvar_weights: null pointer");
	const int64_t blocks = (n + FVP_CH - 1) / FVP_CH;
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_fvp_wmin, dim3((unsigned)blocks), dim3(256), 0, st, n, d_best, d_ws);
	NRM_TRY(nrm_check_launch("k_fvp_wmin"));
	hipLaunchKernelGGL(k_fvp_w, dim3((unsigned)blocks), dim3(256), 0, st, n, blocks, d_best, d_ws, d_w, d_flags);
	return nrm_check_launch("k_fvp_w");
}

// ---- 64 .. nrm_wide_covariates() covariates: the iteration on an orthonormal basis B (r, n) of the covariates' row space (normalisr_amd/norm.py: _fitvar_bases) ----
// B diag(u) spans what C diag(u) spans, so the first regression's fitted values are those on B u, and M = (B u)(B u)^T is positive definite with condition
// <= (u_max / u_min)^2: nrm_gram_f64_whole and nrm_chol_inverse (csrc/nrm_chol_inverse.hip) take the place of k_fvp_design's triangles and k_fvp_pinv.  That M has the
// rank the reference's rule gives C diag(u^2) C^T is certified as in norm._wide_basis, here, because u is known here only: flags[2] counts the iterations without it.
// The second regression is the projection B1^T (B1 l) on an orthonormal basis B1 (r1, n) of span([C;1]).
//   k_fvw_design   u = 1 / s, Bu = B u into the Gram kernel's padded operand (rows to 128, cells to 16, padding zero), cw = Bu u; a chunk's extrema of u
//   k_fvw_cert     kappa from the chunks' extrema in order; flags[2] += !(hi >= safety tol kappa && (full || lo < tol / (safety kappa)))
//   k_fvw_logsum   l = log sqrt v, per chunk of FVP_LCH cells the partial sums of B1 l
//   k_fvw_coef     coef = the chunks added in order
//   k_fvw_new      new = exp(coef^T B1_k) s_k, the workgroup's minimum;  then k_fvp_apply and k_fvp_state as above
#define FVW_ROWS 16  // rows of Bu per workgroup of the design pass

__global__ void __launch_bounds__(256) k_fvw_design(const double* __restrict__ b, int r, int64_t ldb, int64_t n, int rows_pad, int64_t kp, const double* __restrict__ s,
													 const double* __restrict__ state, double eps, double* __restrict__ u, double* __restrict__ bu, double* __restrict__ cw,
													 double* __restrict__ umin, double* __restrict__ umax) {
	__shared__ double sm[4];
	if (fvp_stopped(state, eps)) return;
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + threadIdx.x;
	const double uk = k < n ? 1.0 / s[k] : 0.0;
	const int r0 = blockIdx.y * FVW_ROWS;
	if (k < kp)
		for (int q = r0; q < r0 + FVW_ROWS && q < rows_pad; q++) {
			double v = 0.0;
			if (q < r && k < n) {
				v = b[(int64_t)q * ldb + k] * uk;
				cw[(int64_t)q * n + k] = v * uk;
			}
			bu[(int64_t)q * kp + k] = v;
		}
	if (blockIdx.y == 0 && (int64_t)blockIdx.x * FVP_CH < n) {  // (a chunk of padding cells only has no extrema)
		if (k < n) u[k] = uk;
		const double lo = fvp_block_ext<false>(k < n ? uk : __longlong_as_double(0x7ff0000000000000LL), sm);
		const double hi = fvp_block_ext<true>(k < n ? uk : 0.0, sm);
		if (threadIdx.x == 0) umin[blockIdx.x] = lo, umax[blockIdx.x] = hi;
	}
}

__global__ void __launch_bounds__(256) k_fvw_cert(int64_t blocks, const double* __restrict__ umin, const double* __restrict__ umax, const double* __restrict__ state, double eps,
												   double hi, double lo, double tol, double safety, int full, int32_t* __restrict__ flags) {
	__shared__ double sm[4];
	if (fvp_stopped(state, eps)) return;
	const double a = fvp_all_ext<false>(umin, blocks, sm), z = fvp_all_ext<true>(umax, blocks, sm);
	const double kappa = (z / a) * (z / a);
	if (threadIdx.x == 0 && !(hi >= safety * tol * kappa && (full || lo < tol / (safety * kappa)))) flags[2] += 1;
}

__global__ void __launch_bounds__(256) k_fvw_logsum(const double* __restrict__ v, const double* __restrict__ b1, int r1, int64_t ldb1, int64_t n, const double* __restrict__ state,
													 double eps, double* __restrict__ gpart) {
	__shared__ double sl[FVP_LCH];
	if (fvp_stopped(state, eps)) return;
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
	const int64_t k0 = (int64_t)blockIdx.x * FVP_LCH;
	for (int j = tid; j < FVP_LCH; j += 256) sl[j] = k0 + j < n ? log(sqrt(v[k0 + j])) : 0.0;
	__syncthreads();
	for (int q = wid; q < r1; q += 4) {
		double t = 0.0;
		for (int j = lane; j < FVP_LCH; j += 64)
			if (k0 + j < n) t = fma(b1[(int64_t)q * ldb1 + k0 + j], sl[j], t);
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
		if (lane == 0) gpart[(int64_t)blockIdx.x * r1 + q] = t;
	}
}

__global__ void __launch_bounds__(256) k_fvw_coef(const double* __restrict__ gpart, int64_t lchunks, int r1, const double* __restrict__ state, double eps, double* __restrict__ coef) {
	if (fvp_stopped(state, eps)) return;
	const int q = blockIdx.x * 256 + threadIdx.x;
	if (q < r1) {
		double t = 0.0;
		for (int64_t c = 0; c < lchunks; c++) t += gpart[c * r1 + q];
		coef[q] = t;
	}
}

__global__ void __launch_bounds__(256) k_fvw_new(const double* __restrict__ coef, const double* __restrict__ b1, int r1, int64_t ldb1, int64_t n, const double* __restrict__ s,
												  const double* __restrict__ state, double eps, double* __restrict__ snew, double* __restrict__ minpart) {
	__shared__ double cf[NRM_WIDE_NC + 1], sm[4];
	if (fvp_stopped(state, eps)) return;
	for (int q = threadIdx.x; q < r1; q += 256) cf[q] = coef[q];
	__syncthreads();
	const int64_t k = (int64_t)blockIdx.x * FVP_CH + threadIdx.x;
	double nv = __longlong_as_double(0x7ff0000000000000LL);  // (+inf: cells beyond n do not count in the minimum)
	if (k < n) {
		double f = 0.0;
		for (int q = 0; q < r1; q++) f = fma(cf[q], b1[(int64_t)q * ldb1 + k], f);
		nv = exp(f) * s[k];
		snew[k] = nv;
	}
	nv = fvp_block_ext<false>(nv, sm);
	if (threadIdx.x == 0) minpart[blockIdx.x] = nv;
}

// the scratch of the two wide entries, in doubles: the chunks' extrema of u | the chunks' B1 l | coef | a minimum and a maximum per workgroup | the new scale
struct FvwScratch {
	int64_t blocks, lchunks;
	double *umin, *umax, *gpart, *coef, *minpart, *maxpart, *snew;
	int64_t doubles;
	FvwScratch(int64_t n, int64_t r1, double* ws) {
		blocks = (n + FVP_CH - 1) / FVP_CH;
		lchunks = (n + FVP_LCH - 1) / FVP_LCH;
		umin = ws;
		umax = umin + blocks;
		gpart = umax + blocks;
		coef = gpart + lchunks * r1;
		minpart = coef + r1;
		maxpart = minpart + blocks;
		snew = maxpart + blocks;
		doubles = (snew + n) - ws;
	}
};

static bool fvw_sizes(int64_t n, int64_t r, int64_t r1) { return n > 0 && n <= (int64_t)FVP_CH * 0x7fffffff && r >= 1 && r <= NRM_WIDE_NC && r1 >= 1 && r1 <= NRM_WIDE_NC + 1 && n > r; }

extern "C" int64_t nrm_fitvar_wide_workspace(int64_t n, int64_t r, int64_t r1) {
	if (!fvw_sizes(n, r, r1)) return 0;
	return FvwScratch(n, r1, nullptr).doubles;
}

extern "C" int nrm_fitvar_wide_design(const double* d_b, int64_t r, int64_t ldb, int64_t n, const double* d_s, const double* d_state, double eps, double hi, double lo, double tol,
									  double safety, int full, double* d_u, double* d_bu, int64_t rows_pad, int64_t ldbu, double* d_cw, double* d_ws, int32_t* d_flags,
									  void* stream) {
	NRM_REQUIRE(fvw_sizes(n, r, 1), "nrm_fitvar_wide_design: 1 to %d basis rows on more cells than rows", NRM_WIDE_NC);
	NRM_REQUIRE(d_b && d_s && d_state && d_u && d_bu && d_cw && d_ws && d_flags && ldb >= n, "nrm_fitvar_wide_design: bad argument");
	NRM_REQUIRE(rows_pad >= r && rows_pad % 128 == 0 && ldbu >= n && ldbu % 16 == 0, "nrm_fitvar_wide_design: Bu must be padded to 128 rows and 16 cells");
	NRM_REQUIRE(tol > 0 && safety >= 1 && hi > 0 && lo >= 0, "nrm_fitvar_wide_design: bad certificate");
	const FvwScratch w(n, 1, d_ws);
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid((unsigned)((ldbu + FVP_CH - 1) / FVP_CH), (unsigned)((rows_pad + FVW_ROWS - 1) / FVW_ROWS));
	hipLaunchKernelGGL(k_fvw_design, grid, dim3(256), 0, st, d_b, (int)r, ldb, n, (int)rows_pad, ldbu, d_s, d_state, eps, d_u, d_bu, d_cw, w.umin, w.umax);
	NRM_TRY(nrm_check_launch("k_fvw_design"));
	hipLaunchKernelGGL(k_fvw_cert, dim3(1), dim3(256), 0, st, w.blocks, w.umin, w.umax, d_state, eps, hi, lo, tol, safety, full, d_flags);
	return nrm_check_launch("k_fvw_cert");
}

extern "C" int nrm_fitvar_wide_update(const double* d_v, const double* d_b1, int64_t r1, int64_t ldb1, int64_t n, double* d_s, double* d_best, const double* d_state,
									  double* d_state_next, double eps, double* d_ws, void* stream) {
	NRM_REQUIRE(fvw_sizes(n, 1, r1) && n >= r1, "nrm_fitvar_wide_update: 1 to %d basis rows on at least as many cells", NRM_WIDE_NC + 1);
	NRM_REQUIRE(d_v && d_b1 && d_s && d_best && d_state && d_state_next && d_state != d_state_next && d_ws && ldb1 >= n, "nrm_fitvar_wide_update: bad argument");
	const FvwScratch w(n, r1, d_ws);
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_fvw_logsum, dim3((unsigned)w.lchunks), dim3(256), 0, st, d_v, d_b1, (int)r1, ldb1, n, d_state, eps, w.gpart);
	NRM_TRY(nrm_check_launch("k_fvw_logsum"));
	hipLaunchKernelGGL(k_fvw_coef, dim3((unsigned)((r1 + 255) / 256)), dim3(256), 0, st, w.gpart, w.lchunks, (int)r1, d_state, eps, w.coef);
	NRM_TRY(nrm_check_launch("k_fvw_coef"));
	hipLaunchKernelGGL(k_fvw_new, dim3((unsigned)w.blocks), dim3(256), 0, st, w.coef, d_b1, (int)r1, ldb1, n, d_s, d_state, eps, w.snew, w.minpart);
	NRM_TRY(nrm_check_launch("k_fvw_new"));
	hipLaunchKernelGGL(k_fvp_apply, dim3((unsigned)w.blocks), dim3(256), 0, st, n, w.blocks, d_s, d_state, eps, w.snew, w.minpart, w.maxpart);
	NRM_TRY(nrm_check_launch("k_fvp_apply"));
	hipLaunchKernelGGL(k_fvp_state, dim3((unsigned)w.blocks), dim3(256), 0, st, n, w.blocks, w.snew, w.maxpart, d_state, eps, d_s, d_best, d_state_next);
	return nrm_check_launch("k_fvp_state");
}

extern "C" int nrm_fitvar_pinv_host(const double* m, int64_t n, double tol, double* inv, int64_t* rank) {
	NRM_REQUIRE(m && inv && rank && n >= 1 && n <= FVP_NC + 1 && tol > 0, "nrm_fitvar_pinv_host: bad argument");
	const int nn = (int)n;
	double* a = new double[2 * nn * nn + 3 * nn];
	for (int i = 0; i < nn; i++)
		for (int j = 0; j < nn; j++) a[i * nn + j] = 0.5 * (m[i * nn + j] + m[j * nn + i]);
	nrm_pinv_lanes(NrmSerialLanes(), a, a + nn * nn, a + 2 * nn * nn, a + 2 * nn * nn + nn, nn, tol, inv, rank);
	delete[] a;
	return NRM_OK;
}
