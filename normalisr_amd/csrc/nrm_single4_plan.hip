// Resident single=4 plan behind the C ABI (include/normalisr_hip.h: nrm_single4_plan_*): de(dg, dt, dc, single=4) for a high-MOI screen (reference de.py:4-132 over
// association.py:421-576, 926-980, in closed form: DESIGN 6) for a caller that repeats it on a screen of one shape -- numpy and the library are all it needs.  The
// design is filtered (de.py:93), compacted and listed when it is set (nrm_de_design.hip, as for the two other plans of de), written out dense once, and the DESIGN
// side of NrmSingle4Step (nrm_single4_step.h: the record the whole-problem entries run too) runs then, eagerly: M~, its Newton-Schulz inverse, dxx, varx, the
// norms and the rank certificate depend on the design and the covariates alone.  A step is the record's GENE side -- the products, B^T = G N~, the sweep -- then
// the kernels of this file: alpha on request, the re-inflation of de.py:107-122 with the assertions of de.py:124-131 as a count; then nrm_bh.  One stream, launches
// and memset nodes only; from the second step on a route one hipGraphLaunch.
//
// Every buffer of a step on the sparse-design route is taken from the scratch pool at create (sized for all ng0 design rows, so a new design of the same shape
// fits); the lists are sized by the design's entries and are retaken by nrm_single4_plan_design.  The dense route's residual rows (K1 + the fp64 Gram kernel, after
// a hand-back) are taken when they are first needed.
#include <memory>
#include "nrm_device.h"
#include "nrm_host_entry.h"
#include "nrm_design.h"
#include "nrm_de_design.h"
#include "nrm_plan_core.h"
#include "nrm_single4_plan_args.h"
#include "nrm_single4_step.h"

namespace {

// ---- alpha on the device: alpha_y = b_y - B_y b_x, the same for every grouping in the closed form (association.py:551-553) -------------------------------------
// Stage one: the (nt, nc) fp64 matrix.  A wave per gene: its lanes walk the gene's row of B^T (pitch ldbt) 64 design rows at a time, coalesced, each against the
// nc coefficients of its design row, eight covariates at a time in registers; the lanes' sums meet in the shuffle tree.  The order of every sum is fixed by the
// shape alone: the same bits every run, no floating-point atomics.
#define S4A_CB 8
__global__ __launch_bounds__(256) void k_s4_alpha(const double* __restrict__ bt, int64_t ldbt, const double* __restrict__ by, const double* __restrict__ bx, int64_t nx,
												  int64_t nt, int64_t nc, double* __restrict__ amat) {
	const int lane = threadIdx.x & 63;
	const int64_t y = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (y >= nt) return;  // (the same in every lane of a wave)
	const double* __restrict__ row = bt + y * ldbt;
	for (int64_t c0 = 0; c0 < nc; c0 += S4A_CB) {
		double acc[S4A_CB];
#pragma unroll
		for (int k = 0; k < S4A_CB; k++) acc[k] = 0.0;
		for (int64_t i = lane; i < nx; i += 64) {
			const double v = row[i];
#pragma unroll
			for (int k = 0; k < S4A_CB; k++)
				if (c0 + k < nc) acc[k] = fma(v, bx[i * nc + c0 + k], acc[k]);
		}
#pragma unroll
		for (int k = 0; k < S4A_CB; k++) {
			const double s = nrm_wave_sum(acc[k]);
			if (lane == 0 && c0 + k < nc) amat[y * nc + c0 + k] = by[y * nc + c0 + k] - s;
		}
	}
}

// Stage two: the full-size (ng0, nt, nc) array of the output dtype.  Every design row's nt * nc coefficients are the matrix of stage one, rounded once, or zeros
// for a row that was not tested: a thread reads its element of the matrix once (600 KB at 15 000 genes x 5 covariates: it stays in L2) and stores it to the rows
// blockIdx.y, blockIdx.y + gridDim.y, ...; a wave's store is 64 consecutive elements.  Every element is written once.
template <typename T>
__global__ __launch_bounds__(256) void k_s4_alpha_rows(const double* __restrict__ amat, const int32_t* __restrict__ f2c, int64_t ng0, int64_t wide, T* __restrict__ A) {
	const int64_t step = (int64_t)gridDim.x * 256;
	for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < wide; j += step) {
		const T v = (T)amat[j];
		for (int64_t i = blockIdx.y; i < ng0; i += gridDim.y) A[i * wide + j] = f2c[i] >= 0 ? v : (T)0;
	}
}

// ---- the finish kernel: de._inflate (de.py:107-122) and the assertions of de.py:124-131 for single=4, in one pass ------------------------------------------------
// single=4's vart is per grouping: (rows kept, nt), as P and gamma.  Design row i = blockIdx.y (strided): its nt P-values, gammas and variances come from compact
// row f2c[i], or are 1, 0 and 0 for a row that was not tested; varg[i] is varx (rows kept, fp64, the 0 -> 1 rule applied) rounded once to the output dtype, or 0.
// cp == NULL: every row is tested and the sweep wrote the full-size arrays itself -- only varg and the count are left.  The count: P finite within [0, 1], gamma
// finite, varg and vart finite and >= 0; one integer atomic per wave that found any.
template <typename T>
__global__ __launch_bounds__(256) void k_s4_de_finish(const T* __restrict__ cp, const T* __restrict__ cg, const T* __restrict__ cv, const double* __restrict__ varx,
													  const int32_t* __restrict__ f2c, int64_t ng0, int64_t nt, T* __restrict__ P, T* __restrict__ G, T* __restrict__ V,
													  T* __restrict__ varg, int32_t* __restrict__ counter) {
	const T inf = (T)INFINITY;
	const int64_t j0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
	int bad = 0;
	for (int64_t i = blockIdx.y; i < ng0; i += gridDim.y) {
		const int64_t c = f2c[i];
		for (int64_t j = j0; j < nt; j += step) {
			const int64_t o = i * nt + j;
			T p, g, v;
			if (cp != nullptr) {
				p = c >= 0 ? cp[c * nt + j] : (T)1;
				g = c >= 0 ? cg[c * nt + j] : (T)0;
				v = c >= 0 ? cv[c * nt + j] : (T)0;
				P[o] = p, G[o] = g, V[o] = v;
			} else
				p = P[o], g = G[o], v = V[o];
			bad += !(p >= (T)0 && p <= (T)1) ? 1 : 0;
			bad += !(g > -inf && g < inf) ? 1 : 0;
			bad += !(v >= (T)0 && v < inf) ? 1 : 0;
		}
		if (blockIdx.x == 0 && threadIdx.x == 0) {
			const T vg = c >= 0 ? (T)varx[c] : (T)0;
			varg[i] = vg;
			bad += !(vg >= (T)0 && vg < inf) ? 1 : 0;
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
	if ((threadIdx.x & 63) == 0 && bad > 0) atomicAdd(counter, bad);
}

}  // namespace

// the plan's counters (int32[8]): [0], [1] nrm_single4_sweep; [2] rows handed back by the sparse-design kernels; [4] the finish kernel; [6], [7] nrm_bh
#define S4P_BOUNDS 4
#define S4P_BH 6

struct nrm_single4_plan : NrmPlanCore {
	static constexpr const char* name = "nrm_single4_plan";
	int64_t ng0 = 0, nt = 0, n = 0, nc = 0, ngk = 0;
	int t_dtype = NRM_F64, out_dtype = NRM_F64;
	bool adopted = false, want_alpha = false, want_q = false;
	int64_t bh_bytes = 0, reruns = 0, list_bytes = 0;
	std::vector<double> c64;  // the covariates on the host: the certificates' C C^T, at every design
	std::unique_ptr<NrmDesignLists> L;
	NrmSingle4Step s;  // the sizes, buffers and launches of both sides; s.d_y, the matrix a step reads: own_dt, or the caller's
	// set at create, for all ng0 rows; amat: alpha's (nt, nc) fp64 matrix
	DevBuf own_dt, dc, dci, mask, c2f, f2c, cp, cg, cv, P, G, V, A, amat, varg, q, bhwork;
	~nrm_single4_plan() { shutdown(); }  // (its body runs before the DevBuf members go back to the pool: NrmPlanCore::shutdown)
	bool all_rows() const { return ngk == ng0; }
};

namespace {

// The record's design side on the rows kept, first on the route at hand and, when a design row is handed back, on the dense one.  The compacted design is written
// out dense from its lists for the duration (their CSR form holds every entry of the rows kept): the product kernel and K1 read design rows as rows.
int plan_design_side(nrm_single4_plan* pl, hipStream_t st) {
	NrmSingle4Step& s = pl->s;
	auto take = [pl](DevBuf& b, size_t bytes) { return pl->take(b, bytes); };
	DevBuf gd;
	NRM_TRY(gd.alloc((size_t)pl->ngk * pl->n * 8));
	NRM_TRY(nrm_design_csr_dense(pl->L->row_ptr.as<int64_t>(), pl->L->cells.as<int32_t>(), pl->L->row_vals.p, NRM_F64, pl->ngk, pl->n, gd.p, NRM_F64, pl->n, st));
	s.d_x = gd.p, s.x_dtype = NRM_F64, s.ldx = pl->n;
	int rc = NRM_OK;
	for (int pass = 0; pass < 2; pass++) {
		rc = s.sparse ? s.alloc_sparse(take, st) : s.alloc_dense(take);
		int64_t handed = 0;
		if (rc == NRM_OK) rc = s.alloc_design_side(st, &handed);
		if (rc != NRM_OK || handed == 0) break;
		s.sparse = false;
	}
	if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();  // (gd goes back to the pool with this scope)
	s.d_x = nullptr;
	return rc;
}

// The design of the plan from `in`: de's row filter, the row map, the rows kept compacted and their lists with the ELL form (nrm_de_design.hip), the degrees of
// freedom, then the design side.  The caller has synchronised the device and dropped the graph.
int plan_set_design(nrm_single4_plan* pl, const NrmDePlanDesign& in) {
	hipStream_t st = pl->own;
	NrmDeDesign d;
	NRM_TRY(nrm_de_design_set("nrm_single4_plan", in, pl->ng0, pl->n, pl->mask.as<uint8_t>(), pl->c2f.as<int64_t>(), pl->f2c.as<int32_t>(), true, 0.0, st, d));
	NRM_REQUIRE(d.L->ok, "nrm_single4_plan: the design has no entries");
	NrmSingle4Step& s = pl->s;
	if (pl->n <= d.ngk + s.rank + s.dimreduce) {  // (rank nx - 1 + rank per grouping: dof = n - nx - rank - dimreduce, association.py:558)
		nrm_set_error("Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.");
		return NRM_E_DEVICE;
	}
	if (d.ngk != pl->ng0 && !pl->cp.p) {  // the compact results the finish kernel re-inflates: only a plan that drops rows needs them
		const size_t ob = (size_t)pl->ng0 * pl->nt * nrm_esize(pl->out_dtype);
		NRM_TRY(pl->take(pl->cp, ob));
		NRM_TRY(pl->take(pl->cg, ob));
		NRM_TRY(pl->take(pl->cv, ob));
	}
	pl->bytes += d.list_bytes - pl->list_bytes;
	pl->list_bytes = d.list_bytes;
	pl->L = std::move(d.L);
	s.L = pl->L.get();
	s.nx = pl->ngk = d.ngk;
	s.sparse = true;
	// what the sweep writes: the full-size arrays when every row is tested, the compact ones otherwise
	const bool all = pl->all_rows();
	s.p = all ? pl->P.p : pl->cp.p, s.stat = all ? pl->G.p : pl->cg.p, s.vary = all ? pl->V.p : pl->cv.p;
	pl->fresh = 0;
	return plan_design_side(pl, st);
}

template <typename T>
int plan_finish(nrm_single4_plan* pl, hipStream_t st) {
	const int64_t ng0 = pl->ng0, nt = pl->nt, nc = pl->nc;
	NrmSingle4Step& s = pl->s;
	if (pl->want_alpha) {
		hipLaunchKernelGGL(k_s4_alpha, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, st, s.bt.as<double>(), s.nxp, s.by.as<double>(), s.bx.as<double>(), s.nx, nt, nc,
						   pl->amat.as<double>());
		NRM_TRY(nrm_check_launch("k_s4_alpha"));
		const int64_t wide = nt * nc, gx = std::min<int64_t>((wide + 255) / 256, 512), gy = std::max<int64_t>(1, std::min<int64_t>(ng0, 2048 / gx));
		hipLaunchKernelGGL(k_s4_alpha_rows<T>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, pl->amat.as<double>(), pl->f2c.as<int32_t>(), ng0, wide, pl->A.as<T>());
		NRM_TRY(nrm_check_launch("k_s4_alpha_rows"));
	}
	const bool inflate = !pl->all_rows();
	const dim3 grid((unsigned)std::min<int64_t>((nt + 255) / 256, 64), (unsigned)std::min<int64_t>(ng0, 65535));
	hipLaunchKernelGGL(k_s4_de_finish<T>, grid, dim3(256), 0, st, inflate ? pl->cp.as<T>() : (const T*)nullptr, pl->cg.as<T>(), pl->cv.as<T>(), s.dvarx.as<double>(),
					   pl->f2c.as<int32_t>(), ng0, nt, pl->P.as<T>(), pl->G.as<T>(), pl->V.as<T>(), pl->varg.as<T>(), s.flags.as<int32_t>() + S4P_BOUNDS);
	NRM_TRY(nrm_check_launch("k_s4_de_finish"));
	if (pl->want_q) NRM_TRY(nrm_bh(pl->P.p, pl->out_dtype, ng0, nt, nt, pl->q.p, nt, pl->bhwork.p, pl->bh_bytes, s.flags.as<int32_t>() + S4P_BH, (void*)st));
	return NRM_OK;
}

// the record's gene side, then the kernels of this file
int plan_enqueue(nrm_single4_plan* pl, hipStream_t st) {
	NRM_TRY(pl->s.enqueue(st));
	return pl->out_dtype == NRM_F64 ? plan_finish<double>(pl, st) : plan_finish<float>(pl, st);
}

int plan_upload(nrm_single4_plan* pl, const char* who, const void* h_dt) {
	return nrm_plan_upload(*pl, who, pl->adopted, h_dt, pl->own_dt.p, pl->nt * pl->n * (int64_t)nrm_esize(pl->t_dtype));
}

int plan_counters(nrm_single4_plan* pl, hipStream_t st, int32_t (&hf)[8]) {
	NRM_TRY(nrm_read_flags(pl->s.flags.p, st, hf));
	NRM_TRY(nrm_fill_zero(pl->s.flags.p, 32, (void*)st));
	NRM_HIP(hipStreamSynchronize(st));
	return NRM_OK;
}

// reads and clears the counters once the queued steps are through; the hand-back's rerun; then what the reference would have said; caller holds nrm_host_entry_mutex
int plan_check(nrm_single4_plan* pl, int64_t* handed_back) {
	hipStream_t st = pl->last ? pl->last : pl->own;
	if (handed_back) *handed_back = 0;
	int32_t hf[8];
	NRM_HIP(hipDeviceSynchronize());
	NRM_TRY(plan_counters(pl, st, hf));
	if (pl->s.sparse && pl->steps > 0 && hf[2] > 0) {
		// expression rows all but inside the span of the covariates since the last check: the design side and the step again on K1 and the fp64 Gram kernel from the
		// matrices as they stand, and that route from here on, until the design is replaced
		if (handed_back) *handed_back = hf[2];
		pl->drop_graph();
		pl->s.sparse = false;
		pl->fresh = 1;
		NRM_TRY(plan_design_side(pl, st));
		NRM_TRY(plan_enqueue(pl, st));
		pl->reruns++;
		NRM_TRY(plan_counters(pl, st, hf));
	}
	if (hf[0] || hf[1]) {
		nrm_set_error("association results failed the reference's assertions (association.py:557): %d tiles non-finite, %d tiles with R^2 > 1+1e-8 in the closed form", hf[0], hf[1]);
		return NRM_E_NUMERIC;
	}
	if (hf[S4P_BOUNDS] > 0) {
		nrm_set_error("de results failed the reference's assertions (de.py:124-131): %d entries of P, gamma, varg or vart not finite or out of range", hf[S4P_BOUNDS]);
		return NRM_E_NUMERIC;
	}
	return NRM_OK;
}

}  // namespace

extern "C" int nrm_single4_plan_create(nrm_single4_plan** plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices,
									   int64_t nnz, int dg_on_device, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n_cells, int64_t ldt, int dt_on_device,
									   const void* h_dc, int c_dtype, int64_t nc, const double* h_dci, int rank, int dimreduce, int out_dtype, int want_alpha, int want_q,
									   double tol) {
	NRM_REQUIRE(plan != nullptr, "nrm_single4_plan_create: null plan pointer");
	*plan = nullptr;
	const int64_t n = n_cells;
	if (ldt == 0) ldt = n;
	const NrmDePlanDesign g = nrm_de_plan_design_of(design_form, dg, dg_dtype, ldg, indptr, indices, nnz, dg_on_device, n);
	// every check, the covariates' pseudo-inverse and rank when the caller has none included (host arithmetic, nrm_single4_plan_args.h): all before any device call
	std::vector<double> c64, own_dci;
	NRM_TRY(nrm_single4_plan_create_args(g, ng0, dt, dt_dtype, nt, n, ldt, dt_on_device, h_dc, c_dtype, nc, &h_dci, &rank, dimreduce, out_dtype, tol,
										 nrm_de_sparse_max_covariates(), c64, own_dci));
	int64_t bh_bytes = 0;
	NRM_TRY(nrm_plan_bh_bytes("nrm_single4_plan_create", want_q, ng0 * nt, out_dtype, &bh_bytes));

	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	std::unique_ptr<nrm_single4_plan> pl(new nrm_single4_plan);
	NRM_HIP(hipGetDevice(&pl->device));
	pl->ng0 = ng0, pl->nt = nt, pl->n = n, pl->nc = nc, pl->t_dtype = dt_dtype, pl->out_dtype = out_dtype;
	pl->adopted = dt_on_device != 0;
	pl->want_alpha = want_alpha != 0 && nc > 0, pl->want_q = want_q != 0;
	pl->bh_bytes = bh_bytes;
	pl->c64.swap(c64);
	NrmSingle4Step& s = pl->s;
	s.rows = ng0, s.ny = nt, s.n = n, s.ldy = ldt, s.nc = nc, s.y_dtype = dt_dtype, s.out_dtype = out_dtype, s.rank = rank, s.dimreduce = dimreduce, s.return_dot = 0, s.tol = tol;
	s.want_alpha = pl->want_alpha;
	s.ci = nc ? nrm_constant_row(pl->c64.data(), nc, n, &s.cval) : -1;
	s.who = "nrm_single4_plan";
	s.h_c64 = pl->c64.data();
	auto take = [&pl](DevBuf& b, size_t bytes) { return pl->take(b, bytes); };
	NRM_HIP(hipStreamCreateWithFlags(&pl->own, hipStreamNonBlocking));
	hipStream_t st = pl->own;
	if (!pl->adopted) NRM_TRY(pl->take(pl->own_dt, (size_t)nt * n * nrm_esize(dt_dtype)));
	s.d_y = pl->adopted ? dt : pl->own_dt.p;
	if (nc > 0) {
		NRM_TRY(nrm_take_all(take, {{&pl->dc, nc * n * 8}, {&pl->dci, nc * nc * 8}}));
		NRM_HIP(hipMemcpy(pl->dc.p, pl->c64.data(), (size_t)nc * n * 8, hipMemcpyHostToDevice));
		NRM_HIP(hipMemcpy(pl->dci.p, h_dci, (size_t)nc * nc * 8, hipMemcpyHostToDevice));
	}
	s.d_c = pl->dc.as<double>(), s.d_dci = pl->dci.as<double>();
	NRM_TRY(s.alloc_fixed(take, st));
	const size_t es = nrm_esize(out_dtype), ob = (size_t)ng0 * nt * es;
	NRM_TRY(nrm_take_all(take, {{&pl->mask, ng0}, {&pl->c2f, ng0 * 8}, {&pl->f2c, ng0 * 4}, {&pl->P, ob}, {&pl->G, ob}, {&pl->V, ob}, {&pl->varg, ng0 * es}}));
	if (pl->want_alpha) NRM_TRY(nrm_take_all(take, {{&pl->A, ob * nc}, {&pl->amat, nt * nc * 8}}));
	if (pl->want_q) NRM_TRY(nrm_take_all(take, {{&pl->q, ob}, {&pl->bhwork, bh_bytes}}));
	if (pl->adopted || dg_on_device) NRM_HIP(hipDeviceSynchronize());  // (whatever the caller queued to fill its matrices is through before they are read)
	NRM_TRY(plan_set_design(pl.get(), g));
	if (!pl->adopted) NRM_TRY(plan_upload(pl.get(), "nrm_single4_plan_create", dt));
	NRM_HIP(hipStreamSynchronize(st));
	*plan = pl.release();
	return NRM_OK;
}

extern "C" int nrm_single4_plan_design(nrm_single4_plan* plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices,
									   int64_t nnz, int dg_on_device) {
	NRM_REQUIRE(plan != nullptr, "nrm_single4_plan_design: null plan");
	const NrmDePlanDesign g = nrm_de_plan_design_of(design_form, dg, dg_dtype, ldg, indptr, indices, nnz, dg_on_device, plan->n);
	NRM_TRY(nrm_de_plan_design_args("nrm_single4_plan_design", g, plan->ng0, plan->n));
	return nrm_plan_new_design(plan, g, plan_set_design);
}

extern "C" int nrm_single4_plan_upload(nrm_single4_plan* plan, const void* h_dt) {
	NRM_TRY(plan_bind(plan, "nrm_single4_plan_upload"));
	return plan_upload(plan, "nrm_single4_plan_upload", h_dt);
}

// (the graph is of one route: plan_check drops it when it hands back, and the second step on the dense route is captured anew)
extern "C" int nrm_single4_plan_step(nrm_single4_plan* plan, void* stream) {
	NRM_TRY(plan_bind(plan, "nrm_single4_plan_step"));
	return nrm_plan_step(*plan, "nrm_single4_plan_step", stream, [plan](hipStream_t st) { return plan_enqueue(plan, st); });
}

extern "C" int nrm_single4_plan_check(nrm_single4_plan* plan, int64_t* handed_back) {
	NRM_REQUIRE(plan != nullptr, "nrm_single4_plan_check: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_single4_plan_check"));
	return plan_check(plan, handed_back);
}

extern "C" int nrm_single4_plan_results(nrm_single4_plan* plan, void* h_p, void* h_gamma, void* h_alpha, void* h_varg, void* h_vart, void* h_q) {
	NRM_REQUIRE(plan != nullptr, "nrm_single4_plan_results: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_single4_plan_results"));
	NRM_REQUIRE(plan->steps > 0, "nrm_single4_plan_results: no step has run");
	NRM_REQUIRE(!h_alpha || plan->want_alpha, "nrm_single4_plan_results: the plan was created without alpha");
	NRM_REQUIRE(!h_q || plan->want_q, "nrm_single4_plan_results: the plan was created without q-values");
	NRM_TRY(plan_check(plan, nullptr));
	const size_t es = nrm_esize(plan->out_dtype), ob = (size_t)plan->ng0 * plan->nt * es;
	NRM_TRY(copy_out(h_p, plan->P.p, ob));
	NRM_TRY(copy_out(h_gamma, plan->G.p, ob));
	NRM_TRY(copy_out(h_alpha, plan->A.p, ob * plan->nc));
	NRM_TRY(copy_out(h_varg, plan->varg.p, (size_t)plan->ng0 * es));
	NRM_TRY(copy_out(h_vart, plan->V.p, ob));
	NRM_TRY(copy_out(h_q, plan->q.p, ob));
	return NRM_OK;
}

extern "C" int nrm_single4_plan_device_results(nrm_single4_plan* plan, void** d_p, void** d_gamma, void** d_alpha, void** d_varg, void** d_q, void** d_vart, void** d_mask,
											   int64_t* ld) {
	NRM_REQUIRE(plan != nullptr, "nrm_single4_plan_device_results: null plan");
	if (d_p) *d_p = plan->P.p;
	if (d_gamma) *d_gamma = plan->G.p;
	if (d_alpha) *d_alpha = plan->A.p;
	if (d_varg) *d_varg = plan->varg.p;
	if (d_q) *d_q = plan->q.p;
	if (d_vart) *d_vart = plan->V.p;
	if (d_mask) *d_mask = plan->mask.p;
	if (ld) *ld = plan->nt;
	return NRM_OK;
}

extern "C" int nrm_single4_plan_stream(nrm_single4_plan* plan, void** stream) {
	return nrm_plan_stream(plan, "nrm_single4_plan_stream", stream);
}

extern "C" int nrm_single4_plan_info(nrm_single4_plan* plan, int64_t info[8]) {
	NRM_REQUIRE(plan != nullptr && info != nullptr, "nrm_single4_plan_info: null pointer");
	info[0] = plan->s.sparse ? 0 : 1, info[1] = plan->exec ? 1 : 0, info[2] = plan->steps, info[3] = plan->reruns, info[4] = plan->s.rank, info[5] = (int64_t)plan->s.dof(),
	info[6] = plan->bytes, info[7] = plan->ngk;
	return NRM_OK;
}

extern "C" int nrm_single4_plan_time(nrm_single4_plan* plan, int64_t steps, double* ms_per_step) {
	NRM_TRY(plan_bind(plan, "nrm_single4_plan_time"));
	return nrm_plan_time(*plan, "nrm_single4_plan_time", steps, ms_per_step, [plan] { return nrm_single4_plan_step(plan, nullptr); });
}

extern "C" int nrm_single4_plan_destroy(nrm_single4_plan* plan) { return nrm_plan_destroy(plan); }
