// Resident single=1 plan behind the C ABI (include/normalisr_hip.h: nrm_single1_plan_*): de(dg, dt, dc, single=1) for a low-MOI screen (reference de.py:4-132 over
// association.py:263-390, 911-925) for a caller that repeats it on a screen of one shape -- numpy and the library are all it needs.  The design is filtered (de.py:93),
// compacted and listed when it is set (nrm_de_design.hip, as for the single=0 plan), BEFORE the cell selection sees it: an all-ones row de drops would otherwise leave no
// cell that carries exactly one grouping.  A step is the launch sequence of normalisr_amd.single1.Single1Plan on two streams -- nrm_single1_select; beside each other
// nrm_single1_common_gram + the groupings' statistics and nrm_single1_stream; nrm_single1_cells -- then the kernel of this file: the re-inflation of de.py:107-122 with
// single=1's per-grouping variances, and the assertions of de.py:124-131 as a count; then nrm_bh.  From the second step on one hipGraphLaunch.
//
// Every buffer whose size the shape decides is taken from the scratch pool at create (sized for all ng0 design rows, so a new design of the same shape fits); what the
// design's entries size (the selection's lists, the stream kernel's transposed output) is retaken by nrm_single1_plan_design.
#include <memory>
#include "nrm_device.h"
#include "nrm_host_entry.h"
#include "nrm_design.h"
#include "nrm_de_design.h"
#include "nrm_plan_core.h"
#include "nrm_single1_plan_args.h"

namespace {

// ---- the finish kernel: de._inflate (de.py:107-122) and the assertions of de.py:124-131 for single=1, in one pass ------------------------------------------------
// single=1's variances are per grouping: varx (rows kept) fp64 and vary (rows kept, nt).  Design row i = blockIdx.y (strided): its nt P-values, gammas and vary and its
// nt * nc coefficients come from compact row f2c[i], or are 1, 0, 0 and 0 for a row that was not tested; varg[i] is varx rounded once to the output dtype, or 0.  cp ==
// NULL: every row is tested and the sweep wrote the full-size arrays itself -- only varg and the count are left.  The count: P finite within [0, 1], gamma finite, varg
// and vart finite and >= 0; entries that fail are added up over the workgroup and counted with one integer atomic per workgroup that found any.
template <typename T>
__global__ __launch_bounds__(256) void k_s1_de_finish(const T* __restrict__ cp, const T* __restrict__ cg, const T* __restrict__ cv, const T* __restrict__ ca,
													  const double* __restrict__ varx, const int32_t* __restrict__ f2c, int64_t ng0, int64_t nt, int64_t nc, T* __restrict__ P,
													  T* __restrict__ G, T* __restrict__ V, T* __restrict__ A, T* __restrict__ varg, int32_t* __restrict__ counter) {
	__shared__ int wbad[4];
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
		if (cp != nullptr && A != nullptr) {
			const int64_t wide = nt * nc;
			for (int64_t j = j0; j < wide; j += step) A[i * wide + j] = c >= 0 ? ca[c * wide + j] : (T)0;
		}
		if (blockIdx.x == 0 && threadIdx.x == 0) {
			const T vg = c >= 0 ? (T)varx[c] : (T)0;
			varg[i] = vg;
			bad += !(vg >= (T)0 && vg < inf) ? 1 : 0;
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
	if ((threadIdx.x & 63) == 0) wbad[threadIdx.x >> 6] = bad;
	__syncthreads();
	if (threadIdx.x == 0) {
		const int total = wbad[0] + wbad[1] + wbad[2] + wbad[3];
		if (total > 0) atomicAdd(counter, total);
	}
}

}  // namespace

// the plan's counters (int32[8]): [0], [1] nrm_single1_cells; [2], [3], [4] nrm_single1_group_info; [5] the finish kernel; [6], [7] nrm_bh
#define S1P_BOUNDS 5
#define S1P_BH 6

struct nrm_single1_plan : NrmPlanCore {
	static constexpr const char* name = "nrm_single1_plan";
	int64_t ng0 = 0, nt = 0, n = 0, ldt = 0, nc = 0, ngk = 0, nnz = 0, n_kept = 0, ldye = 0, pitch = 0;
	int t_dtype = NRM_F64, out_dtype = NRM_F64, dimreduce = 0;
	bool adopted = false, want_alpha = false, want_q = false;
	const void* dt = nullptr;  // the matrix a step reads: own_dt, or the caller's
	int64_t bh_bytes = 0;
	std::unique_ptr<NrmDesignLists> L;
	// set at create, for all ng0 rows
	DevBuf own_dt, dc, mask, c2f, f2c, flags, cnt, code, seg, rowinfo, sel_info, gpart, gs, common, info, varx, cp, cg, cv, ca, P, G, V, A, varg, q, bhwork;
	// sized by the design's entries
	DevBuf idx, xe, ce, ye;
	hipStream_t side = nullptr;  // the fork of a step: plan_enqueue
	hipEvent_t forked = nullptr, joined = nullptr;
	int64_t design_bytes = 0;
	// (its body runs before the DevBuf members go back to the pool: NrmPlanCore::shutdown, which leaves the device idle and no graph that names the side stream)
	~nrm_single1_plan() {
		shutdown();
		if (forked) (void)hipEventDestroy(forked);
		if (joined) (void)hipEventDestroy(joined);
		if (side) (void)hipStreamDestroy(side);
	}
	bool all_rows() const { return ngk == ng0; }
	// what nrm_single1_cells writes: the full-size arrays when every row is tested, the compact ones otherwise
	void* sweep_p() const { return all_rows() ? P.p : cp.p; }
	void* sweep_g() const { return all_rows() ? G.p : cg.p; }
	void* sweep_v() const { return all_rows() ? V.p : cv.p; }
	void* sweep_a() const { return !want_alpha ? nullptr : (all_rows() ? A.p : ca.p); }
};

namespace {

// the cell selection from the lists of the rows kept (association.py:914-918); the shared cells' Gram matrix is left to nrm_single1_common_gram
int plan_select(nrm_single1_plan* pl, hipStream_t st) {
	NrmDesignLists& L = *pl->L;
	return nrm_single1_select(L.row_ptr.as<int64_t>(), L.cells.as<int32_t>(), L.row_vals.as<double>(), pl->ngk, pl->n, pl->nnz, pl->dc.as<double>(), pl->n, pl->nc,
							  pl->cnt.as<int32_t>(), pl->code.as<int32_t>(), pl->seg.as<int64_t>(), pl->idx.as<int64_t>(), pl->xe.as<double>(), pl->ce.as<double>(),
							  pl->rowinfo.as<double>(), nullptr, pl->sel_info.as<int64_t>(), st);
}

// The design of the plan from `in`, in this order: de's row filter, the compaction of the rows kept, their entry lists as NrmDesignLists::build(ell = false,
// max_density = 0.25) builds them (nrm_de_design.hip), the selection once for the count of cells that carry exactly one grouping (the one read-back of sizes,
// as Single1Plan._build), the stream kernel's transposed output sized from it.  The caller has synchronised the device and dropped the graph.
int plan_set_design(nrm_single1_plan* pl, const NrmDePlanDesign& in) {
	hipStream_t st = pl->own;
	NrmDeDesign d;
	NRM_TRY(nrm_de_design_set("nrm_single1_plan", in, pl->ng0, pl->n, pl->mask.as<uint8_t>(), pl->c2f.as<int64_t>(), pl->f2c.as<int32_t>(), false, 0.25, st, d));
	const int bits = d.L->bits;
	if (!(bits & NRM_DESIGN_HAS1) || (bits & (NRM_DESIGN_GT1 | NRM_DESIGN_NAN))) {
		nrm_set_error("the largest entry of dx must be 1 (association.py:914)");
		return NRM_E_NUMERIC;
	}
	if (!d.L->ok || (bits & NRM_DESIGN_NEG)) {
		nrm_set_error("nrm_single1_plan covers designs with entries >= 0 of which at most a quarter are set (the package's masked-Gram path takes the others)");
		return NRM_E_UNSUPPORTED;
	}
	const int64_t nnz = d.L->nnz, nc = pl->nc;
	pl->idx.release(), pl->xe.release(), pl->ce.release(), pl->ye.release();
	NRM_TRY(pl->idx.alloc((size_t)nnz * 8));
	NRM_TRY(pl->xe.alloc((size_t)nnz * 8));
	if (nc) NRM_TRY(pl->ce.alloc((size_t)nnz * nc * 8));
	pl->L = std::move(d.L);
	pl->ngk = d.ngk;
	pl->nnz = nnz;
	NRM_TRY(plan_select(pl, st));
	int64_t h[8];
	NRM_HIP(hipMemcpyAsync(h, pl->sel_info.p, sizeof(h), hipMemcpyDeviceToHost, st));
	NRM_HIP(hipStreamSynchronize(st));
	NRM_REQUIRE(h[4] >= 0 && h[4] <= nnz, "nrm_single1_plan: the selection does not match the design's lists");
	pl->n_kept = h[4];
	const size_t yb = (size_t)(pl->n_kept > 0 ? pl->n_kept : 1) * pl->ldye * nrm_esize(pl->t_dtype) + 64;
	NRM_TRY(pl->ye.alloc(yb));
	if (!pl->all_rows() && !pl->cp.p) {  // the compact results the finish kernel re-inflates: only a plan that drops rows needs them
		const size_t ob = (size_t)pl->ng0 * pl->nt * nrm_esize(pl->out_dtype);
		NRM_TRY(pl->take(pl->cp, ob));
		NRM_TRY(pl->take(pl->cg, ob));
		NRM_TRY(pl->take(pl->cv, ob));
		if (pl->want_alpha) NRM_TRY(pl->take(pl->ca, ob * nc));
	}
	const int64_t db = d.list_bytes + nnz * 16 + nnz * nc * 8 + (int64_t)yb;
	pl->bytes += db - pl->design_bytes;
	pl->design_bytes = db;
	pl->fresh = 0;
	return NRM_OK;
}

template <typename T>
int plan_finish(nrm_single1_plan* pl, hipStream_t st) {
	const int64_t ng0 = pl->ng0, nt = pl->nt;
	const bool inflate = !pl->all_rows();
	const int64_t wide = (inflate && pl->want_alpha) ? nt * pl->nc : nt, gx = std::min<int64_t>((wide + 255) / 256, 64);
	const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(ng0, 65535));
	hipLaunchKernelGGL(k_s1_de_finish<T>, grid, dim3(256), 0, st, inflate ? pl->cp.as<T>() : (const T*)nullptr, pl->cg.as<T>(), pl->cv.as<T>(),
					   pl->want_alpha ? pl->ca.as<T>() : (const T*)nullptr, pl->varx.as<double>(), pl->f2c.as<int32_t>(), ng0, nt, pl->nc, pl->P.as<T>(), pl->G.as<T>(), pl->V.as<T>(),
					   pl->want_alpha ? pl->A.as<T>() : (T*)nullptr, pl->varg.as<T>(), pl->flags.as<int32_t>() + S1P_BOUNDS);
	NRM_TRY(nrm_check_launch("k_s1_de_finish"));
	if (pl->want_q)
		NRM_TRY(nrm_bh(pl->P.p, pl->out_dtype, ng0, nt, nt, pl->q.p, nt, pl->bhwork.p, pl->bh_bytes, pl->flags.as<int32_t>() + S1P_BH, (void*)st));
	return NRM_OK;
}

// The launches of Single1Plan._launch, in its order and on its two streams: the groupings' statistics need the selection only and the stream kernel nothing of them,
// so they run beside it on the plan's side stream -- a fork and a join by events, which a capture of `st` records as two branches.
int plan_enqueue(nrm_single1_plan* pl, hipStream_t st) {
	const int64_t nc = pl->nc, n = pl->n, nt = pl->nt, nx = pl->ngk;
	const double* d_c = pl->dc.as<double>();
	int32_t* flags = pl->flags.as<int32_t>();
	NRM_TRY(plan_select(pl, st));
	NRM_HIP(hipEventRecord(pl->forked, st));
	NRM_HIP(hipStreamWaitEvent(pl->side, pl->forked, 0));
	if (nc) NRM_TRY(nrm_single1_common_gram(pl->cnt.as<int32_t>(), n, d_c, n, nc, pl->gpart.as<double>(), (void*)pl->side));
	if (nc > 8) {
		NRM_TRY(nrm_single1_group_stats_wide(pl->seg.as<int64_t>(), pl->xe.as<double>(), pl->ce.as<double>(), nc, nx, pl->gs.as<double>(), (void*)pl->side));
		NRM_TRY(nrm_single1_group_info_wide(pl->gs.as<double>(), pl->gpart.as<double>(), pl->rowinfo.as<double>(), pl->sel_info.as<int64_t>(), nc, nx, pl->dimreduce,
											pl->info.as<double>(), pl->pitch, pl->varx.as<double>(), flags, (void*)pl->side));
	} else {
		NRM_TRY(nrm_single1_group_stats(pl->seg.as<int64_t>(), pl->idx.as<int64_t>(), pl->xe.as<double>(), d_c, n, nc, nx, pl->gs.as<double>(), (void*)pl->side));
		NRM_TRY(nrm_single1_group_info(pl->gs.as<double>(), pl->gpart.as<double>(), pl->rowinfo.as<double>(), pl->sel_info.as<int64_t>(), nc, nx, pl->dimreduce,
									   pl->info.as<double>(), pl->pitch, pl->varx.as<double>(), flags, (void*)pl->side));
	}
	NRM_HIP(hipEventRecord(pl->joined, pl->side));
	NRM_TRY(nrm_single1_stream(pl->dt, pl->t_dtype, pl->ldt, d_c, n, nc, pl->code.as<int32_t>(), n, nt, pl->common.as<double>(), pl->ye.p, pl->ldye, (void*)st));
	NRM_HIP(hipStreamWaitEvent(st, pl->joined, 0));
	NRM_TRY(nrm_single1_cells(pl->ye.p, pl->t_dtype, pl->ldye, pl->ce.as<double>(), pl->xe.as<double>(), pl->seg.as<int64_t>(), pl->common.as<double>(), pl->info.as<double>(),
							  pl->pitch, nc, nx, nt, 0, pl->sweep_p(), pl->sweep_g(), pl->sweep_v(), pl->sweep_a(), pl->out_dtype, nt, flags, (void*)st));
	return pl->out_dtype == NRM_F64 ? plan_finish<double>(pl, st) : plan_finish<float>(pl, st);
}

int plan_upload(nrm_single1_plan* pl, const char* who, const void* h_dt) {
	return nrm_plan_upload(*pl, who, pl->adopted, h_dt, pl->own_dt.p, pl->nt * pl->n * (int64_t)nrm_esize(pl->t_dtype));
}

// reads and clears the counters once the queued steps are through, and says what the reference would have, in its order: the selection (association.py:917-918), the
// SVD's finiteness check, the cell count, the results (:248,252), de's own assertions (de.py:124-131); caller holds nrm_host_entry_mutex
int plan_check(nrm_single1_plan* pl) {
	hipStream_t st = pl->last ? pl->last : pl->own;
	int32_t hf[8];
	NRM_HIP(hipDeviceSynchronize());
	NRM_TRY(nrm_read_flags(pl->flags.p, st, hf));
	NRM_TRY(nrm_fill_zero(pl->flags.p, 32, (void*)st));
	NRM_HIP(hipStreamSynchronize(st));
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
	if (hf[S1P_BOUNDS] > 0) {
		nrm_set_error("de results failed the reference's assertions (de.py:124-131): %d entries of P, gamma, varg or vart not finite or out of range", hf[S1P_BOUNDS]);
		return NRM_E_NUMERIC;
	}
	return NRM_OK;
}

}  // namespace

extern "C" int nrm_single1_plan_create(nrm_single1_plan** plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices,
									   int64_t nnz, int dg_on_device, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n_cells, int64_t ldt, int dt_on_device,
									   const void* h_dc, int c_dtype, int64_t nc, int dimreduce, int out_dtype, int want_alpha, int want_q) {
	NRM_REQUIRE(plan != nullptr, "nrm_single1_plan_create: null plan pointer");
	*plan = nullptr;
	const int64_t n = n_cells;
	if (ldt == 0) ldt = n;
	const NrmDePlanDesign g = nrm_de_plan_design_of(design_form, dg, dg_dtype, ldg, indptr, indices, nnz, dg_on_device, n);
	// every check (host arithmetic, nrm_single1_plan_args.h): all before any device call
	std::vector<double> c64;
	NRM_TRY(nrm_single1_plan_create_args(g, ng0, dt, dt_dtype, nt, n, ldt, dt_on_device, h_dc, c_dtype, nc, dimreduce, out_dtype, c64));
	int64_t bh_bytes = 0;
	NRM_TRY(nrm_plan_bh_bytes("nrm_single1_plan_create", want_q, ng0 * nt, out_dtype, &bh_bytes));

	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	std::unique_ptr<nrm_single1_plan> pl(new nrm_single1_plan);
	NRM_HIP(hipGetDevice(&pl->device));
	pl->ng0 = ng0, pl->nt = nt, pl->n = n, pl->ldt = ldt, pl->nc = nc, pl->t_dtype = dt_dtype, pl->out_dtype = out_dtype, pl->dimreduce = dimreduce;
	pl->adopted = dt_on_device != 0;
	pl->want_alpha = want_alpha != 0 && nc > 0, pl->want_q = want_q != 0;
	pl->ldye = nrm_round_up(nt, 8);
	pl->pitch = 26 + nc + nc * nc;
	pl->bh_bytes = bh_bytes;
	NRM_HIP(hipStreamCreateWithFlags(&pl->own, hipStreamNonBlocking));
	NRM_HIP(hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking));
	NRM_HIP(hipEventCreateWithFlags(&pl->forked, hipEventDisableTiming));
	NRM_HIP(hipEventCreateWithFlags(&pl->joined, hipEventDisableTiming));
	hipStream_t st = pl->own;
	if (pl->adopted)
		pl->dt = dt;
	else {
		NRM_TRY(pl->take(pl->own_dt, (size_t)nt * n * nrm_esize(dt_dtype)));
		pl->dt = pl->own_dt.p;
	}
	if (nc > 0) {
		NRM_TRY(pl->take(pl->dc, c64.size() * 8));
		NRM_HIP(hipMemcpy(pl->dc.p, c64.data(), c64.size() * 8, hipMemcpyHostToDevice));
		const int64_t nb = (nc + 7) / 8;  // (an 8 x 8 block of covariates per pair bi <= bj: nrm_single1_common_gram)
		NRM_TRY(pl->take(pl->gpart, (size_t)(nb * (nb + 1) / 2) * nrm_single1_select_gram_blocks() * 64 * 8));
	}
	const size_t es = nrm_esize(out_dtype), ob = (size_t)ng0 * nt * es;
	NRM_TRY(pl->take(pl->mask, (size_t)ng0));
	NRM_TRY(pl->take(pl->c2f, (size_t)ng0 * 8));
	NRM_TRY(pl->take(pl->f2c, (size_t)ng0 * 4));
	NRM_TRY(pl->take(pl->flags, 32));
	NRM_TRY(pl->take(pl->cnt, (size_t)n * 4));
	NRM_TRY(pl->take(pl->code, (size_t)n * 4));
	NRM_TRY(pl->take(pl->seg, (size_t)(ng0 + 1) * 8));
	NRM_TRY(pl->take(pl->rowinfo, (size_t)ng0 * 3 * 8));
	NRM_TRY(pl->take(pl->sel_info, 64));
	NRM_TRY(pl->take(pl->gs, (size_t)ng0 * (nc * (nc + 1) / 2 + nc + 1) * 8));
	NRM_TRY(pl->take(pl->common, (size_t)(nc + 1) * nt * 8));
	NRM_TRY(pl->take(pl->info, (size_t)ng0 * pl->pitch * 8));
	NRM_TRY(pl->take(pl->varx, (size_t)ng0 * 8));
	NRM_TRY(pl->take(pl->P, ob));
	NRM_TRY(pl->take(pl->G, ob));
	NRM_TRY(pl->take(pl->V, ob));
	if (pl->want_alpha) NRM_TRY(pl->take(pl->A, ob * nc));
	NRM_TRY(pl->take(pl->varg, (size_t)ng0 * es));
	if (pl->want_q) {
		NRM_TRY(pl->take(pl->q, ob));
		NRM_TRY(pl->take(pl->bhwork, (size_t)bh_bytes));
	}
	NRM_TRY(nrm_fill_zero(pl->flags.p, 32, (void*)st));
	if (pl->adopted || dg_on_device) NRM_HIP(hipDeviceSynchronize());  // (whatever the caller queued to fill its matrices is through before they are read)
	NRM_TRY(plan_set_design(pl.get(), g));
	if (!pl->adopted) NRM_TRY(plan_upload(pl.get(), "nrm_single1_plan_create", dt));
	NRM_HIP(hipStreamSynchronize(st));
	*plan = pl.release();
	return NRM_OK;
}

extern "C" int nrm_single1_plan_design(nrm_single1_plan* plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices,
									   int64_t nnz, int dg_on_device) {
	NRM_REQUIRE(plan != nullptr, "nrm_single1_plan_design: null plan");
	const NrmDePlanDesign g = nrm_de_plan_design_of(design_form, dg, dg_dtype, ldg, indptr, indices, nnz, dg_on_device, plan->n);
	NRM_TRY(nrm_de_plan_design_args("nrm_single1_plan_design", g, plan->ng0, plan->n));
	return nrm_plan_new_design(plan, g, plan_set_design);
}

extern "C" int nrm_single1_plan_upload(nrm_single1_plan* plan, const void* h_dt) {
	NRM_TRY(plan_bind(plan, "nrm_single1_plan_upload"));
	return plan_upload(plan, "nrm_single1_plan_upload", h_dt);
}

// (in the capture of the second step on a design the side stream joins through the fork event: plan_enqueue)
extern "C" int nrm_single1_plan_step(nrm_single1_plan* plan, void* stream) {
	NRM_TRY(plan_bind(plan, "nrm_single1_plan_step"));
	return nrm_plan_step(*plan, "nrm_single1_plan_step", stream, [plan](hipStream_t st) { return plan_enqueue(plan, st); });
}

extern "C" int nrm_single1_plan_check(nrm_single1_plan* plan) {
	NRM_REQUIRE(plan != nullptr, "nrm_single1_plan_check: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_single1_plan_check"));
	return plan_check(plan);
}

extern "C" int nrm_single1_plan_results(nrm_single1_plan* plan, void* h_p, void* h_gamma, void* h_alpha, void* h_varg, void* h_vart, void* h_q) {
	NRM_REQUIRE(plan != nullptr, "nrm_single1_plan_results: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_single1_plan_results"));
	NRM_REQUIRE(plan->steps > 0, "nrm_single1_plan_results: no step has run");
	NRM_REQUIRE(!h_alpha || plan->want_alpha, "nrm_single1_plan_results: the plan was created without alpha");
	NRM_REQUIRE(!h_q || plan->want_q, "nrm_single1_plan_results: the plan was created without q-values");
	NRM_TRY(plan_check(plan));
	const size_t es = nrm_esize(plan->out_dtype), ob = (size_t)plan->ng0 * plan->nt * es;
	NRM_TRY(copy_out(h_p, plan->P.p, ob));
	NRM_TRY(copy_out(h_gamma, plan->G.p, ob));
	NRM_TRY(copy_out(h_alpha, plan->A.p, ob * plan->nc));
	NRM_TRY(copy_out(h_varg, plan->varg.p, (size_t)plan->ng0 * es));
	NRM_TRY(copy_out(h_vart, plan->V.p, ob));
	NRM_TRY(copy_out(h_q, plan->q.p, ob));
	return NRM_OK;
}

extern "C" int nrm_single1_plan_device_results(nrm_single1_plan* plan, void** d_p, void** d_gamma, void** d_alpha, void** d_varg, void** d_q, void** d_vart, void** d_mask,
											   int64_t* ld) {
	NRM_REQUIRE(plan != nullptr, "nrm_single1_plan_device_results: null plan");
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

extern "C" int nrm_single1_plan_stream(nrm_single1_plan* plan, void** stream) {
	return nrm_plan_stream(plan, "nrm_single1_plan_stream", stream);
}

extern "C" int nrm_single1_plan_info(nrm_single1_plan* plan, int64_t info[8]) {
	NRM_REQUIRE(plan != nullptr && info != nullptr, "nrm_single1_plan_info: null pointer");
	info[0] = 0, info[1] = plan->exec ? 1 : 0, info[2] = plan->steps, info[3] = plan->n_kept, info[4] = plan->nc, info[5] = 0, info[6] = plan->bytes, info[7] = plan->ngk;
	return NRM_OK;
}

extern "C" int nrm_single1_plan_time(nrm_single1_plan* plan, int64_t steps, double* ms_per_step) {
	NRM_TRY(plan_bind(plan, "nrm_single1_plan_time"));
	return nrm_plan_time(*plan, "nrm_single1_plan_time", steps, ms_per_step, [plan] { return nrm_single1_plan_step(plan, nullptr); });
}

extern "C" int nrm_single1_plan_destroy(nrm_single1_plan* plan) { return nrm_plan_destroy(plan); }
