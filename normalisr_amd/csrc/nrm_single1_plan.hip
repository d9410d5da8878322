// Resident single=1 plan behind the C ABI (include/normalisr_hip.h: nrm_single1_plan_*): de(dg, dt, dc, single=1) for a low-MOI screen (reference de.py:4-132 over
// association.py:263-390, 911-925) for a caller that repeats it on a screen of one shape -- numpy and the library are all it needs.  The design is filtered (de.py:93),
// compacted and listed when it is set (nrm_de_design.hip, as for the single=0 plan), BEFORE the cell selection sees it: an all-ones row de drops would otherwise leave no
// cell that carries exactly one grouping.  A step is NrmSingle1Step::enqueue (nrm_single1_step.h: the record the whole-problem entry runs too) on two streams -- the
// selection; beside each other the groupings' statistics and the stream kernel; the results -- then the kernel of this file: the re-inflation of de.py:107-122 with
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
#include "nrm_single1_step.h"

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
	int64_t ng0 = 0, nt = 0, n = 0, nc = 0, ngk = 0;
	int t_dtype = NRM_F64, out_dtype = NRM_F64;
	bool adopted = false, want_alpha = false, want_q = false;
	int64_t bh_bytes = 0;
	std::unique_ptr<NrmDesignLists> L;
	NrmSingle1Step s;  // the step's sizes, buffers and launches; s.d_y, the matrix a step reads: own_dt, or the caller's
	// set at create, for all ng0 rows
	DevBuf own_dt, dc, mask, c2f, f2c, cp, cg, cv, ca, P, G, V, A, varg, q, bhwork;
	hipStream_t side = nullptr;  // the fork of a step: NrmSingle1Step::enqueue
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
};

namespace {

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
	NrmSingle1Step& s = pl->s;
	int64_t db = d.list_bytes;  // what the design's entries size is counted apart: a new design retakes it
	auto take = [&db](DevBuf& b, size_t bytes) { return db += (int64_t)bytes, b.alloc(bytes); };
	s.idx.release(), s.xe.release(), s.ce.release(), s.ye.release();
	NRM_TRY(s.alloc_design(d.L->nnz, take));
	pl->L = std::move(d.L);
	s.L = pl->L.get();
	s.nx = pl->ngk = d.ngk;
	NRM_TRY(s.alloc_kept("nrm_single1_plan", take, st));
	if (!pl->all_rows() && !pl->cp.p) {  // the compact results the finish kernel re-inflates: only a plan that drops rows needs them
		const size_t ob = (size_t)pl->ng0 * pl->nt * nrm_esize(pl->out_dtype);
		NRM_TRY(pl->take(pl->cp, ob));
		NRM_TRY(pl->take(pl->cg, ob));
		NRM_TRY(pl->take(pl->cv, ob));
		if (pl->want_alpha) NRM_TRY(pl->take(pl->ca, ob * pl->nc));
	}
	// what nrm_single1_cells writes: the full-size arrays when every row is tested, the compact ones otherwise
	const bool all = pl->all_rows();
	s.p = all ? pl->P.p : pl->cp.p, s.stat = all ? pl->G.p : pl->cg.p, s.vary = all ? pl->V.p : pl->cv.p;
	s.alpha = !pl->want_alpha ? nullptr : (all ? pl->A.p : pl->ca.p);
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
					   pl->want_alpha ? pl->ca.as<T>() : (const T*)nullptr, pl->s.varx.as<double>(), pl->f2c.as<int32_t>(), ng0, nt, pl->nc, pl->P.as<T>(), pl->G.as<T>(), pl->V.as<T>(),
					   pl->want_alpha ? pl->A.as<T>() : (T*)nullptr, pl->varg.as<T>(), pl->s.flags.as<int32_t>() + S1P_BOUNDS);
	NRM_TRY(nrm_check_launch("k_s1_de_finish"));
	if (pl->want_q)
		NRM_TRY(nrm_bh(pl->P.p, pl->out_dtype, ng0, nt, nt, pl->q.p, nt, pl->bhwork.p, pl->bh_bytes, pl->s.flags.as<int32_t>() + S1P_BH, (void*)st));
	return NRM_OK;
}

// The record's step on the plan's two streams (the launches of Single1Plan._launch, in its order), then the finish kernel.
int plan_enqueue(nrm_single1_plan* pl, hipStream_t st) {
	NRM_TRY(pl->s.enqueue(st, pl->side, pl->forked, pl->joined));
	return pl->out_dtype == NRM_F64 ? plan_finish<double>(pl, st) : plan_finish<float>(pl, st);
}

int plan_upload(nrm_single1_plan* pl, const char* who, const void* h_dt) {
	return nrm_plan_upload(*pl, who, pl->adopted, h_dt, pl->own_dt.p, pl->nt * pl->n * (int64_t)nrm_esize(pl->t_dtype));
}

// reads and clears the counters once the queued steps are through, and says what the reference would have: nrm_single1_status (nrm_single1_plan_args.h), then de's own
// assertions (de.py:124-131); caller holds nrm_host_entry_mutex
int plan_check(nrm_single1_plan* pl) {
	hipStream_t st = pl->last ? pl->last : pl->own;
	int32_t hf[8];
	NRM_HIP(hipDeviceSynchronize());
	NRM_TRY(nrm_read_flags(pl->s.flags.p, st, hf));
	NRM_TRY(nrm_fill_zero(pl->s.flags.p, 32, (void*)st));
	NRM_HIP(hipStreamSynchronize(st));
	NRM_TRY(nrm_single1_status(hf));
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
	pl->ng0 = ng0, pl->nt = nt, pl->n = n, pl->nc = nc, pl->t_dtype = dt_dtype, pl->out_dtype = out_dtype;
	pl->adopted = dt_on_device != 0;
	pl->want_alpha = want_alpha != 0 && nc > 0, pl->want_q = want_q != 0;
	pl->bh_bytes = bh_bytes;
	NrmSingle1Step& s = pl->s;
	s.rows = ng0, s.ny = nt, s.n = n, s.ldy = ldt, s.nc = nc, s.y_dtype = dt_dtype, s.out_dtype = out_dtype, s.dimreduce = dimreduce;
	auto take = [&pl](DevBuf& b, size_t bytes) { return pl->take(b, bytes); };
	NRM_HIP(hipStreamCreateWithFlags(&pl->own, hipStreamNonBlocking));
	NRM_HIP(hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking));
	NRM_HIP(hipEventCreateWithFlags(&pl->forked, hipEventDisableTiming));
	NRM_HIP(hipEventCreateWithFlags(&pl->joined, hipEventDisableTiming));
	hipStream_t st = pl->own;
	if (!pl->adopted) NRM_TRY(pl->take(pl->own_dt, (size_t)nt * n * nrm_esize(dt_dtype)));
	s.d_y = pl->adopted ? dt : pl->own_dt.p;
	if (nc > 0) {
		NRM_TRY(pl->take(pl->dc, c64.size() * 8));
		NRM_HIP(hipMemcpy(pl->dc.p, c64.data(), c64.size() * 8, hipMemcpyHostToDevice));
		s.d_c = pl->dc.as<double>();
	}
	NRM_TRY(s.alloc_fixed(take, st));
	const size_t es = nrm_esize(out_dtype), ob = (size_t)ng0 * nt * es;
	NRM_TRY(nrm_take_all(take, {{&pl->mask, ng0}, {&pl->c2f, ng0 * 8}, {&pl->f2c, ng0 * 4}, {&pl->P, ob}, {&pl->G, ob}, {&pl->V, ob}, {&pl->varg, ng0 * es}}));
	if (pl->want_alpha) NRM_TRY(pl->take(pl->A, ob * nc));
	if (pl->want_q) {
		NRM_TRY(pl->take(pl->q, ob));
		NRM_TRY(pl->take(pl->bhwork, (size_t)bh_bytes));
	}
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
	info[0] = 0, info[1] = plan->exec ? 1 : 0, info[2] = plan->steps, info[3] = plan->s.n_kept, info[4] = plan->nc, info[5] = 0, info[6] = plan->bytes, info[7] = plan->ngk;
	return NRM_OK;
}

extern "C" int nrm_single1_plan_time(nrm_single1_plan* plan, int64_t steps, double* ms_per_step) {
	NRM_TRY(plan_bind(plan, "nrm_single1_plan_time"));
	return nrm_plan_time(*plan, "nrm_single1_plan_time", steps, ms_per_step, [plan] { return nrm_single1_plan_step(plan, nullptr); });
}

extern "C" int nrm_single1_plan_destroy(nrm_single1_plan* plan) { return nrm_plan_destroy(plan); }
