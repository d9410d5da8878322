// Resident de plan behind the C ABI (include/normalisr_hip.h: nrm_de_plan_*): de(dg, dt, dc) with single=0 on a sparse design (reference de.py:4-132 over
// association.py:224-249) for a caller that repeats it on a screen of one shape -- numpy and the library are all it needs.  The design is filtered (de.py:93), compacted
// and turned into the lists of csrc/nrm_design_lists.hip when it is set (nrm_de_design.hip, shared with the single=1 plan); a step is NrmDeSparseStep
// (nrm_de_sparse_step.h: the record nrm_host_de_sparse runs too), then the kernels of this file: the re-inflation of de.py:107-122, the variances, the assertions of
// de.py:124-131 as a count, and nrm_bh.  One stream, launches and memset nodes only; from the second step on a route one hipGraphLaunch.
//
// Every buffer a step needs is taken from the scratch pool at create (sized for all ng0 design rows, so a new design of the same shape fits); the lists are sized by the
// design's entries and are retaken by nrm_de_plan_design.  The buffers of the dense route (K1 + the fp64 Gram kernel, after a hand-back) are taken when check first needs them.
#include <memory>
#include "nrm_device.h"
#include "nrm_host_entry.h"
#include "nrm_design.h"
#include "nrm_de_design.h"
#include "nrm_plan_core.h"
#include "nrm_de_sparse_step.h"

namespace {

// ---- the finish kernel: de._inflate on the device (de.py:107-122) ----------------------------------------------------------------------------------------------
// Design row i = blockIdx.y (strided): its nt P-values and gammas and its nt * nc coefficients come from compact row f2c[i], or are 1, 0 and 0 for a row that was
// not tested.  Every element of the three full-size arrays is written once.  (A plan that tests every row has the sweep write the full-size arrays itself.)
template <typename T>
__global__ __launch_bounds__(256) void k_de_inflate(const T* __restrict__ cp, const T* __restrict__ cg, const T* __restrict__ ca, const int32_t* __restrict__ f2c, int64_t ng0,
													int64_t nt, int64_t nc, T* __restrict__ P, T* __restrict__ G, T* __restrict__ A) {
	const int64_t j0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
	for (int64_t i = blockIdx.y; i < ng0; i += gridDim.y) {
		const int64_t c = f2c[i];
		for (int64_t j = j0; j < nt; j += step) {
			P[i * nt + j] = c >= 0 ? cp[c * nt + j] : (T)1;
			G[i * nt + j] = c >= 0 ? cg[c * nt + j] : (T)0;
		}
		if (A != nullptr) {
			const int64_t wide = nt * nc;
			for (int64_t j = j0; j < wide; j += step) A[i * wide + j] = c >= 0 ? ca[c * wide + j] : (T)0;
		}
	}
}

// varg (ng0) = ss / n with the 0 -> 1 rule for a tested row, 0 for the others, rounded once to the output dtype (the genes' variances: k_plan_var, nrm_host_entry.h)
template <typename T>
__global__ void k_de_varg(const double* __restrict__ ssx, const int32_t* __restrict__ f2c, int64_t ng0, double n, T* __restrict__ varg) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= ng0) return;
	const int64_t c = f2c[i];
	double v = 0.0;
	if (c >= 0) {
		v = ssx[c] / n;
		if (v == 0.0) v = 1.0;
	}
	varg[i] = (T)v;
}

// ---- the bounds kernel: the assertions of de.py:124-131 as a count ---------------------------------------------------------------------------------------------
// P finite within [0, 1], gamma finite, varg and the vart vector finite and >= 0.  Entries that fail are counted by wave and added with one integer atomic per wave
// that found any: the count does not depend on the order.
template <typename T>
__global__ __launch_bounds__(256) void k_de_bounds(const T* __restrict__ P, const T* __restrict__ G, int64_t cnt, const T* __restrict__ varg, int64_t ng0,
												   const T* __restrict__ vart, int64_t nt, int32_t* __restrict__ counter) {
	const T inf = (T)INFINITY;
	const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
	int bad = 0;
	for (int64_t i = t0; i < cnt; i += step) {
		const T p = P[i], g = G[i];
		bad += !(p >= (T)0 && p <= (T)1) ? 1 : 0;
		bad += !(g > -inf && g < inf) ? 1 : 0;
	}
	for (int64_t i = t0; i < ng0; i += step) bad += !(varg[i] >= (T)0 && varg[i] < inf) ? 1 : 0;
	for (int64_t i = t0; i < nt; i += step) bad += !(vart[i] >= (T)0 && vart[i] < inf) ? 1 : 0;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
	if ((threadIdx.x & 63) == 0 && bad > 0) atomicAdd(counter, bad);
}

}  // namespace

struct nrm_de_plan : NrmPlanCore {
	static constexpr const char* name = "nrm_de_plan";
	int64_t ng0 = 0, nt = 0, n = 0, ldt = 0, nc = 0, ngk = 0;
	int g_dtype = NRM_F64, t_dtype = NRM_F64, out_dtype = NRM_F64, rank = 0, dimreduce = 0;
	bool adopted = false, want_alpha = false, want_q = false, dense_route = false, dense_ready = false;
	double guard_tol = 0.0;
	const void* dt = nullptr;  // the matrix a step reads: own_dt, or the caller's
	int64_t kp = 0, bh_bytes = 0;
	std::unique_ptr<NrmDesignLists> L;
	NrmDeSparseStep s;  // the sparse step's sizes, buffers and launches; the dense route writes the same ssx, bx, ssy, by, dot and counters
	// set at create, for all ng0 rows
	DevBuf own_dt, dc, dci, cmax, mask, c2f, f2c, cp, cg, ca, P, G, A, varg, vart, q, bhwork;
	// the dense route
	DevBuf gd, rx, ry, gwork;
	int64_t reruns = 0, list_bytes = 0;
	~nrm_de_plan() { shutdown(); }  // (its body runs before the DevBuf members go back to the pool: NrmPlanCore::shutdown)
	bool all_rows() const { return ngk == ng0; }
	// what the sweep and nrm_alpha write: the full-size arrays when every row is tested, the compact ones otherwise
	void* sweep_p() const { return all_rows() ? P.p : cp.p; }
	void* sweep_g() const { return all_rows() ? G.p : cg.p; }
	void* sweep_a() const { return all_rows() ? A.p : ca.p; }
};

namespace {

// The design of the plan from `in` (nrm_de_design.hip: the row filter, the row map, the rows kept compacted, their lists with the ELL form).  The caller has synchronised
// the device and dropped the graph.
int plan_set_design(nrm_de_plan* pl, const NrmDePlanDesign& in) {
	NrmDeDesign d;
	NRM_TRY(nrm_de_design_set("nrm_de_plan", in, pl->ng0, pl->n, pl->mask.as<uint8_t>(), pl->c2f.as<int64_t>(), pl->f2c.as<int32_t>(), true, 0.0, pl->own, d));
	NRM_REQUIRE(d.L->ok, "nrm_de_plan: the design has no entries");
	if (d.ngk != pl->ng0 && !pl->cp.p) {  // the compact results the finish kernel re-inflates: only a plan that drops rows needs them
		const size_t ob = (size_t)pl->ng0 * pl->nt * nrm_esize(pl->out_dtype);
		NRM_TRY(pl->take(pl->cp, ob));
		NRM_TRY(pl->take(pl->cg, ob));
		if (pl->want_alpha) NRM_TRY(pl->take(pl->ca, ob * pl->nc));
	}
	pl->bytes += d.list_bytes - pl->list_bytes;
	pl->list_bytes = d.list_bytes;
	pl->L = std::move(d.L);
	pl->s.L = pl->L.get();
	pl->s.nx = pl->ngk = d.ngk;
	pl->g_dtype = (in.form == 0 || in.values) ? in.dtype : NRM_F64;
	pl->dense_route = false;
	pl->dense_ready = false;
	pl->fresh = 0;
	return NRM_OK;
}

// the record's step, into the full-size arrays or the compact ones
int plan_enqueue_sparse(nrm_de_plan* pl, hipStream_t st) {
	NRM_TRY(pl->s.enqueue_products(st));
	return pl->s.enqueue_sweep(st, pl->sweep_p(), pl->sweep_g(), nullptr, nullptr, pl->sweep_a(), 1);
}

// the same step on K1 and the fp64 Gram kernel (nrm_association_tests_host's second pass): the rows residualised first, no digit planes
int plan_enqueue_dense(nrm_de_plan* pl, hipStream_t st) {
	const int64_t nc = pl->nc, n = pl->n, nt = pl->nt, nx = pl->ngk, mp = nrm_round_up(nx, NRM_ROW_TILE);
	if (pl->want_alpha) {
		NRM_HIP(hipMemsetAsync(pl->s.bx.p, 0, (size_t)nx * nc * 8, st));
		NRM_HIP(hipMemsetAsync(pl->s.by.p, 0, (size_t)nt * nc * 8, st));
	}
	NRM_TRY(nrm_assoc_k1(pl->gd.p, pl->g_dtype, nx, n, n, pl->dc.as<double>(), nc, pl->dci.as<double>(), pl->rank, pl->kp, mp, pl->s.ssx.as<double>(),
						 pl->want_alpha ? pl->s.bx.as<double>() : nullptr, 0, nullptr, nullptr, pl->cmax.as<double>(), nullptr, pl->rx.as<double>(), st));
	NRM_TRY(nrm_assoc_k1(pl->dt, pl->t_dtype, nt, n, pl->ldt, pl->dc.as<double>(), nc, pl->dci.as<double>(), pl->rank, pl->kp, pl->s.nyp, pl->s.ssy.as<double>(),
						 pl->want_alpha ? pl->s.by.as<double>() : nullptr, 0, nullptr, nullptr, pl->cmax.as<double>(), nullptr, pl->ry.as<double>(), st));
	NrmAssocOperands o;
	o.rx = pl->rx.as<double>(), o.ry = pl->ry.as<double>(), o.ssx = pl->s.ssx.as<double>(), o.ssy = pl->s.ssy.as<double>();
	o.nx = nx, o.ny = nt, o.n = n, o.mp = mp, o.np_ = pl->s.nyp, o.kp = pl->kp;
	o.nslices = 0, o.samexy = 0, o.stat_kind = 1, o.out_dtype = pl->out_dtype, o.dof = pl->s.dof, o.guard_tol = pl->guard_tol;
	o.dot = pl->s.dot.as<double>(), o.gwork = pl->gwork.p, o.flags = pl->s.flags.as<int32_t>();
	o.p = pl->sweep_p(), o.stat = pl->sweep_g();
	for (int64_t a = 0; a < nx; a += NRM_ASSOC_BAND) NRM_TRY(nrm_assoc_band(o, a, std::min(nx, a + NRM_ASSOC_BAND), st));
	if (pl->want_alpha)
		NRM_TRY(nrm_alpha(pl->sweep_g(), pl->out_dtype, nt, 1, pl->s.ssx.as<double>(), n, pl->s.bx.as<double>(), pl->s.by.as<double>(), nx, nt, nc, pl->sweep_a(), pl->out_dtype, st));
	return NRM_OK;
}

template <typename T>
int plan_finish(nrm_de_plan* pl, hipStream_t st) {
	const int64_t ng0 = pl->ng0, nt = pl->nt;
	if (!pl->all_rows()) {
		const int64_t wide = pl->want_alpha ? nt * pl->nc : nt, gx = std::min<int64_t>((wide + 255) / 256, 64);
		const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(ng0, 65535));
		hipLaunchKernelGGL(k_de_inflate<T>, grid, dim3(256), 0, st, pl->cp.as<T>(), pl->cg.as<T>(), pl->want_alpha ? pl->ca.as<T>() : (const T*)nullptr, pl->f2c.as<int32_t>(), ng0,
						   nt, pl->nc, pl->P.as<T>(), pl->G.as<T>(), pl->want_alpha ? pl->A.as<T>() : (T*)nullptr);
		NRM_TRY(nrm_check_launch("k_de_inflate"));
	}
	hipLaunchKernelGGL(k_de_varg<T>, dim3((unsigned)((ng0 + 255) / 256)), dim3(256), 0, st, pl->s.ssx.as<double>(), pl->f2c.as<int32_t>(), ng0, (double)pl->n, pl->varg.as<T>());
	NRM_TRY(nrm_check_launch("k_de_varg"));
	hipLaunchKernelGGL(k_plan_var<T>, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, pl->s.ssy.as<double>(), nt, (double)pl->n, pl->vart.p);
	NRM_TRY(nrm_check_launch("k_plan_var"));
	const int64_t cnt = ng0 * nt, blocks = std::min<int64_t>((cnt + 1023) / 1024, 2048);
	hipLaunchKernelGGL(k_de_bounds<T>, dim3((unsigned)blocks), dim3(256), 0, st, pl->P.as<T>(), pl->G.as<T>(), cnt, pl->varg.as<T>(), ng0, pl->vart.as<T>(), nt,
					   pl->s.flags.as<int32_t>() + 4);
	NRM_TRY(nrm_check_launch("k_de_bounds"));
	if (pl->want_q)
		NRM_TRY(nrm_bh(pl->P.p, pl->out_dtype, ng0, nt, nt, pl->q.p, nt, pl->bhwork.p, pl->bh_bytes, pl->s.flags.as<int32_t>() + 6, (void*)st));
	return NRM_OK;
}

int plan_enqueue(nrm_de_plan* pl, hipStream_t st) {
	NRM_TRY(pl->dense_route ? plan_enqueue_dense(pl, st) : plan_enqueue_sparse(pl, st));
	return pl->out_dtype == NRM_F64 ? plan_finish<double>(pl, st) : plan_finish<float>(pl, st);
}

int plan_upload(nrm_de_plan* pl, const char* who, const void* h_dt) {
	return nrm_plan_upload(*pl, who, pl->adopted, h_dt, pl->own_dt.p, pl->nt * pl->n * (int64_t)nrm_esize(pl->t_dtype));
}

// the dense route's buffers, once, and the compacted design as a matrix: written from the entries of the lists (their CSR form holds every entry of the rows kept)
int plan_dense_ready(nrm_de_plan* pl, hipStream_t st) {
	const int64_t mp0 = pl->s.nxp;
	if (!pl->rx.p) {
		NRM_TRY(pl->take(pl->gd, (size_t)pl->ng0 * pl->n * 8));  // (room for fp64: a later design of the plan may be one)
		NRM_TRY(pl->take(pl->rx, (size_t)mp0 * pl->kp * 8));
		NRM_TRY(pl->take(pl->ry, (size_t)pl->s.nyp * pl->kp * 8));
		NRM_TRY(pl->take(pl->gwork, (size_t)nrm_gram_workspace_bytes()));
	}
	NrmDesignLists& L = *pl->L;
	NRM_TRY(nrm_design_csr_dense(L.row_ptr.as<int64_t>(), L.cells.as<int32_t>(), L.row_vals.p, NRM_F64, pl->ngk, pl->n, pl->gd.p, pl->g_dtype, pl->n, st));
	pl->dense_ready = true;
	return NRM_OK;
}

int plan_counters(nrm_de_plan* pl, hipStream_t st, int32_t (&hf)[8]) {
	NRM_TRY(nrm_read_flags(pl->s.flags.p, st, hf));
	NRM_TRY(nrm_fill_zero(pl->s.flags.p, 32, (void*)st));
	NRM_HIP(hipStreamSynchronize(st));
	NRM_TRY(nrm_assoc_assertions(hf, " tiles"));
	if (hf[4] > 0) {
		nrm_set_error("de results failed the reference's assertions (de.py:124-131): %d entries of P, gamma, varg or vart not finite or out of range", hf[4]);
		return NRM_E_NUMERIC;
	}
	return NRM_OK;
}

// reads and clears the counters once the queued steps are through; the hand-back's rerun; caller holds nrm_host_entry_mutex
int plan_check(nrm_de_plan* pl, int64_t* handed_back) {
	hipStream_t st = pl->last ? pl->last : pl->own;
	if (handed_back) *handed_back = 0;
	int32_t hf[8];
	NRM_HIP(hipDeviceSynchronize());
	NRM_TRY(plan_counters(pl, st, hf));
	if (pl->dense_route || pl->steps == 0 || hf[2] <= 0) return NRM_OK;
	// rows all but inside the span of the covariates since the last check: the step again on K1 and the fp64 Gram kernel from the matrices as they stand, and that
	// route from here on, until the design is replaced
	if (handed_back) *handed_back = hf[2];
	NRM_TRY(plan_dense_ready(pl, st));
	pl->drop_graph();
	pl->dense_route = true;
	pl->fresh = 1;
	NRM_TRY(plan_enqueue(pl, st));
	pl->reruns++;
	return plan_counters(pl, st, hf);
}

}  // namespace

extern "C" int nrm_de_plan_create(nrm_de_plan** plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
								  int dg_on_device, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n_cells, int64_t ldt, int dt_on_device, const void* h_dc,
								  int c_dtype, int64_t nc, const double* h_dci, int rank, int dimreduce, int out_dtype, int want_alpha, int want_q) {
	NRM_REQUIRE(plan != nullptr, "nrm_de_plan_create: null plan pointer");
	*plan = nullptr;
	const int64_t n = n_cells;
	if (ldt == 0) ldt = n;
	const NrmDePlanDesign g = nrm_de_plan_design_of(design_form, dg, dg_dtype, ldg, indptr, indices, nnz, dg_on_device, n);
	// every check, the covariates' pseudo-inverse and rank when the caller has none included (host arithmetic, nrm_de_plan_args.h): all before any device call
	std::vector<double> c64, own_dci;
	NRM_TRY(nrm_de_plan_create_args(g, ng0, dt, dt_dtype, nt, n, ldt, dt_on_device, h_dc, c_dtype, nc, &h_dci, &rank, dimreduce, out_dtype, nrm_de_sparse_max_covariates(), c64,
									own_dci));
	int64_t bh_bytes = 0;
	NRM_TRY(nrm_plan_bh_bytes("nrm_de_plan_create", want_q, ng0 * nt, out_dtype, &bh_bytes));

	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	std::unique_ptr<nrm_de_plan> pl(new nrm_de_plan);
	NRM_HIP(hipGetDevice(&pl->device));
	pl->ng0 = ng0, pl->nt = nt, pl->n = n, pl->ldt = ldt, pl->nc = nc, pl->t_dtype = dt_dtype, pl->out_dtype = out_dtype, pl->rank = rank, pl->dimreduce = dimreduce;
	pl->adopted = dt_on_device != 0;
	pl->want_alpha = want_alpha != 0 && nc > 0, pl->want_q = want_q != 0;
	pl->guard_tol = nrm_guard_tolerance();
	pl->kp = nrm_round_up(n, NRM_K_TILE);
	NrmDeSparseStep& s = pl->s;
	s.rows = ng0, s.ny = nt, s.n = n, s.ldy = ldt, s.nc = nc, s.y_dtype = dt_dtype, s.out_dtype = out_dtype, s.want_alpha = pl->want_alpha;
	s.dof = (double)(n - 1 - rank - dimreduce);
	s.ncu = (rank > 0 && nc > 0) ? nc : 0;  // (covariates of rank 0 -- all zero -- leave the rows as they are: association.py:899-903)
	s.ci = s.ncu ? nrm_constant_row(c64.data(), nc, n, &s.cval) : -1;
	pl->bh_bytes = bh_bytes;
	NRM_HIP(hipStreamCreateWithFlags(&pl->own, hipStreamNonBlocking));
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
		NRM_TRY(covariate_bounds(c64, nc, n, h_dci, rank, pl->cmax, pl->dci));
		pl->bytes += nc * 8 + nc * nc * 8;
	}
	s.d_y = pl->dt, s.d_c = pl->dc.as<double>(), s.d_dci = pl->dci.as<double>();
	auto take = [&pl](DevBuf& b, size_t bytes) { return pl->take(b, bytes); };
	NRM_TRY(s.alloc(take, st));
	const size_t es = nrm_esize(out_dtype), ob = (size_t)ng0 * nt * es;
	NRM_TRY(nrm_take_all(take, {{&pl->mask, ng0}, {&pl->c2f, ng0 * 8}, {&pl->f2c, ng0 * 4}, {&pl->P, ob}, {&pl->G, ob}, {&pl->varg, ng0 * es}, {&pl->vart, nt * es}}));
	if (pl->want_alpha) NRM_TRY(pl->take(pl->A, ob * nc));
	if (pl->want_q) {
		NRM_TRY(pl->take(pl->q, ob));
		NRM_TRY(pl->take(pl->bhwork, (size_t)bh_bytes));
	}
	if (pl->adopted || dg_on_device) NRM_HIP(hipDeviceSynchronize());  // (whatever the caller queued to fill its matrices is through before they are read)
	NRM_TRY(plan_set_design(pl.get(), g));
	if (!pl->adopted) NRM_TRY(plan_upload(pl.get(), "nrm_de_plan_create", dt));
	NRM_HIP(hipStreamSynchronize(st));
	*plan = pl.release();
	return NRM_OK;
}

extern "C" int nrm_de_plan_design(nrm_de_plan* plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
								  int dg_on_device) {
	NRM_REQUIRE(plan != nullptr, "nrm_de_plan_design: null plan");
	const NrmDePlanDesign g = nrm_de_plan_design_of(design_form, dg, dg_dtype, ldg, indptr, indices, nnz, dg_on_device, plan->n);
	NRM_TRY(nrm_de_plan_design_args("nrm_de_plan_design", g, plan->ng0, plan->n));
	return nrm_plan_new_design(plan, g, plan_set_design);
}

extern "C" int nrm_de_plan_upload(nrm_de_plan* plan, const void* h_dt) {
	NRM_TRY(plan_bind(plan, "nrm_de_plan_upload"));
	return plan_upload(plan, "nrm_de_plan_upload", h_dt);
}

// (the graph is of one route: plan_check drops it when it hands back, and the second step on the dense route is captured anew)
extern "C" int nrm_de_plan_step(nrm_de_plan* plan, void* stream) {
	NRM_TRY(plan_bind(plan, "nrm_de_plan_step"));
	return nrm_plan_step(*plan, "nrm_de_plan_step", stream, [plan](hipStream_t st) { return plan_enqueue(plan, st); });
}

extern "C" int nrm_de_plan_check(nrm_de_plan* plan, int64_t* handed_back) {
	NRM_REQUIRE(plan != nullptr, "nrm_de_plan_check: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_de_plan_check"));
	return plan_check(plan, handed_back);
}

extern "C" int nrm_de_plan_results(nrm_de_plan* plan, void* h_p, void* h_gamma, void* h_alpha, void* h_varg, void* h_vart, void* h_q) {
	NRM_REQUIRE(plan != nullptr, "nrm_de_plan_results: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_de_plan_results"));
	NRM_REQUIRE(plan->steps > 0, "nrm_de_plan_results: no step has run");
	NRM_REQUIRE(!h_alpha || plan->want_alpha, "nrm_de_plan_results: the plan was created without alpha");
	NRM_REQUIRE(!h_q || plan->want_q, "nrm_de_plan_results: the plan was created without q-values");
	NRM_TRY(plan_check(plan, nullptr));
	const size_t es = nrm_esize(plan->out_dtype), ob = (size_t)plan->ng0 * plan->nt * es;
	NRM_TRY(copy_out(h_p, plan->P.p, ob));
	NRM_TRY(copy_out(h_gamma, plan->G.p, ob));
	NRM_TRY(copy_out(h_alpha, plan->A.p, ob * plan->nc));
	NRM_TRY(copy_out(h_varg, plan->varg.p, (size_t)plan->ng0 * es));
	NRM_TRY(copy_out(h_q, plan->q.p, ob));
	if (h_vart) {  // the broadcast of de.py:120-122: the genes' variances on every tested row, zero on the others
		std::vector<char> vec, m;
		NRM_TRY(download(vec, plan->vart.p, (size_t)plan->nt * es));
		NRM_TRY(download(m, plan->mask.p, (size_t)plan->ng0));
		const size_t row = (size_t)plan->nt * es;
		for (int64_t i = 0; i < plan->ng0; i++) {
			if (m[(size_t)i])
				memcpy((char*)h_vart + (size_t)i * row, vec.data(), row);
			else
				memset((char*)h_vart + (size_t)i * row, 0, row);
		}
	}
	return NRM_OK;
}

extern "C" int nrm_de_plan_device_results(nrm_de_plan* plan, void** d_p, void** d_gamma, void** d_alpha, void** d_varg, void** d_q, void** d_vart, void** d_mask, int64_t* ld) {
	NRM_REQUIRE(plan != nullptr, "nrm_de_plan_device_results: null plan");
	if (d_p) *d_p = plan->P.p;
	if (d_gamma) *d_gamma = plan->G.p;
	if (d_alpha) *d_alpha = plan->A.p;
	if (d_varg) *d_varg = plan->varg.p;
	if (d_q) *d_q = plan->q.p;
	if (d_vart) *d_vart = plan->vart.p;
	if (d_mask) *d_mask = plan->mask.p;
	if (ld) *ld = plan->nt;
	return NRM_OK;
}

extern "C" int nrm_de_plan_stream(nrm_de_plan* plan, void** stream) {
	return nrm_plan_stream(plan, "nrm_de_plan_stream", stream);
}

extern "C" int nrm_de_plan_info(nrm_de_plan* plan, int64_t info[8]) {
	NRM_REQUIRE(plan != nullptr && info != nullptr, "nrm_de_plan_info: null pointer");
	info[0] = plan->dense_route ? 1 : 0, info[1] = plan->exec ? 1 : 0, info[2] = plan->steps, info[3] = plan->reruns, info[4] = plan->rank, info[5] = (int64_t)plan->s.dof,
	info[6] = plan->bytes, info[7] = plan->ngk;
	return NRM_OK;
}

extern "C" int nrm_de_plan_time(nrm_de_plan* plan, int64_t steps, double* ms_per_step) {
	NRM_TRY(plan_bind(plan, "nrm_de_plan_time"));
	return nrm_plan_time(*plan, "nrm_de_plan_time", steps, ms_per_step, [plan] { return nrm_de_plan_step(plan, nullptr); });
}

extern "C" int nrm_de_plan_destroy(nrm_de_plan* plan) { return nrm_plan_destroy(plan); }
