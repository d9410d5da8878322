// Resident coex plan behind the C ABI (include/normalisr_hip.h: nrm_coex_plan_*): the problem of coex (dy = dx, single=0; reference coex.py:4-48 over
// association.py:761-1093) stays in HBM, a step is K1 -> K2 -> K3 -> variances enqueued on one stream, and from the second step on one hipGraphLaunch (nrm_plan_core.h).  numpy and
// the library are all a caller needs: no torch, no LAPACK (nrm_covariates_pinv).  The launch sequence is the one nrm_association_tests_host runs
// (nrm_assoc_k1 / nrm_assoc_band, nrm_host_entry.h), so a step's results are that entry's results.
//
// Inside a step: kernel launches only.  Every buffer is taken from the scratch pool at create and given back at destroy; the covariates, their pseudo-inverse and
// max |C_c| are uploaded at create; the result counters are read and cleared by check, never by a step; the guard's tolerance and the K2 engine are fixed at create.
#include <memory>
#include "nrm_device.h"
#include "nrm_host_entry.h"
#include "nrm_plan_core.h"

struct nrm_coex_plan : NrmPlanCore {
	int64_t ng = 0, n = 0, ld = 0, nc = 0, mp = 0, kp = 0;
	int x_dtype = NRM_F64, out_dtype = NRM_F64, nslices = 0, rank = 0, dimreduce = 0;
	bool adopted = false;
	double dof = 0.0, guard_tol = 0.0;
	const void* dt = nullptr;  // the matrix a step reads: own_dt, or the caller's
	DevBuf own_dt, dc, dci, cmax, q, e, fix, rows, ss, dot, gwork, flags, p, stat, var;
	int64_t reruns = 0;
	~nrm_coex_plan() { shutdown(); }  // (its body runs before the DevBuf members go back to the pool: NrmPlanCore::shutdown)
};

namespace {

// K1 -> K2 -> K3 -> variances, on st.  nslices / d_rows: the plan's engine and buffers, or 0 and fp64 rows of one pass for the guard's rerun.
int plan_enqueue(nrm_coex_plan* pl, int nslices, double* d_rows, hipStream_t st) {
	NRM_TRY(nrm_assoc_k1(pl->dt, pl->x_dtype, pl->ng, pl->n, pl->ld, pl->dc.as<double>(), pl->nc, pl->dci.as<double>(), pl->rank, pl->kp, pl->mp, pl->ss.as<double>(), nullptr,
						 nslices, pl->q.p, pl->e.as<int32_t>(), pl->cmax.as<double>(), pl->fix.as<double>(), d_rows, st));
	NrmAssocOperands o;
	o.qx = o.qy = pl->q.p, o.ex = o.ey = pl->e.as<int32_t>(), o.fx = o.fy = pl->fix.as<double>(), o.rx = o.ry = d_rows, o.ssx = o.ssy = pl->ss.as<double>();
	o.nx = o.ny = pl->ng, o.n = pl->n, o.mp = o.np_ = pl->mp, o.kp = pl->kp;
	o.nslices = nslices, o.samexy = 1, o.stat_kind = 0, o.out_dtype = pl->out_dtype, o.dof = pl->dof, o.guard_tol = pl->guard_tol;
	o.dot = pl->dot.as<double>(), o.gwork = pl->gwork.p, o.flags = pl->flags.as<int32_t>();
	o.p = pl->p.p, o.stat = pl->stat.p;
	NRM_TRY(nrm_assoc_band(o, 0, pl->ng, st));  // all rows as one band: the entry cuts bands to ship finished rows meanwhile, here nothing leaves HBM (and every band has a tail)
	const dim3 grid((unsigned)((pl->ng + 255) / 256));
	if (pl->out_dtype == NRM_F64)
		hipLaunchKernelGGL(k_plan_var<double>, grid, dim3(256), 0, st, pl->ss.as<double>(), pl->ng, (double)pl->n, pl->var.p);
	else
		hipLaunchKernelGGL(k_plan_var<float>, grid, dim3(256), 0, st, pl->ss.as<double>(), pl->ng, (double)pl->n, pl->var.p);
	return nrm_check_launch("k_plan_var");
}

int plan_bind(nrm_coex_plan* pl, const char* who) {
	NRM_REQUIRE(pl != nullptr, "%s: null plan", who);
	NRM_HIP(hipSetDevice(pl->device));
	return NRM_OK;
}

int plan_upload(nrm_coex_plan* pl, const char* who, const void* h_dt) {
	return nrm_plan_upload(*pl, who, pl->adopted, h_dt, pl->own_dt.p, pl->ng * pl->n * (int64_t)nrm_esize(pl->x_dtype));
}

// reads and clears the counters once the last step is through; the guard's rerun; caller holds nrm_host_entry_mutex
int plan_check(nrm_coex_plan* pl, int64_t* guard_hits, double* guard_worst) {
	hipStream_t st = pl->last ? pl->last : pl->own;
	if (guard_hits) *guard_hits = 0;
	if (guard_worst) *guard_worst = 0.0;
	int32_t hf[4];
	NRM_HIP(hipDeviceSynchronize());  // (steps may have gone to several streams since the last check: all of them are through before the counters are read)
	NRM_TRY(nrm_read_flags(pl->flags.p, st, hf));
	NRM_TRY(nrm_fill_zero(pl->flags.p, 16, (void*)st));
	NRM_HIP(hipStreamSynchronize(st));
	NRM_TRY(nrm_assoc_assertions(hf, " tiles"));
	if (!pl->nslices) return NRM_OK;
	float w;
	memcpy(&w, &hf[3], 4);
	if (guard_worst) *guard_worst = (double)w;
	if (hf[2] <= 0) return NRM_OK;
	// pairs the guard could not certify since the last check: the step again on the fp64 Gram kernel, from the matrix as it stands (what nrm_association_tests_host does)
	if (guard_hits) *guard_hits = hf[2];
	DevBuf rows;
	NRM_TRY(rows.alloc((size_t)pl->mp * pl->kp * 8));
	NRM_TRY(plan_enqueue(pl, 0, rows.as<double>(), st));
	pl->reruns++;
	NRM_TRY(nrm_read_flags(pl->flags.p, st, hf));
	NRM_TRY(nrm_fill_zero(pl->flags.p, 16, (void*)st));
	NRM_HIP(hipStreamSynchronize(st));
	return nrm_assoc_assertions(hf, " tiles");
}

}  // namespace

extern "C" int nrm_coex_plan_create(nrm_coex_plan** plan, const void* dt, int dt_dtype, int64_t ng, int64_t n_cells, int64_t ld, int dt_on_device, const void* h_dc, int c_dtype,
									int64_t nc, const double* h_dci, int rank, int dimreduce, int out_dtype) {
	NRM_REQUIRE(plan != nullptr, "nrm_coex_plan_create: null plan pointer");
	*plan = nullptr;
	NRM_REQUIRE((dt_dtype == NRM_F32 || dt_dtype == NRM_F64) && (out_dtype == NRM_F32 || out_dtype == NRM_F64) && (nc <= 0 || c_dtype == NRM_F32 || c_dtype == NRM_F64),
				"nrm_coex_plan_create: bad dtype");
	const int64_t n = n_cells;
	if (ld == 0) ld = n;
	// the covariates' pseudo-inverse and rank when the caller has none (host arithmetic), then every check of the whole-problem entry: all before any device call
	std::vector<double> c64, own_dci;
	NRM_REQUIRE(nc >= 0 && (nc == 0 || h_dc) && n > 0, "Incorrect dx/dy/dc size.");
	nrm_covariates_to_f64(h_dc, c_dtype, (size_t)(nc * n), c64);
	if (!h_dci && nc > 0) {
		if (nc > 32) {
			nrm_set_error("nrm_coex_plan_create: the library computes the pseudo-inverse of at most 32 covariates (pass h_dci and rank for more)");
			return NRM_E_UNSUPPORTED;
		}
		own_dci.resize((size_t)(nc * nc));
		NRM_TRY(nrm_covariates_pinv_f64(c64.data(), nc, n, 1e-8, own_dci.data(), &rank));
		h_dci = own_dci.data();
	}
	NRM_TRY(nrm_assoc_check_args(dt, ng, ng, h_dc, nc, n, rank, dimreduce));
	NRM_REQUIRE(dimreduce >= 0, "dimreduce must be a non-negative integer.");
	NRM_REQUIRE(dt_on_device ? ld >= n : ld == n, "nrm_coex_plan_create: row pitch smaller than the row (a host matrix is contiguous)");

	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	std::unique_ptr<nrm_coex_plan> pl(new nrm_coex_plan);
	NRM_HIP(hipGetDevice(&pl->device));
	pl->ng = ng, pl->n = n, pl->ld = ld, pl->nc = nc, pl->x_dtype = dt_dtype, pl->out_dtype = out_dtype, pl->rank = rank, pl->dimreduce = dimreduce;
	pl->adopted = dt_on_device != 0;
	pl->dof = (double)(n - 1 - rank - dimreduce);
	pl->guard_tol = nrm_guard_tolerance();
	pl->mp = nrm_round_up(ng, NRM_ROW_TILE), pl->kp = nrm_round_up(n, NRM_K_TILE);
	NRM_HIP(hipStreamCreateWithFlags(&pl->own, hipStreamNonBlocking));
	if (pl->adopted)
		pl->dt = dt;
	else {
		NRM_TRY(pl->take(pl->own_dt, (size_t)ng * n * nrm_esize(dt_dtype)));
		pl->dt = pl->own_dt.p;
	}
	// K1's fused quantiser reads 16-byte aligned rows: a matrix that has none takes the fp64 kernel
	NRM_TRY(nrm_assoc_engine(n, (uintptr_t)pl->dt % 16 == 0 && ld % 4 == 0, &pl->nslices));
	const int64_t mp = pl->mp, kp = pl->kp;
	if (nc > 0) {
		NRM_TRY(pl->take(pl->dc, c64.size() * 8));
		NRM_HIP(hipMemcpy(pl->dc.p, c64.data(), c64.size() * 8, hipMemcpyHostToDevice));
		NRM_TRY(covariate_bounds(c64, nc, n, h_dci, rank, pl->cmax, pl->dci));
		pl->bytes += nc * 8 + nc * nc * 8;
	}
	if (pl->nslices) {
		NRM_TRY(pl->take(pl->q, (size_t)nrm_quant_bytes(mp, kp, pl->nslices)));
		NRM_TRY(pl->take(pl->e, (size_t)mp * 4));
		NRM_TRY(pl->take(pl->fix, (size_t)mp * NRM_FIX_STRIDE * 8));
	} else
		NRM_TRY(pl->take(pl->rows, (size_t)mp * kp * 8));
	NRM_TRY(pl->take(pl->ss, (size_t)mp * 8));
	NRM_TRY(pl->take(pl->dot, (size_t)mp * mp * 8));
	NRM_TRY(pl->take(pl->gwork, (size_t)nrm_gram_workspace_bytes()));
	NRM_TRY(pl->take(pl->flags, 16));
	const size_t ob = (size_t)ng * ng * nrm_esize(out_dtype);
	NRM_TRY(pl->take(pl->p, ob));
	NRM_TRY(pl->take(pl->stat, ob));
	NRM_TRY(pl->take(pl->var, (size_t)ng * nrm_esize(out_dtype)));
	NRM_TRY(nrm_fill_zero(pl->flags.p, 16, (void*)pl->own));
	if (pl->adopted)
		NRM_HIP(hipDeviceSynchronize());  // (whatever the caller queued to fill its matrix is through before the first step reads it)
	else
		NRM_TRY(plan_upload(pl.get(), "nrm_coex_plan_create", dt));
	*plan = pl.release();
	return NRM_OK;
}

extern "C" int nrm_coex_plan_upload(nrm_coex_plan* plan, const void* h_dt) {
	NRM_TRY(plan_bind(plan, "nrm_coex_plan_upload"));
	return plan_upload(plan, "nrm_coex_plan_upload", h_dt);
}

extern "C" int nrm_coex_plan_step(nrm_coex_plan* plan, void* stream) {
	NRM_TRY(plan_bind(plan, "nrm_coex_plan_step"));
	return nrm_plan_step(*plan, "nrm_coex_plan_step", stream, [plan](hipStream_t st) { return plan_enqueue(plan, plan->nslices, plan->rows.as<double>(), st); });
}

extern "C" int nrm_coex_plan_check(nrm_coex_plan* plan, int64_t* guard_hits, double* guard_worst) {
	NRM_REQUIRE(plan != nullptr, "nrm_coex_plan_check: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_coex_plan_check"));
	return plan_check(plan, guard_hits, guard_worst);
}

extern "C" int nrm_coex_plan_results(nrm_coex_plan* plan, void* h_p, void* h_dot, void* h_var) {
	NRM_REQUIRE(plan != nullptr, "nrm_coex_plan_results: null plan");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(plan_bind(plan, "nrm_coex_plan_results"));
	NRM_REQUIRE(plan->steps > 0, "nrm_coex_plan_results: no step has run");
	NRM_TRY(plan_check(plan, nullptr, nullptr));
	const size_t es = nrm_esize(plan->out_dtype), ob = (size_t)plan->ng * plan->ng * es;
	NRM_TRY(copy_out(h_p, plan->p.p, ob));
	NRM_TRY(copy_out(h_dot, plan->stat.p, ob));
	return copy_out(h_var, plan->var.p, (size_t)plan->ng * es);
}

extern "C" int nrm_coex_plan_device_results(nrm_coex_plan* plan, void** d_p, void** d_dot, void** d_var, int64_t* ld) {
	NRM_REQUIRE(plan != nullptr, "nrm_coex_plan_device_results: null plan");
	if (d_p) *d_p = plan->p.p;
	if (d_dot) *d_dot = plan->stat.p;
	if (d_var) *d_var = plan->var.p;
	if (ld) *ld = plan->ng;
	return NRM_OK;
}

extern "C" int nrm_coex_plan_stream(nrm_coex_plan* plan, void** stream) {
	return nrm_plan_stream(plan, "nrm_coex_plan_stream", stream);
}

extern "C" int nrm_coex_plan_info(nrm_coex_plan* plan, int64_t info[8]) {
	NRM_REQUIRE(plan != nullptr && info != nullptr, "nrm_coex_plan_info: null pointer");
	info[0] = plan->nslices, info[1] = plan->exec ? 1 : 0, info[2] = plan->steps, info[3] = plan->reruns, info[4] = plan->rank, info[5] = (int64_t)plan->dof, info[6] = plan->bytes, info[7] = 0;
	return NRM_OK;
}

extern "C" int nrm_coex_plan_time(nrm_coex_plan* plan, int64_t steps, double* ms_per_step) {
	NRM_TRY(plan_bind(plan, "nrm_coex_plan_time"));
	return nrm_plan_time(*plan, "nrm_coex_plan_time", steps, ms_per_step, [plan] { return nrm_coex_plan_step(plan, nullptr); });
}

extern "C" int nrm_coex_plan_destroy(nrm_coex_plan* plan) { return nrm_plan_destroy(plan); }
