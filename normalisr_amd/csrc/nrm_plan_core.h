// What every resident plan behind the C ABI has and does alike (nrm_coex_plan.hip, nrm_de_plan.hip, nrm_single1_plan.hip, nrm_single4_plan.hip): its device and streams, the graph of its
// step, the counts of steps and pool bytes -- and, written once, the step (eager first, captured second, replayed from then on, eager for good when a capture fails),
// the timing between device events, the upload behind the barrier on `last`, and the teardown.  A plan's struct derives from NrmPlanCore and adds its own fields; what
// it enqueues comes in as a callable.
#pragma once
#include "nrm_host_entry.h"

struct NrmPlanCore {
	int device = 0;
	bool eager_only = false;
	hipStream_t own = nullptr, last = nullptr;  // the plan's own stream; the stream of the last step
	hipGraph_t graph = nullptr;
	hipGraphExec_t exec = nullptr;
	int64_t steps = 0, fresh = 0, bytes = 0;  // fresh: steps since the plan last changed what a step enqueues (a new design, another route)
	int take(DevBuf& b, size_t bytes_) {
		NRM_TRY(b.alloc(bytes_));
		bytes += (int64_t)bytes_;
		return NRM_OK;
	}
	void drop_graph() {
		if (exec) (void)hipGraphExecDestroy(exec);
		if (graph) (void)hipGraphDestroy(graph);
		exec = nullptr, graph = nullptr;
	}
	// Teardown: the device synchronised, the graph destroyed, the stream destroyed.  The plan's destructor BODY calls this (and then destroys what streams and events of
	// its own it has): a destructor's body runs before the members of its class are destroyed, so the DevBuf members go back to the pool only after it.  A destructor
	// of this base would be too late -- it runs after the derived class's members are gone.
	void shutdown() {
		(void)hipSetDevice(device);
		(void)hipDeviceSynchronize();
		drop_graph();
		if (own) (void)hipStreamDestroy(own);
		own = nullptr;
	}
};

// the step stays eager from here on; nrm_last_error keeps the reason (StepGraph's rule, normalisr_amd/distributed.py)
template <typename Enqueue>
int plan_stay_eager(NrmPlanCore& c, const char* entry, const char* what, hipError_t e, hipStream_t st, Enqueue& enqueue) {
	(void)hipGetLastError();
	c.eager_only = true;
	char why[256];
	snprintf(why, sizeof(why), "%s: not captured as a HIP graph (%s: %s); the plan runs eagerly", entry, what, e == hipSuccess ? nrm_last_error() : hipGetErrorString(e));
	NRM_TRY(enqueue(st));
	nrm_set_error("%s", why);
	return NRM_OK;
}

// One step of a bound plan on `stream` (NULL: the plan's own); enqueue(hipStream_t) queues the plan's launches and returns a status.  Eager while fresh < 2 (and with
// NRM_DEBUG graph=0, and after a capture that failed); the second step: recorded, not run (thread-local capture: other threads' HIP calls are none of its business),
// instantiated, launched; one hipGraphLaunch from then on, until drop_graph.
template <typename Enqueue>
int nrm_plan_step(NrmPlanCore& c, const char* entry, void* stream, Enqueue enqueue) {
	hipStream_t st = stream ? (hipStream_t)stream : c.own;
	c.last = st;
	c.steps++;
	c.fresh++;
	if (c.exec) {
		NRM_HIP(hipGraphLaunch(c.exec, st));
		return NRM_OK;
	}
	if (c.eager_only || c.fresh < 2 || nrm_debug_is("graph", "0")) return enqueue(st);
	hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
	if (e != hipSuccess) return plan_stay_eager(c, entry, "hipStreamBeginCapture", e, st, enqueue);
	const int rc = enqueue(st);
	hipGraph_t g = nullptr;
	e = hipStreamEndCapture(st, &g);
	if (rc != NRM_OK || e != hipSuccess || !g) {
		if (g) (void)hipGraphDestroy(g);
		return plan_stay_eager(c, entry, rc != NRM_OK ? "a launch inside the capture" : "hipStreamEndCapture", rc != NRM_OK ? hipSuccess : (e != hipSuccess ? e : hipErrorUnknown), st,
							   enqueue);
	}
	hipGraphExec_t x = nullptr;
	e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
	if (e != hipSuccess || !x) {
		(void)hipGraphDestroy(g);
		return plan_stay_eager(c, entry, "hipGraphInstantiate", e != hipSuccess ? e : hipErrorUnknown, st, enqueue);
	}
	c.graph = g, c.exec = x;
	NRM_HIP(hipGraphLaunch(c.exec, st));
	return NRM_OK;
}

// Milliseconds per step over `steps` steps of a bound plan, between two device events on its own stream; step() is the plan's step entry on that stream.
template <typename Step>
int nrm_plan_time(NrmPlanCore& c, const char* entry, int64_t steps, double* ms_per_step, Step step) {
	NRM_REQUIRE(steps > 0 && ms_per_step != nullptr, "%s: bad arguments", entry);
	while (c.fresh < 2) NRM_TRY(step());  // (the eager step and the capture are not what is timed)
	hipEvent_t t0 = nullptr, t1 = nullptr;
	NRM_HIP(hipEventCreate(&t0));
	hipError_t e = hipEventCreate(&t1);
	int rc = NRM_OK;
	float ms = 0.f;
	if (e == hipSuccess) e = hipEventRecord(t0, c.own);
	for (int64_t i = 0; i < steps && e == hipSuccess && rc == NRM_OK; i++) rc = step();
	if (e == hipSuccess && rc == NRM_OK) e = hipEventRecord(t1, c.own);
	if (e == hipSuccess && rc == NRM_OK) e = hipEventSynchronize(t1);
	if (e == hipSuccess && rc == NRM_OK) e = hipEventElapsedTime(&ms, t0, t1);
	(void)hipEventDestroy(t0);
	if (t1) (void)hipEventDestroy(t1);
	NRM_TRY(rc);
	NRM_HIP(e);
	*ms_per_step = (double)ms / (double)steps;
	return NRM_OK;
}

// New values into the plan's own copy `d` of its matrix (`adopted`: it has none), behind whatever step may still read the copy; returns once they are there.
static inline int nrm_plan_upload(NrmPlanCore& c, const char* entry, bool adopted, const void* h, void* d, int64_t bytes) {
	NRM_REQUIRE(!adopted, "%s: the plan adopted the caller's device matrix (rewrite it in place)", entry);
	NRM_REQUIRE(h != nullptr, "%s: null matrix", entry);
	if (c.last && c.last != c.own) NRM_HIP(hipStreamSynchronize(c.last));  // (a step on the caller's stream may still read the copy)
	NRM_TRY(nrm_upload(h, d, bytes, 0, (void*)c.own));
	NRM_HIP(hipStreamSynchronize(c.own));
	return NRM_OK;
}

static inline int nrm_plan_stream(NrmPlanCore* c, const char* entry, void** stream) {
	NRM_REQUIRE(c != nullptr && stream != nullptr, "%s: null pointer", entry);
	*stream = (void*)c->own;
	return NRM_OK;
}

template <typename Plan>
int nrm_plan_destroy(Plan* plan) {
	if (!plan) return NRM_OK;
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	delete plan;  // (its destructor's body synchronises the device and destroys the graph and the streams; then the buffers go back to the pool)
	return NRM_OK;
}
