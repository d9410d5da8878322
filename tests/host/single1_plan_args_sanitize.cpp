// The argument checks of the resident single=1 plan (csrc/nrm_single1_plan_args.h: free of HIP headers) under g++ -fsanitize=address,undefined;
// tests/test_single1_plan_cpu.py builds and runs it.  Every operand is a heap buffer of the exact size, so a check that read a cell too many would be caught: the
// design's forms, the shapes, the dtypes, the pitches, dimreduce, the covariate limit, the covariates converted to fp64.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../normalisr_amd/csrc/nrm_single1_plan_args.h"

static char g_err[1024];
void nrm_set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}
#define CHECK(c)                                                                  \
	do {                                                                          \
		if (!(c)) {                                                               \
			fprintf(stderr, "%s:%d: check failed: %s (%s)\n", __FILE__, __LINE__, #c, g_err); \
			exit(1);                                                              \
		}                                                                         \
	} while (0)

struct Problem {
	int64_t ng0 = 4, nt = 3, n = 12, nc = 2;
	std::vector<double> dg, dt, dc;
	std::vector<float> dc32;
	std::vector<int64_t> indptr;
	std::vector<int32_t> indices;
	NrmDePlanDesign g;
	explicit Problem(int64_t nc_ = 2, int64_t n_ = 12) : n(n_), nc(nc_) {
		dg.assign((size_t)(ng0 * n), 0.0);
		for (int64_t i = 0; i < ng0; i++) dg[(size_t)(i * n + i % n)] = 1.0;
		dt.assign((size_t)(nt * n), 0.5);
		dc.assign((size_t)(nc * n), 1.0);
		for (int64_t c = 1; c < nc; c++)
			for (int64_t k = 0; k < n; k++) dc[(size_t)(c * n + k)] = (double)((k * (c + 1)) % 7) - 0.25 * (double)c;
		dc32.assign(dc.begin(), dc.end());
		g.form = 0, g.values = dg.data(), g.dtype = NRM_F64, g.ld = n;
	}
	int run(int dimreduce = 0, int dt_dtype = NRM_F64, int out_dtype = NRM_F64, int64_t ldt = -1, int dt_dev = 0, int c_dtype = NRM_F64, bool null_dc = false, bool null_dt = false) {
		std::vector<double> c64;
		const void* c = null_dc || !nc ? nullptr : (c_dtype == NRM_F32 ? (const void*)dc32.data() : (const void*)dc.data());
		const int rc = nrm_single1_plan_create_args(g, ng0, null_dt ? nullptr : dt.data(), dt_dtype, nt, n, ldt < 0 ? n : ldt, dt_dev, c, c_dtype, nc, dimreduce, out_dtype, c64);
		if (rc == NRM_OK) {
			CHECK((int64_t)c64.size() == nc * n);
			for (size_t k = 0; k < c64.size(); k++) CHECK(c64[k] == (c_dtype == NRM_F32 ? (double)dc32[k] : dc[k]));
		}
		return rc;
	}
};

int main() {
	{  // a good problem, fp64 and fp32 covariates; dimreduce; dtypes; pitches
		Problem p;
		CHECK(p.run() == NRM_OK);
		CHECK(p.run(0, NRM_F32, NRM_F32, -1, 0, NRM_F32) == NRM_OK);
		CHECK(p.run(1000) == NRM_OK);  // (too few cells is the device's to say, per grouping)
		CHECK(p.run(-1) == NRM_E_ARG && !strcmp(g_err, "dimreduce must be a non-negative integer."));
		CHECK(p.run(0, 7) == NRM_E_ARG && !strcmp(g_err, "nrm_single1_plan_create: bad dtype"));
		CHECK(p.run(0, NRM_F32, 5) == NRM_E_ARG && !strcmp(g_err, "nrm_single1_plan_create: bad dtype"));
		CHECK(p.run(0, NRM_F64, NRM_F64, -1, 0, 9) == NRM_E_ARG && !strcmp(g_err, "nrm_single1_plan_create: bad dtype"));
		CHECK(p.run(0, NRM_F64, NRM_F64, p.n + 4, 0) == NRM_E_ARG && strstr(g_err, "row pitch"));
		CHECK(p.run(0, NRM_F64, NRM_F64, p.n + 4, 1) == NRM_OK);  // an adopted matrix may be pitched
		CHECK(p.run(0, NRM_F64, NRM_F64, p.n - 1, 1) == NRM_E_ARG && strstr(g_err, "row pitch"));
		CHECK(p.run(0, NRM_F64, NRM_F64, -1, 0, NRM_F64, true) == NRM_E_ARG && !strcmp(g_err, "Unmatching dx/dy/dc dimensions."));
		CHECK(p.run(0, NRM_F64, NRM_F64, -1, 0, NRM_F64, false, true) == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.nc = -1;
		CHECK(p.run(0, NRM_F64, NRM_F64, -1, 0, NRM_F64, true) == NRM_E_ARG && !strcmp(g_err, "Unmatching dx/dy/dc dimensions."));
	}
	{  // the design's forms
		Problem p;
		p.g.values = nullptr;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.g.values = p.dg.data(), p.g.dtype = 9;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "bad dtype"));
		p.g.dtype = NRM_F64, p.g.form = 2;
		CHECK(p.run() == NRM_E_ARG);
		p.g.form = 0, p.g.ld = p.n - 1;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "row pitch"));
		p.g.ld = p.n + 3, p.g.on_device = 1;
		CHECK(p.run() == NRM_OK);
		// canonical CSR: one entry per row, all ones
		p.indptr = {0, 1, 2, 3, 4};
		p.indices = {0, 1, 2, 3};
		p.g = NrmDePlanDesign();
		p.g.form = 1, p.g.indptr = p.indptr.data(), p.g.indices = p.indices.data(), p.g.nnz = 4, p.g.dtype = NRM_F32;
		CHECK(p.run() == NRM_OK);
		p.g.indices = nullptr;
		CHECK(p.run() == NRM_E_ARG);
		p.g.nnz = 0;
		CHECK(p.run() == NRM_OK);  // (an empty design is refused once its rows are looked at, on the device)
		p.g.indptr = nullptr;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.g.indptr = p.indptr.data(), p.g.indices = p.indices.data(), p.g.nnz = p.ng0 * p.n + p.ng0;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "more stored entries"));
		p.g.nnz = -1;
		CHECK(p.run() == NRM_E_ARG);
	}
	{  // shapes
		Problem p;
		p.ng0 = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.ng0 = 4, p.nt = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.nt = 3, p.ng0 = (1ll << 31);
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "2^31"));
		p.ng0 = 4, p.nt = (1ll << 31);
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "2^31"));
	}
	{  // no covariates; 32: the most; 33: beyond the kernels
		Problem p0(0);
		CHECK(p0.run() == NRM_OK);
		Problem p32(32, 40);
		CHECK(p32.run() == NRM_OK);
		Problem p33(33, 40);
		CHECK(p33.run() == NRM_E_UNSUPPORTED && strstr(g_err, "up to 32 covariates"));
	}
	printf("single1 plan args ok\n");
	return 0;
}
