// The argument checks of the resident single=4 plan (csrc/nrm_single4_plan_args.h: free of HIP headers) under g++ -fsanitize=address,undefined;
// tests/test_single4_plan_cpu.py builds and runs it.  Every operand is a heap buffer of the exact size, so a check that read a cell too many would be caught: the
// shapes, the dtypes, the pitches, dimreduce, tol, the covariate limit, the library's own pseudo-inverse and rank, the caller's rank.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../normalisr_amd/csrc/nrm_single4_plan_args.h"

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
	std::vector<double> dg, dt, dc, c64, own;
	NrmDePlanDesign g;
	int rank = -7;
	explicit Problem(int64_t nc_ = 2, int64_t n_ = 12) : n(n_), nc(nc_) {
		dg.assign((size_t)(ng0 * n), 0.0);
		for (int64_t i = 0; i < ng0; i++) dg[(size_t)(i * n + i % n)] = 1.0;
		dt.assign((size_t)(nt * n), 0.5);
		dc.assign((size_t)(nc * n), 1.0);
		for (int64_t c = 1; c < nc; c++)
			for (int64_t k = 0; k < n; k++) dc[(size_t)(c * n + k)] = std::sin((double)(k * (c + 1))) - 0.25 * (double)c;
		g.form = 0, g.values = dg.data(), g.dtype = NRM_F64, g.ld = n;
	}
	// dci: NULL (the library's own) or the caller's with `caller_rank`
	int run(double tol = 1e-8, int dimreduce = 0, const double* dci = nullptr, int caller_rank = 0, int64_t ldt = -1, int64_t max_cov = 64, bool null_dc = false) {
		rank = caller_rank;
		const double* h_dci = dci;
		const int rc = nrm_single4_plan_create_args(g, ng0, dt.data(), NRM_F64, nt, n, ldt < 0 ? n : ldt, 0, null_dc || !nc ? nullptr : dc.data(), NRM_F64, nc, &h_dci, &rank, dimreduce,
													NRM_F64, tol, max_cov, c64, own);
		if (rc == NRM_OK) {
			CHECK((int64_t)c64.size() == nc * n);
			for (size_t k = 0; k < c64.size(); k++) CHECK(c64[k] == dc[k]);
			CHECK(nc == 0 || h_dci != nullptr);
			if (!dci && nc) CHECK(h_dci == own.data() && (int64_t)own.size() == nc * nc);
		}
		return rc;
	}
};

int main() {
	{  // a good problem: the library's pseudo-inverse and rank; the caller's; no covariates
		Problem p;
		CHECK(p.run() == NRM_OK && p.rank == 2);
		std::vector<double> dci(4, 0.0);
		CHECK(p.run(1e-8, 0, dci.data(), 2) == NRM_OK && p.rank == 2);
		CHECK(p.run(1e-8, 0, dci.data(), 1) == NRM_OK && p.rank == 1);  // (rank-deficient covariates are the plan's to take)
		CHECK(p.run(1e-8, 1000) == NRM_OK);                            // (too few cells waits for the design: the rows kept count)
		Problem q(0);
		CHECK(q.run(1e-8, 0, nullptr, 5) == NRM_OK && q.rank == 0);
	}
	{  // tol, dimreduce, the rank, the pitch, the covariates
		Problem p;
		for (double tol : {0.0, -1e-8, 1.0, 2.0, (double)NAN, (double)INFINITY}) CHECK(p.run(tol) == NRM_E_ARG && !strcmp(g_err, "nrm_single4_plan_create: tol must be a positive number below 1"));
		CHECK(p.run(1e-8, -1) == NRM_E_ARG && !strcmp(g_err, "dimreduce must be a non-negative integer."));
		std::vector<double> dci(4, 0.0);
		CHECK(p.run(1e-8, 0, dci.data(), -1) == NRM_E_ARG && !strcmp(g_err, "Negative dcr detected."));
		CHECK(p.run(1e-8, 0, dci.data(), 3) == NRM_E_ARG && !strcmp(g_err, "dcr higher than covariate dimension."));
		CHECK(p.run(1e-8, 0, dci.data(), 0) == NRM_E_UNSUPPORTED && strstr(g_err, "covariates of rank 0"));
		CHECK(p.run(1e-8, 0, nullptr, 0, p.n + 4) == NRM_E_ARG && strstr(g_err, "row pitch smaller than the row"));
		CHECK(p.run(1e-8, 0, nullptr, 0, -1, 64, true) == NRM_E_ARG && !strcmp(g_err, "Unmatching dx/dy/dc dimensions."));
		CHECK(p.run(1e-8, 0, nullptr, 0, -1, 1) == NRM_E_UNSUPPORTED && strstr(g_err, "at most 1 covariates"));
	}
	{  // all-zero covariates: the library's own rank is 0
		Problem p;
		std::fill(p.dc.begin(), p.dc.end(), 0.0);
		const int rc = p.run();
		CHECK(rc == NRM_E_UNSUPPORTED || rc == NRM_E_ARG || rc == NRM_E_NUMERIC);  // (nrm_covariates_pinv_f64's own refusal, or rank 0)
	}
	{  // 33 covariates without a pseudo-inverse: the library computes at most 32
		Problem p(33, 40);
		CHECK(p.run() == NRM_E_UNSUPPORTED && strstr(g_err, "at most 32 covariates"));
		std::vector<double> dci(33 * 33, 0.0);
		CHECK(p.run(1e-8, 0, dci.data(), 33) == NRM_OK);
	}
	printf("single4 plan args ok\n");
	return 0;
}
