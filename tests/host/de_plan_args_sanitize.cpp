// The argument checks of the resident de plan (csrc/nrm_de_plan_args.h: free of HIP headers) under g++ -fsanitize=address,undefined; tests/test_de_plan_cpu.py builds
// it beside csrc/nrm_small_pinv.hip (the pseudo-inverse of the covariates) and runs it.  Every operand is a heap buffer of the exact size, so a check that read
// a cell too many would be caught: the design's forms, the shapes, the dtypes, the covariate limits, the reference's words for too few cells, the library's own rank.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../normalisr_amd/csrc/nrm_de_plan_args.h"

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
		g.form = 0, g.values = dg.data(), g.dtype = NRM_F64, g.ld = n;
	}
	int run(const double* dci, int rank, int dimreduce, int* rank_out = nullptr, int dt_dtype = NRM_F64, int out_dtype = NRM_F64, int64_t ldt = -1, int dt_dev = 0) {
		std::vector<double> c64, own;
		const double* d = dci;
		int r = rank;
		const int rc = nrm_de_plan_create_args(g, ng0, dt.data(), dt_dtype, nt, n, ldt < 0 ? n : ldt, dt_dev, nc ? dc.data() : nullptr, NRM_F64, nc, &d, &r, dimreduce, out_dtype, 32,
											   c64, own);
		if (rc == NRM_OK) {
			CHECK((int64_t)c64.size() == nc * n);
			CHECK(nc == 0 || d != nullptr);
			if (!dci && nc) CHECK((int64_t)own.size() == nc * nc && d == own.data());
		}
		if (rank_out) *rank_out = r;
		return rc;
	}
};

int main() {
	{  // a good problem: the library's own pseudo-inverse, rank 2
		Problem p;
		int r = -1;
		CHECK(p.run(nullptr, 0, 0, &r) == NRM_OK && r == 2);
		CHECK(p.run(nullptr, 0, 9, &r) == NRM_E_ARG && !strcmp(g_err, "Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1."));
		CHECK(p.run(nullptr, 0, -1) == NRM_E_ARG && !strcmp(g_err, "dimreduce must be a non-negative integer."));
		std::vector<double> dci(4, 0.0);
		CHECK(p.run(dci.data(), 3, 0) == NRM_E_ARG && !strcmp(g_err, "dcr higher than covariate dimension."));
		CHECK(p.run(dci.data(), -1, 0) == NRM_E_ARG && !strcmp(g_err, "Negative dcr detected."));
		CHECK(p.run(dci.data(), 2, 0) == NRM_OK);
		CHECK(p.run(nullptr, 0, 0, nullptr, 7) == NRM_E_ARG && strstr(g_err, "bad dtype"));
		CHECK(p.run(nullptr, 0, 0, nullptr, NRM_F32, 5) == NRM_E_ARG && strstr(g_err, "bad dtype"));
		CHECK(p.run(nullptr, 0, 0, nullptr, NRM_F64, NRM_F64, p.n + 4, 0) == NRM_E_ARG && strstr(g_err, "row pitch"));
		CHECK(p.run(nullptr, 0, 0, nullptr, NRM_F64, NRM_F64, p.n + 4, 1) == NRM_OK);  // an adopted matrix may be pitched
		CHECK(p.run(nullptr, 0, 0, nullptr, NRM_F64, NRM_F64, p.n - 1, 1) == NRM_E_ARG);
	}
	{  // the design's forms
		Problem p;
		p.g.values = nullptr;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.g.values = p.dg.data(), p.g.dtype = 9;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && strstr(g_err, "bad dtype"));
		p.g.dtype = NRM_F64, p.g.form = 2;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG);
		p.g.form = 0, p.g.ld = p.n - 1;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && strstr(g_err, "row pitch"));
		p.g.ld = p.n + 3, p.g.on_device = 1;
		CHECK(p.run(nullptr, 0, 0) == NRM_OK);
		// canonical CSR: one entry per row, all ones
		p.indptr = {0, 1, 2, 3, 4};
		p.indices = {0, 1, 2, 3};
		p.g = NrmDePlanDesign();
		p.g.form = 1, p.g.indptr = p.indptr.data(), p.g.indices = p.indices.data(), p.g.nnz = 4, p.g.dtype = NRM_F32;
		CHECK(p.run(nullptr, 0, 0) == NRM_OK);
		p.g.indices = nullptr;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG);
		p.g.nnz = 0;
		CHECK(p.run(nullptr, 0, 0) == NRM_OK);  // (an empty design is refused once its rows are looked at, on the device)
		p.g.indptr = nullptr;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG);
		p.g.indptr = p.indptr.data(), p.g.indices = p.indices.data(), p.g.nnz = p.ng0 * p.n + p.ng0;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && strstr(g_err, "more stored entries"));
		p.g.nnz = -1;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG);
	}
	{  // shapes
		Problem p;
		p.ng0 = 0;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && !strcmp(g_err, "Incorrect dx/dy/dc size."));
		p.ng0 = 4, p.nt = 0;
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG);
		p.nt = 3, p.ng0 = (1ll << 31);
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && strstr(g_err, "2^31"));
	}
	{  // no covariates; 33 without a pseudo-inverse; 33 with one: beyond the kernel
		Problem p0(0);
		int r = -1;
		CHECK(p0.run(nullptr, 0, 0, &r) == NRM_OK && r == 0);
		Problem p33(33, 40);
		std::vector<double> dci(33 * 33, 0.0);
		CHECK(p33.run(nullptr, 0, 0) == NRM_E_UNSUPPORTED);
		CHECK(p33.run(dci.data(), 2, 0) == NRM_E_UNSUPPORTED && strstr(g_err, "at most 32 covariates"));
		Problem p32(32, 40);
		CHECK(p32.run(nullptr, 0, 0, &r) == NRM_OK && r >= 1 && r <= 32);
	}
	{  // the library's own rank decides "too few cells": three cells, two independent covariates
		Problem p(2, 3);
		CHECK(p.run(nullptr, 0, 0) == NRM_E_ARG && !strcmp(g_err, "Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1."));
	}
	printf("de plan args ok\n");
	return 0;
}
