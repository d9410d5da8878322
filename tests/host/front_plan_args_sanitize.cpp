// The argument checks of the resident front-half plan (csrc/nrm_front_plan_args.h: free of HIP headers) under g++ -fsanitize=address,undefined;
// tests/test_front_plan_cpu.py builds and runs it.  Every operand is a heap buffer of the exact size, so a check that read a cell too many would be caught: null
// pointers, dtypes, shapes and pitches, the covariate bound, a user row that is not finite, a constant user row, eps, stepmax, tol, ntot, count_cap; normcov's row
// classification; and the reading of the plan's sixteen counters in the reference's order: every combination of the ten it reads, and of the two that compute_var
// and normvar each have (nrm_compute_var_status, nrm_normvar_status: what the whole-problem entries say too).  The messages are written out here in full.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../normalisr_amd/csrc/nrm_front_plan_args.h"

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

static const int64_t MAX_COV = 8, TABLE_CAP = 1 << 24;
static const char* const CONSTANT = "Detected constant covariate. Please only provide full-rank covariate without constant covariate.";

struct Problem {
	int64_t rows = 5, n = 12;
	std::vector<int32_t> reads;
	std::vector<double> cov;
	NrmFrontPlanArgs a;
	explicit Problem(int64_t n_cov = 2) {
		reads.assign((size_t)(rows * n), 1);
		cov.assign((size_t)(n_cov * n), 0.0);
		for (int64_t r = 0; r < n_cov; r++)
			for (int64_t k = 0; k < n; k++) cov[(size_t)(r * n + k)] = r == 0 ? (double)(k % 2) : 0.25 * (double)((k * (r + 1)) % 7) - (double)r;  // row 0 one-hot, the others continuous
		a.reads = reads.data(), a.dtype = NRM_I32, a.rows = rows, a.n = n, a.ld = n, a.h_cov = n_cov ? cov.data() : nullptr, a.n_cov = n_cov, a.count_cap = 256;
	}
	int run() { return nrm_front_plan_create_args(a, MAX_COV, TABLE_CAP); }
};

int main() {
	{  // a good problem; the classes of its user rows; every count dtype; both output dtypes; an adopted, pitched matrix
		Problem p;
		CHECK(p.run() == NRM_OK && nrm_normcov_row_class(p.cov.data(), p.n) == NRM_COV_BINARY && nrm_normcov_row_class(p.cov.data() + p.n, p.n) == NRM_COV_CONTINUOUS);
		const int dtypes[4] = {NRM_I64, NRM_I32, NRM_I16, NRM_U8};
		for (int d : dtypes) {
			p.a.dtype = d;  // (the checks never read the counts)
			CHECK(p.run() == NRM_OK);
		}
		p.a.dtype = NRM_F32;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "counts are NRM_I64"));
		p.a.dtype = 7;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "counts are NRM_I64"));
		p.a.dtype = NRM_I32, p.a.out_dtype = NRM_F32;
		CHECK(p.run() == NRM_OK);
		p.a.out_dtype = NRM_I32;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "out_dtype"));
		p.a.out_dtype = NRM_F64, p.a.ld = p.n + 4;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "row pitch"));
		p.a.on_device = 1;
		CHECK(p.run() == NRM_OK);
		p.a.ld = p.n - 1;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "row pitch"));
	}
	{  // null pointers and shapes
		Problem p;
		p.a.reads = nullptr;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "null pointer"));
		Problem q;
		q.a.h_cov = nullptr;
		CHECK(q.run() == NRM_E_ARG && strstr(g_err, "null pointer"));
		q.a.n_cov = -1;
		CHECK(q.run() == NRM_E_ARG && strstr(g_err, "null pointer"));
		Problem r;
		r.a.rows = 0;
		CHECK(r.run() == NRM_E_ARG && !strcmp(g_err, "reads must not be empty."));
		r.a.rows = 5, r.a.n = 0, r.a.ld = 0;
		CHECK(r.run() == NRM_E_ARG && !strcmp(g_err, "reads must not be empty."));
		Problem s(0);
		s.a.rows = NRM_FRONT_MAX_ROWS + 1;
		CHECK(s.run() == NRM_E_ARG && strstr(g_err, "genes"));
		s.a.rows = 5, s.a.n = s.a.ld = 1ll << 31;
		CHECK(s.run() == NRM_E_ARG && strstr(g_err, "2^31"));
	}
	{  // the covariate bound: n_cov + 3 + 1 <= 8, refused beyond with the bound in the text; lifted with the bound
		Problem p0(0), p4(4), p5(5);
		CHECK(p0.run() == NRM_OK);
		CHECK(p4.run() == NRM_OK);
		CHECK(p5.run() == NRM_E_UNSUPPORTED && strstr(g_err, "the 8 covariates") && strstr(g_err, "= 9"));
		CHECK(nrm_front_plan_create_args(p5.a, 9, TABLE_CAP) == NRM_OK);
		Problem p12(12);
		CHECK(nrm_front_plan_create_args(p12.a, 64, TABLE_CAP) == NRM_E_UNSUPPORTED && strstr(g_err, "the 15 covariates"));  // (the plan's own Jacobi kernel: 16 rows of [dc;1])
	}
	{  // eps, stepmax, tol, ntot, count_cap
		Problem p;
		p.a.eps = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "eps and stepmax must be positive."));
		p.a.eps = -1e-6;
		CHECK(p.run() == NRM_E_ARG);
		p.a.eps = NAN;
		CHECK(p.run() == NRM_E_ARG);
		p.a.eps = 1e-6, p.a.stepmax = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "eps and stepmax must be positive."));
		p.a.stepmax = NRM_FRONT_MAX_STEPS + 1;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "steps"));
		p.a.stepmax = NRM_FRONT_MAX_STEPS;
		CHECK(p.run() == NRM_OK);
		p.a.stepmax = 1, p.a.tol = 0;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "tol"));
		p.a.tol = 1;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "tol"));
		p.a.tol = 1e-8, p.a.ntot = 0;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "ntot must be positive"));
		p.a.ntot = 1000000000;
		CHECK(p.run() == NRM_OK);
		p.a.ntot = -1;
		const int64_t bad_caps[4] = {1, 0, -5, TABLE_CAP + 1}, good_caps[2] = {2, TABLE_CAP};
		for (int64_t c : bad_caps) {
			p.a.count_cap = c;
			CHECK(p.run() == NRM_E_ARG && strstr(g_err, "count_cap must lie in [2, 16777216]"));
		}
		for (int64_t c : good_caps) {
			p.a.count_cap = c;
			CHECK(p.run() == NRM_OK);
		}
	}
	{  // user rows: not finite, constant (zeros, ones, any value), and the classification itself
		Problem p(3);
		p.cov[(size_t)(2 * p.n + p.n - 1)] = INFINITY;  // the last cell of the last row
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "array must not contain infs or NaNs"));
		p.cov[(size_t)(2 * p.n + p.n - 1)] = NAN;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "array must not contain infs or NaNs"));
		const double values[3] = {0.0, 1.0, -2.5};
		for (double v : values) {
			Problem q(3);
			for (int64_t k = 0; k < q.n; k++) q.cov[(size_t)(q.n + k)] = v;
			CHECK(q.run() == NRM_E_ARG && !strcmp(g_err, CONSTANT));
		}
		std::vector<double> row(7, 1.0);
		CHECK(nrm_normcov_row_class(row.data(), 7) == NRM_COV_CONSTANT);
		row[6] = 0.0;
		CHECK(nrm_normcov_row_class(row.data(), 7) == NRM_COV_BINARY);
		row[0] = 0.0;
		CHECK(nrm_normcov_row_class(row.data(), 7) == NRM_COV_BINARY);
		row[3] = 1.0 + 1e-15;
		CHECK(nrm_normcov_row_class(row.data(), 7) == NRM_COV_CONTINUOUS);
		row.assign(7, 2.0);
		row[6] = 3.0;  // differs in its last cell only
		CHECK(nrm_normcov_row_class(row.data(), 7) == NRM_COV_CONTINUOUS);
		row.assign(1, 0.5);
		CHECK(nrm_normcov_row_class(row.data(), 1) == NRM_COV_CONSTANT);
	}
	{  // the counters, in the reference's order: each alone, and each in front of everything after it
		struct Want {
			int slot, rc;
			const char* words;
		};
		const Want order[10] = {{0, NRM_E_ARG, "Negative value in d detected."},
								{2, NRM_E_NUMERIC, "holds no read"},
								{1, NRM_E_ARG, "Found cell with no read at all. Please remove."},
								{3, NRM_E_UNSUPPORTED, "count_cap = 256; the largest count here is 300."},
								{4, NRM_E_ARG, CONSTANT},
								{8, NRM_E_NUMERIC, "genes with a constant residual"},
								{9, NRM_E_NUMERIC, "weights are not finite and positive"},
								{6, NRM_E_NUMERIC, "scaling_factor"},
								{12, NRM_E_DEVICE, "Zero-rank covariates found."},
								{13, NRM_E_NUMERIC, "non-finite results"}};
		int32_t f[16];
		memset(f, 0, sizeof(f));
		CHECK(nrm_front_plan_status(f, 256, 0) == NRM_OK);
		f[5] = 3;  // near-constant rows: a warning, never a refusal
		CHECK(nrm_front_plan_status(f, 256, 0) == NRM_OK);
		for (int i = 0; i < 10; i++) {
			memset(f, 0, sizeof(f));
			f[order[i].slot] = 2;
			CHECK(nrm_front_plan_status(f, 256, 300) == order[i].rc && strstr(g_err, order[i].words));
			for (int j = i + 1; j < 10; j++) f[order[j].slot] = 1;
			CHECK(nrm_front_plan_status(f, 256, 300) == order[i].rc && strstr(g_err, order[i].words));
		}
	}
	{  // all 2^10 on/off combinations of the ten counters nrm_front_plan_status reads: the code and the whole message are those of the first one set, in the order
	   // lcpm, cap, normcov, compute_var, scaling_factor, normvar; a counter that is set holds slot + 2, so that a message with a count shows whose it printed
		struct Full {
			int slot, rc;
			const char* text;
		};
		const Full order[10] = {{0, NRM_E_ARG, "Negative value in d detected."},
								{2, NRM_E_NUMERIC, "lcpm: the matrix holds no read (t0 = sum + 2 > 2, lcpm.py:95)"},
								{1, NRM_E_ARG, "Found cell with no read at all. Please remove."},
								{3, NRM_E_UNSUPPORTED, "nrm_front_plan: the plan tabulates psi(1 + count) for counts below count_cap = 256; the largest count here is 300."},
								{4, NRM_E_ARG, CONSTANT},
								{8, NRM_E_NUMERIC, "compute_var: 10 genes with a constant residual, whose spread divides (norm.py:108,125)"},
								{9, NRM_E_NUMERIC, "compute_var: 11 weights are not finite and positive (norm.py:125-127)"},
								{6, NRM_E_NUMERIC, "scaling_factor: no gene has a zero entry, or a value is not finite (lcpm.py:278-282)"},
								{12, NRM_E_DEVICE, "Zero-rank covariates found."},
								{13, NRM_E_NUMERIC, "normvar: non-finite results (norm.py:286)"}};
		for (int mask = 0; mask < 1024; mask++) {
			int32_t f[16];
			memset(f, 0, sizeof(f));
			f[5] = mask & 1 ? 3 : 0, f[7] = 5, f[10] = f[11] = f[14] = f[15] = 7;  // a warning and the words nobody reads: never a refusal
			int first = -1;
			for (int i = 9; i >= 0; i--)
				if (mask >> i & 1) f[order[i].slot] = order[i].slot + 2, first = i;
			strcpy(g_err, "untouched");
			const int rc = nrm_front_plan_status(f, 256, 300);
			if (first < 0)
				CHECK(rc == NRM_OK && !strcmp(g_err, "untouched"));
			else
				CHECK(rc == order[first].rc && !strcmp(g_err, order[first].text));
		}
	}
	{  // the stages' own readings, which the whole-problem entries share with the plan: every on/off combination of compute_var's two counters and of normvar's two
		for (int mask = 0; mask < 4; mask++) {
			const int32_t f[2] = {mask & 1 ? 4 : 0, mask & 2 ? 9 : 0};
			strcpy(g_err, "untouched");
			const int cv = nrm_compute_var_status(f);
			if (mask & 1)
				CHECK(cv == NRM_E_NUMERIC && !strcmp(g_err, "compute_var: 4 genes with a constant residual, whose spread divides (norm.py:108,125)"));
			else if (mask & 2)
				CHECK(cv == NRM_E_NUMERIC && !strcmp(g_err, "compute_var: 9 weights are not finite and positive (norm.py:125-127)"));
			else
				CHECK(cv == NRM_OK && !strcmp(g_err, "untouched"));
			strcpy(g_err, "untouched");
			const int nv = nrm_normvar_status(f);
			if (mask & 1)
				CHECK(nv == NRM_E_DEVICE && !strcmp(g_err, "Zero-rank covariates found."));
			else if (mask & 2)
				CHECK(nv == NRM_E_NUMERIC && !strcmp(g_err, "normvar: non-finite results (norm.py:286)"));
			else
				CHECK(nv == NRM_OK && !strcmp(g_err, "untouched"));
		}
	}
	printf("front plan args ok\n");
	return 0;
}
