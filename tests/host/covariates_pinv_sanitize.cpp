// The covariates' pseudo-inverse of csrc/nrm_host_math.h (nrm_covariates_to_f64, nrm_covariates_pinv_f64) and its C entry nrm_covariates_pinv
// (csrc/nrm_small_pinv.hip: host code) under g++ -fsanitize=address,undefined; tests/test_coex_plan_cpu.py builds the two files together and runs the program.
// On heap buffers of the exact size:
//  * full-rank random covariates of 1 .. 32 rows, odd cell counts: rank == nc, M M^+ = I, M^+ symmetric;
//  * an intercept with one-hot batches (rank nc - 1) and a duplicated row: the four Moore-Penrose conditions;
//  * all-zero covariates: rank 0 and a zero pseudo-inverse; fp32 covariates: the fp64 answer of the converted values, bit for bit;
//  * nc = 0: rank 0 and nothing written; nc = 33: NRM_E_UNSUPPORTED; a NaN: NRM_E_ARG.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include "../../normalisr_amd/csrc/nrm_host_math.h"

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
static unsigned long long g_st = 0x9E3779B97F4A7C15ull;
static double rnd() {
	g_st ^= g_st << 13;
	g_st ^= g_st >> 7;
	g_st ^= g_st << 17;
	return (double)(g_st >> 11) / 9007199254740992.0 - 0.5;
}

typedef std::vector<double> vec;
static vec matmul(const vec& a, const vec& b, int64_t n) {
	vec c((size_t)(n * n), 0.0);
	for (int64_t i = 0; i < n; i++)
		for (int64_t k = 0; k < n; k++)
			for (int64_t j = 0; j < n; j++) c[(size_t)(i * n + j)] += a[(size_t)(i * n + k)] * b[(size_t)(k * n + j)];
	return c;
}
static double maxabs(const vec& a) {
	double m = 0.0;
	for (double v : a) m = std::fmax(m, std::fabs(v));
	return m;
}
static double maxdiff(const vec& a, const vec& b) {
	double m = 0.0;
	for (size_t i = 0; i < a.size(); i++) m = std::fmax(m, std::fabs(a[i] - b[i]));
	return m;
}

// the four Moore-Penrose conditions of p for m = C C^T, relative to the entries' size
static void check_penrose(const vec& c, int64_t nc, int64_t n, const vec& p, double tol) {
	vec m;
	nrm_covariate_gram(c.data(), nc, n, m);
	const vec mp = matmul(m, p, nc), pm = matmul(p, m, nc);
	CHECK(maxdiff(matmul(mp, m, nc), m) <= tol * maxabs(m));
	CHECK(maxdiff(matmul(pm, p, nc), p) <= tol * maxabs(p));
	for (int64_t i = 0; i < nc; i++)
		for (int64_t j = 0; j < nc; j++) {
			CHECK(std::fabs(mp[(size_t)(i * nc + j)] - mp[(size_t)(j * nc + i)]) <= tol);
			CHECK(p[(size_t)(i * nc + j)] == p[(size_t)(j * nc + i)]);
		}
}

static void full_rank() {
	for (int64_t nc : {1, 2, 3, 5, 8, 17, 32}) {
		const int64_t n = 2 * nc + 37;
		vec c((size_t)(nc * n)), p((size_t)(nc * nc), -7.0);
		for (auto& x : c) x = rnd();
		int rank = -1;
		CHECK(nrm_covariates_pinv_f64(c.data(), nc, n, 1e-8, p.data(), &rank) == NRM_OK && rank == (int)nc);
		check_penrose(c, nc, n, p, 1e-9);
		int rank2 = -1;  // the C entry on the same values
		vec p2((size_t)(nc * nc), -7.0);
		CHECK(nrm_covariates_pinv(c.data(), NRM_F64, nc, n, 1e-8, p2.data(), &rank2) == NRM_OK && rank2 == rank);
		CHECK(memcmp(p.data(), p2.data(), p.size() * 8) == 0);
	}
}

static void rank_deficient() {
	const int64_t nb = 4, nc = nb + 2, n = 61;  // intercept, 4 one-hot batches, a copy of batch 1: rank 4 of 6
	vec c((size_t)(nc * n), 0.0), p((size_t)(nc * nc));
	for (int64_t k = 0; k < n; k++) {
		c[(size_t)k] = 1.0;
		c[(size_t)((1 + k % nb) * n + k)] = 1.0;
		c[(size_t)((nc - 1) * n + k)] = c[(size_t)(2 * n + k)];
	}
	int rank = -1;
	CHECK(nrm_covariates_pinv_f64(c.data(), nc, n, 1e-8, p.data(), &rank) == NRM_OK && rank == 4);
	check_penrose(c, nc, n, p, 1e-9);
	vec z((size_t)(nc * n), 0.0);  // all-zero covariates: rank 0, zero pseudo-inverse
	CHECK(nrm_covariates_pinv_f64(z.data(), nc, n, 1e-8, p.data(), &rank) == NRM_OK && rank == 0 && maxabs(p) == 0.0);
}

static void fp32_and_edges() {
	const int64_t nc = 3, n = 29;
	std::vector<float> cf((size_t)(nc * n));
	for (auto& x : cf) x = (float)rnd();
	vec c64, p((size_t)(nc * nc)), q((size_t)(nc * nc));
	nrm_covariates_to_f64(cf.data(), NRM_F32, cf.size(), c64);
	CHECK(c64.size() == cf.size());
	for (size_t i = 0; i < cf.size(); i++) CHECK(c64[i] == (double)cf[i]);
	int r1 = -1, r2 = -1;
	CHECK(nrm_covariates_pinv(cf.data(), NRM_F32, nc, n, 1e-8, p.data(), &r1) == NRM_OK);
	CHECK(nrm_covariates_pinv(c64.data(), NRM_F64, nc, n, 1e-8, q.data(), &r2) == NRM_OK);
	CHECK(r1 == 3 && r2 == 3 && memcmp(p.data(), q.data(), p.size() * 8) == 0);
	nrm_covariates_to_f64(nullptr, NRM_F64, 0, c64);
	CHECK(c64.empty());
	int rank = -1;  // nc = 0: nothing is read or written
	CHECK(nrm_covariates_pinv(nullptr, NRM_F64, 0, n, 1e-8, nullptr, &rank) == NRM_OK && rank == 0);
	vec big((size_t)(33 * n), 1.0), pb((size_t)(33 * 33));
	CHECK(nrm_covariates_pinv(big.data(), NRM_F64, 33, n, 1e-8, pb.data(), &rank) == NRM_E_UNSUPPORTED);
	c64.assign((size_t)(nc * n), 1.0);
	c64[5] = NAN;
	CHECK(nrm_covariates_pinv(c64.data(), NRM_F64, nc, n, 1e-8, p.data(), &rank) == NRM_E_ARG);
	CHECK(nrm_covariates_pinv(c64.data(), NRM_F64, nc, n, 0.0, p.data(), &rank) == NRM_E_ARG);  // tol must be positive
	CHECK(nrm_covariates_pinv(c64.data(), NRM_F64, nc, n, 1e-8, p.data(), nullptr) == NRM_E_ARG);
}

int main() {
	full_rank();
	rank_deficient();
	fp32_and_edges();
	printf("covariates pinv ok\n");
	return 0;
}
