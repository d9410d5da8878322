// The host arithmetic of the whole-problem entries (csrc/nrm_host_math.h: free of HIP headers) under g++ -fsanitize=address,undefined; tests/test_cabi_cpu.py
// builds it beside csrc/nrm_small_pinv.hip (the eigenvalue routine of the full-rank certificate) and runs it.  Exercises, on exact-size heap buffers:
//  * nrm_spd_inverse_host: M M^-1 = I for seeded SPD matrices, false for a zero pivot;
//  * nrm_normvar_coefficients and the rule of csrc/nrm_nv_scale.h (the mark of a gene whose one-pass variance sums have cancelled);
//  * nrm_constant_row, nrm_covariate_gram, the streaming de's covariate permutation and its way back for alpha;
//  * with a file of cases as argv[1] (float64: count, then per case kind, nx, nc, rank, norm_mt, norm_ninv, tol, bx (nx, nc), ss_x (nx), mcc (nc, nc)):
//    one line "verdict <0|1>" per case from nrm_pinv_rank_certified (kind 0) or nrm_full_rank_certified (kind 1) -- the test holds them to their numpy twins.
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
static unsigned long long g_st = 0x2545F4914F6CDD1Dull;
static double rnd() {
	g_st ^= g_st << 13;
	g_st ^= g_st >> 7;
	g_st ^= g_st << 17;
	return (double)(g_st >> 11) / 9007199254740992.0 - 0.5;
}

static void check_spd_inverse() {
	for (int64_t n : {1, 2, 7, 33}) {
		std::vector<double> a((size_t)(n * n)), m((size_t)(n * n));
		for (auto& x : a) x = rnd();
		for (int64_t i = 0; i < n; i++)
			for (int64_t j = 0; j < n; j++) {
				double s = i == j ? 1.0 : 0.0;
				for (int64_t k = 0; k < n; k++) s += a[(size_t)(i * n + k)] * a[(size_t)(j * n + k)];
				m[(size_t)(i * n + j)] = s;
			}
		std::vector<double> inv(m);
		CHECK(nrm_spd_inverse_host(inv, n));
		double worst = 0.0;
		for (int64_t i = 0; i < n; i++)
			for (int64_t j = 0; j < n; j++) {
				double s = i == j ? -1.0 : 0.0;
				for (int64_t k = 0; k < n; k++) s += m[(size_t)(i * n + k)] * inv[(size_t)(k * n + j)];
				worst = std::fmax(worst, std::fabs(s));
			}
		CHECK(worst <= 1e-9);
	}
	std::vector<double> z = {1.0, 1.0, 1.0, 1.0};  // second pivot: 1 - 1 * 1 = 0
	CHECK(!nrm_spd_inverse_host(z, 2));
	std::vector<double> zero = {0.0};
	CHECK(!nrm_spd_inverse_host(zero, 1));
}

static void check_constant_row_and_gram() {
	const int64_t nc = 5, n = 13;
	std::vector<double> c((size_t)(nc * n));
	for (auto& x : c) x = rnd();
	double v = -1.0;
	CHECK(nrm_constant_row(c.data(), nc, n, &v) == -1 && v == 0.0);
	for (int64_t k = 0; k < n; k++) c[(size_t)(1 * n + k)] = 0.0;  // a zero row is constant, and skipped
	for (int64_t k = 0; k < n; k++) c[(size_t)(3 * n + k)] = 2.5;
	for (int64_t k = 0; k < n; k++) c[(size_t)(4 * n + k)] = -1.0;  // the first constant row counts
	CHECK(nrm_constant_row(c.data(), nc, n, &v) == 3 && v == 2.5);
	c[(size_t)(3 * n + n - 1)] = 2.0;  // (constant but for its last cell)
	CHECK(nrm_constant_row(c.data(), nc, n, &v) == 4 && v == -1.0);
	CHECK(nrm_constant_row(c.data(), 1, n, &v) == -1);
	std::vector<double> one = {7.0};  // a single cell
	CHECK(nrm_constant_row(one.data(), 1, 1, &v) == 0 && v == 7.0);
	std::vector<double> mcc;
	nrm_covariate_gram(c.data(), nc, n, mcc);
	CHECK((int64_t)mcc.size() == nc * nc);
	for (int64_t a = 0; a < nc; a++)
		for (int64_t b = 0; b < nc; b++) {
			double s = 0.0;
			for (int64_t k = 0; k < n; k++) s += c[(size_t)(a * n + k)] * c[(size_t)(b * n + k)];
			CHECK(mcc[(size_t)(a * nc + b)] == mcc[(size_t)(b * nc + a)]);
			CHECK(mcc[(size_t)(a * nc + b)] == s);
		}
	nrm_covariate_gram(c.data(), 0, n, mcc);
	CHECK(mcc.empty());
}

template <typename E>
static void check_alpha_permutation(int64_t nc, int ci) {
	const int64_t n = 9;
	const size_t cnt = 11;
	const std::vector<int64_t> perm = nrm_const_last_perm(nc, ci);
	std::vector<int> seen((size_t)nc, 0);
	for (int64_t p : perm) {
		CHECK(p >= 0 && p < nc);
		seen[(size_t)p]++;
	}
	for (int s : seen) CHECK(s == 1);
	if (ci >= 0) CHECK(perm[(size_t)nc - 1] == ci);
	for (int64_t c = 0; c + 1 < nc - (ci >= 0 ? 1 : 0); c++) CHECK(perm[(size_t)c] < perm[(size_t)c + 1]);  // the others keep their order
	std::vector<double> c64((size_t)(nc * n)), dci((size_t)(nc * nc)), hc, hd;
	for (auto& x : c64) x = rnd();
	for (auto& x : dci) x = rnd();
	nrm_permute_covariates(c64.data(), dci.data(), perm, n, hc, hd);
	for (int64_t a = 0; a < nc; a++) {
		for (int64_t k = 0; k < n; k++) CHECK(hc[(size_t)(a * n + k)] == c64[(size_t)(perm[(size_t)a] * n + k)]);
		for (int64_t b = 0; b < nc; b++) CHECK(hd[(size_t)(a * nc + b)] == dci[(size_t)(perm[(size_t)a] * nc + perm[(size_t)b])]);
	}
	nrm_permute_covariates(c64.data(), nullptr, perm, n, hc, hd);
	for (double x : hd) CHECK(x == 0.0);
	// the round trip: coefficients in the caller's order -> Z's order (what the kernels write) -> back
	std::vector<E> alpha(cnt * (size_t)nc), z(alpha.size()), back(alpha.size(), (E)-7);
	for (auto& x : alpha) x = (E)rnd();
	for (size_t i = 0; i < cnt; i++)
		for (int64_t c = 0; c < nc; c++) z[i * (size_t)nc + (size_t)c] = alpha[i * (size_t)nc + (size_t)perm[(size_t)c]];
	nrm_alpha_unpermute((const char*)z.data(), perm, cnt, sizeof(E), back.data());
	for (size_t i = 0; i < alpha.size(); i++) CHECK(back[i] == alpha[i]);
}

static void check_store() {
	const std::vector<double> v = {1.0, 0.1, -3.5};
	std::vector<double> d(3);
	std::vector<float> f(3);
	nrm_store_as(NRM_F64, d.data(), v.data(), 3);
	nrm_store_as(NRM_F32, f.data(), v.data(), 3);
	for (size_t i = 0; i < 3; i++) CHECK(d[i] == v[i] && f[i] == (float)v[i]);
}

// nrm_normvar_coefficients: b = M^+ a row by row, the one-pass scale, and the mark of csrc/nrm_nv_scale.h where either difference has cancelled
static void check_normvar_coefficients() {
	const int64_t rows = 5, nc = 2, n = 100, lda = 3;  // (a pitch above nc)
	std::vector<double> mi((size_t)(rows * nc * nc)), ga((size_t)(rows * lda)), s1((size_t)rows), s2((size_t)rows), wt = {0.7, 0.7, 0.7, 0.0, 1.5}, hb, hs;
	for (int64_t g = 0; g < rows; g++) {
		mi[(size_t)(g * 4)] = 0.5, mi[(size_t)(g * 4 + 1)] = mi[(size_t)(g * 4 + 2)] = 0.125, mi[(size_t)(g * 4 + 3)] = 0.25;
		ga[(size_t)(g * lda)] = 2.0, ga[(size_t)(g * lda + 1)] = -4.0, ga[(size_t)(g * lda + 2)] = 1e300;  // (the pitch padding is not read)
	}
	// b = (0.5, -0.75), a . b = 4.  rows: 0 ordinary; 1 a flat row (s2 / n - mean^2 = 0); 2 a row the covariates explain (s2 - a . b = 2^-30 s2); 3 the same with wt = 0; 4 ordinary
	s1 = {10.0, 300.0, 10.0, 300.0, -50.0};
	s2 = {400.0, 900.0, 4.0 / (1.0 - 0x1p-30), 900.0, 1000.0};
	nrm_normvar_coefficients(mi.data(), ga.data(), lda, s1.data(), s2.data(), wt.data(), rows, nc, n, 1, hb, hs);
	CHECK((int64_t)hb.size() == rows * nc && (int64_t)hs.size() == rows);
	for (int64_t g = 0; g < rows; g++) CHECK(hb[(size_t)(g * 2)] == 0.5 && hb[(size_t)(g * 2 + 1)] == -0.75);
	CHECK(hs[1] == NRM_NV_MARK && hs[2] == NRM_NV_MARK && hs[3] == 1.0);
	for (int64_t g : {0, 4}) {  // the unmarked genes: the one-pass expressions as they have always stood
		const double mean = s1[(size_t)g] / (double)n;
		const double dv = std::sqrt(std::fmax(s2[(size_t)g] / (double)n - mean * mean, 0.0));
		const double dv2 = std::sqrt(std::fmax(s2[(size_t)g] - 4.0, 0.0) / (double)n);
		CHECK(hs[(size_t)g] == std::pow(dv / dv2, wt[(size_t)g]) && hs[(size_t)g] > 0);
	}
	// the threshold itself: a difference of exactly tau x its minuend is not below it
	CHECK(nrm_nv_scale(0.0, 1.0, 1.0 - NRM_NV_TAU, 1.0, 1.0) != NRM_NV_MARK && nrm_nv_scale(0.0, 1.0, 1.0 - NRM_NV_TAU / 2, 1.0, 1.0) == NRM_NV_MARK);
	CHECK(nrm_nv_scale(0.0, 1.0, 1.0, 1.0, 0.0) == 1.0);  // wt == 0: never marked, x^0 = 1 even for 0 / 0
	nrm_normvar_coefficients(mi.data(), ga.data(), lda, s1.data(), s2.data(), wt.data(), rows, nc, n, 0, hb, hs);
	for (double v : hs) CHECK(v == 1.0);  // keepvar == 0
}

static void certificates(const char* path) {
	FILE* fh = fopen(path, "rb");
	CHECK(fh != nullptr);
	CHECK(fseek(fh, 0, SEEK_END) == 0);
	const long bytes = ftell(fh);
	CHECK(bytes >= 8 && bytes % 8 == 0 && fseek(fh, 0, SEEK_SET) == 0);
	std::vector<double> all((size_t)bytes / 8);
	CHECK(fread(all.data(), 8, all.size(), fh) == all.size());
	fclose(fh);
	size_t at = 0;
	auto take = [&](size_t count) {
		CHECK(at + count <= all.size());
		std::vector<double> out(all.begin() + (long)at, all.begin() + (long)(at + count));  // (a buffer of the exact size per operand)
		at += count;
		return out;
	};
	const int64_t cases = (int64_t)take(1)[0];
	for (int64_t q = 0; q < cases; q++) {
		const std::vector<double> h = take(7);
		const int kind = (int)h[0];
		const int64_t nx = (int64_t)h[1], nc = (int64_t)h[2];
		const int rank = (int)h[3];
		CHECK((kind == 0 || kind == 1) && nx > 0 && nc > 0 && nc <= 32);
		const std::vector<double> bx = take((size_t)(nx * nc)), ssx = take((size_t)nx);
		std::vector<double> mcc = take((size_t)(nc * nc));
		bool ok = false;
		if (kind == 0)
			ok = nrm_pinv_rank_certified(mcc, nc, rank, bx.data(), ssx.data(), nx, h[4], h[5], h[6]);
		else
			CHECK(nrm_full_rank_certified(h[4], h[5], bx.data(), mcc.data(), nx, nc, h[6], &ok) == NRM_OK);
		printf("verdict %d\n", ok ? 1 : 0);
	}
	CHECK(at == all.size());
}

int main(int argc, char** argv) {
	check_spd_inverse();
	check_constant_row_and_gram();
	for (int64_t nc : {1, 2, 5, 31})
		for (int ci : {-1, 0, (int)(nc / 2), (int)nc - 1}) {
			check_alpha_permutation<float>(nc, ci);
			check_alpha_permutation<double>(nc, ci);
		}
	check_store();
	check_normvar_coefficients();
	bool ok = false;  // no covariates: the norms of M~ alone
	CHECK(nrm_full_rank_certified(2.0, 0.5, nullptr, nullptr, 3, 0, 1e-8, &ok) == NRM_OK && ok);
	CHECK(nrm_full_rank_certified(2.0, 1e9, nullptr, nullptr, 3, 0, 1e-8, &ok) == NRM_OK && !ok);
	if (argc > 1) certificates(argv[1]);
	printf("entry math ok\n");
	return 0;
}
