// The host arithmetic of the front-half entries (csrc/nrm_host_math.h: nrm_lcpm_tables, nrm_lcpm_cov_rows, nrm_pinv_gram_unit_rows, nrm_qc_thresholds) under
// g++ -fsanitize=address,undefined; tests/test_front_entries_cpu.py builds this file, writes the inputs, runs the program and compares what it prints with numpy.
// `front_entry_math_sanitize IN OUT`.  IN, 8-byte little-endian words, every array on a heap buffer of its exact size:
//   int64 len, double psi_t0, double psi[len]                       -> "tab", "etab" (len values each), "unit"
//   int64 rows, n, int64 cell_total[n], cell_nnz[n]                 -> "cov_stop" (the first cell without a read, or -1), "cov" (3 n values; only when -1)
//   the same block once more (a matrix with an empty cell)
//   int64 r, n, double x[r n]                                       -> "pinv_rank", "pinv" (r r values)
//   int64 cases, per case double params[6], int64 nt, ns            -> "thr" (6 integers) per case
// Doubles are printed with 17 significant digits, which round-trip.
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

static FILE *g_in, *g_out;
static int64_t read_int() {
	int64_t v = 0;
	CHECK(fread(&v, 8, 1, g_in) == 1);
	return v;
}
template <typename T>
static std::vector<T> read_vec(int64_t count) {
	CHECK(count >= 0 && count < (1 << 26));
	std::vector<T> v((size_t)count);
	v.shrink_to_fit();
	if (count) CHECK(fread(v.data(), sizeof(T), (size_t)count, g_in) == (size_t)count);
	return v;
}
static void print_doubles(const char* name, const double* v, int64_t count) {
	fprintf(g_out, "%s", name);
	for (int64_t i = 0; i < count; i++) fprintf(g_out, " %.17g", v[i]);
	fprintf(g_out, "\n");
}

static void tables() {
	const int64_t len = read_int();
	const std::vector<double> t0 = read_vec<double>(1), psi = read_vec<double>(len);
	std::vector<double> tab, etab;
	const double unit = nrm_lcpm_tables(psi.data(), t0[0], len, tab, etab);
	CHECK((int64_t)tab.size() == len && (int64_t)etab.size() == len);
	print_doubles("tab", tab.data(), len);
	print_doubles("etab", etab.data(), len);
	print_doubles("unit", &unit, 1);
	std::vector<double> one_tab, one_etab;  // a matrix whose largest count is 0 has a table of one entry and no stored term
	CHECK(nrm_lcpm_tables(psi.data(), t0[0], 1, one_tab, one_etab) == 0.0 && one_tab.size() == 1 && one_tab[0] == tab[0]);
}

static void covariates() {
	const int64_t rows = read_int(), n = read_int();
	const std::vector<int64_t> total = read_vec<int64_t>(n), nnz = read_vec<int64_t>(n);
	std::vector<double> cov((size_t)(3 * n), -7.0);
	cov.shrink_to_fit();
	const int64_t stop = nrm_lcpm_cov_rows(total.data(), nnz.data(), rows, n, cov.data());
	fprintf(g_out, "cov_stop %lld\n", (long long)stop);
	if (stop < 0) print_doubles("cov", cov.data(), 3 * n);
}

static void pinv() {
	const int64_t r = read_int(), n = read_int();
	const std::vector<double> x = read_vec<double>(r * n);
	std::vector<double> inv((size_t)(r * r), -7.0);
	inv.shrink_to_fit();
	int64_t rank = -1;
	nrm_pinv_gram_unit_rows(x.data(), r, n, 1e-8, inv.data(), &rank);
	fprintf(g_out, "pinv_rank %lld\n", (long long)rank);
	print_doubles("pinv", inv.data(), r * r);
	for (int64_t i = 0; i < r; i++)
		for (int64_t j = 0; j < r; j++) CHECK(inv[(size_t)(i * r + j)] == inv[(size_t)(j * r + i)]);
	// 64 rows, the most the Jacobi routine takes (63 covariates and the ones row), two of them equal and one all zero: finite, rank 62
	const int64_t rr = 64, nn = 71;
	std::vector<double> big((size_t)(rr * nn)), binv((size_t)(rr * rr));
	unsigned long long st = 0x9E3779B97F4A7C15ull;
	for (auto& v : big) {
		st ^= st << 13, st ^= st >> 7, st ^= st << 17;
		v = (double)(st >> 11) / 9007199254740992.0 - 0.5;
	}
	for (int64_t k = 0; k < nn; k++) big[(size_t)(5 * nn + k)] = 1e6 * big[(size_t)(9 * nn + k)], big[(size_t)(17 * nn + k)] = 0.0;
	nrm_pinv_gram_unit_rows(big.data(), rr, nn, 1e-8, binv.data(), &rank);
	CHECK(rank == 62);
	for (double v : binv) CHECK(std::isfinite(v));
}

static void thresholds() {
	const int64_t cases = read_int();
	for (int64_t c = 0; c < cases; c++) {
		const std::vector<double> params = read_vec<double>(6);
		const int64_t nt = read_int(), ns = read_int();
		std::vector<int64_t> thr(6, -1);
		thr.shrink_to_fit();
		nrm_qc_thresholds(params.data(), nt, ns, thr.data());
		fprintf(g_out, "thr");
		for (int i = 0; i < 6; i++) fprintf(g_out, " %lld", (long long)thr[(size_t)i]);
		fprintf(g_out, "\n");
	}
}

int main(int argc, char** argv) {
	CHECK(argc == 3);
	g_in = fopen(argv[1], "rb");
	g_out = fopen(argv[2], "w");
	CHECK(g_in && g_out);
	tables();
	covariates();
	covariates();
	pinv();
	thresholds();
	CHECK(fgetc(g_in) == EOF);
	fclose(g_in);
	CHECK(fclose(g_out) == 0);
	printf("front entry math ok\n");
	return 0;
}
