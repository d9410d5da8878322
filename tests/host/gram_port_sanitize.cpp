// CPU build of the fp64 Gram kernel's schedule (csrc/nrm_host_logic.h: gram_plan, gram_split_phases, gram_pieces_of) for g++ -fsanitize=address,undefined
// (tests/test_s4_reference_cpu.py builds and runs it).  Reads launches from the file named on the command line, one per line:
//     m_pad n_pad nkt symmetric m_rows n_rows row0 row1 nwg whole
// and prints, per launch, every field of the GramSched that gram_plan makes of it (whole != 0: as nrm_gram_f64_whole rewrites it) and a checksum over the
// piece list of every workgroup in launch order.  The test compares each line with the Python port of the schedule in tests/s4_reference.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include "../../normalisr_amd/csrc/nrm_host_logic.h"

static char g_err[512];
void nrm_set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

int main(int argc, char** argv) {
	if (argc != 2) return 2;
	FILE* f = fopen(argv[1], "r");
	if (!f) return 2;
	const int kMaxWg = 1024;
	double* work = (double*)malloc((size_t)nrm_host_gram_workspace_doubles(kMaxWg) * sizeof(double));  // never touched: slab pointers are formed inside an object that exists
	if (!work) return 2;
	long long v[10];
	int lines = 0;
	while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9]) == 10) {
		if (v[8] > kMaxWg) return 3;
		GramSched s;
		if (gram_plan(s, v[0], v[1], v[2], (int)v[3], v[4], v[5], v[6], v[7], (int)v[8], work) != NRM_OK) {
			fprintf(stderr, "gram_plan: %s\n", g_err);
			return 1;
		}
		if (v[9]) {
			s.tiles_dp += s.tiles_al + s.tiles_sk;
			s.tiles_al = s.tiles_sk = s.units_per_wg = 0;
			s.parts = 1;
		}
		const unsigned long long mod = (1ULL << 61) - 1;
		unsigned long long h = 0;
		for (int block = 0; block < s.nwg; block++)
			gram_pieces_of(s, block, [&](int t, int k0, int k1, double* slab) {
				const long long idx = slab ? (long long)((slab - work) / (GM * GN)) : -1;
				const long long vals[5] = {block, t, k0, k1, idx};
				for (int q = 0; q < 5; q++) h = (unsigned long long)(((unsigned __int128)h * 1000003ULL + (unsigned long long)(vals[q] + 7)) % mod);
			});
		printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %llu\n", s.m_rows, s.n_rows, s.ntm, s.ntn, s.nkt, s.tiles_dp, s.tiles_al, s.parts, s.tiles_sk, s.units_per_wg, s.nwg,
			   s.tile0, s.accumulate, s.fold, h);
		lines++;
	}
	fclose(f);
	free(work);
	printf("gram schedule printed: %d launches\n", lines);
	return 0;
}
