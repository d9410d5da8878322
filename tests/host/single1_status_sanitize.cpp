// nrm_single1_status (csrc/nrm_single1_plan_args.h: free of HIP headers) -- what single=1's device counters mean, for the whole-problem entry and the resident plan
// alike -- under g++ -fsanitize=address,undefined; tests/test_single1_plan_cpu.py builds and runs it.  All 32 combinations of counters [0..4] set or clear, in a heap
// buffer of exactly eight words: the status and the message are those of the counter that comes first in [2], [4], [3], [0] / [1]; none set is NRM_OK.
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
#define CHECK(c)                                                                                                \
	do {                                                                                                        \
		if (!(c)) {                                                                                             \
			fprintf(stderr, "%s:%d: check failed: %s (mask %d: %s)\n", __FILE__, __LINE__, #c, mask, g_err); \
			exit(1);                                                                                            \
		}                                                                                                       \
	} while (0)

int main() {
	for (int mask = 0; mask < 32; mask++) {
		std::vector<int32_t> hf(8, 0);
		for (int k = 0; k < 5; k++) hf[(size_t)k] = (mask >> k & 1) ? 10 + k : 0;
		strcpy(g_err, "untouched");
		const int rc = nrm_single1_status(hf.data());
		if (mask & 4) {
			CHECK(rc == NRM_E_NUMERIC && !strcmp(g_err, "12 groupings take a single value on the cells selected for them (association.py:917-918)"));
		} else if (mask & 16) {
			CHECK(rc == NRM_E_ARG && !strcmp(g_err, "array must not contain infs or NaNs"));
		} else if (mask & 8) {
			CHECK(rc == NRM_E_DEVICE && !strcmp(g_err, "Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1."));
		} else if (mask & 3) {
			char want[256];
			snprintf(want, sizeof(want), "association results failed the reference's assertions (association.py:248,252): %d non-finite, %d with R^2 > 1+1e-8", hf[0], hf[1]);
			CHECK(rc == NRM_E_NUMERIC && !strcmp(g_err, want));
		} else {
			CHECK(rc == NRM_OK && !strcmp(g_err, "untouched"));
		}
	}
	printf("single1 status ok\n");
	return 0;
}
