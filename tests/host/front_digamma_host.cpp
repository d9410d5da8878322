// csrc/nrm_digamma.h -- the digamma evaluation the front-half plan's table kernel runs per entry -- built for the host under g++ -fsanitize=address,undefined;
// tests/test_front_plan_cpu.py builds and runs it.  `front_digamma_host IN OUT`: IN holds doubles z, OUT receives psi(z) for each, for the test to hold against
// scipy's values (golden G18) and against nrm_lcpm_digamma.  Arguments that are not positive give NaN and the loop of the upward shift must still end.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../normalisr_amd/csrc/nrm_digamma.h"

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 3;
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	std::vector<double> z((size_t)bytes / 8), psi((size_t)bytes / 8);
	if (fread(z.data(), 8, z.size(), f) != z.size()) return 4;
	fclose(f);
	for (size_t i = 0; i < z.size(); i++) psi[i] = nrm_digamma(z[i]);
	const double bad[3] = {0.0, -3.5, -1e300};
	for (double b : bad) {
		const double v = nrm_digamma(b);
		if (v == v) return 5;  // NaN, and no endless shift
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(psi.data(), 8, psi.size(), f) != psi.size()) return 6;
	fclose(f);
	printf("front digamma ok %zu\n", z.size());
	return 0;
}
