// CPU build of K1's routing (csrc/nrm_host_logic.h: nrm_k1_vec, nrm_k1_stream_rows, nrm_k1_rows8, nrm_k1_rows8_pays -- the conditions launch_residualize takes) for
// tests/test_k1_rows8_route_cpu.py.  Reads one call per line from standard input -- element bytes of x, ldx, has_out, ldo, active, ldc, nc, n, rows_pad
// (pointers 16-byte aligned) -- and prints "vec stream_rows rows8 pays" for each.
#include <cstdarg>
#include <cstdio>
#include "../../normalisr_amd/csrc/nrm_host_logic.h"

void nrm_set_error(const char*, ...) {}

int main() {
	long long xb, ldx, has_out, ldo, active, ldc, nc, n, rows_pad;
	while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &xb, &ldx, &has_out, &ldo, &active, &ldc, &nc, &n, &rows_pad) == 9) {
		const bool vec = nrm_k1_vec(0, xb, ldx, has_out != 0, 0, ldo, (int)active, 0, ldc);
		const bool stream = nrm_k1_stream_rows((int)active, xb, nc, n);
		printf("%d %d %d %d\n", (int)vec, (int)stream, (int)nrm_k1_rows8(vec, (int)active, nc, rows_pad, stream), (int)nrm_k1_rows8_pays(n));
	}
	return 0;
}
