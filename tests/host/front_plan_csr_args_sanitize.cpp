// What the resident front-half plan decides on the host about CSR counts (csrc/nrm_front_plan_args.h: free of HIP headers) under g++ -fsanitize=address,undefined;
// tests/test_front_plan_csr_cpu.py builds and runs it.  Every operand is a heap buffer of the exact size -- indptr holds rows + 1 offsets and not one more -- so a
// check that read past an array would be caught: the argument checks of nrm_front_plan_create_csr (null pointers, nnz and nnz_cap, alignment, the shape bounds, the
// O(rows) structure of host offsets, and everything create checks too), those of nrm_front_plan_upload_csr, and the reading of the counters with the malformed
// word in front of the sixteen.
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
static const char* const MALFORMED = "Malformed CSR matrix: indptr must rise from 0 to the number of stored entries, and the columns of every row must lie in [0, n_cell) and "
									 "increase strictly (sum duplicates and sort the indices first).";

// 5 genes x 12 cells, two stored entries per gene, in arrays of exactly nnz elements
struct Problem {
	int64_t rows = 5, n = 12, nnz = 10;
	std::vector<int64_t> indptr;
	std::vector<int32_t> indices, data;
	std::vector<double> cov;
	NrmFrontPlanArgs a;
	explicit Problem(int64_t n_cov = 1) {
		for (int64_t r = 0; r <= rows; r++) indptr.push_back(2 * r);
		for (int64_t r = 0; r < rows; r++) indices.push_back((int32_t)r), indices.push_back((int32_t)(r + 6));
		data.assign((size_t)nnz, 3);
		cov.assign((size_t)(n_cov * n), 0.0);
		for (int64_t r = 0; r < n_cov; r++)
			for (int64_t k = 0; k < n; k++) cov[(size_t)(r * n + k)] = r == 0 ? (double)(k % 2) : 0.25 * (double)((k * (r + 1)) % 7) - (double)r;
		a.csr = 1, a.indptr = indptr.data(), a.indices = indices.data(), a.reads = data.data(), a.nnz = nnz, a.nnz_cap = nnz;
		a.dtype = NRM_I32, a.rows = rows, a.n = n, a.ld = n, a.h_cov = n_cov ? cov.data() : nullptr, a.n_cov = n_cov, a.count_cap = 256;
	}
	int run() { return nrm_front_plan_create_csr_args(a, MAX_COV, TABLE_CAP); }
};

int main() {
	{  // a good problem; a capacity above the count; every count dtype (the checks never read the values); the dense entry refuses the record and the other way round
		Problem p;
		CHECK(p.run() == NRM_OK);
		p.a.nnz_cap = 1000;
		CHECK(p.run() == NRM_OK);
		const int dtypes[4] = {NRM_I64, NRM_I32, NRM_I16, NRM_U8};
		for (int d : dtypes) {
			p.a.dtype = d;
			CHECK(p.run() == NRM_OK);
		}
		p.a.dtype = NRM_F64;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "counts are NRM_I64"));
		p.a.dtype = NRM_I32;
		CHECK(nrm_front_plan_create_args(p.a, MAX_COV, TABLE_CAP) == NRM_E_ARG && strstr(g_err, "nrm_front_plan_create_csr takes CSR counts"));
		p.a.csr = 0;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "nrm_front_plan_create takes a dense matrix"));
	}
	{  // null pointers, one at a time
		Problem p, q, r, s;
		p.a.indptr = nullptr;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "nrm_front_plan_create_csr: null pointer"));
		q.a.indices = nullptr;
		CHECK(q.run() == NRM_E_ARG && !strcmp(g_err, "nrm_front_plan_create_csr: null pointer"));
		r.a.reads = nullptr;
		CHECK(r.run() == NRM_E_ARG && !strcmp(g_err, "nrm_front_plan_create_csr: null pointer"));
		s.a.h_cov = nullptr;
		CHECK(s.run() == NRM_E_ARG && !strcmp(g_err, "nrm_front_plan_create_csr: null pointer"));
	}
	{  // nnz and nnz_cap, for host arrays and for adopted ones (whose offsets are never read here: the pointer is an address nobody may touch)
		for (int on_device = 0; on_device < 2; on_device++) {
			Problem p;
			p.a.on_device = on_device;
			if (on_device) p.a.indptr = reinterpret_cast<const int64_t*>((uintptr_t)4096);
			CHECK(p.run() == NRM_OK);
			p.a.nnz = -1;
			CHECK(p.run() == NRM_E_ARG && strstr(g_err, "0 <= nnz <= nnz_cap"));
			p.a.nnz = p.nnz, p.a.nnz_cap = p.nnz - 1;
			CHECK(p.run() == NRM_E_ARG && strstr(g_err, "0 <= nnz <= nnz_cap"));
			p.a.nnz = 0, p.a.nnz_cap = 0;
			CHECK(p.run() == NRM_E_ARG && strstr(g_err, "nnz_cap >= 1"));
			p.a.nnz_cap = -3;
			CHECK(p.run() == NRM_E_ARG && strstr(g_err, "nnz_cap >= 1"));
		}
		Problem z;  // no stored entry at all is a matrix (check() says that it holds no read), in arrays of one element
		std::fill(z.indptr.begin(), z.indptr.end(), 0);
		z.a.nnz = 0, z.a.nnz_cap = 1;
		CHECK(z.run() == NRM_OK);
	}
	{  // alignment of the three arrays
		Problem p;
		p.a.on_device = 1;
		p.a.indptr = reinterpret_cast<const int64_t*>((uintptr_t)4100);
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "misaligned CSR arrays"));
		p.a.indptr = reinterpret_cast<const int64_t*>((uintptr_t)4096), p.a.indices = reinterpret_cast<const int32_t*>((uintptr_t)8194);
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "misaligned CSR arrays"));
		p.a.indices = reinterpret_cast<const int32_t*>((uintptr_t)8192), p.a.reads = reinterpret_cast<const void*>((uintptr_t)12290);
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "misaligned CSR arrays"));
		p.a.dtype = NRM_I16;
		CHECK(p.run() == NRM_OK);
	}
	{  // shapes: empty, too many genes, 2^31 cells (with no covariates: nothing of n cells is read)
		Problem p(0);
		p.a.rows = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "reads must not be empty."));
		p.a.rows = p.rows, p.a.n = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "reads must not be empty."));
		p.a.n = 1ll << 31;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "2^31"));
		p.a.n = 0x7fffffffLL;
		CHECK(p.run() == NRM_OK);
		p.a.n = p.n, p.a.rows = NRM_FRONT_MAX_ROWS + 1, p.a.on_device = 1;  // (adopted: the offsets of so many rows are not read)
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "genes"));
	}
	{  // the O(rows) structure of host offsets: not from 0, decreasing, ending elsewhere than nnz -- and none of it read for adopted arrays
		Problem p;
		p.indptr[0] = 1;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		p.a.on_device = 1;
		CHECK(p.run() == NRM_OK);
		Problem q;
		q.indptr[2] = 7, q.indptr[3] = 5;
		CHECK(q.run() == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		Problem r;
		r.indptr[r.rows] = r.nnz - 1;
		CHECK(r.run() == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		r.indptr[r.rows] = r.nnz + 1, r.a.nnz_cap = r.nnz + 4;
		CHECK(r.run() == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		r.a.nnz = r.nnz + 1;  // (the offsets and nnz agree: how many elements the arrays hold is the caller's word, as for every pointer)
		CHECK(r.run() == NRM_OK);
		Problem s;  // the last row alone decreasing
		s.indptr[s.rows - 1] = s.nnz + 1;
		CHECK(s.run() == NRM_E_ARG && !strcmp(g_err, MALFORMED));
	}
	{  // what create checks as well: the covariate bound, the options, the user rows
		Problem p4(4), p5(5);
		CHECK(p4.run() == NRM_OK);
		CHECK(p5.run() == NRM_E_UNSUPPORTED && strstr(g_err, "nrm_front_plan_create_csr") && strstr(g_err, "the 8 covariates") && strstr(g_err, "= 9"));
		Problem p;
		p.a.eps = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "eps and stepmax must be positive."));
		p.a.eps = 1e-6, p.a.stepmax = 0;
		CHECK(p.run() == NRM_E_ARG && !strcmp(g_err, "eps and stepmax must be positive."));
		p.a.stepmax = 1, p.a.tol = 1;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "tol"));
		p.a.tol = 1e-8, p.a.ntot = 0;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "ntot must be positive"));
		p.a.ntot = -1, p.a.out_dtype = NRM_I32;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "out_dtype"));
		p.a.out_dtype = NRM_F32, p.a.count_cap = 1;
		CHECK(p.run() == NRM_E_ARG && strstr(g_err, "count_cap must lie in [2, 16777216]"));
		p.a.count_cap = TABLE_CAP;
		CHECK(p.run() == NRM_OK);
		Problem q(2);
		q.cov[(size_t)(q.n + q.n - 1)] = NAN;
		CHECK(q.run() == NRM_E_ARG && !strcmp(g_err, "array must not contain infs or NaNs"));
		for (int64_t k = 0; k < q.n; k++) q.cov[(size_t)(q.n + k)] = 2.5;
		CHECK(q.run() == NRM_E_ARG && strstr(g_err, "Detected constant covariate."));
	}
	{  // upload_csr: a dense plan, an adopted matrix, null pointers, nnz beyond the capacity, the offsets
		Problem p;
		const int64_t cap = 16;
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, p.indptr.data(), p.indices.data(), p.data.data(), p.nnz) == NRM_OK);
		CHECK(nrm_front_plan_upload_csr_args(false, false, p.rows, cap, p.indptr.data(), p.indices.data(), p.data.data(), p.nnz) == NRM_E_ARG && strstr(g_err, "holds a dense matrix"));
		CHECK(nrm_front_plan_upload_csr_args(true, true, p.rows, cap, p.indptr.data(), p.indices.data(), p.data.data(), p.nnz) == NRM_E_ARG && strstr(g_err, "adopted"));
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, nullptr, p.indices.data(), p.data.data(), p.nnz) == NRM_E_ARG && strstr(g_err, "null pointer"));
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, p.indptr.data(), nullptr, p.data.data(), p.nnz) == NRM_E_ARG && strstr(g_err, "null pointer"));
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, p.indptr.data(), p.indices.data(), nullptr, p.nnz) == NRM_E_ARG && strstr(g_err, "null pointer"));
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, p.nnz - 1, p.indptr.data(), p.indices.data(), p.data.data(), p.nnz) == NRM_E_ARG &&
			  strstr(g_err, "10 stored entries, beyond the plan's nnz_cap = 9"));
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, p.indptr.data(), p.indices.data(), p.data.data(), -1) == NRM_E_ARG && strstr(g_err, "nnz_cap"));
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, p.indptr.data(), p.indices.data(), p.data.data(), p.nnz - 1) == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		p.indptr[1] = 5, p.indptr[2] = 3;
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, p.indptr.data(), p.indices.data(), p.data.data(), p.nnz) == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		std::vector<int64_t> none((size_t)(p.rows + 1), 0);  // no stored entry: the other two arrays may be absent
		CHECK(nrm_front_plan_upload_csr_args(true, false, p.rows, cap, none.data(), nullptr, nullptr, 0) == NRM_OK);
	}
	{  // the counters: the malformed word alone, in front of every one of the sixteen, and absent -- then nrm_front_plan_status's own answer, whatever it is
		int32_t f[16];
		memset(f, 0, sizeof(f));
		CHECK(nrm_front_plan_status_csr(0, f, 256, 0) == NRM_OK);
		CHECK(nrm_front_plan_status_csr(1, f, 256, 0) == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		CHECK(nrm_front_plan_status_csr(7, f, 256, 0) == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		const int read[10] = {0, 2, 1, 3, 4, 8, 9, 6, 12, 13};
		for (int mask = 1; mask < 1024; mask++) {
			memset(f, 0, sizeof(f));
			for (int i = 0; i < 10; i++)
				if (mask >> i & 1) f[read[i]] = read[i] + 2;
			CHECK(nrm_front_plan_status_csr(3, f, 256, 300) == NRM_E_ARG && !strcmp(g_err, MALFORMED));
			char dense[1024];
			const int want = nrm_front_plan_status(f, 256, 300);
			strcpy(dense, g_err);
			strcpy(g_err, "untouched");
			CHECK(want != NRM_OK && nrm_front_plan_status_csr(0, f, 256, 300) == want && !strcmp(g_err, dense));
		}
		memset(f, 0, sizeof(f));
		f[0] = 1;  // a negative entry is second
		CHECK(nrm_front_plan_status_csr(1, f, 256, 0) == NRM_E_ARG && !strcmp(g_err, MALFORMED));
		CHECK(nrm_front_plan_status_csr(0, f, 256, 0) == NRM_E_ARG && !strcmp(g_err, "Negative value in d detected."));
	}
	printf("front plan csr args ok\n");
	return 0;
}
