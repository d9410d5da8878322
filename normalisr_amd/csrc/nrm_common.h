// Shared host-side helpers for libnormalisr_hip.so (gfx950 only; no CUDA/compat paths).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include "../../include/normalisr_hip.h"

void nrm_set_error(const char* fmt, ...);
bool nrm_debug_is(const char* key, const char* value);  // NRM_DEBUG="key=value,..." holds `key` with exactly `value` (csrc/nrm_api.hip)

#define NRM_HIP(call)                                                                      \
	do {                                                                                   \
		hipError_t e_ = (call);                                                            \
		if (e_ != hipSuccess) {                                                            \
			(void)hipGetLastError(); /* the error is reported here: do not leave it for the next launch check */ \
			nrm_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
						  __LINE__);                                                       \
			return NRM_E_DEVICE;                                                           \
		}                                                                                  \
	} while (0)

#define NRM_REQUIRE(cond, ...)      \
	do {                            \
		if (!(cond)) {              \
			nrm_set_error(__VA_ARGS__); \
			return NRM_E_ARG;       \
		}                           \
	} while (0)

#define NRM_TRY(call)        \
	do {                     \
		int rc_ = (call);    \
		if (rc_) return rc_; \
	} while (0)

static inline int nrm_check_launch(const char* what) {
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) {
		nrm_set_error("launch of %s failed: %s", what, hipGetErrorString(e));
		return NRM_E_DEVICE;
	}
	return NRM_OK;
}

// Count matrices (lcpm, qc): bytes of an element of the dtype, 0 for a dtype counts do not come in; GO(type) for the dtype, checked before
static inline int nrm_count_elem(int dtype) { return dtype == NRM_I64 ? 8 : dtype == NRM_I32 ? 4 : dtype == NRM_I16 ? 2 : dtype == NRM_U8 ? 1 : 0; }

#define NRM_BY_COUNT_DTYPE(GO)           \
	switch (dtype) {                     \
		case NRM_I64: GO(int64_t); break; \
		case NRM_I32: GO(int32_t); break; \
		case NRM_I16: GO(int16_t); break; \
		default: GO(uint8_t); break;     \
	}

// the arrays of a CSR matrix (int64 indptr, int32 indices, data of elem bytes) as every entry that takes one checks them
static inline int nrm_csr_args_check(const char* what, const void* d_indptr, const void* d_indices, const void* d_data, int elem, int64_t rows, int64_t n, int64_t nnz) {
	NRM_REQUIRE(d_indptr && rows > 0 && n > 0 && nnz >= 0 && n <= 0x7fffffffLL, "%s: bad shape", what);
	NRM_REQUIRE(nnz == 0 || (d_indices && d_data), "%s: null pointer", what);
	NRM_REQUIRE((uintptr_t)d_indptr % 8 == 0 && (uintptr_t)d_indices % 4 == 0 && (uintptr_t)d_data % elem == 0, "%s: misaligned CSR arrays", what);
	return NRM_OK;
}

// covariates compute_var and normvar take (nrm_wide_covariates(); csrc/nrm_fitvar.hip, csrc/nrm_normvar_wide.hip): the workgroup's coefficient table,
// 4 rows of this many doubles in dynamic LDS, is 32 KiB
#define NRM_WIDE_NC 1024

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef float f16_t __attribute__((ext_vector_type(16)));
