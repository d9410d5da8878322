// C ABI glue: error reporting, device selection and the whole-problem host entry
// (numpy buffers in, numpy buffers out) that stands where association_tests() does
// (association.py:761-771,1093) for single=0.
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <cctype>
#include <strings.h>
#include <vector>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>
#include "nrm_common.h"
#include "nrm_host_logic.h"
#include "nrm_host_entry.h"

static thread_local char g_err[512] = "";

void nrm_set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

extern "C" int nrm_version(void) { return 100; }
extern "C" const char* nrm_last_error(void) { return g_err; }

extern "C" int nrm_device_count(int* count) {
	NRM_REQUIRE(count != nullptr, "nrm_device_count: null pointer");
	NRM_HIP(hipGetDeviceCount(count));
	return NRM_OK;
}

// The GPU the library's whole-problem entries run on.  hipSetDevice is per THREAD: the entry a Python thread calls, the helper threads that page-lock
// the caller's result arrays beside the kernels, and a second Python thread calling the next entry must all bind to the same device, and the scratch pool
// and the upload ring hold memory OF a device.  nrm_set_device records the choice for the process (validated: NRM_E_ARG -> ValueError for an index
// that is not there), releases what was cached for another device, and binds the calling thread; nrm_bind_device() binds any other thread.
static std::atomic<int> g_device{-1};
static NrmDevPool g_pool;

extern "C" int nrm_set_device(int device) {
	int count = 0;
	NRM_HIP(hipGetDeviceCount(&count));
	NRM_REQUIRE(device >= 0 && device < count, "GPU %d requested, %d visible", device, count);
	const int prev = g_device.exchange(device);
	if (prev != device && prev >= 0) {  // (scratch blocks and page-locked ring slots belong to the device they were made on)
		(void)hipSetDevice(prev);
		(void)hipDeviceSynchronize();
		g_pool.release();
		(void)nrm_upload_release();
	}
	NRM_HIP(hipSetDevice(device));
	return NRM_OK;
}

int nrm_bind_device(void) {
	const int d = g_device.load();
	if (d >= 0) NRM_HIP(hipSetDevice(d));
	return NRM_OK;
}

// h[0:a, a:b] = h[a:b, 0:a]^T on the host, for a row-major matrix of elem_bytes (4 or 8) elements with ld_bytes between rows: the rows
// a..b of a symmetric result matrix have arrived over PCIe up to column b, their mirror image above the diagonal is made here instead
// of travelling too (the reference's gather loop mirrors on the host as well: association.py:1049-1057).  32 x 32 tiles, the destination
// rows shared out over `threads` host threads (0: one per 4 hardware threads, at most 32).
template <typename E>
static void mirror_rows(char* h, int64_t ld, int64_t a, int64_t b, int64_t r0, int64_t r1) {
	constexpr int64_t TB = 32;
	for (int64_t i0 = r0; i0 < r1; i0 += TB)      // destination rows (columns of the source block)
		for (int64_t j0 = a; j0 < b; j0 += TB) {   // destination columns (rows of the source block)
			const int64_t i1 = std::min(i0 + TB, r1), j1 = std::min(j0 + TB, b);
			for (int64_t i = i0; i < i1; i++) {
				E* dst = reinterpret_cast<E*>(h + i * ld) + j0;
				for (int64_t j = j0; j < j1; j++) dst[j - j0] = reinterpret_cast<const E*>(h + j * ld)[i];
			}
		}
}

extern "C" int nrm_host_mirror_rows(void* h, int64_t ld_bytes, int elem_bytes, int64_t a, int64_t b, int threads) {
	NRM_REQUIRE(h && (elem_bytes == 4 || elem_bytes == 8) && 0 <= a && a <= b && ld_bytes >= b * elem_bytes, "nrm_host_mirror_rows: bad arguments");
	if (a == 0 || a == b) return NRM_OK;
	if (threads <= 0) threads = (int)std::min<int64_t>(32, std::max<int64_t>(1, std::thread::hardware_concurrency() / 4));
	threads = (int)std::min<int64_t>(threads, (a + 31) / 32);
	auto work = [&](int64_t r0, int64_t r1) {
		if (elem_bytes == 4)
			mirror_rows<uint32_t>((char*)h, ld_bytes, a, b, r0, r1);
		else
			mirror_rows<uint64_t>((char*)h, ld_bytes, a, b, r0, r1);
	};
	if (threads <= 1) {
		work(0, a);
		return NRM_OK;
	}
	const int64_t per = ((a + threads - 1) / threads + 31) / 32 * 32;
	std::vector<std::thread> pool;
	for (int t = 0; t < threads; t++) {
		const int64_t r0 = t * per, r1 = std::min<int64_t>(a, r0 + per);
		if (r1 > r0) pool.emplace_back(work, r0, r1);
	}
	for (auto& th : pool) th.join();
	return NRM_OK;
}

extern "C" int nrm_host_pin(void* ptr, int64_t bytes, int threads) {
	NRM_REQUIRE(ptr != nullptr && bytes > 0, "nrm_host_pin: empty range");
	NRM_TRY(nrm_bind_device());  // (called from the entries' helper threads too: a fresh thread's current device is 0)
	const int64_t page = 4096;
	if (threads <= 0) {
		threads = (int)std::min<int64_t>(16, std::max<int64_t>(1, bytes / (8 << 20)));
		threads = (int)std::min<int64_t>(threads, std::max(1u, std::thread::hardware_concurrency()));
	}
	// first touch from several threads: page faults of a fresh mapping are the cost of page-locking it (a single thread
	// faults ~13 GB/s, hipHostRegister of an untouched range ~22 GB/s, 16 threads > 100 GB/s)
	auto touch = [=](int64_t lo, int64_t hi) {
		volatile char* q = (volatile char*)ptr;
		for (int64_t o = lo; o < hi; o += page) q[o] = q[o];
		if (hi > lo) q[hi - 1] = q[hi - 1];
	};
	if (threads == 1) {
		touch(0, bytes);
	} else {
		const int64_t chunk = ((bytes + threads - 1) / threads + page - 1) / page * page;
		std::vector<std::thread> pool;
		for (int t = 0; t < threads; t++) {
			const int64_t lo = t * chunk, hi = std::min<int64_t>(bytes, lo + chunk);
			if (hi > lo) pool.emplace_back(touch, lo, hi);
		}
		for (auto& th : pool) th.join();
	}
	NRM_HIP(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
	return NRM_OK;
}

extern "C" int nrm_host_unpin(void* ptr) {
	NRM_REQUIRE(ptr != nullptr, "nrm_host_unpin: null pointer");
	NRM_HIP(hipHostUnregister(ptr));
	return NRM_OK;
}

extern "C" int nrm_host_alloc(void** ptr, int64_t bytes) {
	NRM_REQUIRE(ptr != nullptr && bytes > 0, "nrm_host_alloc: empty request");
	NRM_HIP(hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault));
	return NRM_OK;
}

extern "C" int nrm_host_free(void* ptr) {
	if (ptr) NRM_HIP(hipHostFree(ptr));
	return NRM_OK;
}

extern "C" int nrm_copy_to_host(void* h_dst, const void* d_src, int64_t bytes, void* stream) {
	NRM_REQUIRE(bytes >= 0, "nrm_copy_to_host: negative size");
	if (bytes == 0) return NRM_OK;
	NRM_REQUIRE(h_dst && d_src, "nrm_copy_to_host: null pointer");
	NRM_HIP(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
	return NRM_OK;
}

// (Measured, tools/time_duplex.py: on this platform a 1-D hipMemcpy runs at 56 GB/s in either direction but an upload and a
// download queue behind each other -- 200 MB + 200 MB take 7.2 ms together; this rectangular copy is served by a blit kernel at
// 27 GB/s that does run beside an upload, 4.5 ms together; a hand-written kernel storing into mapped host memory reaches the same
// 27 GB/s with 16 to 4096 workgroups and was slower end to end, it competes with K2 for the CUs.)
extern "C" int nrm_copy_rect_to_host(void* h_dst, int64_t dst_pitch, const void* d_src, int64_t src_pitch, int64_t row_bytes, int64_t rows,
									 void* stream) {
	NRM_REQUIRE(row_bytes >= 0 && rows >= 0 && dst_pitch >= row_bytes && src_pitch >= row_bytes, "nrm_copy_rect_to_host: pitches smaller than the row");
	if (row_bytes == 0 || rows == 0) return NRM_OK;
	NRM_REQUIRE(h_dst && d_src, "nrm_copy_rect_to_host: null pointer");
	NRM_HIP(hipMemcpy2DAsync(h_dst, (size_t)dst_pitch, d_src, (size_t)src_pitch, (size_t)row_bytes, (size_t)rows, hipMemcpyDeviceToHost,
							 (hipStream_t)stream));
	return NRM_OK;
}

// Fills and device-to-device row copies as kernels of the library rather than hipMemsetAsync / hipMemcpy2DAsync: these run inside the steps
// a resident plan captures as a HIP graph (DePlan: the result counters, the padded rows, the Z buffer), and a memset or copy node of a
// replayed graph was seen to leave the 16 bytes of a DePlan's counters holding two addresses once other launches and host copies had run
// between replays -- the third replay after a rewrite, every time; as kernels, the same sequence gives the counters it should
// (tests/test_gpu_plan_rewrites.py).
namespace {
constexpr int FILL_THREADS = 256;

inline unsigned fill_blocks(uint64_t units) {
	uint64_t b = (units + FILL_THREADS - 1) / FILL_THREADS;
	return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));  // (grid-stride loops below)
}

__global__ void k_fill_zero16(uint4* __restrict__ d, uint64_t n16) {
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) d[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void k_fill_bytes(unsigned char* __restrict__ d, uint64_t n, unsigned char v) {
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) d[i] = v;
}

__global__ void k_fill_i32(int32_t* __restrict__ d, uint64_t n, int32_t v) {
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) d[i] = v;
}

// rows x per_row units of type T; pitches in units of T
template <typename T>
__global__ void k_copy_rows(T* __restrict__ d, uint64_t dp, const T* __restrict__ s, uint64_t sp, uint64_t per_row, uint64_t rows) {
	const uint64_t total = per_row * rows;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t r = i / per_row, c = i - r * per_row;
		d[r * dp + c] = s[r * sp + c];
	}
}
}  // namespace

extern "C" int nrm_fill_zero(void* d_dst, int64_t bytes, void* stream) {
	NRM_REQUIRE(bytes >= 0, "nrm_fill_zero: negative size");
	if (bytes == 0) return NRM_OK;
	NRM_REQUIRE(d_dst != nullptr, "nrm_fill_zero: null pointer");
	hipStream_t st = (hipStream_t)stream;
	unsigned char* d = (unsigned char*)d_dst;
	uint64_t n = (uint64_t)bytes, n16 = ((uintptr_t)d % 16 == 0) ? n / 16 : 0;
	if (n16) {
		hipLaunchKernelGGL(k_fill_zero16, dim3(fill_blocks(n16)), dim3(FILL_THREADS), 0, st, (uint4*)d, n16);
		NRM_HIP(hipGetLastError());
	}
	if (n > n16 * 16) {
		hipLaunchKernelGGL(k_fill_bytes, dim3(fill_blocks(n - n16 * 16)), dim3(FILL_THREADS), 0, st, d + n16 * 16, n - n16 * 16, (unsigned char)0);
		NRM_HIP(hipGetLastError());
	}
	return NRM_OK;
}

extern "C" int nrm_fill_i32(void* d_dst, int32_t value, int64_t count, void* stream) {
	NRM_REQUIRE(count >= 0, "nrm_fill_i32: negative size");
	if (count == 0) return NRM_OK;
	NRM_REQUIRE(d_dst != nullptr && (uintptr_t)d_dst % 4 == 0, "nrm_fill_i32: bad pointer");
	hipLaunchKernelGGL(k_fill_i32, dim3(fill_blocks((uint64_t)count)), dim3(FILL_THREADS), 0, (hipStream_t)stream, (int32_t*)d_dst, (uint64_t)count, value);
	NRM_HIP(hipGetLastError());
	return NRM_OK;
}

extern "C" int nrm_copy_rows(void* d_dst, int64_t dst_pitch, const void* d_src, int64_t src_pitch, int64_t row_bytes, int64_t rows,
							 void* stream) {
	NRM_REQUIRE(row_bytes >= 0 && rows >= 0 && dst_pitch >= row_bytes && src_pitch >= row_bytes, "nrm_copy_rows: pitches smaller than the row");
	if (row_bytes == 0 || rows == 0) return NRM_OK;
	NRM_REQUIRE(d_dst && d_src, "nrm_copy_rows: null pointer");
	hipStream_t st = (hipStream_t)stream;
	const uint64_t a = (uint64_t)(uintptr_t)d_dst | (uint64_t)(uintptr_t)d_src | (uint64_t)dst_pitch | (uint64_t)src_pitch | (uint64_t)row_bytes;
	const uint64_t r = (uint64_t)rows;
	if (a % 16 == 0) {
		const uint64_t per = (uint64_t)row_bytes / 16;
		hipLaunchKernelGGL(k_copy_rows<uint4>, dim3(fill_blocks(per * r)), dim3(FILL_THREADS), 0, st, (uint4*)d_dst, (uint64_t)dst_pitch / 16,
						   (const uint4*)d_src, (uint64_t)src_pitch / 16, per, r);
	} else if (a % 4 == 0) {
		const uint64_t per = (uint64_t)row_bytes / 4;
		hipLaunchKernelGGL(k_copy_rows<uint32_t>, dim3(fill_blocks(per * r)), dim3(FILL_THREADS), 0, st, (uint32_t*)d_dst, (uint64_t)dst_pitch / 4,
						   (const uint32_t*)d_src, (uint64_t)src_pitch / 4, per, r);
	} else {
		hipLaunchKernelGGL(k_copy_rows<unsigned char>, dim3(fill_blocks((uint64_t)row_bytes * r)), dim3(FILL_THREADS), 0, st, (unsigned char*)d_dst,
						   (uint64_t)dst_pitch, (const unsigned char*)d_src, (uint64_t)src_pitch, (uint64_t)row_bytes, r);
	}
	NRM_HIP(hipGetLastError());
	return NRM_OK;
}

static std::mutex g_host_entry;
NrmDevPool& nrm_host_pool() { return g_pool; }
std::mutex& nrm_host_entry_mutex() { return g_host_entry; }

namespace {
struct CopyStream {
	hipStream_t s = nullptr;
	std::vector<hipEvent_t> events;
	~CopyStream() {
		for (hipEvent_t e : events) (void)hipEventDestroy(e);
		if (s) (void)hipStreamDestroy(s);
	}
};
}  // namespace

extern "C" int nrm_release_cache(void) {
	g_pool.release();
	return NRM_OK;
}

// the pool's own accounting: bytes of device memory it holds, and how many of them are taken (by a running entry or a live plan)
extern "C" int nrm_cache_bytes(int64_t* held, int64_t* in_use) {
	std::lock_guard<std::mutex> g(g_pool.mu);
	int64_t h = 0, u = 0;
	for (const auto& b : g_pool.blocks) {
		h += (int64_t)b.cap;
		if (b.used) u += (int64_t)b.cap;
	}
	if (held) *held = h;
	if (in_use) *in_use = u;
	return NRM_OK;
}

// Verdict of the integer engine's accuracy guard (csrc/nrm_fix.h) for the last whole-problem call of this thread: pairs it could not
// certify on the first pass (0: the integer engine's results were returned; > 0: the call was redone on the fp64 Gram kernel),
// and the largest error estimate of a P-value (relative) among the pairs it looked at.
static thread_local int64_t g_guard_hits = 0;
static thread_local double g_guard_worst = 0.0;

extern "C" int nrm_last_guard(int64_t* hits, double* worst) {
	if (hits) *hits = g_guard_hits;
	if (worst) *worst = g_guard_worst;
	return NRM_OK;
}

// NRM_DEBUG="key=value,key=value" read the way normalisr_amd/_opts.py reads it: split on ',', key and value trimmed, the key compared without case --
// so that a switch means the same to the package's engine and to the library's own entries.  true: `key` is there with exactly `value`.
bool nrm_debug_is(const char* key, const char* value) {
	const char* d = getenv("NRM_DEBUG");
	if (!d) return false;
	const size_t kl = strlen(key), vl = strlen(value);
	while (*d) {
		const char* end = strchr(d, ',');
		if (!end) end = d + strlen(d);
		const char* eq = (const char*)memchr(d, '=', (size_t)(end - d));
		if (eq) {
			const char *k0 = d, *k1 = eq, *v0 = eq + 1, *v1 = end;
			while (k0 < k1 && isspace((unsigned char)*k0)) k0++;
			while (k1 > k0 && isspace((unsigned char)k1[-1])) k1--;
			while (v0 < v1 && isspace((unsigned char)*v0)) v0++;
			while (v1 > v0 && isspace((unsigned char)v1[-1])) v1--;
			if ((size_t)(k1 - k0) == kl && (size_t)(v1 - v0) == vl && !strncasecmp(k0, key, kl) && !strncmp(v0, value, vl)) return true;
		}
		d = *end ? end + 1 : end;
	}
	return false;
}

static bool de_path_general() {  // NRM_DEBUG="de_path=general" (or NRM_DE_PATH=general): no streaming de kernel, as in normalisr_amd/_opts.py
	if (nrm_debug_is("de_path", "general")) return true;
	const char* e = getenv("NRM_DE_PATH");
	return e && !strcmp(e, "general");
}

static int association_tests_host_impl(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny,
										  const void* h_dc, int c_dtype, int64_t nc, int64_t n, const double* h_dci, int rank,
										  int dimreduce, int return_dot, void* h_p, void* h_stat, void* h_alpha, void* h_varx,
										  void* h_vary, void* h_r, void* h_t, int out_dtype, int nslices, int64_t* guard_hits, bool allow_sparse, int p_kind);

extern "C" int nrm_association_tests_host_pk(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny,
											 const void* h_dc, int c_dtype, int64_t nc, int64_t n, const double* h_dci, int rank,
											 int dimreduce, int return_dot, void* h_p, void* h_stat, void* h_alpha, void* h_varx,
											 void* h_vary, void* h_r, void* h_t, int out_dtype, int p_kind) {
	NRM_REQUIRE(p_kind == 0 || p_kind == 1, "p_kind must be 0 (P-values) or 1 (their natural logarithms)");
	std::lock_guard<std::mutex> serial(g_host_entry);
	NRM_TRY(nrm_bind_device());
	// K2 engine as in the Python host (NRM_GRAM): exact fixed-point contraction on the int8 matrix cores (6 slices = 46 bits; i8x5: 5
	// slices = 38 bits), or the fp64 matrix-core kernel (f64).  With the integer engine K1 writes the digit planes itself and the
	// fp64 residuals are never stored.
	int nslices = 0;
	NRM_TRY(nrm_assoc_engine(n, n % 4 == 0, &nslices));  // (K1's fused quantiser needs 16-byte aligned rows of the unpadded host matrices)
	g_guard_hits = 0;
	g_guard_worst = 0.0;
	int64_t hits = 0;
	int rc = association_tests_host_impl(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, h_p, h_stat,
										 h_alpha, h_varx, h_vary, h_r, h_t, out_dtype, nslices, &hits, true, p_kind);
	if (rc == NRM_OK && hits > 0) {  // pairs the guard could not certify (or rows the sparse-design kernels handed back): the whole call again on the fp64 matrix cores
		g_guard_hits = hits;
		if (p_kind) {
			// ln P: the guard's rule differs from the one for P (csrc/nrm_fix.h), and p_kind changes the first result only.  So everything else is what the call
			// returns without it -- its own verdict and rerun included --, and ln P alone comes from the fp64 pass, whose other results go to scratch.
			int64_t lin = 0;
			rc = association_tests_host_impl(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, h_p, h_stat, h_alpha, h_varx, h_vary,
											 h_r, h_t, out_dtype, nslices, &lin, true, 0);
			if (rc == NRM_OK && lin > 0)
				rc = association_tests_host_impl(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, h_p, h_stat, h_alpha, h_varx,
												 h_vary, h_r, h_t, out_dtype, 0, nullptr, false, 0);
			if (rc != NRM_OK) return rc;
			const size_t rows_y = (size_t)(h_dy ? ny : nx), ob = (size_t)nx * rows_y * nrm_esize(out_dtype);
			std::vector<char> s_stat(ob), s_alpha(h_alpha ? ob * (size_t)nc : 0), s_varx(h_varx ? (size_t)nx * 8 : 0), s_vary(rows_y * 8), s_r(h_r ? ob : 0), s_t(h_t ? ob : 0);
			return association_tests_host_impl(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, h_p, s_stat.data(),
											   h_alpha ? s_alpha.data() : nullptr, h_varx ? s_varx.data() : nullptr, s_vary.data(), h_r ? s_r.data() : nullptr,
											   h_t ? s_t.data() : nullptr, out_dtype, 0, nullptr, false, 1);
		}
		rc = association_tests_host_impl(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, h_p, h_stat,
										 h_alpha, h_varx, h_vary, h_r, h_t, out_dtype, 0, nullptr, false, p_kind);
	}
	return rc;
}

extern "C" int nrm_association_tests_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny,
										  const void* h_dc, int c_dtype, int64_t nc, int64_t n, const double* h_dci, int rank,
										  int dimreduce, int return_dot, void* h_p, void* h_stat, void* h_alpha, void* h_varx,
										  void* h_vary, void* h_r, void* h_t, int out_dtype) {
	return nrm_association_tests_host_pk(h_dx, x_dtype, nx, h_dy, y_dtype, ny, h_dc, c_dtype, nc, n, h_dci, rank, dimreduce, return_dot, h_p, h_stat, h_alpha, h_varx, h_vary,
										 h_r, h_t, out_dtype, 0);
}

static int association_tests_host_impl(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny,
										  const void* h_dc, int c_dtype, int64_t nc, int64_t n, const double* h_dci, int rank,
										  int dimreduce, int return_dot, void* h_p, void* h_stat, void* h_alpha, void* h_varx,
										  void* h_vary, void* h_r, void* h_t, int out_dtype, int nslices, int64_t* guard_hits, bool allow_sparse, int p_kind) {
	const bool samexy = (h_dy == nullptr);
	if (samexy) {
		ny = nx;
		y_dtype = x_dtype;
	}
	NRM_TRY(nrm_assoc_check_args(h_dx, nx, ny, h_dc, nc, n, rank, dimreduce));
	NRM_REQUIRE(h_p && h_stat && h_vary, "nrm_association_tests_host: null output");
	const double dof = (double)(n - 1 - rank - dimreduce);
	hipStream_t st = nullptr;
	const int64_t kp = nrm_round_up(n, NRM_K_TILE), mp = nrm_round_up(nx, NRM_ROW_TILE), np_ = nrm_round_up(ny, NRM_ROW_TILE);

	DevBuf cmax, dx, dy, dc, dci, rx, ry, ssx, ssy, bx, by, dot, flags, oalpha;
	NrmAssocOut out;
	// the caller's result arrays are page-locked in place by a helper thread while K1/K2 run (started after the uploads:
	// a hipHostRegister racing a pageable H2D copy was measured to stall that copy by ~20 ms)
	const size_t ob = (size_t)nx * ny * nrm_esize(out_dtype);
	NrmHostPin pin_p, pin_s, pin_r, pin_t;
	std::thread pinner;
	NrmJoiner joiner{pinner};
	std::vector<double> c64;
	NRM_TRY(covariates_f64(h_dc, c_dtype, nc, n, c64, dc));
	NRM_TRY(covariate_bounds(c64, nc, n, h_dci, rank, cmax, dci));
	const bool want_alpha = h_alpha != nullptr && nc > 0;
	NRM_REQUIRE(!(want_alpha && samexy), "alpha is not provided for dy == NULL (meaningless in the reference, association.py:1066-1068)");
	DevBuf qx, qy, ex, ey, fx, fy;
	const double guard_tol = nrm_guard_tolerance();
	NRM_TRY(upload_matrix(h_dx, x_dtype, nx, n, dx, st));
	// A design matrix with few entries (a CRISPR screen's gRNA incidence): the sparse-design kernels -- the expression rows read once, raw, the
	// contraction replaced by gathers at the design's entries (nrm_host_de.hip; what normalisr_amd.engine does for the Python host), for the calls
	// nrm_de_sparse_wanted (nrm_host_entry.h) names.
	// de with few design rows (case-control DE, BASELINE configs[2]): the raw expression rows streamed once against [C; X~], as the Python engine does
	// (engine.association_de_streaming); NRM_DEBUG de_path=general keeps K1 + K2
	if (allow_sparse && !samexy && nx + nc <= 32 && !de_path_general()) {
		return nrm_host_de_streaming(dx.p, x_dtype, nx, h_dy, y_dtype, ny, c64.data(), nc, n, h_dci, rank, dof, return_dot ? 0 : 1, h_p, h_stat, want_alpha ? h_alpha : nullptr,
									 h_varx, h_vary, h_r, h_t, out_dtype, p_kind);
	}
	bool dy_up = false;
	if (allow_sparse && !samexy && nrm_de_sparse_wanted(nx, ny, n, nc)) {
		NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, dy, st));
		dy_up = true;
		int taken = 0;
		int64_t back = 0;
		NRM_TRY(nrm_host_de_sparse(dx.p, x_dtype, nx, dy.p, y_dtype, ny, dc.as<double>(), c64.data(), nc, n, dci.as<double>(), rank, dof, (return_dot ? 0 : 1), h_p, h_stat,
								   want_alpha ? h_alpha : nullptr, h_varx, h_vary, h_r, h_t, out_dtype, &taken, &back, p_kind));
		if (taken) {
			if (back > 0 && guard_hits) *guard_hits = back;
			return NRM_OK;
		}
	}
	NRM_TRY(ssx.alloc((size_t)mp * 8));
	if (want_alpha) NRM_TRY(bx.alloc_zero((size_t)nx * nc * 8, st));
	if (nslices) {
		NRM_TRY(qx.alloc((size_t)nrm_quant_bytes(mp, kp, nslices)));
		NRM_TRY(ex.alloc((size_t)mp * 4));
		NRM_TRY(fx.alloc((size_t)mp * 8 * 8));
	} else {
		NRM_TRY(rx.alloc((size_t)mp * kp * 8));
	}
	NRM_TRY(nrm_assoc_k1(dx.p, x_dtype, nx, n, n, dc.as<double>(), nc, dci.as<double>(), rank, kp, mp, ssx.as<double>(), want_alpha ? bx.as<double>() : nullptr, nslices, qx.p,
						 ex.as<int32_t>(), cmax.as<double>(), fx.as<double>(), rx.as<double>(), st));
	if (!samexy) {
		if (!dy_up) NRM_TRY(upload_matrix(h_dy, y_dtype, ny, n, dy, st));
		NRM_TRY(ssy.alloc((size_t)np_ * 8));
		if (want_alpha) NRM_TRY(by.alloc_zero((size_t)ny * nc * 8, st));
		if (nslices) {
			NRM_TRY(qy.alloc((size_t)nrm_quant_bytes(np_, kp, nslices)));
			NRM_TRY(ey.alloc((size_t)np_ * 4));
			NRM_TRY(fy.alloc((size_t)np_ * 8 * 8));
		} else {
			NRM_TRY(ry.alloc((size_t)np_ * kp * 8));
		}
		NRM_TRY(nrm_assoc_k1(dy.p, y_dtype, ny, n, n, dc.as<double>(), nc, dci.as<double>(), rank, kp, np_, ssy.as<double>(), want_alpha ? by.as<double>() : nullptr, nslices, qy.p,
							 ey.as<int32_t>(), cmax.as<double>(), fy.as<double>(), ry.as<double>(), st));
	}
	const double* sx = ssx.as<double>();
	const double* sy = samexy ? sx : ssy.as<double>();
	pinner = std::thread([&] {
		pin_p.try_pin(h_p, (int64_t)ob);
		pin_s.try_pin(h_stat, (int64_t)ob);
		pin_r.try_pin(h_r, (int64_t)ob);
		pin_t.try_pin(h_t, (int64_t)ob);
	});
	NRM_TRY(dot.alloc((size_t)mp * np_ * 8));
	DevBuf gwork;
	NRM_TRY(gwork.alloc((size_t)nrm_gram_workspace_bytes()));
	NRM_TRY(flags.alloc_zero(16, st));
	NRM_TRY(out.alloc(ob, h_r != nullptr, h_t != nullptr));
	// coex always converts to covariance (association.py:1037-1039); de keeps gamma unless return_dot
	const int stat_kind = (samexy || return_dot) ? 0 : 1;
	// K2 -> K3 per band of output rows; finished bands are copied out on a second stream while later bands compute
	// (the reference's gather loop, association.py:997-1034, consumes finished tiles the same way)
	const int64_t band = NRM_ASSOC_BAND;
	NrmAssocOperands ops;
	ops.qx = qx.p, ops.ex = ex.as<int32_t>(), ops.fx = fx.as<double>(), ops.rx = rx.as<double>(), ops.ssx = sx;
	ops.qy = samexy ? qx.p : qy.p, ops.ey = samexy ? ops.ex : ey.as<int32_t>(), ops.fy = samexy ? ops.fx : fy.as<double>(), ops.ry = samexy ? ops.rx : ry.as<double>(), ops.ssy = sy;
	ops.nx = nx, ops.ny = ny, ops.n = n, ops.mp = mp, ops.np_ = np_, ops.kp = kp;
	ops.nslices = nslices, ops.samexy = samexy ? 1 : 0, ops.stat_kind = stat_kind, ops.out_dtype = out_dtype, ops.dof = dof, ops.guard_tol = guard_tol;
	ops.p_kind = p_kind;
	ops.dot = dot.as<double>(), ops.gwork = gwork.p, ops.flags = flags.as<int32_t>();
	ops.p = out.p.p, ops.stat = out.stat.p, ops.r = out.r.p, ops.t = out.t.p;
	CopyStream cs;
	NRM_HIP(hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking));
	for (int64_t a = 0; a < nx; a += band) {
		const int64_t b = std::min(nx, a + band);
		NRM_TRY(nrm_assoc_band(ops, a, b, st));
		hipEvent_t ev;
		NRM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
		cs.events.push_back(ev);
		NRM_HIP(hipEventRecord(ev, st));
	}
	if (pinner.joinable()) pinner.join();
	const size_t row = (size_t)ny * nrm_esize(out_dtype);
	for (int64_t a = 0, i = 0; a < nx; a += band, i++) {
		const int64_t b = std::min(nx, a + band);
		NRM_HIP(hipStreamWaitEvent(cs.s, cs.events[(size_t)i], 0));
		const size_t off = (size_t)a * row, len = (size_t)(b - a) * row;
		NRM_HIP(hipMemcpyAsync((char*)h_p + off, (const char*)out.p.p + off, len, hipMemcpyDeviceToHost, cs.s));
		NRM_HIP(hipMemcpyAsync((char*)h_stat + off, (const char*)out.stat.p + off, len, hipMemcpyDeviceToHost, cs.s));
		if (h_r) NRM_HIP(hipMemcpyAsync((char*)h_r + off, (const char*)out.r.p + off, len, hipMemcpyDeviceToHost, cs.s));
		if (h_t) NRM_HIP(hipMemcpyAsync((char*)h_t + off, (const char*)out.t.p + off, len, hipMemcpyDeviceToHost, cs.s));
	}
	if (want_alpha) {
		// alpha comes from gamma whatever return_dot says (association.py:238-243 vs :1044-1048)
		NRM_TRY(oalpha.alloc(ob * nc));
		NRM_TRY(nrm_alpha(out.stat.p, out_dtype, ny, stat_kind, ssx.as<double>(), n, bx.as<double>(), by.as<double>(), nx, ny, nc, oalpha.p,
						  out_dtype, st));
	}
	NRM_HIP(hipStreamSynchronize(st));
	NRM_HIP(hipStreamSynchronize(cs.s));
	int32_t hf[4];
	NRM_TRY(nrm_read_flags(flags.p, st, hf));
	NRM_TRY(nrm_assoc_assertions(hf, " tiles"));
	if (nslices) {
		float w;
		memcpy(&w, &hf[3], 4);
		g_guard_worst = (double)w;
		if (guard_hits) *guard_hits = hf[2];
		if (hf[2] > 0 && guard_hits) return NRM_OK;  // the caller redoes the call on the fp64 kernel: nothing more to bring back from this pass
	}
	if (want_alpha) NRM_HIP(hipMemcpy(h_alpha, oalpha.p, ob * nc, hipMemcpyDeviceToHost));
	NRM_TRY(emit_var(sy, ny, n, h_vary, out_dtype));
	if (h_varx && !samexy) NRM_TRY(emit_var(sx, nx, n, h_varx, out_dtype));
	return NRM_OK;
}
