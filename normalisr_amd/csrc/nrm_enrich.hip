// Gene-set enrichment of study sets in a background of N genes: overlap counts, a two-sided Fisher exact test per (study, set) pair, the top set per study.
// Studies are the rows of a byte matrix (a binary network: one study per gene, or one row for a list of principal genes), sets the rows of a bit matrix
// packed on the host once per ontology (normalisr_amd/enrich.py).  W = ceil(G / 64) 64-bit words per row, bit g % 64 of word g / 64 for gene g.
//   k_enrich_pack     a wave per study row: 64 lanes read 64 adjacent bytes, the ballot of `byte != 0` IS the word; ANDed with the background, n[s] = its popcount
//   k_enrich_setsize  a wave per set: K[t] = popcount(sets[t] & bg)
//   k_enrich_overlap  k[s][t] = popcount(study[s] & sets[t]): a 64 x 64 tile per workgroup, 4 x 4 pairs per lane, 16 words of both operands at a time in LDS
//   k_enrich_fisher   a lane per pair: the recurrence of csrc/nrm_fisher.h in fp64, and the odds ratio
//   k_enrich_top      a workgroup per study: the qualifying set of smallest p, the lower index of equals
// Counts are integers and every floating-point value is computed by one lane alone: the same bits on every run.  No matrix cores: AND and popcount on the
// vector ALU (2.25e12 bit products at 15 000 x 10 000 x 15 000 are 3.5e10 word pairs, four instructions each).
#include "nrm_common.h"
#include "nrm_fisher.h"
#include "nrm_host_entry.h"

#define EN_TILE 64    // studies and sets per workgroup of k_enrich_overlap
#define EN_WORDS 16   // words of a row in LDS at a time
#define EN_PITCH 66   // LDS row of a word plane: 64 rows + 2 (a multiple of 16 bytes: the 4-row reads stay aligned; the transposed writes spread over the banks)

typedef unsigned long long en_u64;

struct EnrichTop {  // the record of nrm_enrich_top (include/normalisr_hip.h)
	int64_t index, k, K;
	double p;
};

// ---- pack ---------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_enrich_pack(const uint8_t* __restrict__ x, int64_t S, int64_t G, int64_t ld, int64_t W, const en_u64* __restrict__ bg,
													  en_u64* __restrict__ words, int32_t* __restrict__ cnt) {
	const int lane = threadIdx.x & 63;
	const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s >= S) return;  // (wave-uniform)
	const uint8_t* row = x + s * ld;
	en_u64* out = words + s * W;
	int n = 0;
	for (int64_t w0 = 0; w0 < W; w0 += 8) {  // eight loads in flight; a lane never reads at or beyond G, so the pad bits are zero
		uint8_t b[8];
#pragma unroll
		for (int u = 0; u < 8; u++) {
			const int64_t g = (w0 + u) * 64 + lane;
			b[u] = g < G ? row[g] : (uint8_t)0;
		}
		en_u64 mine = 0;
#pragma unroll
		for (int u = 0; u < 8; u++) {
			const en_u64 word = __ballot(b[u] != 0);
			if (lane == u) mine = word;
		}
		const int64_t w = w0 + lane;
		if (lane < 8 && w < W) {
			if (bg) mine &= bg[w];
			out[w] = mine;
			n += __popcll(mine);
		}
	}
#pragma unroll
	for (int o = 4; o > 0; o >>= 1) n += __shfl_down(n, o, 64);  // (lanes 0..7 hold the counts)
	if (lane == 0) cnt[s] = n;
}

__global__ void __launch_bounds__(256) k_enrich_setsize(const en_u64* __restrict__ sets, int64_t T, int64_t W, const en_u64* __restrict__ bg, int32_t* __restrict__ K) {
	const int lane = threadIdx.x & 63;
	const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= T) return;
	const en_u64* row = sets + t * W;
	int n = 0;
	for (int64_t w = lane; w < W; w += 64) n += __popcll(bg ? row[w] & bg[w] : row[w]);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
	if (lane == 0) K[t] = n;
}

// ---- overlap ------------------------------------------------------------------------------------------------------------------------------------------------------
// lane (ty, tx) of 16 x 16 owns studies s0 + 4 ty .. + 3 and sets t0 + 4 tx .. + 3.  A word plane of LDS holds word w of the tile's 64 rows side by side, so a
// lane reads its four studies and its four sets as 32 adjacent bytes each; the 16 lanes of equal ty read the same studies (a broadcast).
__global__ void __launch_bounds__(256) k_enrich_overlap(const en_u64* __restrict__ a, int64_t S, const en_u64* __restrict__ b, int64_t T, int64_t W,
														 int32_t* __restrict__ k) {
	__shared__ __attribute__((aligned(16))) en_u64 sa[EN_WORDS][EN_PITCH];
	__shared__ __attribute__((aligned(16))) en_u64 sb[EN_WORDS][EN_PITCH];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int64_t s0 = (int64_t)blockIdx.y * EN_TILE, t0 = (int64_t)blockIdx.x * EN_TILE;
	int acc[4][4];
#pragma unroll
	for (int i = 0; i < 4; i++)
#pragma unroll
		for (int j = 0; j < 4; j++) acc[i][j] = 0;
	for (int64_t w0 = 0; w0 < W; w0 += EN_WORDS) {
		__syncthreads();  // (the planes of the step before are still being read)
#pragma unroll
		for (int r0 = 0; r0 < EN_TILE; r0 += 16) {  // 16 lanes read 16 adjacent words of a row: 128 bytes
			const int r = r0 + ty;
			const int64_t w = w0 + tx;
			sa[tx][r] = (s0 + r < S && w < W) ? a[(s0 + r) * W + w] : 0ull;
			sb[tx][r] = (t0 + r < T && w < W) ? b[(t0 + r) * W + w] : 0ull;
		}
		__syncthreads();
#pragma unroll
		for (int w = 0; w < EN_WORDS; w++) {
			en_u64 av[4], bv[4];
#pragma unroll
			for (int i = 0; i < 4; i++) av[i] = sa[w][ty * 4 + i];
#pragma unroll
			for (int j = 0; j < 4; j++) bv[j] = sb[w][tx * 4 + j];
#pragma unroll
			for (int i = 0; i < 4; i++)
#pragma unroll
				for (int j = 0; j < 4; j++) acc[i][j] += __popcll(av[i] & bv[j]);
		}
	}
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int64_t s = s0 + ty * 4 + i;
		if (s >= S) continue;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int64_t t = t0 + tx * 4 + j;
			if (t < T) k[s * T + t] = acc[i][j];
		}
	}
}

// ---- Fisher exact test --------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_enrich_fisher(const int32_t* __restrict__ k, const int32_t* __restrict__ n, const int32_t* __restrict__ K, int64_t S, int64_t T,
														int64_t N, double* __restrict__ p, double* __restrict__ odds) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= S * T) return;
	const int64_t s = i / T, t = i - s * T;
	const int64_t kk = k[i], nn = n[s], KK = K[t];
	p[i] = nrm_fisher_p(N, KK, nn, kk);
	odds[i] = nrm_enrich_odds(N, KK, nn, kk);
}

// ---- selection ----------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_enrich_top(const int32_t* __restrict__ k, const int32_t* __restrict__ K, const double* __restrict__ p,
													 const double* __restrict__ odds, int64_t T, int64_t nmin, EnrichTop* __restrict__ top) {
	__shared__ double s_p[256];
	__shared__ int64_t s_i[256];
	const int tid = threadIdx.x;
	const int64_t s = blockIdx.x;
	const int32_t* kr = k + s * T;
	const double* pr = p + s * T;
	const double* orow = odds + s * T;
	double best = 2.0;  // (above any P-value: nothing found yet)
	int64_t at = T;
	for (int64_t t = tid; t < T; t += 256)  // (rising t: the first of equals stays)
		if (nrm_enrich_qualifies(orow[t], kr[t], nmin) && nrm_enrich_better(pr[t], t, best, at)) best = pr[t], at = t;
	s_p[tid] = best;
	s_i[tid] = at;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) {
		if (tid < o && nrm_enrich_better(s_p[tid + o], s_i[tid + o], s_p[tid], s_i[tid])) {
			s_p[tid] = s_p[tid + o];
			s_i[tid] = s_i[tid + o];
		}
		__syncthreads();
	}
	if (tid == 0) {
		const int64_t t = s_i[0];
		EnrichTop r;
		if (t < T) {
			r.index = t, r.k = kr[t], r.K = K[t], r.p = pr[t];
		} else {
			r.index = -1, r.k = 0, r.K = 0, r.p = 1.0;
		}
		top[s] = r;
	}
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------------------------
#define EN_MAX 0x7fffffffLL

extern "C" int nrm_enrich_pack(const uint8_t* d_study, int64_t S, int64_t G, int64_t ld, const uint64_t* d_bg, uint64_t* d_words, int32_t* d_n, void* stream) {
	NRM_REQUIRE(d_study && d_words && d_n, "nrm_enrich_pack: null pointer");
	NRM_REQUIRE(S > 0 && G > 0 && ld >= G, "nrm_enrich_pack: bad shape (S, G > 0, ld >= G)");
	NRM_REQUIRE(G <= EN_MAX && S <= EN_MAX, "nrm_enrich_pack: at most 2^31 - 1 genes and studies");
	NRM_REQUIRE((uintptr_t)d_words % 8 == 0 && (uintptr_t)d_bg % 8 == 0 && (uintptr_t)d_n % 4 == 0, "nrm_enrich_pack: misaligned word buffer");
	const int64_t W = (G + 63) / 64;
	hipLaunchKernelGGL(k_enrich_pack, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_study, S, G, ld, W, (const en_u64*)d_bg, (en_u64*)d_words, d_n);
	return nrm_check_launch("k_enrich_pack");
}

extern "C" int nrm_enrich_overlap(const uint64_t* d_study, int64_t S, const uint64_t* d_sets, int64_t T, int64_t G, const uint64_t* d_bg, int32_t* d_k, int32_t* d_K,
								   void* stream) {
	NRM_REQUIRE(d_study && d_sets && d_k && d_K, "nrm_enrich_overlap: null pointer");
	NRM_REQUIRE(S > 0 && T > 0 && G > 0, "nrm_enrich_overlap: bad shape (S, T, G > 0)");
	NRM_REQUIRE(G <= EN_MAX && S <= EN_MAX && T <= EN_MAX, "nrm_enrich_overlap: at most 2^31 - 1 genes, studies and sets");
	NRM_REQUIRE((S + EN_TILE - 1) / EN_TILE <= 65535, "nrm_enrich_overlap: at most 65535 x 64 studies in one call");
	NRM_REQUIRE((uintptr_t)d_study % 8 == 0 && (uintptr_t)d_sets % 8 == 0 && (uintptr_t)d_bg % 8 == 0 && (uintptr_t)d_k % 4 == 0 && (uintptr_t)d_K % 4 == 0,
				"nrm_enrich_overlap: misaligned word buffer");
	const int64_t W = (G + 63) / 64;
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(k_enrich_setsize, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, (const en_u64*)d_sets, T, W, (const en_u64*)d_bg, d_K);
	NRM_TRY(nrm_check_launch("k_enrich_setsize"));
	hipLaunchKernelGGL(k_enrich_overlap, dim3((unsigned)((T + EN_TILE - 1) / EN_TILE), (unsigned)((S + EN_TILE - 1) / EN_TILE)), dim3(256), 0, st, (const en_u64*)d_study, S,
					   (const en_u64*)d_sets, T, W, d_k);
	return nrm_check_launch("k_enrich_overlap");
}

extern "C" int nrm_enrich_fisher(const int32_t* d_k, const int32_t* d_n, const int32_t* d_K, int64_t S, int64_t T, int64_t N, double* d_p, double* d_odds, void* stream) {
	NRM_REQUIRE(d_k && d_n && d_K && d_p && d_odds, "nrm_enrich_fisher: null pointer");
	NRM_REQUIRE(S > 0 && T > 0 && N > 0, "nrm_enrich_fisher: bad shape (S, T, N > 0)");
	NRM_REQUIRE(N <= EN_MAX && S <= EN_MAX && T <= EN_MAX && (S * T + 255) / 256 <= EN_MAX, "nrm_enrich_fisher: at most 2^31 - 1 genes, and 2^39 pairs");
	NRM_REQUIRE((uintptr_t)d_p % 8 == 0 && (uintptr_t)d_odds % 8 == 0 && (uintptr_t)d_k % 4 == 0 && (uintptr_t)d_n % 4 == 0 && (uintptr_t)d_K % 4 == 0,
				"nrm_enrich_fisher: misaligned buffer");
	hipLaunchKernelGGL(k_enrich_fisher, dim3((unsigned)((S * T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_k, d_n, d_K, S, T, N, d_p, d_odds);
	return nrm_check_launch("k_enrich_fisher");
}

extern "C" int nrm_enrich_top(const int32_t* d_k, const int32_t* d_K, const double* d_p, const double* d_odds, int64_t S, int64_t T, int64_t nmin, void* d_top,
							   void* stream) {
	NRM_REQUIRE(d_k && d_K && d_p && d_odds && d_top, "nrm_enrich_top: null pointer");
	NRM_REQUIRE(S > 0 && T > 0 && S <= EN_MAX && T <= EN_MAX, "nrm_enrich_top: bad shape (0 < S, T < 2^31)");
	NRM_REQUIRE((uintptr_t)d_p % 8 == 0 && (uintptr_t)d_odds % 8 == 0 && (uintptr_t)d_top % 8 == 0 && (uintptr_t)d_k % 4 == 0 && (uintptr_t)d_K % 4 == 0,
				"nrm_enrich_top: misaligned buffer");
	if (nmin < 1) nmin = 1;
	hipLaunchKernelGGL(k_enrich_top, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, d_k, d_K, d_p, d_odds, T, nmin, (EnrichTop*)d_top);
	return nrm_check_launch("k_enrich_top");
}

// the recurrence of the kernel on host arrays: no device
extern "C" int nrm_fisher_host(const int64_t* N, const int64_t* K, const int64_t* n, const int64_t* k, int64_t count, double* out_p) {
	NRM_REQUIRE(count >= 0 && (count == 0 || (N && K && n && k && out_p)), "nrm_fisher_host: null pointer");
	for (int64_t i = 0; i < count; i++) {
		const int64_t lo = n[i] + K[i] - N[i] > 0 ? n[i] + K[i] - N[i] : 0, hi = n[i] < K[i] ? n[i] : K[i];
		NRM_REQUIRE(N[i] > 0 && N[i] <= EN_MAX && K[i] >= 0 && K[i] <= N[i] && n[i] >= 0 && n[i] <= N[i] && k[i] >= lo && k[i] <= hi,
					"nrm_fisher_host: table %lld is not one (0 <= K, n <= N < 2^31, max(0, n + K - N) <= k <= min(n, K))", (long long)i);
	}
	for (int64_t i = 0; i < count; i++) out_p[i] = nrm_fisher_p(N[i], K[i], n[i], k[i]);
	return NRM_OK;
}

// the selection of k_enrich_top on host arrays, one study after the other: no device
extern "C" int nrm_enrich_top_host(const int32_t* k, const int32_t* K, const double* p, const double* odds, int64_t S, int64_t T, int64_t nmin, void* top) {
	NRM_REQUIRE(k && K && p && odds && top, "nrm_enrich_top_host: null pointer");
	NRM_REQUIRE(S > 0 && T > 0 && S <= EN_MAX && T <= EN_MAX, "nrm_enrich_top_host: bad shape (0 < S, T < 2^31)");
	NRM_REQUIRE((uintptr_t)p % 8 == 0 && (uintptr_t)odds % 8 == 0 && (uintptr_t)top % 8 == 0 && (uintptr_t)k % 4 == 0 && (uintptr_t)K % 4 == 0,
				"nrm_enrich_top_host: misaligned buffer");
	if (nmin < 1) nmin = 1;
	for (int64_t s = 0; s < S; s++) {
		double best = 2.0;
		int64_t at = T;
		for (int64_t t = 0; t < T; t++)
			if (nrm_enrich_qualifies(odds[s * T + t], k[s * T + t], nmin) && nrm_enrich_better(p[s * T + t], t, best, at)) best = p[s * T + t], at = t;
		EnrichTop r;
		if (at < T) {
			r.index = at, r.k = k[s * T + at], r.K = K[at], r.p = best;
		} else {
			r.index = -1, r.k = 0, r.K = 0, r.p = 1.0;
		}
		((EnrichTop*)top)[s] = r;
	}
	return NRM_OK;
}

// ---- the whole problem from host buffers (no torch) -------------------------------------------------------------------------------------------------------------
extern "C" int nrm_enrich_host(const uint8_t* h_study, int64_t S, int64_t G, int64_t ld, const uint64_t* h_sets, int64_t T, const uint64_t* h_bg, int64_t nmin,
								int32_t* h_k, int32_t* h_K, int32_t* h_n, double* h_p, double* h_odds, void* h_top, int64_t* h_N) {
	NRM_REQUIRE(h_study && h_sets && h_k && h_K && h_n && h_p && h_odds && h_top && h_N, "nrm_enrich_host: null pointer");
	NRM_REQUIRE(S > 0 && T > 0 && G > 0 && ld >= G, "nrm_enrich_host: bad shape (S, T, G > 0, ld >= G)");
	NRM_REQUIRE(G <= EN_MAX && S <= EN_MAX && T <= EN_MAX, "nrm_enrich_host: at most 2^31 - 1 genes, studies and sets");
	NRM_REQUIRE((uintptr_t)h_sets % 8 == 0 && (uintptr_t)h_bg % 8 == 0, "nrm_enrich_host: misaligned word buffer");
	const int64_t W = (G + 63) / 64;
	int64_t N = G;
	if (h_bg) {
		N = 0;
		for (int64_t w = 0; w < W; w++) N += __builtin_popcountll(w == W - 1 && (G & 63) ? h_bg[w] & ((1ull << (G & 63)) - 1) : h_bg[w]);
	}
	NRM_REQUIRE(N > 0, "nrm_enrich_host: the background is empty");
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	hipStream_t st = nullptr;
	DevBuf x, sets, bg, words, n, K, k, p, odds, top;
	const size_t xb = (size_t)((S - 1) * ld + G), pairs = (size_t)S * T;
	NRM_TRY(x.alloc(xb));
	NRM_TRY(nrm_upload(h_study, x.p, (int64_t)xb, 0, (void*)st));
	NRM_TRY(sets.alloc((size_t)T * W * 8));
	NRM_TRY(nrm_upload(h_sets, sets.p, T * W * 8, 0, (void*)st));
	if (h_bg) {
		NRM_TRY(bg.alloc((size_t)W * 8));
		NRM_HIP(hipMemcpy(bg.p, h_bg, (size_t)W * 8, hipMemcpyHostToDevice));
	}
	NRM_TRY(words.alloc((size_t)S * W * 8));
	NRM_TRY(n.alloc((size_t)S * 4));
	NRM_TRY(K.alloc((size_t)T * 4));
	NRM_TRY(k.alloc(pairs * 4));
	NRM_TRY(p.alloc(pairs * 8));
	NRM_TRY(odds.alloc(pairs * 8));
	NRM_TRY(top.alloc((size_t)S * sizeof(EnrichTop)));
	NRM_TRY(nrm_enrich_pack(x.as<uint8_t>(), S, G, ld, bg.as<uint64_t>(), words.as<uint64_t>(), n.as<int32_t>(), st));
	NRM_TRY(nrm_enrich_overlap(words.as<uint64_t>(), S, sets.as<uint64_t>(), T, G, bg.as<uint64_t>(), k.as<int32_t>(), K.as<int32_t>(), st));
	NRM_TRY(nrm_enrich_fisher(k.as<int32_t>(), n.as<int32_t>(), K.as<int32_t>(), S, T, N, p.as<double>(), odds.as<double>(), st));
	NRM_TRY(nrm_enrich_top(k.as<int32_t>(), K.as<int32_t>(), p.as<double>(), odds.as<double>(), S, T, nmin, top.p, st));
	NRM_HIP(hipStreamSynchronize(st));
	NRM_HIP(hipMemcpy(h_k, k.p, pairs * 4, hipMemcpyDeviceToHost));
	NRM_HIP(hipMemcpy(h_K, K.p, (size_t)T * 4, hipMemcpyDeviceToHost));
	NRM_HIP(hipMemcpy(h_n, n.p, (size_t)S * 4, hipMemcpyDeviceToHost));
	NRM_HIP(hipMemcpy(h_p, p.p, pairs * 8, hipMemcpyDeviceToHost));
	NRM_HIP(hipMemcpy(h_odds, odds.p, pairs * 8, hipMemcpyDeviceToHost));
	NRM_HIP(hipMemcpy(h_top, top.p, (size_t)S * sizeof(EnrichTop), hipMemcpyDeviceToHost));
	*h_N = N;
	return NRM_OK;
}
