// bh: Benjamini-Hochberg q-values over ALL entries of a P-value matrix that lies in HBM (reference binnet.py:77-131 with weight=None) -- what a screen's de step
// delivers, without the result leaving the device.  For N valid entries (finite, in [0, 1]) the reference reduces to
//   u = the sorted distinct values (-0.0 counts as 0.0),  c(u) = #{entries <= u} (an exact integer),  w = fl(c / N),  q(u) = fl(u / w), non-finite -> 1,
//   clipped to [0, 1],  q(u) <- min over u' >= u of q(u'),  output q(pv[i]) in the input's dtype
// -- two divisions in the input's dtype and an exact minimum, so the result here equals the reference's bit for bit.  fp64: both divisions in IEEE fp64.  fp32: both
// in fp64, each rounded once to fp32 (for fp32 operands that is the correctly rounded fp32 quotient, 53 >= 2 * 24 + 2) as long as c and N are exact in fp32, N <= 2^24.
// Beyond 2^24 fp32 entries the reference's fp32 cumsum of ones stalls at 2^24; the counts here stay exact: a documented departure.
// This file must not be built with relaxed division (normalisr_amd/build.py has no such flag).
//
// The work is a sort.  Keys are the entries' IEEE bit patterns as unsigned integers (monotone for non-negative finite values; the pattern of -0.0 becomes 0):
//   k_bh_keys       one pass over the P-values: keys into the workspace, entries that are NaN, infinite, < 0 or > 1 counted into d_flags[0]
//   LSD radix sort, keys only (equal keys cannot be told apart, so nothing is carried along), 8-bit digits: 4 passes for fp32, 8 for fp64, three launches each
//     k_bh_hist     a workgroup's tile of BH_TILE keys -> its 256 digit counts (LDS integer atomics: the sums do not depend on their order)
//     scan          exclusive sums over the (digit, workgroup) table: one workgroup for up to BH_TILE entries, else per-chunk sums, their scan by ONE workgroup
//                   that walks them chunk by chunk, and a per-chunk apply -- a second level of launches, never a workgroup that waits for another
//     k_bh_scatter  stable: a wave ranks its keys per digit from ballots over the digit's bits and a per-wave LDS count, the waves' counts are prefixed in LDS
//   k_bh_ends / k_bh_q / k_bh_q_apply   on the sorted keys: c = (last position of the same key) + 1 by a backward minimum over "a key ends here" positions,
//                   q as above, then the suffix minimum of q -- both as per-tile minimum, exclusive backward scan of the tiles' minima by one workgroup, apply;
//                   a tie group may span any number of tiles.  d_flags[1] = more than one distinct key.
//   k_bh_sample / k_bh_lookup   a thread per entry: lower-bound search of its key in the sorted keys, on sampled levels of them (a cache line per level),
//                   that position's q into d_q
// The launch sequence depends on (N, dtype) only, never on the data, and nothing is read back: nrm_bh can be queued behind a plan's step and captured into a HIP graph.
// Every digit indexes a 256-bin table and every search stays inside [0, N), so entries that are not P-values cannot send an access out of range.
//
// The ln form (nrm_bh_pk with p_kind = 1): the entries are ln P -- <= 0 and no NaN, -inf being the exact zero of the linear form -- and the
// output is ln q(u) = min(0, u + (ln N - ln c(u))), then the minimum over u' >= u, evaluated in fp64 for both dtypes and rounded once at the store.  k_bh_keys, k_bh_q
// and k_bh_lookup take p_kind as a compile-time parameter: keys are the complemented bit patterns of |ln P| (ascending key = ascending ln P, -inf first, both zeros the
// largest key); the sort, the scans, the tie ends, the suffix minimum and the sampled levels are the same launches on the same workspace, so the launch sequence
// depends on (N, dtype, p_kind) only.  The p_kind = 0 instantiations are the code they were.
#include "nrm_device.h"
#include "nrm_host_entry.h"

#define BH_THREADS 256
#define BH_NW (BH_THREADS / 64)
#define BH_ITEMS 16
#define BH_TILE (BH_THREADS * BH_ITEMS)  // keys per workgroup of the sort and scan kernels: nrm_bh_tile()
#define BH_RADIX 256
static_assert(BH_RADIX == BH_THREADS, "a thread per digit");

template <typename T>
struct BhKey;
template <>
struct BhKey<float> {
	typedef uint32_t type;
};
template <>
struct BhKey<double> {
	typedef uint64_t type;
};
// the bit pattern of p + 0 (integer form: nothing here depends on a denormal mode)
__device__ __forceinline__ uint32_t bh_key(float p) {
	const uint32_t k = __float_as_uint(p);
	return k == 0x80000000u ? 0u : k;
}
__device__ __forceinline__ uint64_t bh_key(double p) {
	const uint64_t k = (uint64_t)__double_as_longlong(p);
	return k == 0x8000000000000000ull ? 0ull : k;
}
__device__ __forceinline__ float bh_value(uint32_t k) { return __uint_as_float(k); }
__device__ __forceinline__ double bh_value(uint64_t k) { return __longlong_as_double((long long)k); }

// The ln form (p_kind = 1): the complemented bit pattern of |ln P|.  Ascending key is ascending ln P, -inf (the exact zero of the linear form) comes first, both
// zeros (ln 1) share the largest key; whatever the input bits, the key is an unsigned integer like any other and the sort treats it as one.
__device__ __forceinline__ uint32_t bh_key_ln(float p) { return ~(__float_as_uint(p) & 0x7fffffffu); }
__device__ __forceinline__ uint64_t bh_key_ln(double p) { return ~((uint64_t)__double_as_longlong(p) & 0x7fffffffffffffffull); }
// ln P of a key of the ln form, in fp64: -|ln P|, and +0.0 for ln 1
__device__ __forceinline__ double bh_value_ln(uint32_t k) { return k == 0xffffffffu ? 0.0 : -(double)__uint_as_float(~k); }
__device__ __forceinline__ double bh_value_ln(uint64_t k) { return k == 0xffffffffffffffffull ? 0.0 : -__longlong_as_double((long long)~k); }
template <int PK, typename T>
__device__ __forceinline__ typename BhKey<T>::type bh_key_of(T p) {
	if constexpr (PK)
		return bh_key_ln(p);
	else
		return bh_key(p);
}

template <typename V>
__device__ __forceinline__ V bh_min(V a, V b) {
	return b < a ? b : a;
}

// entries i0 .. i0 + 3 of the flattened (rows, cols) matrix with pitch ld; 0 at and beyond n.  VEC: contiguous and 16-byte aligned
template <typename T, bool VEC>
__device__ __forceinline__ void bh_load4(const T* p, int64_t i0, int64_t n, int64_t cols, int64_t ld, T (&v)[4]) {
	if constexpr (VEC)
		nrm_ld4<T, true>(p, i0, n, v);
	else {
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int64_t i = i0 + j;
			v[j] = i < n ? p[(i / cols) * ld + i % cols] : (T)0;
		}
	}
}

// the thread's BH_ITEMS consecutive entries a[t0 ..] of an array of n (its start 32-byte aligned, t0 a multiple of BH_ITEMS); `fill` at and beyond n
template <typename V>
__device__ __forceinline__ void bh_load_items(const V* __restrict__ a, int64_t t0, int64_t n, V fill, V (&v)[BH_ITEMS]) {
	if (t0 + BH_ITEMS <= n) {
#pragma unroll
		for (int g = 0; g < BH_ITEMS / 4; g++) {
			V q[4];
			nrm_ld4<V, true>(a + t0 + 4 * g, q);
#pragma unroll
			for (int j = 0; j < 4; j++) v[4 * g + j] = q[j];
		}
	} else {
#pragma unroll
		for (int j = 0; j < BH_ITEMS; j++) v[j] = t0 + j < n ? a[t0 + j] : fill;
	}
}

// ---- a. keys ----------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC, int PK = 0>
__global__ void __launch_bounds__(BH_THREADS) k_bh_keys(const T* __restrict__ p, int64_t n, int64_t cols, int64_t ld, typename BhKey<T>::type* __restrict__ keys,
														 int32_t* __restrict__ flags) {
	__shared__ double sm[BH_NW];
	const int64_t i0 = ((int64_t)blockIdx.x * BH_THREADS + threadIdx.x) * 4;
	T v[4];
	bh_load4<T, VEC>(p, i0, n, cols, ld, v);
	double bad = 0.0;
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (i0 + j < n) {
			if constexpr (PK) {
				if (!(v[j] <= (T)0)) bad += 1.0;  // NaN or > 0: no ln P (-inf is one: ln 0); it still gets a key
			} else {
				if (!(v[j] >= (T)0 && v[j] <= (T)1)) bad += 1.0;  // NaN, infinite, < 0, > 1 (binnet.py:104); it still gets a key
			}
			keys[i0 + j] = bh_key_of<PK, T>(v[j]);
		}
	bad = nrm_block_sum<BH_NW, true>(bad, sm);
	if (threadIdx.x == 0 && bad > 0.0) atomicAdd(&flags[0], (int)bad);
}

// ---- b. the sort ------------------------------------------------------------------------------------------------------------------------------------------------
// table[digit * nb + workgroup]: the scan's order is the scatter's order (digit first, then workgroup)
template <typename K>
__global__ void __launch_bounds__(BH_THREADS) k_bh_hist(const K* __restrict__ keys, int64_t n, int shift, uint32_t* __restrict__ table, int64_t nb) {
	__shared__ unsigned h[BH_RADIX];
	h[threadIdx.x] = 0u;
	__syncthreads();
	const int64_t base = (int64_t)blockIdx.x * BH_TILE;
#pragma unroll
	for (int i = 0; i < BH_ITEMS; i++) {
		const int64_t j = base + i * BH_THREADS + threadIdx.x;
		if (j < n) atomicAdd(&h[(unsigned)(keys[j] >> shift) & (BH_RADIX - 1)], 1u);
	}
	__syncthreads();
	table[(int64_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// Exclusive prefix sums of a[0, len), len <= BH_TILE, in place and started at `carry`; the chunk's own total in every thread.  sm: BH_NW words.
__device__ __forceinline__ unsigned bh_chunk_scan(uint32_t* __restrict__ a, int64_t len, unsigned carry, unsigned* sm) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t t0 = (int64_t)threadIdx.x * BH_ITEMS;
	unsigned v[BH_ITEMS], sum = 0u;
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++) {
		v[j] = t0 + j < len ? a[t0 + j] : 0u;
		sum += v[j];
	}
	unsigned inc = sum;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const unsigned t = __shfl_up(inc, o, 64);
		if (lane >= o) inc += t;
	}
	__syncthreads();  // (sm may still be read from the chunk before)
	if (lane == 63) sm[wave] = inc;
	__syncthreads();
	unsigned before = carry, total = 0u;
#pragma unroll
	for (int w = 0; w < BH_NW; w++) {
		const unsigned s = sm[w];
		if (w < wave) before += s;
		total += s;
	}
	unsigned run = before + inc - sum;
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++) {
		if (t0 + j < len) a[t0 + j] = run;
		run += v[j];
	}
	return total;
}
// level 1 of a table of more than BH_TILE entries: the sum of every chunk of BH_TILE
__global__ void __launch_bounds__(BH_THREADS) k_bh_scan_reduce(const uint32_t* __restrict__ a, int64_t len, uint32_t* __restrict__ sums) {
	__shared__ unsigned sm[BH_NW];
	const int64_t c0 = (int64_t)blockIdx.x * BH_TILE;
	unsigned s = 0u;
#pragma unroll
	for (int i = 0; i < BH_ITEMS; i++) {
		const int64_t j = c0 + i * BH_THREADS + threadIdx.x;
		if (j < len) s += a[j];
	}
	s = nrm_wave_sum(s);
	if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned t = 0u;
#pragma unroll
		for (int w = 0; w < BH_NW; w++) t += sm[w];
		sums[blockIdx.x] = t;
	}
}
// ONE workgroup: exclusive sums of a[0, len) in place, chunk after chunk with the running total carried in a register (the whole table when it fits one chunk, the
// chunk sums of level 1 otherwise: 2^15 of them at 2^31 keys)
__global__ void __launch_bounds__(BH_THREADS) k_bh_scan_top(uint32_t* __restrict__ a, int64_t len) {
	__shared__ unsigned sm[BH_NW];
	unsigned carry = 0u;
	for (int64_t c0 = 0; c0 < len; c0 += BH_TILE) carry += bh_chunk_scan(a + c0, len - c0 < BH_TILE ? len - c0 : BH_TILE, carry, sm);
}
// level 2: every chunk scanned in place, started at its scanned sum
__global__ void __launch_bounds__(BH_THREADS) k_bh_scan_apply(uint32_t* __restrict__ a, int64_t len, const uint32_t* __restrict__ sums) {
	__shared__ unsigned sm[BH_NW];
	const int64_t c0 = (int64_t)blockIdx.x * BH_TILE;
	bh_chunk_scan(a + c0, len - c0 < BH_TILE ? len - c0 : BH_TILE, sums[blockIdx.x], sm);
}

// Stable scatter of a tile by the digit at `shift`.  Wave w owns positions [w * 64 * BH_ITEMS, (w + 1) * 64 * BH_ITEMS) of the tile, 64 consecutive ones per round: the
// lanes holding the same digit are found from ballots over the digit's 8 bits, a key's rank among the wave's keys of that digit is the per-wave LDS count so far plus
// the equal-digit lanes below it, and the group's lowest lane adds the group to the count.  A wave's LDS accesses are carried out in the order they are issued.
template <typename K>
__global__ void __launch_bounds__(BH_THREADS) k_bh_scatter(const K* __restrict__ src, K* __restrict__ dst, int64_t n, int shift, const uint32_t* __restrict__ table, int64_t nb) {
	__shared__ unsigned cnt[BH_NW][BH_RADIX];
	__shared__ unsigned first[BH_NW][BH_RADIX];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int w = 0; w < BH_NW; w++) cnt[w][threadIdx.x] = 0u;
	__syncthreads();
	const int64_t wbase = (int64_t)blockIdx.x * BH_TILE + (int64_t)wave * (64 * BH_ITEMS) + lane;
	K key[BH_ITEMS];
	unsigned rank[BH_ITEMS];
#pragma unroll
	for (int i = 0; i < BH_ITEMS; i++) key[i] = wbase + i * 64 < n ? src[wbase + i * 64] : (K)0;
	const uint64_t below = (1ull << lane) - 1ull;
	volatile unsigned* mine = cnt[wave];
#pragma unroll
	for (int i = 0; i < BH_ITEMS; i++) {
		const bool ok = wbase + i * 64 < n;
		const unsigned d = (unsigned)(key[i] >> shift) & (BH_RADIX - 1);
		uint64_t m = __ballot(ok);
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const bool bit = (d >> b) & 1u;
			const uint64_t bb = __ballot(ok && bit);
			m &= bit ? bb : ~bb;
		}
		unsigned pre = 0u;
		if (ok) pre = mine[d];
		__builtin_amdgcn_wave_barrier();
		if (ok && (m & below) == 0ull) mine[d] = pre + (unsigned)__popcll(m);
		__builtin_amdgcn_wave_barrier();
		rank[i] = pre + (unsigned)__popcll(m & below);
	}
	__syncthreads();
	{  // thread d: where the tile's keys of digit d start (the scanned table), then wave by wave
		unsigned run = table[(int64_t)threadIdx.x * nb + blockIdx.x];
#pragma unroll
		for (int w = 0; w < BH_NW; w++) {
			first[w][threadIdx.x] = run;
			run += cnt[w][threadIdx.x];
		}
	}
	__syncthreads();
#pragma unroll
	for (int i = 0; i < BH_ITEMS; i++) {
		if (wbase + i * 64 < n) {
			const unsigned d = (unsigned)(key[i] >> shift) & (BH_RADIX - 1);
			const int64_t pos = (int64_t)first[wave][d] + rank[i];
			if (pos < n) dst[pos] = key[i];  // (always, for a table counted from these keys)
		}
	}
}

// ---- c. q on the sorted keys ------------------------------------------------------------------------------------------------------------------------------------
// The workgroup's minimum of v in every thread; sm: BH_NW values.
template <typename V>
__device__ __forceinline__ V bh_block_min(V v, V* sm) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = bh_min(v, (V)__shfl_down(v, o, 64));
	__syncthreads();
	if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
	__syncthreads();
	V t = sm[0];
#pragma unroll
	for (int w = 1; w < BH_NW; w++) t = bh_min(t, sm[w]);
	return t;
}
// Thread t holds positions t * BH_ITEMS + j of the tile.  v <- the minimum over its own and all later positions of the tile and `carry` (the minimum of everything
// behind the tile); returns the tile's own minimum.  Minimum is exact: any association gives the same bits.
template <typename V>
__device__ __forceinline__ V bh_tile_suffix_min(V (&v)[BH_ITEMS], V carry, V inf, V* sm) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int j = BH_ITEMS - 2; j >= 0; j--) v[j] = bh_min(v[j], v[j + 1]);
	V inc = v[0];
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const V t = __shfl_down(inc, o, 64);
		if (lane + o < 64) inc = bh_min(inc, t);
	}
	V after = __shfl_down(inc, 1, 64);
	if (lane == 63) after = inf;
	__syncthreads();
	if (lane == 0) sm[wave] = inc;
	__syncthreads();
	V tot = inf;
#pragma unroll
	for (int w = 0; w < BH_NW; w++) {
		const V s = sm[w];
		if (w > wave) after = bh_min(after, s);
		tot = bh_min(tot, s);
	}
	after = bh_min(after, carry);
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++) v[j] = bh_min(v[j], after);
	return tot;
}

#define BH_NO_END 0xffffffffu
// e[j] = the position itself where the key differs from the next one (or is the last), BH_NO_END elsewhere
template <typename K>
__device__ __forceinline__ void bh_end_marks(const K* __restrict__ s, int64_t t0, int64_t n, K (&k)[BH_ITEMS], uint32_t (&e)[BH_ITEMS]) {
	bh_load_items<K>(s, t0, n, (K)0, k);
	const K next = t0 + BH_ITEMS < n ? s[t0 + BH_ITEMS] : (K)0;
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++) {
		const int64_t i = t0 + j;
		const K nx = j + 1 < BH_ITEMS ? k[j + 1 < BH_ITEMS ? j + 1 : j] : next;
		e[j] = i < n && (i == n - 1 || nx != k[j]) ? (uint32_t)i : BH_NO_END;
	}
}
// the first position of every tile at which a tie group ends
template <typename K>
__global__ void __launch_bounds__(BH_THREADS) k_bh_ends(const K* __restrict__ s, int64_t n, uint32_t* __restrict__ tile_end) {
	__shared__ uint32_t sm[BH_NW];
	K k[BH_ITEMS];
	uint32_t e[BH_ITEMS];
	bh_end_marks<K>(s, (int64_t)blockIdx.x * BH_TILE + (int64_t)threadIdx.x * BH_ITEMS, n, k, e);
	uint32_t m = BH_NO_END;
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++) m = bh_min(m, e[j]);
	m = bh_block_min<uint32_t>(m, sm);
	if (threadIdx.x == 0) tile_end[blockIdx.x] = m;
}
// ONE workgroup: out[b] = min over b' > b of a[b'] (inf for the last), walked backwards chunk by chunk with the minimum so far carried in a register
template <typename V>
__global__ void __launch_bounds__(BH_THREADS) k_bh_suffix_top(const V* __restrict__ a, int64_t len, V inf, V* __restrict__ out) {
	__shared__ V sm[BH_NW];
	V carry = inf;
	for (int64_t c0 = (len - 1) / BH_TILE * BH_TILE; c0 >= 0; c0 -= BH_TILE) {
		const int64_t t0 = c0 + (int64_t)threadIdx.x * BH_ITEMS;
		V v[BH_ITEMS];
#pragma unroll
		for (int j = 0; j < BH_ITEMS; j++) v[j] = t0 + j + 1 < len ? a[t0 + j + 1] : inf;  // the array shifted by one: an inclusive minimum of it is the exclusive one
		const V tot = bh_tile_suffix_min<V>(v, carry, inf, sm);
#pragma unroll
		for (int j = 0; j < BH_ITEMS; j++)
			if (t0 + j < len) out[t0 + j] = v[j];
		carry = bh_min(carry, tot);
	}
}
// c and q before the suffix minimum for every sorted position, the tile's smallest q, and d_flags[1]
// (PK = 1: ln q = min(0, u + (ln N - ln c)) in fp64 for both dtypes, rounded once at the store; c = N leaves u itself; -inf stays -inf)
template <typename T, int PK = 0>
__global__ void __launch_bounds__(BH_THREADS) k_bh_q(const typename BhKey<T>::type* __restrict__ s, int64_t n, const uint32_t* __restrict__ end_after,
													  uint32_t* __restrict__ cnt, T* __restrict__ q, T* __restrict__ tile_q, int32_t* __restrict__ flags) {
	typedef typename BhKey<T>::type K;
	__shared__ uint32_t sme[BH_NW];
	__shared__ T smq[BH_NW];
	const int64_t t0 = (int64_t)blockIdx.x * BH_TILE + (int64_t)threadIdx.x * BH_ITEMS;
	K k[BH_ITEMS];
	uint32_t e[BH_ITEMS];
	bh_end_marks<K>(s, t0, n, k, e);
	bh_tile_suffix_min<uint32_t>(e, end_after[blockIdx.x], BH_NO_END, sme);  // e[j]: the last position holding the key of position t0 + j
	const double dn = (double)n;
	double ln_n = 0.0;
	if constexpr (PK) ln_n = log(dn);
	T qmin = (T)2;
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++) {
		if (t0 + j < n) {
			const uint32_t c = e[j] + 1u;
			T qv;
			if constexpr (PK) {
				const double lq = bh_value_ln(k[j]) + (ln_n - log((double)c));
				qv = lq < 0.0 ? (T)lq : (T)0;  // (a NaN -- only from entries that are counted as invalid -- becomes 0 as well)
			} else {
				double w = (double)c / dn;
				if (sizeof(T) == 4) w = (double)(float)w;
				qv = (T)((double)bh_value(k[j]) / w);
				if (!isfinite((double)qv)) qv = (T)1;
				qv = qv > (T)1 ? (T)1 : (qv < (T)0 ? (T)0 : qv);
			}
			cnt[t0 + j] = c;
			q[t0 + j] = qv;
			qmin = bh_min(qmin, qv);
		}
	}
	qmin = bh_block_min<T>(qmin, smq);
	if (threadIdx.x == 0) {
		tile_q[blockIdx.x] = qmin;
		if (blockIdx.x == 0) flags[1] = s[0] != s[n - 1] ? 1 : 0;
	}
}
template <typename T>
__global__ void __launch_bounds__(BH_THREADS) k_bh_q_apply(T* __restrict__ q, int64_t n, const T* __restrict__ q_after) {
	__shared__ T sm[BH_NW];
	const int64_t t0 = (int64_t)blockIdx.x * BH_TILE + (int64_t)threadIdx.x * BH_ITEMS;
	T v[BH_ITEMS];
	bh_load_items<T>(q, t0, n, (T)2, v);
	bh_tile_suffix_min<T>(v, q_after[blockIdx.x], (T)2, sm);
#pragma unroll
	for (int j = 0; j < BH_ITEMS; j++)
		if (t0 + j < n) q[t0 + j] = v[j];
}

// ---- d. look-up -------------------------------------------------------------------------------------------------------------------------------------------------
// A plain lower-bound search over the sorted keys is bound by the cache lines its deep probes pull in (24 probes, the last dozen each in a line of its own:
// 2.81 of the call's 4.20 ms at 1.5e7 fp64 entries; with a thread's four searches advancing in step, four loads in flight, 3.04 ms: not latency;
// profiles/bh_lookup_variants.txt).  So the search runs on sampled levels (1.37 ms): level 0 is the sorted keys, level k + 1 holds the last key of every complete group of F = 128 bytes of keys of level k, up to a level
// of at most F keys.  From the top, the number of keys below the wanted one in a group names the group of the level beneath: one cache line per level, and all
// levels but the lowest two stay in L2.
#define BH_MAX_LEVELS 8  // F^8 > 2^31 for F = 16 (fp64) and F = 32 (fp32)
template <typename K>
struct BhLevels {
	const K* a[BH_MAX_LEVELS];
	int64_t n[BH_MAX_LEVELS];
	int count;
};
template <typename K>
__global__ void __launch_bounds__(BH_THREADS) k_bh_sample(const K* __restrict__ src, K* __restrict__ dst, int64_t n_dst) {
	constexpr int F = 128 / sizeof(K);
	const int64_t i = (int64_t)blockIdx.x * BH_THREADS + threadIdx.x;
	if (i < n_dst) dst[i] = src[(i + 1) * F - 1];  // (n_dst = n_src / F: inside src)
}
// (p and out may be the same matrix: a thread reads its four entries before it writes them)
template <typename T, bool VEC, int PK = 0>
__global__ void __launch_bounds__(BH_THREADS) k_bh_lookup(const T* p, int64_t n, int64_t cols, int64_t ldp, const BhLevels<typename BhKey<T>::type> lv,
														   const T* __restrict__ q, T* out, int64_t ldq) {
	typedef typename BhKey<T>::type K;
	constexpr int F = 128 / sizeof(K);
	const int64_t i0 = ((int64_t)blockIdx.x * BH_THREADS + threadIdx.x) * 4;
	T v[4], r[4];
	bh_load4<T, VEC>(p, i0, n, cols, ldp, v);
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const K key = bh_key_of<PK, T>(v[j]);
		int64_t g = 0;  // the group of the level at hand: keys [g F, g F + F) of it, cut at its end (the top level is one group)
		for (int k = lv.count - 1; k >= 0; k--) {
			int64_t lo = g * F, hi = lo + F < lv.n[k] ? lo + F : lv.n[k];  // g <= n[k + 1] = n[k] / F: lo <= n[k], every probe inside [0, n[k])
			const K* __restrict__ a = lv.a[k];
			while (lo < hi) {
				const int64_t mid = (lo + hi) >> 1;
				if (a[mid] < key)
					lo = mid + 1;
				else
					hi = mid;
			}
			g = lo;  // the first key of the level not below the wanted one (the level's size when there is none: then the answer lies in the ragged tail beneath)
		}
		r[j] = q[g < n ? g : n - 1];  // (the key is among the sorted ones: g < n for every entry; the clamp is for the lanes beyond the matrix)
	}
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int64_t i = i0 + j;
		if (i < n) out[(i / cols) * ldq + i % cols] = r[j];
	}
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------
struct BhLayout {
	int64_t nb, tab, chunks;                                                 // tiles, entries of the (digit, tile) table, chunks of that table
	int64_t keys, other, q, table, sums, tile_end, end_after, tile_q, q_after, total;  // byte offsets into the workspace
	int64_t level_n[BH_MAX_LEVELS], level_at[BH_MAX_LEVELS];                            // keys and byte offset of every sampled level
	int levels;
};
static inline int64_t bh_up(int64_t v) { return (v + 255) / 256 * 256; }
static void bh_layout(int64_t n, int dtype, BhLayout& L) {
	const int64_t ksz = dtype == NRM_F64 ? 8 : 4;
	L.nb = (n + BH_TILE - 1) / BH_TILE;
	L.tab = L.nb * BH_RADIX;
	L.chunks = (L.tab + BH_TILE - 1) / BH_TILE;
	int64_t o = 0;
	L.keys = o, o += bh_up(n * ksz);       // the sorted keys after the last pass (an even number of passes)
	L.other = o, o += bh_up(n * ksz);      // the sort's other side; c (uint32) once the keys are sorted
	L.q = o, o += bh_up(n * ksz);
	L.table = o, o += bh_up(L.tab * 4);
	L.sums = o, o += bh_up(L.chunks * 4);
	L.tile_end = o, o += bh_up(L.nb * 4);
	L.end_after = o, o += bh_up(L.nb * 4);
	L.tile_q = o, o += bh_up(L.nb * ksz);
	L.q_after = o, o += bh_up(L.nb * ksz);
	const int64_t f = 128 / ksz;  // the look-up's sampled levels: level 0 is the sorted keys themselves, the top level has at most f keys
	L.levels = 1, L.level_n[0] = n, L.level_at[0] = L.keys;
	while (L.level_n[L.levels - 1] > f) {
		L.level_n[L.levels] = L.level_n[L.levels - 1] / f;
		L.level_at[L.levels] = o, o += bh_up(L.level_n[L.levels] * ksz);
		L.levels++;
	}
	L.total = o;
}
static int bh_size_check(int64_t n, int p_dtype) {
	NRM_REQUIRE(p_dtype == NRM_F32 || p_dtype == NRM_F64, "nrm_bh: bad dtype");
	NRM_REQUIRE(n > 0, "nrm_bh: no P-values (binnet.py:103)");
	if (n > 0x7fffffffLL) {
		nrm_set_error("nrm_bh: at most 2^31 - 1 P-values");
		return NRM_E_UNSUPPORTED;
	}
	return NRM_OK;
}

extern "C" int64_t nrm_bh_tile(void) { return BH_TILE; }

extern "C" int64_t nrm_bh_workspace_bytes(int64_t n, int p_dtype) {
	const int rc = bh_size_check(n, p_dtype);
	if (rc) return rc;
	BhLayout L;
	bh_layout(n, p_dtype, L);
	return L.total;
}

extern "C" int nrm_bh_layout(int64_t n, int p_dtype, int64_t offsets[4]) {
	NRM_TRY(bh_size_check(n, p_dtype));
	NRM_REQUIRE(offsets != nullptr, "nrm_bh_layout: null pointer");
	BhLayout L;
	bh_layout(n, p_dtype, L);
	offsets[0] = L.keys, offsets[1] = L.other, offsets[2] = L.q, offsets[3] = 0;
	return NRM_OK;
}

template <typename T, int PK>
static int bh_run(const T* p, int64_t n, int64_t cols, int64_t ldp, T* out, int64_t ldq, char* work, const BhLayout& L, int32_t* flags, hipStream_t st) {
	typedef typename BhKey<T>::type K;
	K *a = (K*)(work + L.keys), *b = (K*)(work + L.other);
	T *q = (T*)(work + L.q), *tile_q = (T*)(work + L.tile_q), *q_after = (T*)(work + L.q_after);
	uint32_t *table = (uint32_t*)(work + L.table), *sums = (uint32_t*)(work + L.sums), *tile_end = (uint32_t*)(work + L.tile_end), *end_after = (uint32_t*)(work + L.end_after);
	const dim3 wg(BH_THREADS), tiles((unsigned)L.nb), quads((unsigned)((n + 4 * BH_THREADS - 1) / (4 * BH_THREADS)));
	const bool vec_in = (ldp == cols || n == cols) && (uintptr_t)p % 16 == 0;  // the flattened input is one contiguous, 16-byte aligned run
	if (vec_in)
		hipLaunchKernelGGL((k_bh_keys<T, true, PK>), quads, wg, 0, st, p, n, cols, ldp, a, flags);
	else
		hipLaunchKernelGGL((k_bh_keys<T, false, PK>), quads, wg, 0, st, p, n, cols, ldp, a, flags);
	for (int pass = 0; pass < (int)sizeof(K); pass++) {
		const int shift = 8 * pass;
		hipLaunchKernelGGL((k_bh_hist<K>), tiles, wg, 0, st, (const K*)a, n, shift, table, L.nb);
		if (L.chunks == 1)
			hipLaunchKernelGGL(k_bh_scan_top, dim3(1), wg, 0, st, table, L.tab);
		else {
			hipLaunchKernelGGL(k_bh_scan_reduce, dim3((unsigned)L.chunks), wg, 0, st, (const uint32_t*)table, L.tab, sums);
			hipLaunchKernelGGL(k_bh_scan_top, dim3(1), wg, 0, st, sums, L.chunks);
			hipLaunchKernelGGL(k_bh_scan_apply, dim3((unsigned)L.chunks), wg, 0, st, table, L.tab, (const uint32_t*)sums);
		}
		hipLaunchKernelGGL((k_bh_scatter<K>), tiles, wg, 0, st, (const K*)a, b, n, shift, (const uint32_t*)table, L.nb);
		K* t = a;
		a = b, b = t;
	}
	// (an even number of passes: a is the workspace's first buffer again, b is free for c)
	hipLaunchKernelGGL((k_bh_ends<K>), tiles, wg, 0, st, (const K*)a, n, tile_end);
	hipLaunchKernelGGL((k_bh_suffix_top<uint32_t>), dim3(1), wg, 0, st, (const uint32_t*)tile_end, L.nb, BH_NO_END, end_after);
	hipLaunchKernelGGL((k_bh_q<T, PK>), tiles, wg, 0, st, (const K*)a, n, (const uint32_t*)end_after, (uint32_t*)b, q, tile_q, flags);
	hipLaunchKernelGGL((k_bh_suffix_top<T>), dim3(1), wg, 0, st, (const T*)tile_q, L.nb, (T)2, q_after);
	hipLaunchKernelGGL((k_bh_q_apply<T>), tiles, wg, 0, st, q, n, (const T*)q_after);
	BhLevels<K> lv;
	lv.count = L.levels;
	for (int k = 0; k < BH_MAX_LEVELS; k++) {
		lv.a[k] = k < L.levels ? (const K*)(work + L.level_at[k]) : nullptr;
		lv.n[k] = k < L.levels ? L.level_n[k] : 0;
		if (k > 0 && k < L.levels)
			hipLaunchKernelGGL((k_bh_sample<K>), dim3((unsigned)((lv.n[k] + BH_THREADS - 1) / BH_THREADS)), wg, 0, st, lv.a[k - 1], (K*)(work + L.level_at[k]), lv.n[k]);
	}
	if (vec_in)
		hipLaunchKernelGGL((k_bh_lookup<T, true, PK>), quads, wg, 0, st, p, n, cols, ldp, lv, (const T*)q, out, ldq);
	else
		hipLaunchKernelGGL((k_bh_lookup<T, false, PK>), quads, wg, 0, st, p, n, cols, ldp, lv, (const T*)q, out, ldq);
	return nrm_check_launch("nrm_bh");
}

extern "C" int nrm_bh_pk(const void* d_p, int p_dtype, int64_t rows, int64_t cols, int64_t ldp, void* d_q, int64_t ldq, void* d_work, int64_t work_bytes, int32_t* d_flags,
						 int p_kind, void* stream) {
	NRM_REQUIRE(p_kind == 0 || p_kind == 1, "nrm_bh: p_kind is 0 (P) or 1 (ln P)");
	NRM_REQUIRE(rows >= 0 && cols >= 0 && rows <= 0x7fffffffLL && cols <= 0x7fffffffLL, "nrm_bh: bad shape");
	const int64_t n = rows * cols;
	NRM_TRY(bh_size_check(n, p_dtype));
	NRM_REQUIRE(ldp >= cols && ldq >= cols, "nrm_bh: a pitch below the row length");
	NRM_REQUIRE(d_p && d_q && d_work && d_flags, "nrm_bh: null pointer");
	NRM_REQUIRE(d_q != d_p || ldq == ldp, "nrm_bh: in place needs equal pitches");
	const size_t esz = nrm_esize(p_dtype);
	NRM_REQUIRE((uintptr_t)d_p % esz == 0 && (uintptr_t)d_q % esz == 0 && (uintptr_t)d_work % 256 == 0, "nrm_bh: misaligned pointer (the workspace: 256 bytes)");
	BhLayout L;
	bh_layout(n, p_dtype, L);
	NRM_REQUIRE(work_bytes >= L.total, "nrm_bh: the workspace holds %lld bytes, nrm_bh_workspace_bytes asks for %lld", (long long)work_bytes, (long long)L.total);
	hipStream_t st = (hipStream_t)stream;
	NRM_HIP(hipMemsetAsync(d_flags, 0, 2 * sizeof(int32_t), st));
	if (p_kind) {
		if (p_dtype == NRM_F64) return bh_run<double, 1>((const double*)d_p, n, cols, ldp, (double*)d_q, ldq, (char*)d_work, L, d_flags, st);
		return bh_run<float, 1>((const float*)d_p, n, cols, ldp, (float*)d_q, ldq, (char*)d_work, L, d_flags, st);
	}
	if (p_dtype == NRM_F64) return bh_run<double, 0>((const double*)d_p, n, cols, ldp, (double*)d_q, ldq, (char*)d_work, L, d_flags, st);
	return bh_run<float, 0>((const float*)d_p, n, cols, ldp, (float*)d_q, ldq, (char*)d_work, L, d_flags, st);
}

extern "C" int nrm_bh(const void* d_p, int p_dtype, int64_t rows, int64_t cols, int64_t ldp, void* d_q, int64_t ldq, void* d_work, int64_t work_bytes, int32_t* d_flags,
					  void* stream) {
	return nrm_bh_pk(d_p, p_dtype, rows, cols, ldp, d_q, ldq, d_work, work_bytes, d_flags, 0, stream);
}

extern "C" int nrm_bh_host_pk(const void* h_p, int p_dtype, int64_t n, void* h_q, int32_t* identical, int p_kind) {
	std::lock_guard<std::mutex> serial(nrm_host_entry_mutex());
	NRM_TRY(nrm_bind_device());
	NRM_REQUIRE(h_p && h_q && identical, "nrm_bh_host: null pointer");
	NRM_REQUIRE(p_kind == 0 || p_kind == 1, "nrm_bh_host: p_kind is 0 (P) or 1 (ln P)");
	NRM_TRY(bh_size_check(n, p_dtype));
	hipStream_t st = nullptr;
	DevBuf dp, work, flags;
	NRM_TRY(upload_matrix(h_p, p_dtype, 1, n, dp, st));
	BhLayout L;
	bh_layout(n, p_dtype, L);
	NRM_TRY(work.alloc((size_t)L.total));
	NRM_TRY(flags.alloc(16));
	NRM_TRY(nrm_bh_pk(dp.p, p_dtype, 1, n, n, dp.p, n, work.p, L.total, flags.as<int32_t>(), p_kind, st));
	int32_t hf[2];
	NRM_TRY(nrm_read_flags(flags.p, st, hf));
	if (hf[0]) {
		if (p_kind)
			nrm_set_error("ln P-values must be <= 0 and no NaN: %d entries are not", hf[0]);
		else
			nrm_set_error("P-values must be finite and within [0, 1] (binnet.py:104): %d entries are not", hf[0]);
		return NRM_E_NUMERIC;
	}
	*identical = hf[1] ? 0 : 1;
	return copy_out(h_q, dp.p, (size_t)n * nrm_esize(p_dtype));
}

extern "C" int nrm_bh_host(const void* h_p, int p_dtype, int64_t n, void* h_q, int32_t* identical) { return nrm_bh_host_pk(h_p, p_dtype, n, h_q, identical, 0); }
