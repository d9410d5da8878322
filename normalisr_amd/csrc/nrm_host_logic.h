// Host-side logic of the library that needs no GPU: the tile order and persistent schedule of the Gram kernels (whole tiles ->
// K-aligned parts -> stream-K units), the device scratch pool of the whole-problem entry, the P-value plan.  Kept free of HIP
// headers so that g++ can build it with -fsanitize=address,undefined for the CPU test-suite (tests/host_sanitize.cpp); the same
// functions are compiled for the device where the kernels need them (NRM_HD).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>
#include "../../include/normalisr_hip.h"

#if defined(__HIPCC__)
#define NRM_HD __host__ __device__
#else
#define NRM_HD
#endif

void nrm_set_error(const char* fmt, ...);
#ifndef NRM_REQUIRE
#define NRM_REQUIRE(cond, ...)      \
	do {                            \
		if (!(cond)) {              \
			nrm_set_error(__VA_ARGS__); \
			return NRM_E_ARG;       \
		}                           \
	} while (0)
#endif

NRM_HD inline int nrm_imin(int a, int b) { return a < b ? a : b; }

// the checks of association.py:199-216 on a dense single=0 call, in the reference's words (the whole-problem entry and the resident plans, before any device call)
static inline int nrm_assoc_check_args(const void* dx, int64_t nx, int64_t ny, const void* h_dc, int64_t nc, int64_t n, int rank, int dimreduce) {
	NRM_REQUIRE(dx && nx > 0 && ny > 0 && n > 0, "Incorrect dx/dy/dc size.");
	NRM_REQUIRE(nc >= 0 && (nc == 0 || h_dc), "Incorrect dx/dy/dc size.");
	NRM_REQUIRE(rank >= 0, "Negative dcr detected.");
	NRM_REQUIRE(rank <= nc, "dcr higher than covariate dimension.");
	NRM_REQUIRE(n > (int64_t)rank + dimreduce + 1, "Insufficient number of cells: must be greater than degrees of freedom removed + covariate + 1.");
	return NRM_OK;
}
// words 0 and 1 of an entry's result counters as the reference's error; `unit`: what the kernel counted (" tiles" for the tiled sweeps, "" for plain results)
static inline int nrm_assoc_assertions(const int32_t* hf, const char* unit) {
	if (hf[0] || hf[1]) {
		nrm_set_error("association results failed the reference's assertions (association.py:248,252): %d%s non-finite, %d%s with R^2 > 1+1e-8", hf[0], unit, hf[1], unit);
		return NRM_E_NUMERIC;
	}
	return NRM_OK;
}

// ---- K1 routing (csrc/nrm_residualize.hip, launch_residualize) -------------------------------------------------------------------------------------------------
// vec: the 16-byte row loads of k_residualize_v4 / _v8 apply (aligned pointers and pitches; otherwise the scalar k_residualize runs).
static inline bool nrm_k1_vec(uint64_t x_addr, int64_t x_elem_bytes, int64_t ldx, bool has_out, uint64_t out_addr, int64_t ldo, int active, uint64_t c_addr,
							  int64_t ldc) {
	const int64_t xa = 16 / x_elem_bytes;
	return (ldx % xa == 0) && (x_addr % 16 == 0) && (!has_out || ((ldo % 4 == 0) && (out_addr % 16 == 0))) && (!active || (ldc % 2 == 0 && c_addr % 16 == 0));
}
// stream_rows: input rows loaded non-temporally -- fp32 rows against at least 8 MB of covariates, which then stay in L2
static inline bool nrm_k1_stream_rows(int active, int64_t x_elem_bytes, int64_t nc, int64_t n) { return active && x_elem_bytes == 4 && nc * n * 8 >= (8 << 20); }
// rows8: k_residualize_v8, eight rows per workgroup with the covariate slices staged in LDS, CAN run
static inline bool nrm_k1_rows8(bool vec, int active, int64_t nc, int64_t rows_pad, bool stream_rows) {
	return vec && active && nc <= 8 && rows_pad % 8 == 0 && !stream_rows;
}
// ... and pays: rows of at least 16 384 cells.  Measured, alternating with k_residualize_v4 in one process (profiles/k1_rows8_ab.txt, k1_rows8_cross.txt), fp32 rows
// with 3 covariates: 5000 x 10 000 0.180 -> 0.213 ms (625 workgroups, one per CU, are 2.4 rounds of 256 with nothing to fill the last, where the old kernel's
// 1250 half-size ones pack it), x 16 384 0.322 -> 0.324, x 24 576 0.487 -> 0.444, x 32 768 0.641 -> 0.611; 16 000 x 50 000 with 5: 3.27 -> 3.08; the
// 3840 x 500 000 fp64 slice: 9.83 -> 8.22.  NRM_DEBUG="k1_rows8=1" runs it wherever it can (the tests' small shapes), "k1_rows8=0" nowhere.
static inline bool nrm_k1_rows8_pays(int64_t n) { return n >= 16384; }

#define GM 128
#define GN 128

// Tile order: the tile grid is cut into 8x8 super-blocks that are visited one after another (row-major
// inside a super-block).  64 consecutive tiles -- what the 64 co-resident workgroups of one XCD process at
// the same time -- therefore touch 8 A panels and 8 B panels instead of 1 + 64, and those slabs are shared
// through the XCD's L2 while the workgroups advance through K in lockstep.  Symmetric launches keep only
// super-blocks and tiles on or above the diagonal (association.py:893-894).
#define GSB 8
NRM_HD inline __attribute__((always_inline)) void gram_tile_coords(int t, int symmetric, int ntm, int ntn, int& ti, int& tj) {
	const int nbm = (ntm + GSB - 1) / GSB, nbn = (ntn + GSB - 1) / GSB;
	for (int bi = 0; bi < nbm; bi++) {
		const int h = nrm_imin(GSB, ntm - bi * GSB);
		for (int bj = symmetric ? bi : 0; bj < nbn; bj++) {
			const int w = nrm_imin(GSB, ntn - bj * GSB);
			const bool diag = symmetric && bi == bj;
			const int cnt = diag ? h * (h + 1) / 2 : h * w;
			if (t < cnt) {
				int li, lj;
				if (!diag) {
					li = t / w;
					lj = t - li * w;
				} else {
					li = 0;
					int len = h;
					while (t >= len) {
						t -= len;
						li++;
						len--;
					}
					lj = li + t;
				}
				ti = bi * GSB + li;
				tj = bj * GSB + lj;
				return;
			}
			t -= cnt;
		}
	}
	ti = 0;
	tj = 0;
}

struct GramSched {
	int m_rows, n_rows;  // valid (unpadded) rows of A and B
	int ntm, ntn;   // tile grid (M, N)
	int nkt;        // k-tiles (slabs of GK cells)
	int tiles_dp;   // tiles processed whole, one per workgroup per wave
	int tiles_al;   // tiles cut into `parts` equal K ranges, one range per workgroup (K-aligned: slabs still shared in L2)
	int parts;
	int tiles_sk;   // tiles of the tail, cut into unit ranges
	int units_per_wg;
	int nwg;        // persistent workgroups (multiple of 8)
	int tile0;      // first tile of this launch in the gram_tile_coords order (band launches)
	int accumulate; // add to C instead of overwriting it (cell-chunked launches of the sharded path)
	int fold;       // ntn - 1: the ragged last tile column, this one, rides in the diagonal tiles (gram_plan_fold; integer engine only); 0 for everyone else
	double* work;   // slabs of partial pieces: [tiles_al*parts] then [2 per workgroup]
};

// Tile t of a launch.  fold == 0: the gram_tile_coords order.  fold == ntn - 1 > 0 (symmetric, whole matrix, at most 32 valid columns in the last
// tile column): the upper triangle of the leading (ntn - 1) x (ntn - 1) grid in that order, then the corner tile (ntn - 1, ntn - 1).  The
// off-diagonal tiles (i, ntn - 1) are not listed: diagonal tile (i, i), i < ntn - 1, is the HOST of edge tile (i, ntn - 1) -- its two waves
// below the diagonal compute the edge tile's 128 rows x one 32-column block (gram_piece_i8).
NRM_HD inline __attribute__((always_inline)) void gram_sched_coords(const GramSched& s, int t, int symmetric, int& ti, int& tj) {
	if (!s.fold) {
		gram_tile_coords(s.tile0 + t, symmetric, s.ntm, s.ntn, ti, tj);
		return;
	}
	const int lead = s.fold;
	if (t < lead * (lead + 1) / 2)
		gram_tile_coords(t, 1, lead, lead, ti, tj);
	else
		ti = tj = lead;
}
// true: tile (ti, tj) of a folded launch also carries edge tile (ti, ntn - 1)
NRM_HD inline bool gram_is_host(const GramSched& s, int ti, int tj) { return ti == tj && ti < s.fold; }

// The persistent loop of a Gram kernel: calls piece(tile, k0, k1, slab) for every piece of workgroup `block` -- whole tiles
// first (one per workgroup per wave, K-lockstep), then its K-aligned part, then its share of the stream-K tail.
template <typename F>
NRM_HD inline __attribute__((always_inline)) void gram_pieces_of(const GramSched& s, int block, F piece) {
	// workgroups that share an XCD (same block index % 8) take consecutive tiles so that operand panels are shared in its L2
	const int per_xcd = s.nwg >> 3;
	const int p = (block & 7) * per_xcd + (block >> 3);
	int t_dp = p;
	bool al_todo = p < s.tiles_al * s.parts;
	int64_t u = (int64_t)p * s.units_per_wg;
	const int64_t total = (int64_t)s.tiles_sk * s.nkt;
	int64_t uend = u + s.units_per_wg;
	if (uend > total) uend = total;
	int sk_piece = 0;
	for (;;) {
		int t, k0, k1;
		double* slab = nullptr;
		if (t_dp < s.tiles_dp) {
			t = t_dp;
			k0 = 0;
			k1 = s.nkt;
			t_dp += s.nwg;
		} else if (al_todo) {
			al_todo = false;
			const int ta = p / s.parts, part = p - ta * s.parts;
			t = s.tiles_dp + ta;
			k0 = (int)((int64_t)s.nkt * part / s.parts);
			k1 = (int)((int64_t)s.nkt * (part + 1) / s.parts);
			slab = s.work + (int64_t)p * (GM * GN);
		} else if (u < uend) {
			const int ts = (int)(u / s.nkt);
			k0 = (int)(u - (int64_t)ts * s.nkt);
			int64_t k1l = k0 + (uend - u);
			k1 = k1l > s.nkt ? s.nkt : (int)k1l;
			t = s.tiles_dp + s.tiles_al + ts;
			u += k1 - k0;
			if (!(k0 == 0 && k1 == s.nkt)) slab = s.work + ((int64_t)s.tiles_al * s.parts + 2 * p + sk_piece) * (GM * GN);
			sk_piece++;
		} else {
			break;
		}
		piece(t, k0, k1, slab);
	}
}

// Doubles of scratch a launch on nwg persistent workgroups can touch: at most nwg slabs of K-aligned parts (tiles_al * parts <= nwg)
// plus two stream-K slabs per workgroup.
static inline int64_t nrm_host_gram_workspace_doubles(int nwg) { return (int64_t)3 * nwg * GM * GN; }

// Tiles that precede super-block row `bi` in the gram_tile_coords order.
static inline int64_t gram_tiles_before(int64_t bi, int symmetric, int64_t ntm, int64_t ntn) {
	const int64_t nbn = (ntn + GSB - 1) / GSB;
	int64_t t = 0;
	for (int64_t b = 0; b < bi; b++) {
		const int64_t h = std::min<int64_t>(GSB, ntm - b * GSB);
		for (int64_t bj = symmetric ? b : 0; bj < nbn; bj++) {
			const int64_t w = std::min<int64_t>(GSB, ntn - bj * GSB);
			t += (symmetric && b == bj) ? h * (h + 1) / 2 : h * w;
		}
	}
	return t;
}

// The three phases of `tiles` tiles on s.nwg workgroups (s.nkt, s.nwg set), every workgroup does the same amount of work in each:
//  1. whole tiles, one per workgroup per wave (K-lockstep, plain stores);
//  2. of the remaining rem < nwg tiles, nwg/parts tiles are cut into `parts` equal K ranges (still K-aligned within a
//     part, so workgroups of an XCD keep sharing slabs through L2);
//  3. the rest is cut into equal unit ranges (stream-K; different K offsets, no sharing -- kept small).
static inline void gram_split_phases(GramSched& s, int64_t tiles) {
	const int64_t waves = tiles / s.nwg, rem = tiles - waves * s.nwg;
	s.tiles_dp = (int)(waves * s.nwg);
	s.parts = 1;
	s.tiles_al = 0;
	for (int parts = 2; parts <= 8 && s.nkt >= 8 * parts; parts *= 2)
		if (rem >= s.nwg / parts) {
			s.parts = parts;
			s.tiles_al = s.nwg / parts;
			break;
		}
	const int64_t sk = rem - s.tiles_al;
	s.tiles_sk = (int)sk;
	s.units_per_wg = (int)((sk * s.nkt + s.nwg - 1) / s.nwg);
}

// Host side: the schedule of one launch over output rows [row0, row1) with nkt K-units per tile on nwg persistent workgroups.
static inline int gram_plan(GramSched& s, int64_t m_pad, int64_t n_pad, int64_t nkt, int symmetric, int64_t m_rows, int64_t n_rows, int64_t row0,
							int64_t row1, int nwg, double* work) {
	const int64_t ntm = m_pad / GM, ntn = n_pad / GN;
	NRM_REQUIRE((symmetric ? ntn * (ntn + 1) / 2 : ntm * ntn) < (1LL << 30), "nrm_gram: problem too large for one launch");
	const int64_t tile0 = gram_tiles_before(row0 / (GSB * GM), symmetric, ntm, ntn);
	const int64_t tiles = gram_tiles_before((row1 + GSB * GM - 1) / (GSB * GM), symmetric, ntm, ntn) - tile0;
	NRM_REQUIRE(tiles < (1LL << 30) && nkt < (1LL << 30), "nrm_gram: problem too large for one launch");
	s.tile0 = (int)tile0;
	s.accumulate = 0;
	s.fold = 0;
	s.m_rows = (int)((m_rows > 0 && m_rows < m_pad) ? m_rows : m_pad);
	s.n_rows = (int)((n_rows > 0 && n_rows < n_pad) ? n_rows : n_pad);
	s.ntm = (int)ntm;
	s.ntn = (int)ntn;
	s.nkt = (int)nkt;
	s.nwg = nwg - nwg % 8;
	gram_split_phases(s, tiles);
	s.work = work;
	return NRM_OK;
}

// The same with the ragged last tile column folded into the diagonal tiles where that applies: a symmetric launch over the whole matrix
// with at least two tile columns whose last one holds 1 to 32 valid columns (5000 genes = 39 x 128 + 8: 781 tiles instead of 820).  The
// caller vouches for the rest (dense B, not accumulating, a kernel that knows host tiles).  Every other launch gets gram_plan's schedule.
static inline int gram_plan_fold(GramSched& s, int64_t m_pad, int64_t n_pad, int64_t nkt, int symmetric, int64_t m_rows, int64_t n_rows, int64_t row0,
								 int64_t row1, int nwg, double* work) {
	const int rc = gram_plan(s, m_pad, n_pad, nkt, symmetric, m_rows, n_rows, row0, row1, nwg, work);
	if (rc != NRM_OK) return rc;
	const int valid = s.n_rows - (s.ntn - 1) * GN;  // valid columns of the last tile column
	if (symmetric && row0 == 0 && row1 == m_pad && s.ntn >= 2 && s.ntm == s.ntn && s.m_rows == s.n_rows && valid >= 1 && valid <= 32) {
		s.fold = s.ntn - 1;
		gram_split_phases(s, (int64_t)(s.ntn - 1) * s.ntn / 2 + 1);
	}
	return NRM_OK;
}

// ---- P-value plan (host constants of p = I_{1-R^2}(dof/2, 1/2), see nrm_pvalue.h) ----------------------------------------------
// Taylor coefficients h_k of sqrt((s/2)/sinh(s/2)) = sum_k h_k s^(2k)
static const double kNrmH[] = {1.0,
							-0.02083333333333333333333,
							0.000390625,
							-0.000007879670965608465608466,
							1.696766579172178130511e-7,
							-3.805064191721906565657e-9,
							8.748377596315407304061e-11,
							-2.044523359411973817584e-12,
							4.833351797967704408319e-14,
							-1.152434101767385923873e-15,
							2.766052043599370042286e-17};

// ln( Gamma(a+1/2)/Gamma(a) ): recurrence up to a >= 24, then the asymptotic series (DLMF 5.11.13).
static inline double nrm_ln_gamma_ratio_half(double a) {
	double shift = 0.0;
	while (a < 24.0) {
		shift += std::log(a / (a + 0.5));
		a += 1.0;
	}
	double i = 1.0 / a, i2 = i * i;
	double s = i * (-1.0 / 8 + i2 * (1.0 / 192 + i2 * (-1.0 / 640 + i2 * (17.0 / 14336 + i2 * (-31.0 / 18432 + i2 * (691.0 / 180224))))));
	return 0.5 * std::log(a) + s + shift;
}

static inline int nrm_pvalue_plan_init_host(nrm_pvalue_plan* plan, double dof) {
	NRM_REQUIRE(plan != nullptr, "nrm_pvalue_plan_init: null plan");
	NRM_REQUIRE(dof > 0, "Insufficient number of cells: dof = %g must be positive", dof);
	const int K = NRM_PCOEF / 2;  // series terms k = 0..K
	double a = 0.5 * dof;
	plan->a = a;
	plan->alpha = a - 0.25;
	plan->ln_front = nrm_ln_gamma_ratio_half(a) - 0.57236494292470008707;  // - ln(pi)/2
	for (int j = 0; j < NRM_PCOEF; j++) plan->coef[j] = 0.0;
	if (a < 8.0) {
		plan->umax = 0.0;  // asymptotic series in 1/alpha not accurate enough: continued fraction only
		return NRM_OK;
	}
	plan->umax = 1.5;
	// Products of half-integers that do not depend on dof, built once: cp[k] = prod_{i<2k} (i + 1/2), pr[j][k] = prod_{i=j+1}^{2k-1} (i + 1/2).
	// (A single=1 screen asks for a plan per grouping: with powl() and these products inside the loops a plan cost 25 us.)
	struct Tab {
		long double cp[NRM_PCOEF / 2 + 1], pr[NRM_PCOEF][NRM_PCOEF / 2 + 1];
		Tab() {
			for (int k = 0; k <= NRM_PCOEF / 2; k++) {
				cp[k] = 1;
				for (int i = 0; i < 2 * k; i++) cp[k] *= (i + 0.5L);
				for (int j = 0; j < NRM_PCOEF; j++) {
					pr[j][k] = 1;
					for (int i = j + 1; i < 2 * k; i++) pr[j][k] *= (i + 0.5L);
				}
			}
		}
	};
	static const Tab tab;
	long double ipow[NRM_PCOEF + 1];  // alpha^-m
	{
		long double pw = 1;
		ipow[0] = 1;
		for (int m = 1; m <= NRM_PCOEF; m++) {
			pw *= (long double)plan->alpha;
			ipow[m] = 1 / pw;
		}
	}
	// S = sum_k h_k alpha^-2k c'_2k,  c'_m = prod_{i<m} (i + 1/2)
	long double S = 0;
	for (int k = 0; k <= K; k++) S += (long double)kNrmH[k] * ipow[2 * k] * tab.cp[k];
	// coef_j = (1/(S sqrt(pi))) sum_{k: 2k > j} h_k alpha^(j-2k) prod_{i=j+1}^{2k-1} (i + 1/2)
	for (int j = 0; j < NRM_PCOEF; j++) {
		long double c = 0;
		for (int k = 1; k <= K; k++) {
			int m = 2 * k;
			if (j >= m) continue;
			c += (long double)kNrmH[k] * ipow[m - j] * tab.pr[j][k];
		}
		plan->coef[j] = (double)(c / (S * 1.7724538509055160272981674833411L));
	}
	return NRM_OK;
}


// ---- scratch pool of the whole-problem host entry -----------------------------------------------------------------------------
// Device scratch of the host entry, kept between calls (hipMalloc / hipFree of GB-sized buffers cost milliseconds
// each): blocks return to a per-process pool and are reused best-fit; nrm_release_cache() frees them.
template <typename Alloc>
struct DevPoolT {
	Alloc mem;  // raw allocator: void* alloc(size_t) (nullptr on failure), void free(void*)
	struct Block {
		void* p;
		size_t cap;
		bool used;
	};
	std::mutex mu;
	std::vector<Block> blocks;
	void* take(size_t bytes) {
		std::lock_guard<std::mutex> g(mu);
		int best = -1;
		for (size_t i = 0; i < blocks.size(); i++)
			if (!blocks[i].used && blocks[i].cap >= bytes && (best < 0 || blocks[i].cap < blocks[(size_t)best].cap)) best = (int)i;
		if (best >= 0 && blocks[(size_t)best].cap <= 2 * bytes + (1 << 20)) {
			blocks[(size_t)best].used = true;
			return blocks[(size_t)best].p;
		}
		void* p = mem.alloc(bytes);
		if (!p) {  // out of memory: drop the idle blocks and retry once
			for (size_t i = 0; i < blocks.size();) {
				if (!blocks[i].used) {
					mem.free(blocks[i].p);
					blocks.erase(blocks.begin() + (long)i);
				} else {
					i++;
				}
			}
			p = mem.alloc(bytes);
			if (!p) return nullptr;
		}
		blocks.push_back({p, bytes, true});
		return p;
	}
	void give(void* p) {
		std::lock_guard<std::mutex> g(mu);
		for (auto& b : blocks)
			if (b.p == p) b.used = false;
	}
	void release() {
		std::lock_guard<std::mutex> g(mu);
		for (size_t i = 0; i < blocks.size();) {
			if (!blocks[i].used) {
				mem.free(blocks[i].p);
				blocks.erase(blocks.begin() + (long)i);
			} else {
				i++;
			}
		}
	}
};
