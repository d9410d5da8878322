// The two-sided Fisher exact P-value of ONE 2 x 2 table (k, n - k, K - k, N - K - n + k): k of the n study genes lie in a set of K genes, out of a background
// of N.  Host and device run the SAME code (csrc/nrm_enrich.hip: the kernel k_enrich_fisher and the export nrm_fisher_host), so their bits agree.
// The hypergeometric weights over the support lo = max(0, n + K - N) ... hi = min(n, K) are anchored at the mode m = clamp(((n + 1)(K + 1)) div (N + 2), lo, hi)
// with weight 1 and walked both ways by
//   w(j + 1) = w(j) ((K - j)(n - j)) / ((j + 1)(N - K - n + j + 1))        w(j - 1) = w(j) (j (N - K - n + j)) / ((K - j + 1)(n - j + 1))
// so every weight lies in [0, 1]: nothing overflows, no lgamma, and a direction stops once its weight has underflowed to 0 (a subnormal weight may stay put
// while the ratio is above 1/2; every loop ends with the support at the latest).
//   p = sum{w(j) : w(j) <= w(k) (1 + 1e-7)} / sum w(j), at most 1
// (the slack is what scipy.stats.fisher_exact allows for weights that are equal but for rounding).  w(k) comes from a first walk from the mode to k, the two
// sums from a second one over the support: mode, then rising j, then falling j.  A step rounds four times (two products, a quotient, a product) and the sums
// are of positive terms; against exact integer arithmetic the relative error stays below 8 L u for a support of L values (u = 2^-53).
// The factors are formed in fp64 from integers below 2^31 (products below 2^62).  Contraction to fused multiply-adds is switched off: the host has none.
#pragma once
#include <cstdint>

#ifndef NRM_HD
#if defined(__HIPCC__)
#define NRM_HD __host__ __device__
#else
#define NRM_HD
#endif
#endif

#define NRM_FISHER_SLACK 1e-7

// w(j + 1) / w(j)
NRM_HD inline double nrm_fisher_up(int64_t N, int64_t K, int64_t n, int64_t j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double num = (double)(K - j) * (double)(n - j), den = (double)(j + 1) * (double)(N - K - n + j + 1);
	return num / den;
}

// w(j - 1) / w(j)
NRM_HD inline double nrm_fisher_down(int64_t N, int64_t K, int64_t n, int64_t j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double num = (double)j * (double)(N - K - n + j), den = (double)(K - j + 1) * (double)(n - j + 1);
	return num / den;
}

// 0 <= K, n <= N < 2^31 and lo <= k <= hi are the caller's to check (a k outside the support is taken at its nearer end; every loop is bounded by the support)
NRM_HD inline double nrm_fisher_p(int64_t N, int64_t K, int64_t n, int64_t k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (n <= 0 || K <= 0) return 1.0;
	const int64_t lo = n + K - N > 0 ? n + K - N : 0, hi = n < K ? n : K;
	if (hi <= lo) return 1.0;
	if (k < lo) k = lo;
	if (k > hi) k = hi;
	int64_t mode = ((n + 1) * (K + 1)) / (N + 2);
	if (mode < lo) mode = lo;
	if (mode > hi) mode = hi;
	double wk = 1.0;
	for (int64_t j = mode; j < k && wk > 0.0; j++) wk = wk * nrm_fisher_up(N, K, n, j);
	for (int64_t j = mode; j > k && wk > 0.0; j--) wk = wk * nrm_fisher_down(N, K, n, j);
	const double thr = wk * (1.0 + NRM_FISHER_SLACK);
	double total = 1.0, tail = 1.0 <= thr ? 1.0 : 0.0, w = 1.0;
	for (int64_t j = mode; j < hi; j++) {
		w = w * nrm_fisher_up(N, K, n, j);
		if (w == 0.0) break;
		total = total + w;
		if (w <= thr) tail = tail + w;
	}
	w = 1.0;
	for (int64_t j = mode; j > lo; j--) {
		w = w * nrm_fisher_down(N, K, n, j);
		if (w == 0.0) break;
		total = total + w;
		if (w <= thr) tail = tail + w;
	}
	const double p = tail / total;
	return p < 1.0 ? p : 1.0;
}

// (k / n) / (K / N), 0 when the study or the set is empty
NRM_HD inline double nrm_enrich_odds(int64_t N, int64_t K, int64_t n, int64_t k) {
	if (n <= 0 || K <= 0) return 0.0;
	return ((double)k / (double)n) / ((double)K / (double)N);
}

// the selection rule: a set qualifies with odds > 1 and k >= nmin; of two qualifying sets the one of smaller p is better, the lower index of equals
NRM_HD inline bool nrm_enrich_qualifies(double odds, int64_t k, int64_t nmin) { return odds > 1.0 && k >= nmin; }
NRM_HD inline bool nrm_enrich_better(double p, int64_t t, double best_p, int64_t best_t) { return p < best_p || (p == best_p && t < best_t); }
