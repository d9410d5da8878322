"""Yardsticks for the gene-set enrichment (normalisr_amd/enrich.py, csrc/nrm_enrich.hip), independent of the library:
  fisher_exact_fraction  the two-sided Fisher exact P-value in exact integer arithmetic: math.comb weights compared as integers, P as a Fraction
  fisher_recurrence      a plain Python restatement of the recurrence of csrc/nrm_fisher.h (Python floats are IEEE doubles without fused multiply-adds)
  enrich_numpy           a plain numpy restatement of the whole study: counts by boolean matrices, P-values from one of the two above, the selection rule
  tables                 the tables the tests run on, with their exact P-values"""
import functools
import math
from fractions import Fraction

import numpy as np

UNIT = 2.0**-53
LARGE = ((20000, 300, 100, 12), (30000, 2000, 1000, 200), (20000, 10000, 100, 50), (15000, 7500, 1024, 512))  # (N, K, n, k)


def support(N, K, n):
	return max(0, n + K - N), min(n, K)


def fisher_exact_fraction(N, K, n, k):
	"""sum{w(j) : w(j) <= w(k)} / sum w(j) with w(j) = C(K, j) C(N - K, n - j), exactly."""
	lo, hi = support(N, K, n)
	w = [math.comb(K, j) * math.comb(N - K, n - j) for j in range(lo, hi + 1)]
	wk = w[k - lo]
	return Fraction(sum(v for v in w if v <= wk), sum(w))


def relative_error(p, exact):
	"""|p - exact| / exact for a float p and a Fraction, itself exact until the last division."""
	return float(abs(Fraction(p) - exact) / exact)


def fisher_recurrence(N, K, n, k):
	if n <= 0 or K <= 0:
		return 1.0
	lo, hi = support(N, K, n)
	if hi <= lo:
		return 1.0
	mode = min(max(((n + 1) * (K + 1)) // (N + 2), lo), hi)
	up = lambda j: (float(K - j) * float(n - j)) / (float(j + 1) * float(N - K - n + j + 1))
	down = lambda j: (float(j) * float(N - K - n + j)) / (float(K - j + 1) * float(n - j + 1))
	wk = 1.0
	for j in range(mode, k):
		wk = wk * up(j)
	for j in range(mode, k, -1):
		wk = wk * down(j)
	thr = wk * (1.0 + 1e-7)
	total, tail, w = 1.0, (1.0 if 1.0 <= thr else 0.0), 1.0
	for j in range(mode, hi):
		w = w * up(j)
		if w == 0.0:
			break
		total += w
		if w <= thr:
			tail += w
	w = 1.0
	for j in range(mode, lo, -1):
		w = w * down(j)
		if w == 0.0:
			break
		total += w
		if w <= thr:
			tail += w
	return min(tail / total, 1.0)


def tables_small(nmax=12):
	"""Every table with 1 <= N <= nmax: (N, K, n, k) int64 columns."""
	out = []
	for N in range(1, nmax + 1):
		for K in range(N + 1):
			for n in range(N + 1):
				lo, hi = support(N, K, n)
				out.extend((N, K, n, k) for k in range(lo, hi + 1))
	return np.array(out, dtype=np.int64)


def tables_seeded(count=3000, seed=20240611):
	"""`count` seeded tables with N < 400; every fifth has N even and K = N / 2, where the weights are symmetric about the mode: true ties on both sides."""
	rng = np.random.default_rng(seed)
	out = []
	for i in range(count):
		N = int(rng.integers(2, 400))
		if i % 5 == 0:
			N -= N % 2
			K = N // 2
		else:
			K = int(rng.integers(0, N + 1))
		n = int(rng.integers(0, N + 1))
		lo, hi = support(N, K, n)
		out.append((N, K, n, int(rng.integers(lo, hi + 1))))
	return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tables(name):
	"""'small', 'seeded' or 'large': (the tables as (count, 4) int64, their exact P-values as Fractions, their support lengths), computed once and shared."""
	tab = dict(small=tables_small, seeded=tables_seeded, large=lambda: np.array(LARGE, dtype=np.int64))[name]()
	exact = [fisher_exact_fraction(*row) for row in tab.tolist()]
	length = np.array([hi - lo + 1 for lo, hi in (support(N, K, n) for N, K, n, k in tab.tolist())])
	return tab, exact, length


def enrich_numpy(study, member, bg=None, nmin=5, pvalue=fisher_recurrence):
	"""study (S, G) and member (T, G) as anything numpy reads as non-zero / zero, bg (G) bool or None.  Returns k (S, T), K (T), n (S), N, p, odds, top."""
	study, member = np.asarray(study) != 0, np.asarray(member) != 0
	bg = np.ones(study.shape[1], dtype=bool) if bg is None else np.asarray(bg, dtype=bool)
	a, b = (study & bg).astype(np.int64), (member & bg).astype(np.int64)
	k, K, n, N = a @ b.T, b.sum(axis=1), a.sum(axis=1), int(bg.sum())
	S, T = k.shape
	p, odds = np.ones((S, T)), np.zeros((S, T))
	top = np.full(S, -1, dtype=np.int64)
	nmin = max(int(nmin), 1)
	for s in range(S):
		for t in range(T):
			if n[s] > 0 and K[t] > 0:
				p[s, t] = pvalue(N, int(K[t]), int(n[s]), int(k[s, t]))
				odds[s, t] = (k[s, t] / n[s]) / (K[t] / N)
			if odds[s, t] > 1 and k[s, t] >= nmin and (top[s] < 0 or p[s, t] < p[s, top[s]]):
				top[s] = t
	return k, K, n, N, p, odds, top
