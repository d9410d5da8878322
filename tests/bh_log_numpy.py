"""A numpy restatement of the ln form of bh and binnet (normalisr_amd/csrc/nrm_bh.hip and nrm_binnet.hip with p_kind = 1), stage by stage --
keys, sorted keys, c, ln q per sorted position, the looked-up output --, a per-row ln binnet, the definitions evaluated in longdouble, the derived bound on ln q,
and the case generators the CPU and GPU tests share.  tests/test_bh_log_cpu.py holds the restatement to the longdouble evaluation and to the linear form;
tests/test_gpu_bh_log.py and tests/test_gpu_binnet_log.py hold the device to the restatement.  Nothing here touches torch or the library."""
import numpy as np

import bh_numpy

KEY = bh_numpy.KEY
DTYPES = bh_numpy.DTYPES
ABS = {np.dtype(np.float32): np.uint32(0x7fffffff), np.dtype(np.float64): np.uint64(0x7fffffffffffffff)}


def keys(lnp):
	"""The complemented bit patterns of |ln P|: ascending key is ascending ln P, -inf comes first, both zeros share the largest key."""
	lnp = np.ascontiguousarray(lnp)
	return ~(lnp.view(KEY[lnp.dtype]) & ABS[lnp.dtype])


def values(k, dtype):
	"""ln P of keys, in fp64: -|ln P|, and +0.0 for ln 1."""
	k = np.ascontiguousarray(k)
	v = -((~k).view(np.dtype(dtype)).astype(np.float64))
	v[k == ~KEY[np.dtype(dtype)](0)] = 0.0
	return v


def stages(lnp):
	"""dict(keys, sorted, c, q, out) for a flat fp32 / fp64 array of valid ln P: q is ln q per sorted position after the suffix minimum, out the looked-up output.
	ln q(u) = min(0, u + (ln N - ln c)) in fp64, rounded once to the dtype; the minimum is taken on the rounded values (rounding is monotone: the same thing)."""
	lnp = np.ascontiguousarray(lnp).ravel()
	dt, n = lnp.dtype, lnp.size
	k = keys(lnp)
	s = np.sort(k)
	c = np.searchsorted(s, s, side='right').astype(np.uint32)
	u = values(s, dt)
	lq = u + (np.log(np.float64(n)) - np.log(c.astype(np.float64)))
	lq = np.where(lq < 0, lq, 0.0).astype(dt)
	lq = np.minimum.accumulate(lq[::-1])[::-1].copy()
	out = lq[np.searchsorted(s, k, side='left')]
	return dict(keys=k, sorted=s, c=c, q=lq, out=out)


def bh(lnp):
	return stages(lnp)['out']


def exact(lnp):
	"""ln q of every entry by the definition, in longdouble: over the distinct values u, c(u) = #{entries <= u}, min(0, u + ln N - ln c(u)), minimum over u' >= u."""
	lnp = np.ascontiguousarray(lnp).ravel()
	u, ids, cnt = np.unique(lnp.astype(np.longdouble) + np.longdouble(0), return_inverse=True, return_counts=True)
	c = np.cumsum(cnt)
	lq = u + np.log(np.longdouble(lnp.size)) - np.log(c.astype(np.longdouble))
	lq = np.where(lq < 0, lq, np.longdouble(0))
	lq = np.minimum.accumulate(lq[::-1])[::-1]
	return lq[ids], c[ids]


def bound(lq, dtype):
	"""|delta ln q| allowed against the longdouble value (derived in the issue and in DESIGN.md section 4g): two fp64 logarithms of at most 1 ulp at magnitudes below
	32, their difference and the sum with ln P one rounding each: 2^-46 + 2^-52 |ln q|; an fp32 output adds its one rounding, 2^-24 |ln q|."""
	a = np.abs(np.asarray(lq, dtype=np.float64))
	a = np.where(np.isfinite(a), a, 0.0)
	return 2.0**-46 + 2.0**-52 * a + (2.0**-24 * a if np.dtype(dtype) == np.float32 else 0.0)


def excess(got, want, dtype):
	"""max over the entries of |got - want| / bound (<= 1: inside), infinities required to agree exactly; also the largest absolute error."""
	got, want = np.asarray(got).ravel().astype(np.longdouble), np.asarray(want).ravel()
	inf = np.isinf(want)
	assert np.array_equal(np.isinf(got), inf) and (got[inf] == want[inf]).all() and not np.isnan(got).any()
	if inf.all():
		return 0.0, 0.0
	err = np.abs(got[~inf] - want[~inf]).astype(np.float64)
	return float((err / bound(want[~inf], dtype)).max()), float(err.max())


def binnet(lnp, qcut, rows=None, row0=0):
	"""The ln binnet by the definition, in fp64, row by row: row i (gene row0 + i of an (ng, ng) matrix; lnp holds the rows [row0, row0 + rows)) has m = ng - 1
	off-diagonal entries, c_v = #{entries <= v}, tau* = max{v : v + (ln m - ln c_v) <= ln qcut}, edges {lnp <= tau*}, the diagonal False.
	-> (net, margin): margin is the smallest |v + (ln m - ln c_v) - ln qcut| over every row and distinct finite value, what the comparisons with the device and with the
	linear form rest on."""
	lnp = np.asarray(lnp)
	ng = lnp.shape[1]
	net = np.zeros(lnp.shape, dtype=bool)
	lq0, lm = np.log(np.float64(qcut)), np.log(np.float64(ng - 1))
	margin = np.inf
	for i in range(lnp.shape[0]):
		off = np.ones(ng, dtype=bool)
		off[row0 + i] = False
		x = lnp[i, off].astype(np.float64)
		u, cnt = np.unique(x + 0.0, return_counts=True)
		c = np.cumsum(cnt).astype(np.float64)
		lq = u + (lm - np.log(c))
		ok = lq <= lq0
		fin = np.isfinite(lq)
		if fin.any():
			margin = min(margin, float(np.abs(lq[fin] - lq0).min()))
		if ok.any():
			net[i, off] = x <= u[ok].max()
	return net, margin


def sizes(tile):
	return bh_numpy.sizes(tile)


def _lntiny(dt):
	return np.array([-np.inf, 0.0, -0.0, -0.5, -0.25, -745.5, -9e6, -np.finfo(dt).smallest_subnormal, -1e-30], dtype=dt)


def cases(n, dtype, tile, seed=0):
	"""name -> ln P (n, dtype): the families of bh_numpy.cases mapped to ln P.  uniform: ln of uniform P; ties: a few values, -inf, 0.0 and -0.0 among them; loguniform:
	-|ln P| log-uniform from 1e-6 to 9e6; byte{b}: |ln P| patterns equal in every byte but b (the linear families' patterns, negated); the two tie groups that
	span tiles come from n >= 3 tile + 17 on."""
	dt = np.dtype(dtype)
	lin = bh_numpy.cases(n, dtype, tile, seed)
	rng = np.random.default_rng([seed, n, dt.itemsize, 1])
	with np.errstate(divide='ignore'):
		uni = np.log(lin['uniform'].astype(np.float64)).astype(dt)
	out = {
		'uniform': uni,
		'ties': rng.choice(_lntiny(dt), n),
		'loguniform': (-np.exp(rng.uniform(np.log(1e-6), np.log(9e6), n))).astype(dt),
		'identical': np.full(n, -3.7, dtype=dt),
		'sorted': np.sort(uni),
		'reversed': np.sort(uni)[::-1].copy(),
	}
	for b in range(dt.itemsize):
		out['byte{}'.format(b)] = -lin['byte{}'.format(b)]
	if n >= 3 * tile + 17:
		base = np.sort(-700.0 * (rng.permutation(4 * n)[:n].astype(np.float64) + 1) / (4 * n)).astype(dt)  # distinct values in [-700, 0), ascending
		assert np.unique(base).size == n
		for name, (lo, hi) in TIE_GROUPS(tile).items():
			v = base.copy()
			v[lo:hi] = v[lo]  # one tie group over the sorted positions [lo, hi)
			out[name] = rng.permutation(v)
	return out


def TIE_GROUPS(tile):
	return {'tie_across_tiles': (tile - 1, tile + 2), 'tie_whole_tiles': (tile - 5, 3 * tile + 3)}


ROW_WIDTHS = {np.dtype(np.float32): (257, 2049, 8193, 20481, 30721, 61441, 98305), np.dtype(np.float64): (257, 2049, 8193, 20481, 30721, 61441)}
"""The smallest width that reaches every row policy of nrm_binnet.hip's dispatch (fp32: 8, 32, 80 items of 256 threads, 60 of 512, 60 and 96 of 1024, GlobalRow;
fp64: 8, 32 of 256, 40 and 60 of 512, 60 of 1024, GlobalRow), the widths of the issue among them."""
ROWS_QCUT = 0.05


def rows_case(ng, dtype, rows=3, seed=0):
	"""(lnp (rows, ng), row0): a handful of rows of an (ng, ng) ln P matrix, |ln P| log-uniform from 1e-3 to 1e4, a third rounded to one decimal (ties), some -inf
	and some zeros, the diagonal -inf."""
	rng = np.random.default_rng([seed, ng, np.dtype(dtype).itemsize, 7])
	x = -(10.0 ** rng.uniform(-3, 4, (rows, ng)))
	t = rng.random((rows, ng))
	x = np.where(t < 1 / 3, np.round(x, 1), x)
	x[t > 0.999] = -np.inf
	x[(t > 0.99) & (t <= 0.995)] = 0.0
	x[(t > 0.995) & (t <= 0.999)] = -0.0
	row0 = ng - rows - 5
	x[np.arange(rows), row0 + np.arange(rows)] = -np.inf
	return np.ascontiguousarray(x.astype(dtype)), row0
