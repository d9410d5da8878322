"""A numpy restatement of the device algorithm of bh (normalisr_amd/csrc/nrm_bh.hip), stage by stage -- keys, sorted keys, c, q per sorted position, the looked-up
output -- and the case generator the CPU and GPU tests share.  tests/test_bh_cpu.py holds the restatement to oracle.bh (the reference's steps, binnet.py:77-131)
in bytes; tests/test_gpu_bh.py holds the device's stages to the restatement.  Nothing here touches torch or the library."""
import numpy as np

KEY = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
DTYPES = (np.float64, np.float32)


def keys(pv):
	"""The IEEE bit patterns of p + 0 as unsigned integers: monotone for non-negative finite values, -0.0 folded into +0.0."""
	pv = np.ascontiguousarray(pv)
	return (pv + pv.dtype.type(0)).view(KEY[pv.dtype])


def stages(pv):
	"""dict(keys, sorted, c, q, out) for a flat fp32 / fp64 array of valid P-values."""
	pv = np.ascontiguousarray(pv).ravel()
	dt, n = pv.dtype, pv.size
	k = keys(pv)
	s = np.sort(k)
	c = np.searchsorted(s, s, side='right').astype(np.uint32)  # (index of the last position holding the same key) + 1 = #{entries <= u}
	w = c.astype(np.float64) / np.float64(n)
	u = s.view(dt)
	if dt == np.float32:
		w = w.astype(np.float32).astype(np.float64)  # both divisions in fp64, each rounded once to fp32
	with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
		q = (u.astype(np.float64) / w).astype(dt)
	q[~np.isfinite(q)] = 1
	q = np.clip(q, dt.type(0), dt.type(1))
	q = np.minimum.accumulate(q[::-1])[::-1].copy()
	out = q[np.searchsorted(s, k, side='left')]
	return dict(keys=k, sorted=s, c=c, q=q, out=out)


def bh(pv):
	return stages(pv)['out']


def sizes(tile):
	"""N around the wave (64) and the workgroup's tile, more than one tile, and 16 tiles + 1: the smallest N whose (digit, workgroup) table (256 entries per tile) no
	longer fits one chunk of `tile` entries, so that its scan takes the second level of launches."""
	return (1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17, 16 * tile + 1)


def _tiny(dt):
	return np.array([0, 1, 0.5, 0.25, -0.0, np.finfo(dt).smallest_subnormal, 1e-300 if dt == np.float64 else 1e-40], dtype=dt)


def _byte_family(rng, n, dt, b):
	"""Keys equal in every byte but b, so that pass b alone orders them: P-values in [0, 1) by construction."""
	kt = KEY[np.dtype(dt)]
	nbytes = np.dtype(kt).itemsize
	half = np.array([0.5], dtype=dt).view(kt)[0]
	if b == nbytes - 1:
		base, lim = kt(0), 0x40  # top byte 0x00 .. 0x3f, the rest 0: 0 and powers of two below 1
	else:
		top = kt(0x3f) << kt(8 * (nbytes - 1))
		base = top if b == nbytes - 2 else (half & ~(kt(0xff) << kt(8 * b)))
		lim = (0xf0 if dt == np.float64 else 0x80) if b == nbytes - 2 else 0x100  # below the pattern of 1.0 (0x3ff0..., 0x3f80...)
	k = base | (rng.integers(0, lim, n).astype(kt) << kt(8 * b))
	return k.view(dt)


def cases(n, dtype, tile, seed=0):
	"""name -> P-values (n, dtype): the families of the issue.  The two tie-group families need n >= 3 tile + 17 and come only there."""
	dt = np.dtype(dtype)
	rng = np.random.default_rng([seed, n, dt.itemsize])
	decades = 300 if dt == np.float64 else 38
	uni = rng.random(n).astype(dt)
	out = {
		'uniform': uni,
		'ties': rng.choice(_tiny(dt), n),
		'loguniform': (10.0 ** (-decades * rng.random(n))).astype(dt),
		'identical': np.full(n, 0.37, dtype=dt),
		'sorted': np.sort(uni),
		'reversed': np.sort(uni)[::-1].copy(),
	}
	for b in range(dt.itemsize):
		out['byte{}'.format(b)] = _byte_family(rng, n, dt, b)
	if n >= 3 * tile + 17:
		base = np.sort(rng.permutation(4 * n)[:n].astype(np.float64) / (4 * n)).astype(dt)  # distinct values, ascending (exact in fp32 for these n)
		assert np.unique(base).size == n
		for name, (lo, hi) in (('tie_across_tiles', (tile - 1, tile + 2)), ('tie_whole_tiles', (tile - 5, 3 * tile + 3))):
			v = base.copy()
			v[lo:hi] = v[lo]  # one tie group over the sorted positions [lo, hi)
			out[name] = rng.permutation(v)
	return out
