"""Reference of the single=4 kernels (csrc/nrm_single4.hip) and of K2', the fp64 matrix-core Gram kernel (csrc/nrm_gram.hip, nrm_gram_sched.h, the schedule in
nrm_host_logic.h), stage by stage -- TEST INFRASTRUCTURE ONLY.

numpy in longdouble (64-bit mantissa on x86) and mpmath at 60 digits for P-values; no torch, no GPU.  One plain function per C entry, taking what the entry
takes and returning what it writes, in its layout:

    gram                   nrm_gram_f64 / _band / _whole        dot[i, j] = sum_k A[i, k] B[j, k] on [0, m_rows) x [0, n_rows), symmetric: i <= j only
    fix_dot                nrm_gram_i8_fix_dot                  dot += k3_reference._corr
    spd_prepare            nrm_spd_prepare                      mp, scal[0..1], the padding diagonal
    spd_start              nrm_spd_start                        both starts
    spd_transpose_residual nrm_spd_transpose_residual           tt, ||I - T||_F
    spd_update             nrm_spd_update
    spd_finish             nrm_spd_finish                       N, small (3, nx)
    design_scalars         nrm_single4_design_scalars           dxx, varx, flags[5]
    rss, sweep             nrm_single4_sweep                    rss (d_work), vy, R^2, stat, P; flags[0..1]
    guard                  nrm_single4_sweep_guarded            flags[2..3], gene_hits

Every stage is judged on the inputs it was GIVEN (the fp64 values in HBM are exact inputs; the sweep is judged on the rss its own call left in d_work), so no
bound carries an earlier stage's error.

Running-error bounds (u = 2^-53): u x (sum of the absolute values of the terms) x (the depth of the chain the kernel documents), plus 16 x 2^-64 of the absolute
sum for the reference itself.  Depths, read off the kernels:
    gram        k_pad (an entry is one chain of multiply-adds over the K range of a piece, in any order: the four of an MFMA and the K loop) + (pieces the
                fix-up adds - 1): `parts`, or the number of stream-K contributors of the entry's tile, from the port of gram_split_phases / gram_pieces_of below.
    rss         ceil(m / 64) (a lane's fma chain) + 6 (the wave), then u |rss| for the subtraction.
    spd_rows    ceil(nx / 256) + 1 + 6 + 3; the kappa numerator sum_j |N_ij| sqrt(ss_j) one more, for the rounding of the square root
                (k_spd_rows: fma(v, sqrt(ss[j]), s1)).
    scale       mean of the diagonal: ceil(nx / 1024) + 10, and u for the division; the maximum is exact; NaN in, NaN out.
    ||I - T||_F per tile 4 (fma chain) + 2 (d = delta - t is rounded before it is squared: twice its relative error) + 6 + 3; over
                the tiles ceil(count / 1024) + 10; the root halves the relative error of the sum and adds its own u.
    sweep       termwise on g, vx, rs, n so that the bound carries the cancellation in vy:
                  expl = g^2 vx            d_expl = 2 u |expl|
                  vy = rs / n + expl       d_vy = u |rs / n| + d_expl + u |vy|
                  R^2 = expl / vy          d_R2 = (d_expl + |R^2| d_vy) / (|vy| - d_vy) + u |R^2|      (infinite when d_vy >= |vy|)
                  stat = g | g vx          0 | u |stat|
                fp32 outputs add 2^-24 |value| + 2^-150.  P: k3_reference.p_tolerance + (dof / 2) d_R2 / (1 - R^2) (k3_reference.compare_p_subset).
Bit for bit, no bound: k_spd_sym, k_spd_start, the transpose, k_spd_update (2 x is exact: fl(2 x - xt), one rounding), k_spd_finish's N (fl(x + x^T) / 2), the
diagonal row of small, design_scalars (fl(1 / fl(n d))), fix_dot and gram on exact problems (integer-valued operands, every partial sum below 2^53).

flags[0..1] of the sweep are counted by the kernel's own rule, read off k_s4_sweep: a THREAD adds one when any of its pairs is non-finite (flags[0]) / has
R^2 > 1 + 1e-8 or vy < 0 (flags[1]); a thread's pairs are gene gy = 64 bj + tx and groupings 64 bi + ty + 4 k, k = 0 .. 15 -- so the count is the number of
(gene, grouping // 64, grouping % 4) classes that hold such a pair.

The guard (S4Guard), per pair in longdouble: e_y = 2 (K c_y c* + g_y + g*) sqrt(yy / n), dr = e_y kappa_i / sqrt(vy), num = dr (dof |r| + sqrt(dof)), den =
max(1 - R^2, 1e-150)^2.  The kernel's |r| is a float square root scaled by 1.0000002f: it lies in [|r|, |r| (1 + 4e-7)] (k3_reference's docstring), so num_lo takes
|r| and num_hi |r| (1 + 4e-7); OVER when num_lo > budget den (1 + 1e-9), UNDER when num_hi < budget den (1 - 1e-9), else UNDECIDED.  An over pair is counted
unless its stored P is 0 AND P at max(|r| - dr, 0)^2 is 0 in fp64 (exempt).  This kernel tests every pair by itself (no two-level screen), so with no undecided
pair flags[2] is the number of counted pairs exactly, gene_hits is set for exactly the genes with a counted pair, and flags[3] -- the maximum of
(float)num / (float)den over the pairs that are NOT over -- lies in [(1 - 1e-5) max num_lo / den, (1 + 1e-5) max num_hi / den] over the under pairs.

SLACK multiplies every bound.  It is settled on the CPU (tests/test_s4_reference_cpu.py: the worst ratio of the fp64 emulation to the unslackened bound over every
shape the GPU file uses, rounded up to a power of two, capped at 4).  Measured there: worst ratio 0.71 over the fp64 outputs (rss), 0.994 over the fp32 outputs (whose bound is little more than
their own rounding) -> SLACK = 1.  A device ratio above 1 is a finding about the kernel."""
import functools
import math

import numpy as np

import k3_reference as k3
from k3_reference import LD, U, Worst, ld, worst, same_bits, bits  # noqa: F401

SLACK = 1.0
ULD = 2.0**-64
OWN = 16 * ULD
F32, F64 = np.float32, np.float64
GM = GN = 128
GK = 16
GSB = 8
STRIDE = 8

# ---- the shapes of the GPU file (imported by both test files) -------------------------------------------------------------------------------------------------
# gram: (name, m_pad, n_pad, k_pad, symmetric, m_rows, n_rows, row0, row1 (None: m_pad), whole)
GRAM = [
	('stored-whole', 128, 128, 16, 0, 128, 128, 0, None, False),
	('one-tile-40', 128, 128, 640, 0, 100, 77, 0, None, False),
	('straddle', 128, 384, 6400, 0, 128, 300, 0, None, False),
	('parts8', 1024, 1024, 1024, 0, 1024, 1024, 0, None, False),
	('parts4', 1536, 1536, 512, 0, 1536, 1530, 0, None, False),
	('parts2', 2048, 2048, 256, 0, 2041, 2048, 0, None, False),
	('whole+17', 2944, 2944, 32, 0, 2944, 2944, 0, None, False),
	('sym1000', 1024, 1024, 64, 1, 1000, 1000, 0, None, False),
	('sym65', 256, 256, 48, 1, 65, 65, 0, None, False),
	('band', 2048, 256, 32, 0, 2000, 200, 1024, None, False),
	('whole:straddle', 128, 384, 6400, 0, 128, 300, 0, None, True),
	('whole:whole+17', 2944, 2944, 32, 0, 2944, 2944, 0, None, True),
	('finite:whole-ragged16', 256, 256, 48, 0, 144, 80, 0, None, True),  # (rows and columns end ON a sub-block edge; operands finite throughout: an extra sub-block shows)
]
GRAM_ROWS_FULL = 1 << 25  # m n k up to which the longdouble reference takes every row; above, five rows of every tile row
FIX_ROWS, FIX_COLS, FIX_NS = [1, 15, 16, 17, 70], [1, 63, 64, 65, 130], [5, 6]
SPD = [(1, 128), (63, 128), (65, 128), (128, 128), (255, 256), (257, 384), (1000, 1024), (1023, 1024), (1025, 1152)]
UPDATE_COUNTS = [1, 2, 3, 511, 512, 513, 128 * 128]
SCALARS_NX = [1, 255, 256, 257]
SWEEP_N = [1, 63, 64, 65, 130]
SWEEP_DOF = [3, 2044, 49990]
SWEEP_VARIANTS = [(F64, 0), (F32, 1)]  # (output type, return_dot)
GUARD_CASES = ['ns6', 'ns5']


def sweep_cases():
	"""(nx, ny, extra, dof, dtype, return_dot): every nx and ny of SWEEP_N (crossed with the extremes), both m, both variants, every dof."""
	out = []
	k = 0
	for nx in SWEEP_N:
		for ny in SWEEP_N:
			if nx in (1, 130) or ny in (1, 130) or nx == ny:
				dt, rd = SWEEP_VARIANTS[k % 2]
				out.append((nx, ny, (0, 5)[(k // 2) % 2], SWEEP_DOF[k % 3], dt, rd))
				k += 1
	return out


def gamma(c):
	return c * U / (1.0 - c * U)


def fma64(a, b, c):
	"""fl(a b + c) of fp64 operands: the product of two 53-bit numbers in a 64-bit mantissa, then one sum -- an fma up to a double rounding in 2^-11 of the cases."""
	return np.asarray(ld(a) * ld(b) + ld(c), dtype=F64)


# ---- the schedule of K2' (port of csrc/nrm_host_logic.h: gram_tiles_before, gram_split_phases, gram_plan, gram_tile_coords, gram_pieces_of) ---------------------
def tiles_before(bi, symmetric, ntm, ntn):
	nbn = (ntn + GSB - 1) // GSB
	t = 0
	for b in range(bi):
		h = min(GSB, ntm - b * GSB)
		for bj in range(b if symmetric else 0, nbn):
			w = min(GSB, ntn - bj * GSB)
			t += h * (h + 1) // 2 if (symmetric and b == bj) else h * w
	return t


def split_phases(s, tiles):
	nwg, nkt = s['nwg'], s['nkt']
	waves = tiles // nwg
	rem = tiles - waves * nwg
	s['tiles_dp'], s['parts'], s['tiles_al'] = waves * nwg, 1, 0
	parts = 2
	while parts <= 8 and nkt >= 8 * parts:
		if rem >= nwg // parts:
			s['parts'], s['tiles_al'] = parts, nwg // parts
			break
		parts *= 2
	sk = rem - s['tiles_al']
	s['tiles_sk'] = sk
	s['units_per_wg'] = (sk * nkt + nwg - 1) // nwg


def gram_schedule(m_pad, n_pad, nkt, symmetric, m_rows, n_rows, row0, row1, nwg, whole=False):
	"""gram_plan's GramSched as a dict (whole: as nrm_gram_f64_whole rewrites it)."""
	ntm, ntn = m_pad // GM, n_pad // GN
	tile0 = tiles_before(row0 // (GSB * GM), symmetric, ntm, ntn)
	tiles = tiles_before((row1 + GSB * GM - 1) // (GSB * GM), symmetric, ntm, ntn) - tile0
	s = dict(tile0=tile0, accumulate=0, fold=0, m_rows=m_rows if 0 < m_rows < m_pad else m_pad, n_rows=n_rows if 0 < n_rows < n_pad else n_pad, ntm=ntm, ntn=ntn,
			 nkt=nkt, nwg=nwg - nwg % 8, symmetric=int(symmetric), tiles=tiles)
	split_phases(s, tiles)
	if whole:
		s['tiles_dp'] += s['tiles_al'] + s['tiles_sk']
		s['tiles_al'] = s['tiles_sk'] = s['units_per_wg'] = 0
		s['parts'] = 1
	return s


FIELDS = ['m_rows', 'n_rows', 'ntm', 'ntn', 'nkt', 'tiles_dp', 'tiles_al', 'parts', 'tiles_sk', 'units_per_wg', 'nwg', 'tile0', 'accumulate', 'fold']


def tile_coords(t, symmetric, ntm, ntn):
	nbm, nbn = (ntm + GSB - 1) // GSB, (ntn + GSB - 1) // GSB
	for bi in range(nbm):
		h = min(GSB, ntm - bi * GSB)
		for bj in range(bi if symmetric else 0, nbn):
			w = min(GSB, ntn - bj * GSB)
			diag = symmetric and bi == bj
			cnt = h * (h + 1) // 2 if diag else h * w
			if t < cnt:
				if not diag:
					li, lj = divmod(t, w)
				else:
					li, ln = 0, h
					while t >= ln:
						t -= ln
						li += 1
						ln -= 1
					lj = li + t
				return bi * GSB + li, bj * GSB + lj
			t -= cnt
	return 0, 0


def pieces_of(s, p):
	"""The pieces (tile of the launch, k0, k1, slab index or None) of the workgroup whose index after the XCD remap is p, in its order."""
	out = []
	t_dp = p
	al_todo = p < s['tiles_al'] * s['parts']
	u = p * s['units_per_wg']
	total = s['tiles_sk'] * s['nkt']
	uend = min(u + s['units_per_wg'], total)
	sk_piece = 0
	nkt = s['nkt']
	while True:
		if t_dp < s['tiles_dp']:
			out.append((t_dp, 0, nkt, None))
			t_dp += s['nwg']
		elif al_todo:
			al_todo = False
			ta, part = divmod(p, s['parts'])
			out.append((s['tiles_dp'] + ta, nkt * part // s['parts'], nkt * (part + 1) // s['parts'], p))
		elif u < uend:
			ts = u // nkt
			k0 = u - ts * nkt
			k1 = min(k0 + (uend - u), nkt)
			slab = None if (k0 == 0 and k1 == nkt) else s['tiles_al'] * s['parts'] + 2 * p + sk_piece
			out.append((s['tiles_dp'] + s['tiles_al'] + ts, k0, k1, slab))
			u += k1 - k0
			sk_piece += 1
		else:
			return out


def remap(s, block):
	return (block & 7) * (s['nwg'] >> 3) + (block >> 3)


def pieces_hash(s):
	"""A checksum over every workgroup's piece list in launch order (the host program of the CPU test prints the same from gram_pieces_of)."""
	h = 0
	for block in range(s['nwg']):
		for (t, k0, k1, slab) in pieces_of(s, remap(s, block)):
			for v in (block, t, k0, k1, -1 if slab is None else slab):
				h = (h * 1000003 + v + 7) % ((1 << 61) - 1)
	return h


def fixup_reads(s, b, mutate=None):
	"""Port of k_gram_fixup's slab arithmetic for split tile b: (tile of the launch, slab indices in the order they are added), or None: stored whole."""
	if b < s['tiles_al']:
		return s['tiles_dp'] + b, [b * s['parts'] + q for q in range(s['parts'] - (1 if mutate == 'drop-slab' else 0))]
	ts = b - s['tiles_al']
	u0 = ts * s['nkt']
	u1 = u0 + s['nkt']
	first = u0 // s['units_per_wg']
	last = min((u1 - 1) // s['units_per_wg'], s['nwg'] - 1)
	count = last - first + 1
	if count == 1 and first * s['units_per_wg'] <= u0 and (first + 1) * s['units_per_wg'] >= u1:
		return None
	base = s['tiles_al'] * s['parts']
	local = 0 if (first * s['units_per_wg'] // s['nkt']) == ts else 1
	if mutate == 'drop-second-piece':
		local = 0
	if mutate == 'drop-slab':
		count -= 1
	return s['tiles_dp'] + s['tiles_al'] + ts, [base + 2 * first + local] + [base + 2 * (first + q) for q in range(1, count)]


def tile_map(s):
	"""tile of the launch -> list of (k0, k1, slab) pieces in the order the result is formed (one whole piece, or the fix-up's order), from pieces_of alone."""
	tiles = {}
	for p in range(s['nwg']):
		for (t, k0, k1, slab) in pieces_of(s, p):
			tiles.setdefault(t, []).append((k0, k1, slab))
	return tiles


def branches(s):
	"""Which branches of the schedule and of the fix-up a launch reaches."""
	out = set()
	if s['tiles_dp']:
		out.add('whole-tiles')
	if s['tiles_al']:
		out.add('parts%d' % s['parts'])
	if s['tiles_dp'] and (s['tiles_al'] or s['tiles_sk']):
		out.add('whole+remainder')
	if s['tiles_sk'] and not s['tiles_dp'] and not s['tiles_al']:
		out.add('all-stream-k')
	for b in range(s['tiles_al'], s['tiles_al'] + s['tiles_sk']):
		r = fixup_reads(s, b)
		if r is None:
			out.add('stored-whole')
		elif r[1][0] % 2 != (s['tiles_al'] * s['parts']) % 2:
			out.add('straddle')
	if s['symmetric'] and s['m_rows'] % 16:
		out.add('symmetric-ragged')
	if s['tile0']:
		out.add('band')
	return out


def gram_case(case, nwg):
	name, m_pad, n_pad, k_pad, sym, m_rows, n_rows, row0, row1, whole = case
	return gram_schedule(m_pad, n_pad, k_pad // GK, sym, m_rows, n_rows, row0, m_pad if row1 is None else row1, nwg, whole)


def ceil16(v):
	return (v + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def gram_data(case, exact):
	"""(A, B): (m_pad, k_pad) and (n_pad, k_pad), B is A for symmetric cases.  Rows at and beyond ceil16(rows) are NaN (no row may leak into another); exact:
	integers in [-1000, 1000] (every partial sum below 2^53 in any order).  The padded K columns are the caller's to keep zero: the kernel contracts all of k_pad."""
	name, m_pad, n_pad, k_pad, sym, m_rows, n_rows = case[:7]
	rng = np.random.default_rng([11, m_pad, n_pad, k_pad, int(exact)])

	def mk(rows_pad, rows):
		a = rng.integers(-1000, 1001, (rows_pad, k_pad)).astype(F64) if exact else rng.normal(size=(rows_pad, k_pad)) * np.exp(rng.normal(size=(rows_pad, 1)))
		if not name.startswith('finite'):
			a[ceil16(rows):] = np.nan
		return a
	A = mk(m_pad, m_rows)
	return A, (A if sym else mk(n_pad, n_rows))


def gram_rows(case):
	"""The rows the longdouble reference (and the emulation) take: all of the launch's, or the first, the last and five of every tile row."""
	name, m_pad, n_pad, k_pad, sym, m_rows, n_rows, row0, row1, whole = case
	lo, hi = row0, min(m_rows, m_pad if row1 is None else row1)
	if (hi - lo) * n_rows * k_pad <= GRAM_ROWS_FULL:
		return np.arange(lo, hi)
	rng = np.random.default_rng(m_pad + k_pad)
	picks = {lo, hi - 1}
	for t in range(lo // GM, (hi + GM - 1) // GM):
		for r in rng.integers(0, GM, 5):
			if t * GM + r < hi:
				picks.add(int(t * GM + r))
	return np.array(sorted(picks))


def gram_written(s):
	"""Mask (m_pad, n_pad) of what a launch must write: the `need` sub-blocks of a tile stored by its workgroup, all of a tile the fix-up writes."""
	w = np.zeros((s['ntm'] * GM, s['ntn'] * GN), dtype=bool)
	for t, pcs in tile_map(s).items():
		ti, tj = tile_coords(s['tile0'] + t, s['symmetric'], s['ntm'], s['ntn'])
		if len(pcs) > 1 or pcs[0][2] is not None:
			w[ti * GM:(ti + 1) * GM, tj * GN:(tj + 1) * GN] = True
			continue
		for i in range(0, GM, 16):
			for j in range(0, GN, 16):
				r, c = ti * GM + i, tj * GN + j
				if r < s['m_rows'] and c < s['n_rows'] and (not (s['symmetric'] and ti == tj) or c >= r):
					w[r:r + 16, c:c + 16] = True
	return w


def gram_defined(s, rows):
	"""Mask (len(rows), n_pad) of the entries the entry defines among these rows."""
	n_pad = s['ntn'] * GN
	d = np.zeros((len(rows), n_pad), dtype=bool)
	d[:, :s['n_rows']] = True
	if s['symmetric']:
		d &= np.arange(n_pad)[None, :] >= np.asarray(rows)[:, None]
	return d


def gram(case, s, exact, rows):
	"""dot[rows] in longdouble (exact: fp64, exact), its bound and the mask of defined entries."""
	A, B = gram_data(case, exact)
	n_pad = s['ntn'] * GN
	d = gram_defined(s, rows)
	bz = np.where(np.isnan(B), 0.0, B)
	if exact:
		return dict(dot=A[rows] @ bz.T, mask=d)
	a, b = ld(A[rows]), ld(bz)
	dot, ab = a @ b.T, np.abs(a) @ np.abs(b).T
	pieces = np.ones((len(rows), n_pad))
	tm = tile_map(s)
	for t, pcs in tm.items():
		ti, tj = tile_coords(s['tile0'] + t, s['symmetric'], s['ntm'], s['ntn'])
		sel = (np.asarray(rows) // GM) == ti
		pieces[np.ix_(sel, np.arange(tj * GN, (tj + 1) * GN))] = len(pcs)
	k_pad = s['nkt'] * GK
	return dict(dot=dot, bound=SLACK * U * (k_pad + pieces - 1) * ab + OWN * ab, mask=d)


def judge_gram(got_rows, ref, exact):
	m = ref['mask']
	if exact:
		return dict(dot=bits(np.where(m, got_rows, 0.0), np.where(m, ref['dot'], 0.0), 'dot == exact integer sums'))
	err = np.where(m, np.abs(ld(got_rows) - ref['dot']), 0)
	err = np.where(m & ~np.isfinite(got_rows), np.inf, err)
	return dict(dot=worst(err, np.where(m, ref['bound'], 0), 'dot'))


def judge_gram_placement(case, s, got_rows, rows):
	"""Outside gram_written nothing may be written; inside it, wherever both operand rows are finite, a number must stand."""
	w = gram_written(s)[rows]
	nan = np.isnan(got_rows)
	bad = np.argwhere(~w & ~nan)
	if bad.size:
		return Worst(np.inf, tuple(int(v) for v in bad[0]), 'written outside the need sub-blocks / the launch\'s tiles')
	fin = w.copy()
	if not case[0].startswith('finite'):
		fin &= (np.asarray(rows) < ceil16(s['m_rows']))[:, None] & (np.arange(w.shape[1]) < ceil16(s['n_rows']))[None, :]
	bad = np.argwhere(fin & nan)
	if bad.size:
		return Worst(np.inf, tuple(int(v) for v in bad[0]), 'not written')
	return Worst(0.0, None, 'placement')


def emu_gram(case, s, exact, rows, mutate=None):
	"""fp64 emulation of k_gram_f64 + k_gram_fixup on these rows: every piece one chain over its K range in the kernel's cell order (slab kt; half h; element e;
	lane group lg: cell 2 ((4 h + lg)) + e -- the chunk a lane reads is un-swizzled by the same XOR it was stored with), pieces to slabs, the fix-up's order.
	Mutations: 'swizzle' (the read side forgets the XOR: row r reads chunk c ^ (r & 7)), 'drop-slab', 'drop-second-piece', 'edge' (need: < turned into <=)."""
	A, B = gram_data(case, exact)
	n_pad = s['ntn'] * GN
	out = np.full((len(rows), n_pad), np.nan)
	rows = np.asarray(rows)
	order = [2 * (4 * h + lg) + e for h in range(2) for e in range(2) for lg in range(4)]
	slabs = {}

	def piece(ti, tj, k0, k1, sel):
		a, b = A[rows[sel]], B[tj * GN:(tj + 1) * GN]
		acc = np.zeros((a.shape[0], GN))
		cj = np.arange(tj * GN, (tj + 1) * GN)
		for kt in range(k0, k1):
			for c in order:
				ka = kt * GK + c
				if mutate == 'swizzle':  # B's read side forgets the XOR: column j gets cell chunk ^ (j & 7)
					kb = kt * GK + ((c // 2) ^ (cj & 7)) * 2 + c % 2
					acc = fma64(a[:, ka, None], b[cj - cj[0], kb][None, :], acc)
				else:
					acc = fma64(a[:, ka, None], b[None, :, ka], acc)
		return acc
	for t, pcs in tile_map(s).items():
		ti, tj = tile_coords(s['tile0'] + t, s['symmetric'], s['ntm'], s['ntn'])
		sel = np.nonzero(rows // GM == ti)[0]
		if not sel.size:
			continue
		cols = slice(tj * GN, (tj + 1) * GN)
		for (k0, k1, slab) in pcs:
			v = piece(ti, tj, k0, k1, sel)
			if slab is None:
				need = np.zeros((sel.size, GN), dtype=bool)
				for x, r in enumerate(rows[sel]):
					r16 = r // 16 * 16
					for j in range(0, GN, 16):
						c = tj * GN + j
						lt = (lambda p, q: p <= q) if mutate == 'edge' else (lambda p, q: p < q)
						if lt(r16, s['m_rows']) and lt(c, s['n_rows']) and (not (s['symmetric'] and ti == tj) or c >= r16):
							need[x, j:j + 16] = True
				out[sel, cols] = np.where(need, v, out[sel, cols])
			else:
				slabs[(slab, t)] = v
	for b in range(s['tiles_al'] + s['tiles_sk']):
		r = fixup_reads(s, b, mutate)
		if r is None:
			continue
		t, order_ = r
		ti, tj = tile_coords(s['tile0'] + t, s['symmetric'], s['ntm'], s['ntn'])
		sel = np.nonzero(rows // GM == ti)[0]
		if not sel.size:
			continue
		acc = None
		for q in order_:
			v = slabs.get((q, t))
			if v is None:  # (a slab another tile's piece wrote, or nobody: what a wrong index reads)
				v = np.full((sel.size, GN), np.nan)
			acc = v if acc is None else acc + v
		out[sel, tj * GN:(tj + 1) * GN] = acc
	return out


# ---- fix_dot ---------------------------------------------------------------------------------------------------------------------------------------------------
def fix_problem(rows, cols, ns, exact):
	"""(dot, fr, fc, n) from k3_reference.problem: its records and its raw products."""
	n, dof = 4096, 4093
	pb = k3.problem(exact, False, rows, cols, n, dof, ns)
	return pb.dot.copy(), pb.fx.copy(), pb.fy.copy(), n


def fix_dot(dot, fr, fc, ns, n, exact):
	if exact:
		return dict(dot=dot + np.asarray(k3._corr(fr, fc, ns, n, F64)[0]))
	corr, ca = k3._corr(fr, fc, ns, n)
	out = ld(dot) + corr
	return dict(dot=out, bound=SLACK * (gamma(k3.C_CORR) * ca + U * np.abs(out)) + OWN * (ca + np.abs(ld(dot))))


def judge_fix_dot(got, ref, exact):
	if exact:
		return dict(dot=bits(got, ref['dot'], 'dot + corr, one rounding'))
	return dict(dot=worst(np.abs(ld(got) - ref['dot']), ref['bound'], 'dot'))


def emu_fix_dot(dot, fr, fc, ns, n, mutate=None):
	"""k_fix_dot: prefix sums of the column's record, five fmas against v[top - s], the product with fl(1 / n), one sum."""
	top = ns - 2
	v = np.cumsum(fc[:, :5], axis=1)
	acc = np.zeros(dot.shape)
	for s in range(5):
		idx = (4 - s) if top == 4 else (3 - s)
		if mutate == 'top':
			idx = 4 - s
		y = v[:, idx] if idx >= 0 else np.zeros(fc.shape[0])
		acc = fma64(fr[:, s, None], y[None, :], acc)
	return dot + acc * (1.0 / n)


# ---- the small steps around the Newton-Schulz inverse -----------------------------------------------------------------------------------------------------------
def spd_matrix(nx, seed=0, weak=False):
	"""A symmetric positive definite nx x nx matrix with entries of both signs.  Off-diagonal mass enough that X = diag(1 / M_ii) does not converge (the iteration
	takes the norm start); weak: a twentieth of it, 2 diag(M) - M is positive definite and the diagonal start converges."""
	rng = np.random.default_rng([21, nx, seed])
	q = rng.normal(size=(nx, nx + 3))
	return (0.05 if weak else 1.0) * (q @ q.T) / (nx + 3) + np.diag(rng.uniform(0.5, 2.0, nx))


def rows_sums(a, nx, wgt=None):
	"""(sum_j |a_ij| [w_j], sum of the same absolute terms (equal), depth) over j < nx, in longdouble."""
	v = np.abs(ld(a[:nx, :nx]))
	if wgt is not None:
		v = v * np.sqrt(ld(wgt))[None, :]
	s = v.sum(axis=1)
	depth = -(-nx // 256) + 1 + 6 + 3 + (1 if wgt is not None else 0)
	return s, SLACK * U * depth * s + OWN * s


def spd_prepare(m, nx, nxp):
	"""mp without its padding diagonal (bit for bit), scal and their bounds.  m: (nx, >= nx), the upper triangle is read."""
	up = np.triu(m[:nx, :nx])
	mp = np.zeros((nxp, nxp))
	mp[:nx, :nx] = up + np.triu(up, 1).T
	s, sb = rows_sums(mp, nx)
	dg = ld(np.diagonal(mp)[:nx])
	tot, ab = dg.sum(), np.abs(dg).sum()
	mean = tot / nx
	mb = SLACK * U * ((-(-nx // 1024) + 10) * ab / nx + np.abs(mean)) + OWN * ab / nx
	# ||M||_1 = the largest row sum: each candidate carries its own bound, so the maximum carries the largest of them
	return dict(mp=mp, norm1=s.max() if not np.isnan(s).any() else LD('nan'), norm1_bound=sb.max() if np.isfinite(sb).all() else np.inf, mean=mean, mean_bound=mb)


def judge_spd_prepare(got_mp, got_scal, ref, nx, nxp):
	ws = {}
	body = got_mp.copy()
	pad = np.arange(nx, nxp)
	ws['padding diag'] = bits(body[pad, pad], np.full(len(pad), got_scal[1]), 'mp_ii == scal[1] in the padding')
	body[pad, pad] = 0.0
	ws['mp'] = bits(body, ref['mp'], 'mp == symmetrised m, 0 in the padding')
	for k, name in ((0, 'norm1'), (1, 'mean')):
		if np.isnan(ref[name]):
			ws[name] = Worst(0.0 if np.isnan(got_scal[k]) else np.inf, None, name + ' NaN')
		else:
			ws[name] = worst(np.abs(ld(got_scal[k:k + 1]) - ref[name]), np.asarray([ref[name + '_bound']]), name)
	return ws


def spd_start(mp, nxp, diagonal, scal0):
	x = np.zeros((nxp, nxp))
	i = np.arange(nxp)
	x[i, i] = 1.0 / np.diagonal(mp) if diagonal else 1.0 / scal0
	return x


def spd_transpose_residual(t, nxp):
	d = np.eye(nxp, dtype=LD) - ld(t)
	s = (d * d).sum()
	count = (nxp // 32)**2
	depth = (4 + 2 + 6 + 3) + (-(-count // 1024) + 10)
	res = np.sqrt(s)
	return dict(tt=np.ascontiguousarray(t.T), res=res, res_bound=SLACK * U * (depth / 2 + 1) * res + OWN * res)


def spd_update(x, xt):
	return 2.0 * x - xt


def spd_finish(x, nx, nxp, ss):
	n = np.zeros((nxp, nxp))
	n[:nx, :nx] = 0.5 * (x[:nx, :nx] + x[:nx, :nx].T)
	k, kb = rows_sums(n, nx, ss)
	r, rb = rows_sums(n, nx)
	return dict(n=n, diag=np.diagonal(n)[:nx].copy(), kappa=k, kappa_bound=kb, rowsum=r, rowsum_bound=rb)


def judge_spd_finish(got_n, got_small, ref):
	return dict(N=bits(got_n, ref['n'], 'N == fl(x + x^T) / 2, 0 in the padding'), diag=bits(got_small[0], ref['diag'], 'small[0] == diag N'),
				kappa=worst(np.abs(ld(got_small[1]) - ref['kappa']), ref['kappa_bound'], 'sum |N_ij| sqrt(ss_j)'),
				rowsum=worst(np.abs(ld(got_small[2]) - ref['rowsum']), ref['rowsum_bound'], 'sum |N_ij|'))


def _tree(v):
	"""Pairwise tree over the last axis (length a power of two), the order of the LDS reductions: v[t] += v[t + o], o = len/2 .. 1."""
	v = np.array(v, dtype=F64)
	o = v.shape[-1] // 2
	while o:
		v = v[..., :o] + v[..., o:2 * o]
		o //= 2
	return v[..., 0]


def _wave_down(v):
	"""__shfl_down tree of 64 lanes: lane 0 ends with the sum in the order o = 32 .. 1."""
	return _tree(v)


def emu_spd_rows(a, nx, wgt=None, mutate=None):
	"""k_spd_rows: a thread's chain over j = t, t + 256, ..; 64-lane shuffle tree; the four waves in order."""
	cols = -(-nx // 256) * 256
	v = np.zeros((nx, cols))
	v[:, :nx] = np.abs(a[:nx, :nx])
	if mutate == 'edge':  # (j <= nx: one column too many)
		v[:, nx % cols] += np.abs(a[:nx, min(nx, a.shape[1] - 1)]) if nx < a.shape[1] else 1.0
	w = np.ones(cols)
	if wgt is not None:
		w[:nx] = np.sqrt(wgt)
	acc = np.zeros((nx, 256))
	for c in range(0, cols, 256):
		acc = fma64(v[:, c:c + 256], w[None, c:c + 256], acc) if wgt is not None else acc + v[:, c:c + 256]
	wv = _wave_down(acc.reshape(nx, 4, 64))
	return ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]


def emu_spd_scale(rowsum, diag, nx, mutate=None):
	"""k_spd_scale: 1024 threads stride the rows, LDS tree; NaN carried by hand beside fmax (which drops it)."""
	n = -(-nx // 1024) * 1024
	r, d = np.zeros(n), np.zeros(n)
	r[:nx], d[:nx] = rowsum[:nx], diag[:nx]
	bad = np.isnan(r).reshape(-1, 1024).any(axis=0)
	a = np.fmax.reduce(np.vstack([np.zeros(1024), r.reshape(-1, 1024)]), axis=0)
	mx = a if mutate == 'fmax' else np.where(bad, np.nan, a)
	b = np.zeros(1024)
	for c in range(0, n, 1024):
		b = b + d[c:c + 1024]
	o = 512
	while o:
		lo, hi = mx[:o], mx[o:2 * o]
		mx = np.fmax(lo, hi) if mutate == 'fmax' else np.where(np.isnan(lo) | np.isnan(hi), np.nan, np.fmax(lo, hi))
		o //= 2
	return float(mx[0]), float(_tree(b) / nx)


def emu_spd_residual(t, nxp):
	"""k_spd_transpose_res + k_spd_res: per 32 x 32 tile a thread's four fmas, shuffle tree, four waves in order; the tiles by 1024 threads and an LDS tree."""
	nt = nxp // 32
	d = np.eye(nxp) - t
	part = np.zeros(nt * nt)
	for bi in range(nt):
		blk = d[bi * 32:(bi + 1) * 32].reshape(32, nt, 32)  # [r][bj][tx]
		s = np.zeros((nt, 8, 32))  # thread (ty, tx)
		for k in range(4):
			rr = blk[np.arange(8) + 8 * k]  # rows ty + 8 k: (8, nt, 32)
			s = fma64(rr.transpose(1, 0, 2), rr.transpose(1, 0, 2), s)
		wv = _wave_down(s.reshape(nt, 4, 64))
		part[bi * nt:(bi + 1) * nt] = ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]
	n = -(-len(part) // 1024) * 1024
	p = np.zeros(n)
	p[:len(part)] = part
	b = np.zeros(1024)
	for c in range(0, n, 1024):
		b = b + p[c:c + 1024]
	return float(np.sqrt(_tree(b)))


def emu_spd_sym(m, nx, nxp, mutate=None):
	"""k_spd_sym tile by tile: upper tiles written directly and mirrored from the transposed LDS tile."""
	mp = np.full((nxp, nxp), np.nan)
	nt = nxp // 32
	lim = nx + 1 if mutate == 'edge' else nx
	for bi in range(nt):
		for bj in range(bi, nt):
			i, j = np.meshgrid(np.arange(bi * 32, bi * 32 + 32), np.arange(bj * 32, bj * 32 + 32), indexing='ij')
			ok = (i < lim) & (j < lim)
			ii, jj = np.minimum(i, j), np.maximum(i, j)
			src = np.where(ok, m[np.minimum(ii, m.shape[0] - 1), np.minimum(jj, m.shape[1] - 1)], 0.0)
			mp[bi * 32:bi * 32 + 32, bj * 32:bj * 32 + 32] = src
			if bj > bi:
				mp[bj * 32:bj * 32 + 32, bi * 32:bi * 32 + 32] = src if mutate == 'transpose' else src.T
	return mp


def emu_spd_update(x, xt, mutate=None):
	"""k_spd_update over a flat array: the double2 body for e + 1 < count, the scalar tail for an odd count."""
	x, xt = x.ravel().copy(), xt.ravel()
	count = x.size
	body = count - count % 2
	x[:body] = 2.0 * x[:body] - xt[:body]
	if count % 2 and mutate != 'tail':
		x[count - 1] = 2.0 * x[count - 1] - xt[count - 1]
	return x


def emu_spd_finish(x, nx, nxp, mutate=None):
	"""k_spd_finish: out = (x + mirror tile read through LDS, transposed) / 2 inside nx x nx."""
	mirror = x if mutate == 'untransposed' else x.T
	lim = nx + 1 if mutate == 'edge' else nx
	i, j = np.meshgrid(np.arange(nxp), np.arange(nxp), indexing='ij')
	return np.where((i < lim) & (j < lim), 0.5 * (x + mirror), 0.0)


# ---- design scalars ----------------------------------------------------------------------------------------------------------------------------------------------
def scalars_input(nx):
	"""small (3, nx) with the rows the kernel tells apart: d <= 0, d = inf (v = 0: varx = 1), d NaN, a non-finite kappa numerator or row sum."""
	rng = np.random.default_rng([31, nx])
	small = np.abs(rng.normal(size=(3, nx))) + 0.1
	plant = [(0, 0, -1.0), (0, 1, 0.0), (0, 2, np.inf), (0, 3, np.nan), (1, 4, np.inf), (2, 5, np.nan), (0, nx - 1, -0.0), (0, 255, np.nan), (0, 256, np.inf)]
	for r, c, v in plant:
		if 0 <= c < nx and (nx > 6 or c == nx - 1):
			small[r, c] = v
	return small


def design_scalars(small, nx, n):
	d = small[0]
	with np.errstate(divide='ignore', invalid='ignore'):
		v = 1.0 / (float(n) * d)
	bad = ~(np.isfinite(d) & (d > 0) & np.isfinite(small[1]) & np.isfinite(small[2]))
	return dict(dxx=v, varx=np.where(v == 0, 1.0, v), count=int(bad.sum()))


# ---- rss and the sweep -------------------------------------------------------------------------------------------------------------------------------------------
class SweepProblem:
	"""What nrm_single4_sweep reads -- bt, pt (ny, m), yy (ny), dxx (nx), n, dof -- and the planted pairs (grouping, gene) by name.  sym, pairs() and plants are
	what k3_reference.compare_p_subset asks of a problem."""
	sym = False

	def __init__(self, **k):
		self.__dict__.update(k)

	def pairs(self):
		return np.ones((self.nx, self.ny), dtype=bool)


@functools.lru_cache(maxsize=None)
def sweep_problem(nx, ny, extra, dof, edges=True, seed=0):
	"""m = nx + extra columns.  Genes get an rss of n uniform(0.5, 2) (yy = fl(sum) + that).  Planted (when the shape has room): P near 1, 1e-30, the smallest
	subnormal of fp32 and of fp64, 0; a dxx == 0 row; a gene whose rss is three ulps below zero (its one product exact, every other coefficient 0: vy < 0 there);
	a gene with R^2 = 2 (rss = -n expl / 2); a NaN and an Inf in B.  edges=False: none of the last five (guard cases)."""
	rng = np.random.default_rng([41, nx, ny, extra, int(dof), seed])
	m, n = nx + extra, 4096
	a = dof / 2.0
	dxx = rng.uniform(0.5, 2.0, nx) / n
	rs = n * rng.uniform(0.5, 2.0, ny)
	r = rng.normal(size=(ny, nx)) * min(1.5 / math.sqrt(dof + 1), 0.3)
	strong = rng.random((ny, nx)) < 0.1
	r = np.where(strong, rng.uniform(0.75, 0.95, (ny, nx)) * np.sign(r), np.clip(r, -0.6, 0.6))
	if not edges:  # guard cases: a middle class with ln P in (-60, -20), and no P among the subnormals of either type (strong pairs: far below, the rest: far above)
		mid = (rng.random((ny, nx)) < 0.1) & ~strong
		lp = rng.uniform(20.0, 60.0, (ny, nx))
		r = np.where(mid, np.sqrt(-np.expm1(-lp / a)) * np.sign(r), r)
		r = np.where(~strong & ~mid, np.clip(r, -0.05, 0.05), r)
		if a * math.log1p(-0.75**2) > -800:
			r = np.where(strong, 0.0, r)
	plants = {}
	if edges and dxx.size > 2:
		dxx[2] = 0.0
	vx = np.where(dxx == 0, 1.0, dxx)
	targets = dict(p_one=1e-12, p_1e30=-math.expm1(-69.08 / a), p_sub32=-math.expm1(-103.3 / a), p_sub64=-math.expm1(-744.4 / a), p_zero=1 - 1e-15)
	spots = [(i, j) for i in (0, nx - 1, min(63, nx - 1), min(64, nx - 1)) for j in (ny - 1, 0, min(63, ny - 1), min(64, ny - 1))]
	spots = list(dict.fromkeys(spots))
	for (name, r2), (i, j) in zip(targets.items(), spots if edges else []):
		r[j, i] = math.sqrt(min(r2, 1 - 1e-15))
		plants[name] = (i, j)
	r2 = r * r
	expl = r2 / (1 - r2) * (rs / n)[:, None]
	bt = rng.normal(size=(ny, m))
	bt[:, :nx] = np.sign(r) * np.sqrt(expl / vx[None, :])
	pt = bt * n * rng.uniform(0.5, 2.0, (ny, m)) + rng.normal(size=(ny, m)) * math.sqrt(n) * 0.1  # (P = Y A^T and B = P N: sum_k P B > 0, with some cancellation)
	special = {}
	if edges and ny >= 8 and nx >= 3:
		g = 5  # rss three ulps below zero: one exact product 3 x 5, nothing else
		bt[g] = 0.0
		pt[g] = 0.0
		pt[g, 0], bt[g, 0] = 3.0, 5.0
		special['ulps'] = g
	acc = np.asarray((ld(pt) * ld(bt)).sum(axis=1), dtype=F64)
	yy = acc + rs
	if 'ulps' in special:
		yy[special['ulps']] = np.nextafter(np.nextafter(np.nextafter(15.0, 0.0), 0.0), 0.0)
	if edges and ny >= 8 and nx >= 3:
		g = 6  # R^2 = 2 on grouping 1: rss = -n expl / 2
		e = bt[g, 1]**2 * vx[1]
		yy[g] = acc[g] - 0.5 * n * e
		special['r2'] = g
		bt[3, nx - 1] = np.nan  # (enters gene 3's rss too: the whole gene is non-finite)
		bt[4, 0] = np.inf
		special['nan'], special['inf'] = 3, 4
	return SweepProblem(nx=nx, ny=ny, m=m, n=n, dof=float(dof), bt=bt, pt=pt, yy=yy, dxx=dxx, plants=plants, special=special)


def rss(pb):
	with np.errstate(invalid='ignore', over='ignore'):
		t = ld(pb.pt) * ld(pb.bt)
		acc, ab = t.sum(axis=1), np.abs(t).sum(axis=1)
		out = ld(pb.yy) - acc
		depth = -(-pb.m // 64) + 6
		return dict(rss=out, bound=SLACK * U * (depth * ab + np.abs(out)) + OWN * (ab + np.abs(ld(pb.yy))))


def judge_values(got, want, bound, what):
	"""|got - want| / bound where want is finite; elsewhere got must be non-finite in the same way (NaN for NaN, the same infinity)."""
	g, w = ld(got), ld(want)
	fin = np.isfinite(w)
	with np.errstate(invalid='ignore'):
		err = np.where(fin, np.abs(g - w), np.where(np.isnan(w), np.where(np.isnan(g), 0, np.inf), np.where(g == w, 0, np.inf)))
		err = np.where(fin & ~np.isfinite(g), np.inf, err)
	return worst(err, np.where(fin, bound, 0), what)


def thread_count(flagged):
	"""Threads of k_s4_sweep (module docstring) that hold a flagged pair; flagged: (nx, ny)."""
	nx, ny = flagged.shape
	cnt = 0
	for b0 in range(0, nx, 64):
		blk = flagged[b0:b0 + 64]
		for ty in range(4):
			cnt += int(blk[ty::4].any(axis=0).sum())
	return cnt


def sweep(pb, rs, return_dot, dtype):
	"""Every pair in longdouble from the rss the call computed (rs, fp64): out and bound in the output layout (nx, ny); the counters by the kernel's rule;
	`undecided`: pairs whose flag class is within their bound (must be 0 in the cases of the GPU file)."""
	n = LD(pb.n)
	g = ld(pb.bt[:, :pb.nx]).T
	vx = ld(np.where(pb.dxx == 0, 1.0, pb.dxx))[:, None]
	rs = ld(rs)[None, :]
	with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
		expl = g * g * vx
		vy = rs / n + expl
		r2 = expl / vy
		stat = g * vx if return_dot else g
		d_expl = 2 * U * np.abs(expl)
		d_vy = U * np.abs(rs / n) + d_expl + U * np.abs(vy)
		room = np.abs(vy) - d_vy
		d_r2 = np.where(room > 0, (d_expl + np.abs(r2) * d_vy) / room, np.inf) + U * np.abs(r2)
		d_stat = (U * np.abs(stat)) if return_dot else np.zeros_like(stat)
		own = lambda v: OWN * np.abs(v)
		b = dict(vary=SLACK * d_vy + own(vy) + own(expl), r2=SLACK * d_r2 + own(r2), stat=SLACK * d_stat + own(stat))
		if np.dtype(dtype) == F32:
			for k, v in (('vary', vy), ('stat', stat)):
				b[k] = b[k] + 2.0**-24 * np.abs(v) + 2.0**-150
		nf = ~np.isfinite(r2) | ~np.isfinite(vy)
		rng = (r2 > 1.0 + 1e-8) | (vy < 0)
		fin = np.isfinite(r2) & np.isfinite(vy)
		und = fin & ((np.abs(r2 - (1.0 + 1e-8)) <= 4 * d_r2) | ((np.abs(vy) <= 4 * d_vy)))
	return dict(out=dict(vary=vy, r2=r2, stat=stat), bound=b, flags=(thread_count(nf), thread_count(rng)), nf=nf, rng=rng, undecided=int(und.sum()),
				p_ok=fin & (vy > 0) & (r2 >= 0) & (r2 <= 1))


def judge_sweep(outs, pb, ref, dtype):
	"""outs: 'p', 'stat', 'vary' as (nx, ny).  Every pair's stat and vary; P of the planted pairs and a spread of ln P against mpmath."""
	ws = {k: judge_values(outs[k], ref['out'][k], ref['bound'][k], k) for k in ('stat', 'vary')}
	ok = ref['p_ok']
	sub = SweepProblem(nx=pb.nx, ny=pb.ny, dof=pb.dof, plants={k: v for k, v in pb.plants.items() if ok[v]})
	sub.pairs = lambda: ok
	with np.errstate(invalid='ignore'):
		r2 = np.where(ok, np.asarray(ref['out']['r2'], dtype=F64), 0.0)
		dr2 = np.where(ok, np.asarray(ref['bound']['r2'], dtype=F64), 0.0)
	ws['p mpmath'] = k3.compare_p_subset(outs['p'], sub, r2, dtype, d_r2=dr2)
	p = np.asarray(outs['p'], dtype=F64)
	with np.errstate(invalid='ignore'):
		in01 = np.where(ok, (p >= 0) & (p <= 1), True)
	ws['p range'] = Worst(0.0 if in01.all() else np.inf, None, 'every P of a finite in-range pair in [0, 1]')
	return ws


def emu_sweep(pb, rs, return_dot, dtype, mutate=None):
	"""k_s4_sweep in fp64, statement by statement (P is not emulated): vary, stat, r2 as (nx, ny) and the two counters, counted per thread."""
	g = pb.bt[:, :pb.nx].T.copy()
	if mutate == 'transposed' and pb.nx == pb.ny:
		g = g.T.copy()
	if mutate == 'edge' and pb.m > pb.nx:  # (gi <= nx: the last tile column reads one coefficient further)
		g[pb.nx - 1] = pb.bt[:, pb.nx]
	vx = pb.dxx.copy()[:, None]
	if mutate != 'vx0':
		vx = np.where(vx == 0, 1.0, vx)
	with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
		expl = g * g * vx
		vy = rs[None, :] / float(pb.n) + expl
		r2 = expl / vy
		nf = ~np.isfinite(r2) | ~np.isfinite(vy)
		rng = (r2 > 1.0 + 1e-8) | (vy < 0)
		stat = (g * vx) if (bool(return_dot) != (mutate == 'return_dot')) else g
	return dict(vary=vy.astype(dtype), stat=stat.astype(dtype), r2=r2, flags=(thread_count(nf), thread_count(rng)))


def emu_rss(pb, mutate=None):
	"""k_s4_rss: a lane's fma chain over k = lane, lane + 64, ..; the wave's sum (a tree here); yy - acc."""
	m = pb.m - (1 if mutate == 'edge' else 0)
	cols = -(-m // 64) * 64
	p, b = np.zeros((pb.ny, cols)), np.zeros((pb.ny, cols))
	p[:, :m], b[:, :m] = pb.pt[:, :m], pb.bt[:, :m]
	acc = np.zeros((pb.ny, 64))
	with np.errstate(invalid='ignore', over='ignore'):
		for c in range(0, cols, 64):
			acc = fma64(p[:, c:c + 64], b[:, c:c + 64], acc)
		return pb.yy - _tree(acc)


# ---- the guard ---------------------------------------------------------------------------------------------------------------------------------------------------
def k_const(ns):
	return sum((w + 1) * 256.0**w for w in range(ns - 1))


@functools.lru_cache(maxsize=None)
def guard_case(name):
	"""(problem, fy records (ny, 8), kappa (nx), cstar, gstar, ns, budget): a clean sweep problem (no edge values) at 70 x 130, records of two kinds -- small c and g (dr below 0.1: a zero P-value stays
	zero at |r| - dr, exempt) and four genes with g of 20 .. 100 (dr above |r|: nothing is exempt) --, kappa uniform(0.5, 2); the budget sits in a gap of the per-pair estimates (choose_budget)."""
	ns = int(name[2:])
	dof = 4093 if ns == 6 else 49990
	pb = sweep_problem(70, 130, 5, dof, edges=False, seed=ns)
	rng = np.random.default_rng([51, ns])
	fy = np.zeros((pb.ny, STRIDE))
	fy[:, :5] = rng.normal(size=(pb.ny, 5))
	fy[:, 5] = 10.0**rng.uniform(-9, -8, pb.ny)
	fy[:, 6] = 10.0**rng.uniform(-9, -5, pb.ny)
	big = [7, 63, 64, 129]  # genes whose every pair is far over any budget: |r| - dr < 0, so a zero P-value is not exempt
	fy[big, 6] = rng.uniform(20.0, 100.0, len(big))
	fy[:, 7] = 1.0
	kappa = rng.uniform(0.5, 2.0, pb.nx)
	cstar, gstar = 1e-6, 1e-7
	est = guard_estimates(pb, np.asarray(rss(pb)['rss'], dtype=F64), fy, kappa, cstar, gstar, ns)
	return pb, fy, kappa, cstar, gstar, ns, choose_budget(est['num_lo'] / est['den'])


def choose_budget(ratio, want_over=700):
	"""A budget in the widest gap of the sorted estimates near the want_over-th largest: no pair within 1e-3 of it (k3_reference.choose_budget)."""
	v = np.sort(np.asarray(ratio, dtype=F64).ravel())[::-1]
	lo, hi = max(want_over // 2, 1), min(2 * want_over, v.size - 1)
	k = lo + int(np.argmax(v[lo:hi] / v[lo + 1:hi + 1]))
	assert v[k] / v[k + 1] > 1.002
	return float(np.sqrt(v[k] * v[k + 1]))


def guard_estimates(pb, rs, fy, kappa, cstar, gstar, ns, factor=2):
	n, dof = LD(pb.n), LD(pb.dof)
	ref = sweep(pb, rs, 0, F64)
	vy, r2 = ref['out']['vary'], ref['out']['r2']
	ey = factor * (LD(k_const(ns)) * ld(fy[:, 5]) * LD(cstar) + ld(fy[:, 6]) + LD(gstar)) * np.sqrt(ld(pb.yy) / n)
	dr = ey[None, :] * ld(kappa)[:, None] / np.sqrt(vy)
	ar = np.sqrt(r2)
	den = np.maximum(1 - r2, LD(1e-150))**2
	return dict(dr=dr, ar=ar, den=den, num_lo=dr * (dof * ar + np.sqrt(dof)), num_hi=dr * (dof * ar * (1 + LD(4e-7)) + np.sqrt(dof)), r2=r2)


def guard(pb, rs, fy, kappa, cstar, gstar, ns, budget, dtype):
	"""The classes, the interval of flags[2], the genes that must / must not be in gene_hits and the interval of flags[3] (module docstring)."""
	e = guard_estimates(pb, rs, fy, kappa, cstar, gstar, ns)
	over = e['num_lo'] > budget * e['den'] * (1 + LD(1e-9))
	under = e['num_hi'] < budget * e['den'] * (1 - LD(1e-9))
	undecided = int((~over & ~under).sum())
	counted, exempt, unsure = np.zeros(over.shape, dtype=bool), np.zeros(over.shape, dtype=bool), np.zeros(over.shape, dtype=bool)
	for i, j in np.argwhere(over):
		c = k3._nonzero_class(float(e['r2'][i, j]), pb.dof, dtype)
		if c > 0:
			counted[i, j] = True
		elif c == 0:
			unsure[i, j] = True
		else:
			lo = [max(float(e['ar'][i, j] * f - e['dr'][i, j]), 0.0)**2 for f in (LD(1), 1 + LD(4e-7))]
			cs = {k3._nonzero_class(v, pb.dof, F64) for v in lo}
			if cs == {-1}:
				exempt[i, j] = True
			elif cs == {1}:
				counted[i, j] = True
			else:
				unsure[i, j] = True
	undecided += int(unsure.sum())
	ratio = e['num_lo'] / e['den']
	w_lo = float(ratio[under].max()) * (1 - 1e-5) if under.any() else 0.0
	w_hi = float((e['num_hi'] / e['den'])[~over].max()) * (1 + 1e-5) if (~over).any() else 0.0
	maybe = counted | unsure | (~over & ~under)
	return dict(over=over, under=under, counted=counted, exempt=exempt, undecided=undecided, hits=(int(counted.sum()), int(maybe.sum())), worst=(w_lo, w_hi),
				must=np.nonzero(counted.any(axis=0))[0], must_not=np.nonzero(~maybe.any(axis=0))[0], ratio=ratio)


def check_guard(flags, prefill, hits, g):
	"""flags[2] and flags[3] within their intervals, gene_hits (or None) holding the must-set and none of the must-not set: Worst records."""
	h = int(flags[2]) - int(prefill)
	wf = float(np.asarray(flags[3], dtype=np.int32).view(np.float32))
	ws = dict(hits=Worst(0.0 if g['hits'][0] <= h <= g['hits'][1] else np.inf, None, 'hits %d in [%d, %d]' % ((h, ) + g['hits'])),
			  worst=Worst(0.0 if g['worst'][0] <= wf <= g['worst'][1] else np.inf, None, 'worst %.9g in [%.9g, %.9g]' % ((wf, ) + g['worst'])))
	if hits is not None:
		okay = (hits[g['must']] == 1).all() and (hits[g['must_not']] == 0).all() and np.isin(hits, (0, 1)).all()
		ws['gene_hits'] = Worst(0.0 if okay else np.inf, None, 'gene_hits: %d genes must be set, %d must not' % (len(g['must']), len(g['must_not'])))
	return ws


def emu_guard(pb, rs, fy, kappa, cstar, gstar, ns, budget, dtype, p_stored, mutate=None):
	"""The guard block of k_s4_sweep in fp64 (float for |r| and the diagnostic quotient); P at lo^2 by mpmath's class.  p_stored: (nx, ny) in dtype.
	Mutations: 'factor' (e_y without its 2), 'exemption' (every over pair counted), 'axis' (gene_hits indexed by the grouping), 'worst-all' (flags[3] over the
	counted pairs too)."""
	e = emu_sweep(pb, rs, 0, F64)
	vy, r2 = e['vary'], e['r2']
	ey = (1.0 if mutate == 'factor' else 2.0) * (k_const(ns) * fy[:, 5] * cstar + (fy[:, 6] + gstar)) * np.sqrt(pb.yy / float(pb.n))
	dr = ey[None, :] * kappa[:, None] * (1.0 / np.sqrt(vy))
	ar = (np.sqrt(r2.astype(F32)) * F32(1.0000002)).astype(F64)
	om = np.fmax(1.0 - r2, 1e-150)
	num, den = dr * (pb.dof * ar + math.sqrt(pb.dof)), om * om
	over = (num > budget * den) | np.isnan(num)
	hits = np.zeros(max(pb.ny, pb.nx), dtype=np.int32)
	bad = 0
	counted = np.zeros(over.shape, dtype=bool)
	for i, j in np.argwhere(over):
		lo = max(ar[i, j] - dr[i, j], 0.0)
		if mutate == 'exemption' or p_stored[i, j] != 0 or k3._nonzero_class(lo * lo, pb.dof, F64) > 0:
			bad += 1
			counted[i, j] = True
			hits[i if mutate == 'axis' else j] = 1
	take = ~over | (counted if mutate == 'worst-all' else False)
	w = (num.astype(F32) / den.astype(F32))[take].max() if take.any() else F32(0)
	return dict(flags2=bad, flags3=np.asarray(F32(w)).view(np.int32), hits=hits[:pb.ny])
