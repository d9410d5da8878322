"""The integer Gram kernel with the ragged last tile column folded into the diagonal tiles (csrc/nrm_gram_i8.hip, gram_plan_fold): a symmetric
whole-matrix launch whose last tile column holds 1 to 32 valid columns computes tile (i, last) on the two waves of diagonal tile (i, i) that lie
below the diagonal.  Kernel level (nrm_quantize_rows + nrm_gram_i8_band) against the Python-integer model of the kept digit products that
tests/test_gpu_round2.py::test_integer_gram_is_exact_for_its_fixed_point_operands uses, with the same bound; NRM_DEBUG=gram_fold=0 is the
schedule without the fold, compared entry by entry; and one public call."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import oracle
from test_gpu_parity import I8_FLOOR, close, p_close

pytestmark = pytest.mark.gpu

BOUND = 1e-15  # of |a_i||a_j|: one fp64 rounding per piece of a tile cut along the cells (the existing exactness test's bound)


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd.engine import get_engine
	return get_engine()


@contextmanager
def fold_switch(on):
	"""NRM_DEBUG gram_fold=0 (the library reads it at every launch) for the schedule without the fold; other keys are kept."""
	old = os.environ.get('NRM_DEBUG')
	keep = [p for p in (old or '').split(',') if p.strip() and not p.strip().lower().startswith('gram_fold=')]
	os.environ['NRM_DEBUG'] = ','.join(keep + ([] if on else ['gram_fold=0']))
	try:
		yield
	finally:
		if old is None:
			del os.environ['NRM_DEBUG']
		else:
			os.environ['NRM_DEBUG'] = old


def rows_with_specials(rng, ng, n, kp, v):
	"""ng rows of n cells (padded to a multiple of 128 rows, kp cells) of widely different scales; an all-zero row, a row with one entry of 1e12 and
	a 1 %-dense 0/1 row among the rows of the first tile (host rows) and, as far as v allows, among the last v rows."""
	mp = (ng + 127) // 128 * 128
	a = np.zeros((mp, kp))
	a[:ng, :n] = rng.standard_normal((ng, n)) * np.exp(rng.normal(size=(ng, 1)) * 3) + 0.5 * rng.standard_normal((1, n))
	def special(row, kind):
		a[row] = 0
		if kind == 1:
			a[row, 17 % n] = 1e12
		elif kind == 2:
			a[row, :n] = np.where(rng.random(n) < 0.01, 1.0, 0.0)
			a[row, 3] = 1.0
	zero_rows = [5]
	special(5, 0)
	special(70, 1)
	special(100, 2)
	last = list(range(ng - v, ng))
	kinds = [2, 0, 1] if v >= 3 else ([2, 0] if v == 2 else [2])
	for row, kind in zip(last[::-1], kinds):
		special(row, kind)
		if kind == 0:
			zero_rows.append(row)
	return a, zero_rows


def quantize(eng, a, ns):
	import torch
	from normalisr_amd import _lib
	lib = eng.lib
	mp, kp = a.shape
	d_a = torch.from_numpy(a).cuda()
	q = torch.empty(int(lib.nrm_quant_bytes(mp, kp, ns)), dtype=torch.uint8, device='cuda')
	ex = torch.empty(mp, dtype=torch.int32, device='cuda')
	_lib.check(lib.nrm_quantize_rows(d_a.data_ptr(), mp, kp, kp, ns, q.data_ptr(), ex.data_ptr(), 0, 0, eng._stream()))
	return q, ex


def gram(eng, q, ex, mp, kp, ns, ng, work, fold=True):
	"""The symmetric launch over the whole matrix; untouched entries stay NaN."""
	import torch
	from normalisr_amd import _lib
	dot = torch.full((mp, mp), float('nan'), dtype=torch.float64, device='cuda')
	with fold_switch(fold):
		_lib.check(eng.lib.nrm_gram_i8_band(q.data_ptr(), ex.data_ptr(), 0, q.data_ptr(), ex.data_ptr(), 0, mp, mp, kp, ns, dot.data_ptr(), mp, 1, ng, ng, 0,
											mp, work.data_ptr(), eng._stream()))
	return dot.cpu().numpy()


def workspace(eng):
	import torch
	return torch.empty(int(eng.lib.nrm_gram_workspace_bytes()) // 8, dtype=torch.float64, device='cuda')


def digit_planes(a, q, ex, ns):
	"""The digits the quantiser wrote, (ns, rows, cells padded to 32), checked against round(x 2^-exp), and the row exponents."""
	mp, kp = a.shape
	nks = (kp + 31) // 32
	e = ex.cpu().numpy().astype(np.int64)
	planes = q.cpu().numpy().view(np.int8).reshape(ns, mp // 32, nks, 32, 2, 16)
	d = np.empty((ns, mp, nks * 32), dtype=np.int64)
	for r in range(32):  # row r of a block: its halves are swapped when (r >> 3) & 1
		rows = planes[:, :, :, r]
		if (r >> 3) & 1:
			rows = rows[:, :, :, ::-1]
		d[:, r::32] = rows.reshape(ns, mp // 32, nks * 32)
	qint = sum(d[s] << (8 * s) for s in range(ns))
	want = np.rint(np.ldexp(np.pad(a, ((0, 0), (0, nks * 32 - kp))), -e[:, None])).astype(np.int64)
	assert np.array_equal(qint, want) and np.abs(d[:-1]).max() <= 128 and np.abs(d[-1]).max() <= 64
	return d, e


def exact_gram(d, e, ng, ns):
	"""sum over the kept digit pairs (s + t >= ns - 1) of 256^(s+t) d_s . d_t in Python integers, rounded once, times 2^(e_i + e_j).  The digit
	products of one weight s + t are summed in fp64 matrix products, which are exact here: at most ns 2^14 cells < 2^53."""
	ref = np.zeros((ng, ng), dtype=object)
	for w in range(ns - 1, 2 * ns - 1):
		pairs = [(s, w - s) for s in range(ns) if 0 <= w - s < ns]
		left = np.hstack([d[s][:ng] for s, _ in pairs]).astype(np.float64)
		right = np.hstack([d[t][:ng] for _, t in pairs]).astype(np.float64)
		m = left @ right.T
		assert np.abs(m).max() < 2.0**53
		ref = ref + m.astype(np.int64).astype(object) * (1 << (8 * w))
	ref = np.array([[float(x) for x in row] for row in ref])  # correctly rounded conversion of the exact integers
	return np.ldexp(ref, e[:ng, None] + e[None, :ng])


# (hosts, valid columns of the last tile column, cells, slices): 136, 264 and 392 genes at every cell count; every v; both NS.  96 cells are
# three k-steps (pieces shorter than the ring), 1000 is no multiple of 32, 16384 + 48 spans two int32 chunks (waves 4 and 5 flush in mid-loop).
# All of them have fewer tiles than workgroups: every tile is cut along the cells, the edge sub-tile travels through the slabs and the fix-up.
CASES = [(h, 8, n, 6) for h in (1, 2, 3) for n in (96, 1000, 16384 + 48)] + [(2, v, 1000, 6) for v in (1, 31, 32)] + \
	[(3, 8, 16384 + 48, 5), (1, 32, 96, 5), (2, 31, 1000, 5), (3, 1, 1000, 5)]


@pytest.mark.parametrize('hosts,v,n,ns', CASES)
def test_integer_gram_fold_is_exact_for_its_fixed_point_operands(eng, hosts, v, n, ns):
	"""Every valid upper-triangle entry within 1e-15 |a_i||a_j| of the exact value of the kept digit products, the last column finite, zero rows exact
	zeros; two runs with the fold bitwise equal; without the fold (NRM_DEBUG gram_fold=0) the same entries within the same bound of each other."""
	rng = np.random.default_rng(1000 * hosts + 10 * v + ns)
	ng, kp = hosts * 128 + v, (n + 15) // 16 * 16
	a, zero_rows = rows_with_specials(rng, ng, n, kp, v)
	mp = a.shape[0]
	q, ex = quantize(eng, a, ns)
	work = workspace(eng)
	got = gram(eng, q, ex, mp, kp, ns, ng, work)
	again = gram(eng, q, ex, mp, kp, ns, ng, work)
	plain = gram(eng, q, ex, mp, kp, ns, ng, work, fold=False)
	d, e = digit_planes(a, q, ex, ns)
	ref = exact_gram(d, e, ng, ns)
	iu = np.triu_indices(ng)
	assert np.isfinite(got[:ng, hosts * 128:ng]).all() and np.isfinite(got[iu]).all() and np.isfinite(plain[iu]).all()
	nrm = np.sqrt((a[:ng]**2).sum(axis=1))
	scale = np.maximum(np.outer(nrm, nrm), 1e-300)
	err = float(np.max(np.abs(got[:ng, :ng] - ref)[iu] / scale[iu]))
	err_plain = float(np.max(np.abs(plain[:ng, :ng] - ref)[iu] / scale[iu]))
	diff = float(np.max(np.abs(got[:ng, :ng] - plain[:ng, :ng])[iu] / scale[iu]))
	print('hosts %d v %d cells %d ns %d: fold %.2e, no fold %.2e, fold against no fold %.2e' % (hosts, v, n, ns, err, err_plain, diff))
	assert err < BOUND and err_plain < BOUND and diff < BOUND
	for z in zero_rows:
		assert (got[z, z:ng] == 0).all() and (got[:z + 1, z] == 0).all()
	assert np.array_equal(got, again, equal_nan=True)


@pytest.mark.parametrize('ng', [128 + 33, 256 + 33, 256])
def test_integer_gram_fold_leaves_other_last_columns_alone(eng, ng):
	"""33 valid columns in the last tile column, or a full one: the launch is the one NRM_DEBUG gram_fold=0 gives -- the same entries written (the
	others keep their NaN fill), bit for bit -- and exact as before."""
	ns, n = 6, 1000
	rng = np.random.default_rng(ng)
	kp = (n + 15) // 16 * 16
	a, zero_rows = rows_with_specials(rng, ng, n, kp, 3)
	mp = a.shape[0]
	q, ex = quantize(eng, a, ns)
	work = workspace(eng)
	got = gram(eng, q, ex, mp, kp, ns, ng, work)
	plain = gram(eng, q, ex, mp, kp, ns, ng, work, fold=False)
	assert np.array_equal(got, plain, equal_nan=True)
	d, e = digit_planes(a, q, ex, ns)
	ref = exact_gram(d, e, ng, ns)
	iu = np.triu_indices(ng)
	nrm = np.sqrt((a[:ng]**2).sum(axis=1))
	scale = np.maximum(np.outer(nrm, nrm), 1e-300)
	assert np.isfinite(got[iu]).all() and float(np.max(np.abs(got[:ng, :ng] - ref)[iu] / scale[iu])) < BOUND


def tile_order(nt):
	"""Index of tile (ti, tj), ti <= tj, in the symmetric order of csrc/nrm_host_logic.h (gram_tile_coords): 8 x 8 super-blocks on or above the
	diagonal one after another, row-major inside; a diagonal super-block keeps its upper triangle."""
	order, t = {}, 0
	nb = (nt + 7) // 8
	for bi in range(nb):
		h = min(8, nt - bi * 8)
		for bj in range(bi, nb):
			w = min(8, nt - bj * 8)
			for li in range(h):
				for lj in range(li if bi == bj else 0, w):
					order[(bi * 8 + li, bj * 8 + lj)] = t
					t += 1
	assert t == nt * (nt + 1) // 2
	return order


@pytest.mark.parametrize('n', [96, 16384 + 48])
def test_integer_gram_fold_whole_tiles_are_correctly_rounded(eng, n):
	"""23 x 128 + 8 genes x 96 cells: 277 tiles with the fold (300 without), so on 256 workgroups the first 256 are whole pieces of one int32 chunk.
	Sampled entries of the last column whose host is a whole tile, of host diagonal tiles and of their neighbours equal the CORRECTLY ROUNDED exact
	integer bit for bit, as in test_integer_gram_whole_tiles_are_correctly_rounded; where the entry's tile is cut along the cells -- the corner tile,
	tile 276 of 277, always is -- the pieces are added in fp64 and the entry is held to 1e-15 |a_i||a_j|.  Without the fold the same:
	entries whole in both runs are bit-identical between the runs, all others agree within that bound.
	16384 + 48 cells: a whole piece is two int32 chunks (the small shapes above are cut into pieces far shorter than a chunk, so this is where waves
	4 and 5 flush in mid-loop); its entry is the correctly rounded value of the first 16 384 cells plus that of the rest, one fp64 addition -- bit for bit."""
	import torch
	ns, lead, v = 6, 23, 8
	ng, mp = lead * 128 + v, (lead + 1) * 128
	nwg = torch.cuda.get_device_properties(0).multi_processor_count
	nwg -= nwg % 8
	assert nwg == 256, 'this shape is cut for one workgroup on each of 256 compute units'
	rng = np.random.default_rng(79)
	a = np.zeros((mp, n))
	a[:ng] = rng.standard_normal((ng, n), dtype=np.float32)
	a[:ng] = a[:ng] * np.exp(rng.normal(size=(ng, 1))) + 0.3 * rng.standard_normal((1, n))
	q, ex = quantize(eng, a, ns)
	work = workspace(eng)
	got = gram(eng, q, ex, mp, n, ns, ng, work)
	again = gram(eng, q, ex, mp, n, ns, ng, work)
	plain = gram(eng, q, ex, mp, n, ns, ng, work, fold=False)
	assert np.array_equal(got, again, equal_nan=True)
	e = ex.cpu().numpy().astype(np.int64)
	def digits_of(row, cache={}):  # the balanced radix-256 digits of one row's fixed-point integers
		if row not in cache:
			x = np.rint(np.ldexp(a[row], -e[row])).astype(np.int64)
			out = []
			for s in range(ns):
				dg = x.copy() if s == ns - 1 else ((x & 0xff) ^ 0x80) - 0x80
				x = (x - dg) >> 8
				out.append(dg)
			cache[row] = out
		return cache[row]
	chunks = [(c, min(c + 16384, n)) for c in range(0, n, 16384)]  # cells per int32 accumulation chunk
	on, off = tile_order(lead), tile_order(lead + 1)
	def whole_on(ti, tj):  # the piece that computes tile (ti, tj) with the fold: the host's for the last column, nobody's whole for the corner
		return on[(ti, ti)] < nwg if tj == lead and ti < lead else (tj < lead and on[(ti, tj)] < nwg)
	def whole_off(ti, tj):
		return off[(ti, tj)] < nwg
	pick = []
	hosts_whole = [i for i in range(lead) if whole_on(i, lead)]
	hosts_cut = [i for i in range(lead) if not whole_on(i, lead)]
	assert len(hosts_whole) >= 8 and hosts_cut  # both kinds of host exist at this shape
	for i in hosts_whole[:6] + hosts_whole[-3:] + hosts_cut[:2]:
		for _ in range(8):
			pick.append((i * 128 + int(rng.integers(0, 128)), lead * 128 + int(rng.integers(0, v))))  # the last column
			r, c = sorted(int(z) for z in rng.integers(0, 128, 2))
			pick.append((i * 128 + r, i * 128 + c))  # the host itself (upper triangle)
			if i + 1 < lead:
				pick.append((i * 128 + int(rng.integers(0, 128)), (i + 1) * 128 + int(rng.integers(0, 128))))  # its neighbours
			if i > 0:
				pick.append(((i - 1) * 128 + int(rng.integers(0, 128)), i * 128 + int(rng.integers(0, 128))))
	for _ in range(12):
		r, c = sorted(int(z) for z in rng.integers(0, v, 2))
		pick.append((lead * 128 + r, lead * 128 + c))  # the corner tile
	nrm = np.sqrt((a**2).sum(axis=1))
	exact_hits = 0
	for i, j in pick:
		di, dj = digits_of(i), digits_of(j)
		want = 0.0
		for c0, c1 in chunks:
			exact = 0
			for s in range(ns):
				for t in range(ns):
					if s + t >= ns - 1:
						exact += int(np.dot(di[s][c0:c1], dj[t][c0:c1])) << (8 * (s + t))
			want = want + float(np.ldexp(float(exact), int(e[i] + e[j])))
		ti, tj = i // 128, j // 128
		if whole_on(ti, tj):
			assert got[i, j] == want, ('fold', i, j, float(got[i, j]).hex(), want.hex())
			exact_hits += tj == lead
		else:
			assert abs(got[i, j] - want) < BOUND * nrm[i] * nrm[j], ('fold', i, j)
		if whole_off(ti, tj):
			assert plain[i, j] == want, ('no fold', i, j)
		else:
			assert abs(plain[i, j] - want) < BOUND * nrm[i] * nrm[j], ('no fold', i, j)
	assert exact_hits >= 60
	# the two schedules against each other, every valid upper-triangle entry
	wo = np.zeros((lead + 1, lead + 1), dtype=bool)
	for ti in range(lead + 1):
		for tj in range(ti, lead + 1):
			wo[ti, tj] = whole_on(ti, tj) and whole_off(ti, tj)
	both = np.kron(wo, np.ones((128, 128), dtype=bool))[:ng, :ng]
	iu = np.triu(np.ones((ng, ng), dtype=bool))
	g, p = got[:ng, :ng], plain[:ng, :ng]
	assert np.isfinite(g[iu]).all() and np.isfinite(p[iu]).all()
	assert (both & iu).sum() > 0.7 * iu.sum() and np.array_equal(g[both & iu], p[both & iu])
	rest = iu & ~both
	assert float(np.max(np.abs(g - p)[rest] / np.outer(nrm[:ng], nrm[:ng])[rest])) < BOUND


def test_integer_gram_fold_through_the_public_call(eng, monkeypatch):
	"""association_tests (coex) on 264 genes x 2100 cells -- enough cells for the integer engine, two hosts and 8 columns in the last tile column -- with
	3 covariates: P-values and statistics against the oracle at the tolerances of test_gram_engines_on_config1_shape, nothing left uncertified.
	That the call ran the folded schedule is pinned at the library's entry: one nrm_gram_i8_band launch, symmetric, one operand on both sides, the whole
	matrix, 264 valid rows of 384 -- and the same launch repeated into a NaN-filled matrix leaves columns 32-127 of the last tile column untouched in the
	host rows: only the 32-column edge block is stored there, where the schedule without the fold writes whole 128 x 128 tiles from its slabs."""
	import torch
	from normalisr_amd.association import association_tests
	monkeypatch.setenv('NRM_GRAM', 'i8')
	real, launches, probes = eng.lib.nrm_gram_i8_band, [], []
	def spy(*args):
		rc = real(*args)
		launches.append(args)
		if rc == 0 and not probes:  # operands still alive: the same launch once more, into a matrix of our own
			m_pad, n_pad, ldd = int(args[6]), int(args[7]), int(args[11])
			probe = torch.full((m_pad, ldd), float('nan'), dtype=torch.float64, device='cuda')
			assert real(*(args[:10] + (probe.data_ptr(), ) + args[11:])) == 0
			torch.cuda.synchronize()
			probes.append(probe.cpu().numpy()[:, :n_pad])
		return rc
	monkeypatch.setattr(eng.lib, 'nrm_gram_i8_band', spy)
	rng = np.random.default_rng(2021)
	ng, n = 264, 2100
	dt = rng.normal(size=(ng, n)) * rng.uniform(0.3, 3, (ng, 1)) + 0.3 * rng.normal(size=(ng, 1)) * rng.normal(size=(1, n)) + 5
	dc = np.vstack([rng.normal(size=(2, n)), np.ones((1, n))])
	po, do, ao, vxo, vo = oracle.association_tests(dt, None, dc)
	res = association_tests(dt, None, dc, return_stats=True)
	p, d, st = res[0], res[1], res[5]
	assert eng.gram_slices(n) == 6
	assert len(launches) == 1 and len(probes) == 1
	qa, ea, pa, qb, eb, pb, m_pad, n_pad, k_pad, nsl, _, _, sym, m_rows, n_rows, row0, row1 = launches[0][:17]
	assert (qa, ea, pa) == (qb, eb, pb) and (m_pad, n_pad, nsl, sym, m_rows, n_rows, row0, row1) == (384, 384, 6, 1, ng, ng, 0, 384)
	probe = probes[0]
	assert np.isfinite(probe[:256, 256:ng]).all()
	assert np.isnan(probe[:256, 288:]).all()
	assert not eng.last_guard['fallback'] and eng.last_guard['hits'] == 0
	sc = np.sqrt(np.outer(vo, vo))
	assert p_close(p, po) and close(d / sc, do / sc, floor=I8_FLOOR) and close(res[4], vo, 1e-12)
	ro, to = oracle.pearson_r_t(do, vo, vo, st['dof'])
	off = ~np.eye(ng, dtype=bool)
	assert close(st['r'][off], ro[off], floor=I8_FLOOR) and close(st['t'][off], to[off], floor=I8_FLOOR * 100)
	assert (np.diag(p) == 0).all() and (p == p.T).all() and (d == d.T).all()
	again = association_tests(dt, None, dc, return_stats=True)
	assert np.array_equal(again[0], p) and np.array_equal(again[1], d)
