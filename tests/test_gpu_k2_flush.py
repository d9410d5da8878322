"""The flush of the integer Gram kernel (csrc/nrm_gram_i8.hip): a tile's int32 accumulator sets are combined in fp64, scaled by the row exponents and
stored, or added to what is there, in one burst per 32 x 32 sub-tile.  Kernel level (nrm_gram_i8_band / nrm_gram_i8_chunk on digit planes and row
exponents drawn here, no quantiser), every output compared BIT FOR BIT with the Python-integer model tests/test_gpu_k2_refill.py uses -- the kept
digit pairs summed exactly, each int32 chunk of 512 k-steps rounded once, the chunks of a piece added in fp64 in order -- carried through the
schedule: a tile cut along the cells is the fp64 sum of its pieces in the fix-up's order (tests/s4_reference.py ports the schedule).
Each case is the smallest shape that reaches one path of the flush: the plain store of whole tiles into C (as many tiles as workgroups), the slab
path and the fix-up (1, 2 and 3 tile columns; 264 rows fold the last column into a host tile, 300 rows are too wide to fold), the flush in
mid-piece and the read-modify-write body (513 k-steps), an accumulating chunk call, operand B as gathered blocks; one case is run twice."""
import numpy as np
import pytest

import s4_reference as ref

pytestmark = pytest.mark.gpu

QCHUNK = 512  # k-steps per int32 accumulation chunk (csrc/nrm_gram_i8.hip)


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd.engine import get_engine
	return get_engine()


def n_workgroups():
	import torch
	return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Operand:
	"""Random digit planes in the kernel's tiled layout (plane s, 32-row block, k-step: one 1 KB image [row][2 halves][16 bytes], the halves of row r
	swapped when (r >> 3) & 1), drawn on the device, and random row exponents.  Digits in [-128, 127], the top digit within +-64; padded rows hold
	digits like any other (nothing of them may reach a valid output).  Every shape here is whole k-steps of 32 cells."""

	def __init__(self, rows_pad, cells, ns, seed):
		import torch
		g = torch.Generator(device='cuda').manual_seed(seed)
		self.ns, self.rows, self.cells, self.nks = ns, rows_pad, cells, (cells + 31) // 32
		shape = (rows_pad // 32, self.nks, 32, 2, 16)
		self.planes = torch.empty((ns, ) + shape, dtype=torch.int8, device='cuda')
		for s in range(ns):
			top = 64 if s == ns - 1 else 128
			self.planes[s] = torch.randint(-top, top, shape, dtype=torch.int8, device='cuda', generator=g)
		assert cells % 32 == 0  # (every shape here is whole k-steps)
		self.exps = torch.randint(-40, 20, (rows_pad, ), dtype=torch.int32, device='cuda', generator=g)
		self.e = self.exps.cpu().numpy().astype(np.int64)
		self.plane_bytes = (rows_pad // 32) * self.nks * 1024

	def digits(self, rows):
		"""The digits of the given rows, (ns, len(rows), nks * 32) as float64 (exact)."""
		import torch
		rows = np.asarray(rows)
		idx_b, idx_r = torch.from_numpy(rows // 32).cuda(), torch.from_numpy(rows % 32).cuda()
		x = self.planes.permute(0, 1, 3, 2, 4, 5)[:, idx_b, idx_r].cpu().numpy()  # (ns, n, nks, 2, 16)
		flip = ((rows % 32) >> 3 & 1).astype(bool)
		x[:, flip] = x[:, flip][:, :, :, ::-1]
		return x.reshape(self.ns, len(rows), self.nks * 32).astype(np.float64)


def schedule(m_pad, n_pad, nkt, symmetric, m_rows, n_rows, may_fold):
	"""gram_plan / gram_plan_fold (csrc/nrm_host_logic.h) on this device's workgroup count, and the pieces of every tile in the order they are added."""
	s = ref.gram_schedule(m_pad, n_pad, nkt, symmetric, m_rows, n_rows, 0, m_pad, n_workgroups())
	ntn = s['ntn']
	if may_fold and symmetric and ntn >= 2 and s['ntm'] == ntn and 1 <= n_rows - (ntn - 1) * 128 <= 32:
		s['fold'] = ntn - 1
		ref.split_phases(s, (ntn - 1) * ntn // 2 + 1)
	pieces = {}
	for t, plist in ref.tile_map(s).items():
		if s['fold']:
			lead = s['fold']
			ti, tj = ref.tile_coords(t, 1, lead, lead) if t < lead * (lead + 1) // 2 else (lead, lead)
		else:
			ti, tj = ref.tile_coords(s['tile0'] + t, symmetric, s['ntm'], ntn)
		pieces[(ti, tj)] = plist
		if s['fold'] and ti == tj and ti < s['fold']:
			pieces[(ti, s['fold'])] = plist  # the edge tile rides in its host
	return s, pieces


to_float = np.frompyfunc(float, 1, 1)  # Python's int -> float conversion is correctly rounded


def model(da, ea, db, eb, plist, ns, old=None):
	"""The kernel's value for rows `da` against columns `db` (digits (ns, n, cells), exponents) of a tile whose pieces are `plist` [(k0, k1, slab)]:
	per piece, per chunk of QCHUNK k-steps the exact integer sum_w 256^w sum_{s+t=w} d_s . d_t over the kept pairs rounded once and scaled, chunks added
	in order; pieces added in order; `old` (accumulating launch) added the way the kernel adds it."""
	sh = ea[:, None] + eb[None, :]
	def chunk(c0, c1):
		lo, hi = 0, 0  # the weights 0..2 and 3.. above 256^(ns-1) in int64 (each sum below 2^48: exact), joined as Python integers
		for w in range(ns - 1, 2 * ns - 1):
			pairs = [(s, w - s) for s in range(ns) if 0 <= w - s < ns]
			m = np.hstack([da[s][:, c0:c1] for s, _ in pairs]) @ np.hstack([db[t][:, c0:c1] for _, t in pairs]).T  # (exact: below 2^53)
			assert np.abs(m).max() < 2.0**31  # (what an int32 accumulator set holds)
			if w - (ns - 1) < 3:
				lo = lo + (m.astype(np.int64) << (8 * (w - (ns - 1))))
			else:
				hi = hi + (m.astype(np.int64) << (8 * (w - (ns - 1) - 3)))
		tot = hi.astype(object) * (1 << 24) + lo.astype(object)
		return np.ldexp(to_float(tot).astype(np.float64), sh + 8 * (ns - 1))
	whole = len(plist) == 1 and plist[0][2] is None
	total = None
	for k0, k1, _ in plist:
		pv = old if (whole and old is not None) else None  # a whole tile of an accumulating launch adds chunk after chunk to what is there
		for c in range(k0, k1, QCHUNK):
			v = chunk(c * 32, min(c + QCHUNK, k1) * 32)
			pv = v if pv is None else pv + v
		total = pv if total is None else total + pv
	return total if (whole or old is None) else old + total  # (the fix-up adds the sum of the slabs to what is there)


def launch_symmetric(eng, op, ng, ldd, fill=float('nan')):
	import torch
	from normalisr_amd import _lib
	mp = op.rows
	work = torch.empty(int(eng.lib.nrm_gram_workspace_bytes()) // 8, dtype=torch.float64, device='cuda')
	dot = torch.full((mp, ldd), fill, dtype=torch.float64, device='cuda')
	_lib.check(eng.lib.nrm_gram_i8_band(op.planes.data_ptr(), op.exps.data_ptr(), 0, op.planes.data_ptr(), op.exps.data_ptr(), 0, mp, mp, op.cells, op.ns,
										dot.data_ptr(), ldd, 1, ng, ng, 0, mp, work.data_ptr(), eng._stream()))
	torch.cuda.synchronize()
	return dot.cpu().numpy()


def same_bits(a, b):
	return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def check_tile(op, got, pieces, ti, tj, ng, rows, cols):
	"""Entries rows x cols (tile-local indices) of tile (ti, tj) that are valid and on or above the diagonal, bit for bit against the model."""
	ri, cj = ti * 128 + np.asarray(rows), tj * 128 + np.asarray(cols)
	ri, cj = ri[ri < ng], cj[cj < ng]
	want = model(op.digits(ri), op.e[ri], op.digits(cj), op.e[cj], pieces[(ti, tj)], op.ns)
	keep = ri[:, None] <= cj[None, :]
	g = got[np.ix_(ri, cj)]
	assert keep.any() and np.isfinite(g[keep]).all()
	bad = keep & (g.view(np.int64) != want.view(np.int64))
	assert not bad.any(), ('tile', ti, tj, 'entries that differ', int(bad.sum()), 'first', [(int(ri[a]), int(cj[b]), float(g[a, b]).hex(), float(want[a, b]).hex())
																							for a, b in zip(*np.nonzero(bad))][:3])
	return int(keep.sum())


def many_tiles():
	"""The smallest symmetric problem with at least as many tiles as workgroups whose last tile column (40 valid columns) is too wide to fold."""
	nwg = n_workgroups()
	ntn = 2
	while ntn * (ntn + 1) // 2 < nwg - nwg % 8:
		ntn += 1
	return ntn, (ntn - 1) * 128 + 40


def sampled_tiles(ntn, pieces):
	"""Two tiles of each class -- diagonal, off-diagonal, last column -- one stored whole and, where the schedule has one, one cut along the cells; the corner."""
	whole = lambda t: len(pieces[t]) == 1 and pieces[t][0][2] is None
	classes = [[(i, i) for i in range(ntn - 1)], [(i, j) for i in range(ntn - 1) for j in range(i + 1, ntn - 1)], [(i, ntn - 1) for i in range(ntn - 1)]]
	out = [(ntn - 1, ntn - 1)]
	for cl in classes:
		w, c = [t for t in cl if whole(t)], [t for t in cl if not whole(t)]
		out += w[:1] + w[-1:] + c[-1:]
	return sorted(set(out))


@pytest.fixture(scope='module')
def plain_store(eng):
	"""The many-tile launch at 2048 cells into a NaN-filled output of pitch above the minimum, run twice."""
	ntn, ng = many_tiles()
	op = Operand(ntn * 128, 2048, 6, 11)
	ldd = ntn * 128 + 16
	return op, ng, ntn, launch_symmetric(eng, op, ng, ldd), launch_symmetric(eng, op, ng, ldd)


def test_plain_store_of_whole_tiles(plain_store):
	"""64 x 64 sampled entries of diagonal, off-diagonal and last-column tiles (and the corner), whole and cut, against the model."""
	op, ng, ntn, got, _ = plain_store
	s, pieces = schedule(ntn * 128, ntn * 128, op.nks, 1, ng, ng, True)
	assert s['fold'] == 0 and s['tiles_dp'] >= 8  # whole tiles exist: the store into C
	rng = np.random.default_rng(5)
	checked = 0
	for ti, tj in sampled_tiles(ntn, pieces):
		checked += check_tile(op, got, pieces, ti, tj, ng, np.sort(rng.choice(128, 64, replace=False)), np.sort(rng.choice(128, 64, replace=False)))
	assert checked > 64 * 64 * 4


def test_plain_store_writes_what_it_should_and_nothing_else(plain_store):
	"""Whole tiles write exactly their valid 32 x 32 sub-tiles on or above the diagonal (the rest keeps its NaN fill); a tile cut along the cells is
	written by the fix-up as a whole 128 x 128 tile; tiles below the diagonal and the columns of the pitch past the matrix are never touched; diagonal
	sub-tiles, computed in full, are bitwise symmetric; the second run gives the same bytes."""
	op, ng, ntn, got, again = plain_store
	s, pieces = schedule(ntn * 128, ntn * 128, op.nks, 1, ng, ng, True)
	mp = ntn * 128
	assert np.isnan(got[:, mp:]).all()
	blocks = (ng + 31) // 32  # 32-row blocks with a valid row
	for ti in range(ntn):
		for tj in range(ntn):
			tile = got[ti * 128:(ti + 1) * 128, tj * 128:(tj + 1) * 128]
			if tj < ti:
				assert np.isnan(tile).all(), (ti, tj)
				continue
			if not (len(pieces[(ti, tj)]) == 1 and pieces[(ti, tj)][0][2] is None):
				continue
			for a in range(4):
				for b in range(4):
					sub = tile[a * 32:(a + 1) * 32, b * 32:(b + 1) * 32]
					written = ti * 4 + a < blocks and tj * 4 + b < blocks and (ti < tj or b >= a)
					assert (np.isfinite(sub).all() if written else np.isnan(sub).all()), (ti, tj, a, b)
	iu = np.triu_indices(ng)
	assert np.isfinite(got[iu]).all()
	for b in range(blocks):
		sub = got[b * 32:(b + 1) * 32, b * 32:(b + 1) * 32]
		assert same_bits(sub, sub.T), b
	assert same_bits(got[iu], again[iu]) and np.array_equal(np.isnan(got), np.isnan(again))


@pytest.mark.parametrize('ns', [6, 5])
@pytest.mark.parametrize('n', [2048, 2080])
@pytest.mark.parametrize('ng', [128, 264, 300])
def test_slab_path_and_fixup(eng, ng, n, ns):
	"""1, 2 and 3 tile columns: fewer tiles than workgroups, so every tile is cut along the cells and travels through the slabs and k_gram_fixup (264
	rows: the last column's 8 valid columns ride in two host tiles and are routed by the fix-up).  Every valid entry on or above the diagonal."""
	mp = (ng + 127) // 128 * 128
	op = Operand(mp, n, ns, 100 * ng + n + ns)
	got = launch_symmetric(eng, op, ng, mp)
	s, pieces = schedule(mp, mp, op.nks, 1, ng, ng, True)
	assert s['tiles_dp'] == 0 and (s['fold'] > 0) == (ng == 264)
	ntn = mp // 128
	for ti in range(ntn):
		for tj in range(ti, ntn):
			check_tile(op, got, pieces, ti, tj, ng, np.arange(128), np.arange(128))


@pytest.fixture(scope='module')
def mid_piece(eng):
	"""The many-tile launch at 16 416 cells: 513 k-steps, so a whole tile flushes at QCHUNK and once more at the end, adding to what the first stored."""
	ntn, ng = many_tiles()
	op = Operand(ntn * 128, 16416, 6, 12)
	return op, ng, ntn, launch_symmetric(eng, op, ng, ntn * 128)


def test_mid_piece_flush_and_read_modify_write(mid_piece):
	op, ng, ntn, got = mid_piece
	s, pieces = schedule(ntn * 128, ntn * 128, op.nks, 1, ng, ng, True)
	assert op.nks == QCHUNK + 1 and s['tiles_dp'] >= 8
	rng = np.random.default_rng(6)
	for ti, tj in sampled_tiles(ntn, pieces):
		check_tile(op, got, pieces, ti, tj, ng, np.sort(rng.choice(128, 24, replace=False)), np.sort(rng.choice(128, 24, replace=False)))


def test_repeat_gives_identical_bytes(eng, mid_piece):
	"""The same launch again: every byte of the output the same (also what a ring left in a state the next piece misreads would break)."""
	op, ng, ntn, got = mid_piece
	again = launch_symmetric(eng, op, ng, ntn * 128)
	assert np.array_equal(np.isnan(got), np.isnan(again)) and same_bits(got[~np.isnan(got)], again[~np.isnan(again)])


def rect_launch(eng, a, b, dot, m_rows, n_rows, accumulate, blocks=None):
	import torch
	from normalisr_amd import _lib
	work = torch.empty(int(eng.lib.nrm_gram_workspace_bytes()) // 8, dtype=torch.float64, device='cuda')
	if blocks is None:
		qb, eb, n_pad, desc = b.planes, b.exps, b.rows, (0, 0, 0, 1)
	else:
		qb, eb, n_pad, desc = blocks
	_lib.check(eng.lib.nrm_gram_i8_chunk(a.planes.data_ptr(), a.exps.data_ptr(), 0, qb.data_ptr(), eb.data_ptr(), 0, a.rows, n_pad, a.cells, a.ns,
										 dot.data_ptr(), dot.shape[1], 0, m_rows, n_rows, accumulate, *desc, work.data_ptr(), eng._stream()))
	torch.cuda.synchronize()


def test_accumulate(eng):
	"""nrm_gram_i8_chunk over two cell chunks (operands and exponents of their own) of a 256-row rectangular problem: accumulate = 0 overwrites what the
	output held, accumulate = 1 adds the second chunk's value to it.  All entries."""
	import torch
	ns, m, nb = 6, 256, 256
	g = torch.Generator(device='cuda').manual_seed(3)
	dot = torch.randn((m, nb + 8), dtype=torch.float64, device='cuda', generator=g)
	prefill = dot.cpu().numpy()
	old = None
	for c, cells in enumerate((2048, 2080)):
		a, b = Operand(m, cells, ns, 40 + c), Operand(nb, cells, ns, 50 + c)
		rect_launch(eng, a, b, dot, m, nb, c)
		got = dot.cpu().numpy()
		s, pieces = schedule(m, nb, a.nks, 0, m, nb, False)
		rows = np.arange(128)
		for ti in range(2):
			for tj in range(2):
				ri, cj = ti * 128 + rows, tj * 128 + rows
				want = model(a.digits(ri), a.e[ri], b.digits(cj), b.e[cj], pieces[(ti, tj)], ns, None if old is None else old[np.ix_(ri, cj)])
				assert same_bits(got[np.ix_(ri, cj)], want), (c, ti, tj)
		assert same_bits(got[:, nb:], prefill[:, nb:])
		old = got


def test_gathered_b_blocks(eng):
	"""One rectangular launch whose operand B is two blocks of 128 rows of a gathered buffer, visited cyclically from block 1: tile column 0 reads
	block 1, tile column 1 block 0.  200 valid rows of A; all entries."""
	import torch
	ns, cells, m_rows = 6, 2048, 200
	a = Operand(256, cells, ns, 60)
	blk = [Operand(128, cells, ns, 61), Operand(128, cells, ns, 62)]
	stride = ns * blk[0].plane_bytes + 4096
	buf = torch.zeros(2 * stride, dtype=torch.int8, device='cuda')
	for i, o in enumerate(blk):
		buf[i * stride:i * stride + ns * o.plane_bytes] = o.planes.reshape(-1)
	exps = torch.cat([o.exps for o in blk])
	dot = torch.full((256, 256), float('nan'), dtype=torch.float64, device='cuda')
	rect_launch(eng, a, None, dot, m_rows, 256, 0, blocks=(buf, exps, 256, (128, stride, 1, 2)))
	got = dot.cpu().numpy()
	s, pieces = schedule(256, 256, a.nks, 0, m_rows, 256, False)
	for ti in range(2):
		ri = ti * 128 + np.arange(128)
		ri = ri[ri < m_rows]
		for tj in range(2):
			o = blk[(1 + tj) % 2]
			want = model(a.digits(ri), a.e[ri], o.digits(np.arange(128)), o.e, pieces[(ti, tj)], ns)
			assert same_bits(got[np.ix_(ri, tj * 128 + np.arange(128))], want), (ti, tj)
