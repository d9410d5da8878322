"""The refill of the integer Gram kernel (csrc/nrm_gram_i8.hip): every stage image is fetched by an LDS-DMA whose source is a wave-uniform 64-bit
base in scalar registers plus the lane's constant 16 * lane.  A wrong base, plane step or k-step offset lands another image in the ring, so the
check is the contraction itself: kernel level (nrm_quantize_rows + nrm_gram_i8_band / nrm_gram_i8_chunk) against the Python-integer model of the kept
digit products that tests/test_gpu_round2.py::test_integer_gram_is_exact_for_its_fixed_point_operands uses, with the same bound.
Shapes: symmetric launches of 1, 2 and 3 tile columns -- 392 rows give a host tile beside a plain diagonal tile, 300 rows a last column too wide to
fold --, cells a multiple of the k-step and not, both slice counts; one rectangular launch; one accumulating chunk call."""
import numpy as np
import pytest

from test_gpu_gram_fold import BOUND, digit_planes, exact_gram, gram, quantize, rows_with_specials, workspace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd.engine import get_engine
	return get_engine()


def exact_rect(da, ea, db, eb, m, n, ns):
	"""exact_gram for two operands: rows [0, m) of a against rows [0, n) of b."""
	ref = np.zeros((m, n), dtype=object)
	for w in range(ns - 1, 2 * ns - 1):
		pairs = [(s, w - s) for s in range(ns) if 0 <= w - s < ns]
		left = np.hstack([da[s][:m] for s, _ in pairs]).astype(np.float64)
		right = np.hstack([db[t][:n] for _, t in pairs]).astype(np.float64)
		prod = left @ right.T
		assert np.abs(prod).max() < 2.0**53
		ref = ref + prod.astype(np.int64).astype(object) * (1 << (8 * w))
	ref = np.array([[float(x) for x in row] for row in ref])
	return np.ldexp(ref, ea[:m, None] + eb[None, :n])


@pytest.mark.parametrize('ns', [6, 5])
@pytest.mark.parametrize('n', [2048, 2080])
@pytest.mark.parametrize('ng', [128, 200, 300, 392])
def test_symmetric_launch_is_exact_for_its_fixed_point_operands(eng, ng, n, ns):
	"""Every valid upper-triangle entry within 1e-15 |a_i||a_j| of the exact value of the kept digit products (one fp64 rounding per piece of a tile
	cut along the cells), zero rows exact zeros, two runs bitwise equal."""
	rng = np.random.default_rng(7 * ng + n + ns)
	kp = (n + 15) // 16 * 16
	a, zero_rows = rows_with_specials(rng, ng, n, kp, 3)
	mp = a.shape[0]
	q, ex = quantize(eng, a, ns)
	work = workspace(eng)
	got = gram(eng, q, ex, mp, kp, ns, ng, work)
	again = gram(eng, q, ex, mp, kp, ns, ng, work)
	d, e = digit_planes(a, q, ex, ns)
	ref = exact_gram(d, e, ng, ns)
	iu = np.triu_indices(ng)
	assert np.isfinite(got[iu]).all()
	nrm = np.sqrt((a[:ng]**2).sum(axis=1))
	scale = np.maximum(np.outer(nrm, nrm), 1e-300)
	err = float(np.max(np.abs(got[:ng, :ng] - ref)[iu] / scale[iu]))
	print('rows %d cells %d ns %d: %.2e of |a_i||a_j|' % (ng, n, ns, err))
	assert err < BOUND
	for z in zero_rows:
		assert (got[z, z:ng] == 0).all() and (got[:z + 1, z] == 0).all()
	assert np.array_equal(got, again, equal_nan=True)


def test_rectangular_launch_is_exact_for_its_fixed_point_operands(eng):
	"""200 rows against 300 rows of another operand (2 x 3 tiles, the B side with its own planes and exponents), 2080 cells, 6 slices."""
	import torch
	from normalisr_amd import _lib
	ns, n, m, nb = 6, 2080, 200, 300
	rng = np.random.default_rng(31)
	a, _ = rows_with_specials(rng, m, n, n, 3)
	b, _ = rows_with_specials(rng, nb, n, n, 3)
	(qa, ea), (qb, eb) = quantize(eng, a, ns), quantize(eng, b, ns)
	work = workspace(eng)
	mp, np_ = a.shape[0], b.shape[0]
	dot = torch.full((mp, np_), float('nan'), dtype=torch.float64, device='cuda')
	_lib.check(eng.lib.nrm_gram_i8_band(qa.data_ptr(), ea.data_ptr(), 0, qb.data_ptr(), eb.data_ptr(), 0, mp, np_, n, ns, dot.data_ptr(), np_, 0, m, nb, 0, mp,
										work.data_ptr(), eng._stream()))
	got = dot.cpu().numpy()[:m, :nb]
	(da, xa), (db, xb) = digit_planes(a, qa, ea, ns), digit_planes(b, qb, eb, ns)
	ref = exact_rect(da, xa, db, xb, m, nb, ns)
	scale = np.maximum(np.outer(np.sqrt((a[:m]**2).sum(axis=1)), np.sqrt((b[:nb]**2).sum(axis=1))), 1e-300)
	assert np.isfinite(got).all() and float(np.max(np.abs(got - ref) / scale)) < BOUND


def test_chunk_call_accumulates_exactly(eng):
	"""nrm_gram_i8_chunk on two cell chunks of 2048 and 1056 cells (each a dense operand with exponents of its own), the second accumulating: the sum of
	the two chunks' exact values.  Bound: each launch lies within BOUND of its own chunk's |a_i||b_j| and the two chunks' norms add up to at most the whole
	rows' (Cauchy-Schwarz), the accumulation is one more rounding of the sum: 2 BOUND |a_i||b_j| in all."""
	import torch
	from normalisr_amd import _lib
	ns, m, nb = 6, 200, 300
	rng = np.random.default_rng(32)
	work = workspace(eng)
	mp, np_ = 256, 384
	dot = torch.full((mp, np_), float('nan'), dtype=torch.float64, device='cuda')
	ref, sa, sb = 0.0, 0.0, 0.0
	for c, n in enumerate((2048, 1056)):
		a, _ = rows_with_specials(rng, m, n, n, 3)
		b, _ = rows_with_specials(rng, nb, n, n, 3)
		(qa, ea), (qb, eb) = quantize(eng, a, ns), quantize(eng, b, ns)
		_lib.check(eng.lib.nrm_gram_i8_chunk(qa.data_ptr(), ea.data_ptr(), 0, qb.data_ptr(), eb.data_ptr(), 0, mp, np_, n, ns, dot.data_ptr(), np_, 0, m, nb, c, 0,
											 0, 0, 1, work.data_ptr(), eng._stream()))
		torch.cuda.synchronize()
		(da, xa), (db, xb) = digit_planes(a, qa, ea, ns), digit_planes(b, qb, eb, ns)
		ref = ref + exact_rect(da, xa, db, xb, m, nb, ns)
		sa, sb = sa + (a[:m]**2).sum(axis=1), sb + (b[:nb]**2).sum(axis=1)
	got = dot.cpu().numpy()[:m, :nb]
	scale = np.maximum(np.outer(np.sqrt(sa), np.sqrt(sb)), 1e-300)
	assert np.isfinite(got).all() and float(np.max(np.abs(got - ref) / scale)) < 2 * BOUND
