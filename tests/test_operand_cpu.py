"""CPU: the integer engine's operand (engine.Digits inside engine.Residualized) on CPU tensors -- its plane geometry against k1_longdouble.geometry, and
row blocks as views: where they start, what pitch they carry, and that the digits read through that pitch (k1_longdouble.decode_planes, which knows the
layout from csrc/nrm_gram_i8.hip and nothing of the class) are the rows of the whole operand."""
import numpy as np
import pytest
import torch

import k1_longdouble as k1
from normalisr_amd.engine import Digits, Residualized, plane_bytes

SHAPES = [(1026, 256, None), (2050, 128, 1), (2050, 128, 2), (2050, 128, 3), (33, 128, None), (1026, 384, None), (2050, 256, 3)]  # (cells, rows_pad, chunks)


def operand(n, rows_pad, ns, chunks=None, rows=None, seed=0):
	"""A whole-matrix operand on the CPU with every buffer holding a known pattern."""
	q = Digits.empty(rows_pad, k1.round_up(n, 16), ns, chunks)
	rng = np.random.default_rng(seed)
	q.planes.copy_(torch.from_numpy(rng.integers(0, 256, q.planes.numel(), dtype=np.uint8)))
	q.exps.copy_(torch.arange(rows_pad, dtype=torch.int32) - 40)
	q.fix.copy_(torch.arange(rows_pad * k1.FIX_STRIDE, dtype=torch.float64).reshape(rows_pad, k1.FIX_STRIDE))
	return Residualized(rows_pad if rows is None else rows, n, None, torch.arange(rows_pad, dtype=torch.float64) + 0.5, None, shape=(rows_pad, q.k_pad), digits=q)


def offset_of(view, base):
	return view.data_ptr() - base.data_ptr()


@pytest.mark.parametrize('ns', [6, 5])
@pytest.mark.parametrize('n,rows_pad,chunks', SHAPES)
def test_geometry_is_k1_longdoubles(n, rows_pad, chunks, ns):
	g = k1.geometry(n, rows_pad, ns, chunks or 0)
	q = operand(n, rows_pad, ns, chunks).digits
	assert (q.rows_pad, q.k_pad, q.nslices, q.pitch) == (rows_pad, k1.round_up(n, 16), ns, 0)
	assert q.nks == g['cks'] and q.plane_bytes == g['plane_bytes'] and q.planes.numel() == g['total'] and q.planes.dtype == torch.uint8
	assert q.exps.shape == (rows_pad, ) and q.exps.dtype == torch.int32 and q.fix.shape == (rows_pad, k1.FIX_STRIDE) and q.fix.dtype == torch.float64
	for lo in range(0, rows_pad + 1, 32):
		assert q.plane_offset(lo) == g['plane_bytes'] * lo // rows_pad == plane_bytes(lo, g['cks'])
	if chunks is None:
		assert q.cks is None and q.chunks is None and g['nks'] == g['cks']
	else:
		assert q.cks == g['cks'] == Digits.chunk_ksteps(q.k_pad, chunks) and len(q.chunks) == g['nchunks'] == chunks
		for c, t in enumerate(q.chunks):
			assert t.numel() == g['chunk_bytes'] and offset_of(t, q.planes) == c * g['chunk_bytes']


@pytest.mark.parametrize('ns', [6, 5])
def test_row_block_is_a_view_read_through_the_pitch(ns):
	n = 1026
	whole = operand(n, 256, ns, rows=200)
	g, gw = k1.geometry(n, 128, ns), k1.geometry(n, 256, ns)
	d_whole = k1.decode_planes(whole.digits.planes.numpy(), ns, 256, gw['nks'])
	blk = whole.row_block(128, 256)
	q = blk.digits
	assert offset_of(q.planes, whole.digits.planes) == whole.digits.plane_offset(128) == 4 * gw['nks'] * 1024
	assert q.pitch == whole.digits.plane_bytes == gw['plane_bytes'] and q.plane_bytes == g['plane_bytes'] and q.rows_pad == 128
	assert (blk.rows, blk.n, blk.rows_pad, blk.k_pad, blk.data, blk.coef) == (72, n, 128, whole.k_pad, None, None) and (q.nslices, q.k_pad, q.cks, q.chunks) == (ns, whole.k_pad, None, None)
	for got, src in ((q.exps, whole.digits.exps), (blk.ss, whole.ss), (q.fix, whole.digits.fix), (blk.fix, whole.fix)):
		assert torch.equal(got, src[128:256]) and offset_of(got, src) == 128 * src.stride(0) * src.element_size()
	assert np.array_equal(k1.decode_planes(q.planes.numpy(), ns, 128, g['nks'], plane_pitch=q.pitch), d_whole[:, 128:256])
	first = whole.row_block(0, 128)
	assert first.rows == 128 and offset_of(first.digits.planes, whole.digits.planes) == 0 and first.digits.pitch == gw['plane_bytes']
	assert np.array_equal(k1.decode_planes(first.digits.planes.numpy(), ns, 128, g['nks'], plane_pitch=first.digits.pitch), d_whole[:, :128])
	# rows = min(hi, rows) - lo, not below 0, unless the caller says otherwise
	assert operand(n, 256, ns, rows=100).row_block(128, 256).rows == 0 and whole.row_block(0, 256).rows == 200 and whole.row_block(128, 256, rows=7).rows == 7
	for lo, hi in ((64, 256), (128, 200), (128, 384), (128, 128)):
		with pytest.raises(AssertionError):
			whole.row_block(lo, hi)


@pytest.mark.parametrize('ns', [6, 5])
def test_block_of_a_block_keeps_the_outer_pitch(ns):
	n = 1026
	whole = operand(n, 384, ns, rows=300)
	g, gw = k1.geometry(n, 128, ns), k1.geometry(n, 384, ns)
	d_whole = k1.decode_planes(whole.digits.planes.numpy(), ns, 384, gw['nks'])
	outer = whole.row_block(128, 384)
	inner = outer.row_block(128, 256)  # rows 256 .. 383 of the whole
	assert outer.digits.pitch == inner.digits.pitch == gw['plane_bytes'] and inner.rows == 300 - 256
	assert offset_of(inner.digits.planes, whole.digits.planes) == whole.digits.plane_offset(256)
	assert np.array_equal(k1.decode_planes(outer.digits.planes.numpy(), ns, 256, g['nks'], plane_pitch=outer.digits.pitch), d_whole[:, 128:])
	assert np.array_equal(k1.decode_planes(inner.digits.planes.numpy(), ns, 128, g['nks'], plane_pitch=inner.digits.pitch), d_whole[:, 256:])
	assert torch.equal(inner.digits.exps, whole.digits.exps[256:]) and torch.equal(inner.ss, whole.ss[256:]) and torch.equal(inner.fix, whole.fix[256:])


@pytest.mark.parametrize('ns', [6, 5])
@pytest.mark.parametrize('chunks', [1, 2, 3])
def test_block_of_a_chunked_operand_slices_every_chunk(chunks, ns):
	n = 2050
	whole = operand(n, 256, ns, chunks, rows=256)
	gw = k1.geometry(n, 256, ns, chunks)
	blk = whole.row_block(128, 256)
	q = blk.digits
	assert q.cks == gw['cks'] and len(q.chunks) == chunks and q.planes is None and q.pitch == gw['plane_bytes'] == whole.digits.plane_bytes
	assert torch.equal(q.exps, whole.digits.exps[128:]) and torch.equal(q.fix, whole.digits.fix[128:]) and torch.equal(blk.ss, whole.ss[128:])
	for c in range(chunks):
		assert offset_of(q.chunks[c], whole.digits.chunks[c]) == whole.digits.plane_offset(128) == 4 * gw['cks'] * 1024
		d_chunk = k1.decode_planes(whole.digits.chunks[c].numpy(), ns, 256, gw['cks'])  # (a chunk is a dense operand of cks k-steps)
		assert np.array_equal(k1.decode_planes(q.chunks[c].numpy(), ns, 128, gw['cks'], plane_pitch=q.pitch), d_chunk[:, 128:])
	# the chunks together are the chunked layout of the one buffer
	d = k1.decode_planes(whole.digits.planes.numpy(), ns, 256, gw['nchunks'] * gw['cks'], gw['cks'])
	assert np.array_equal(np.concatenate([k1.decode_planes(t.numpy(), ns, 256, gw['cks']) for t in whole.digits.chunks], axis=2), d)


def test_invariants_raise():
	q = operand(2050, 128, 6, 2).digits
	with pytest.raises(ValueError, match='fix'):
		Digits(q.planes, q.exps, None, 6, q.k_pad)
	with pytest.raises(ValueError, match='cks'):
		Digits(q.planes, q.exps, q.fix, 6, q.k_pad, cks=q.cks)
	with pytest.raises(ValueError, match='cks'):
		Digits(q.planes, q.exps, q.fix, 6, q.k_pad, chunks=q.chunks)
	with pytest.raises(ValueError, match='pitch 0'):
		Digits(q.planes, q.exps, q.fix, 6, q.k_pad, pitch=q.plane_bytes, chunks=q.chunks, cks=q.cks)
	with pytest.raises(ValueError):
		Digits(None, q.exps, q.fix, 6, q.k_pad)
	assert Residualized(5, 2050, torch.zeros((128, 2064), dtype=torch.float64), None, None).fix is None


def test_reusable_is_a_question_of_shape():
	r = operand(2050, 128, 6, rows=33)
	assert r.reusable(33, 2050, 128, 2064, 6)
	for other in ((34, 2050, 128, 2064, 6), (33, 2049, 128, 2064, 6), (33, 2050, 256, 2064, 6), (33, 2050, 128, 2080, 6), (33, 2050, 128, 2064, 5), (33, 2050, 128, 2064, 6, 33)):
		assert not r.reusable(*other)
	ch = operand(2050, 128, 6, 2, rows=33)
	assert ch.reusable(33, 2050, 128, 2064, 6, ch.digits.cks) and not ch.reusable(33, 2050, 128, 2064, 6) and not ch.reusable(33, 2050, 128, 2064, 6, ch.digits.cks + 1)
	assert not operand(2050, 256, 6, rows=200).row_block(128, 256).reusable(72, 2050, 128, 2064, 6)  # a view of a larger operand is not a buffer to hand out
	r.data = torch.zeros((128, 2064), dtype=torch.float64)
	assert not r.reusable(33, 2050, 128, 2064, 6)
