"""GPU: K1 (csrc/nrm_residualize.hip) at kernel level, every output it writes against the extended-precision reference of tests/k1_longdouble.py.

What is checked, on ALL rows_pad rows and all padded cells (K2 and K3 read the padding): out, ss, coef to the running-error bounds of k1_longdouble's
docstring; exps by its two properties; the digit planes bit for bit against rint(out 2^-exps) of the same call; the row records against
tools/i8_error_model.row_stats of the decoded digits.  Inputs sit in buffers whose padding holds a sentinel (a read past a row's end changes the result),
outputs are pre-filled with NaN / 0x5A / a sentinel exponent and followed by a guard (an element K1 leaves unwritten, or writes past the end, is seen).

The cases (k1_longdouble.grid, scalar_cases, exponent_rows, wide_rows) are the ones tests/test_k1_longdouble_cpu.py shows the comparators accept from an
emulation and reject nine mutations of; that file also shows, from the launcher's conditions, that they launch every instantiation of the kernel.
Every test prints its worst error-to-bound ratio per output before it asserts (pytest -rP shows them); the last test prints the table of the run.

Measured on an MI355X, worst error / bound per output over the whole file: see DESIGN.md section 4, "K1 at kernel level"."""
import functools

import numpy as np
import pytest

import k1_longdouble as k1
from k1_longdouble import model

pytestmark = pytest.mark.gpu

SENTINEL = 7.0  # in the padding of x and C
EXP_SENTINEL = 0x7f7f7f7f
WORST = {}  # output -> (ratio, test case): the table the last test prints


@functools.lru_cache(maxsize=None)
def _env():
	import torch
	from normalisr_amd import _lib
	from normalisr_amd import engine
	return torch, _lib, engine.get_engine()


def _place(h, pitch, fill=SENTINEL):
	"""The host matrix (rows, n) in HBM with a row pitch of `pitch` elements, the padding filled: (the (rows, n) view, the allocation)."""
	torch, _, _ = _env()
	h = np.ascontiguousarray(h)
	whole = torch.full((max(h.shape[0], 1), pitch), fill, dtype=getattr(torch, str(h.dtype)), device='cuda')
	view = whole[:h.shape[0], :h.shape[1]]
	view.copy_(torch.from_numpy(h))
	return view, whole


def _filled(shape, value, dtype):
	torch, _, _ = _env()
	return torch.full(shape, value, dtype=dtype, device='cuda')


def run_k1(x, C64, dci, rank, ns, rows_pad=None, keep=True, cmax=True, chunks=0, misalign=False, block=None):
	"""One direct call of nrm_residualize / nrm_residualize_q / nrm_residualize_q_chunked with pitches chosen here: 16-cell padded rows (vector kernel,
	ragged tails included) or -- misalign -- an odd pitch (scalar fallback).  block = (first row, rows of the larger matrix): the digits go into that block
	of a larger plane buffer through the plane pitch.  Returns every output as numpy, guards included."""
	torch, _lib, eng = _env()
	lib = eng.lib
	rows, n = x.shape
	nc = C64.shape[0]
	kp = k1.round_up(n, 16)
	rp = k1.round_up(max(rows, 1), 128 if ns else 4) if rows_pad is None else rows_pad
	xd, x_all = _place(x, kp + 1 if misalign else kp)
	cd, c_all = _place(C64, kp) if nc else (None, None)
	dd = torch.from_numpy(np.ascontiguousarray(dci, dtype=np.float64)).cuda() if nc else None
	cm = torch.from_numpy(np.abs(C64).max(axis=1)).cuda() if (nc and cmax) else None
	t64 = torch.float64
	out = _filled((rp + 1, kp), float('nan'), t64) if keep else None
	ss = _filled((rp + 1, ), float('nan'), t64)
	active = rank > 0 and nc > 0
	coef = _filled((rows, nc), float('nan') if active else 0.0, t64) if (nc and not chunks) else None  # (the chunked entry writes no coefficients)
	ptr = lambda t: 0 if t is None else t.data_ptr()
	code = _lib.NRM_F64 if x.dtype == np.float64 else _lib.NRM_F32
	st = eng._stream()
	dev = dict(rows=rows, n=n, rows_pad=rp, ns=ns, kp=kp)
	if not ns:
		_lib.check(lib.nrm_residualize(xd.data_ptr(), code, rows, n, xd.stride(0), ptr(cd), nc, kp, ptr(dd), int(rank), out.data_ptr(), kp, rp, ss.data_ptr(),
									   ptr(coef), st))
	else:
		g = k1.geometry(n, rp, ns, chunks)
		total, pitch, first = g['total'], 0, 0
		if block is not None:
			gw = k1.geometry(n, block[1], ns)
			total, pitch, first = gw['total'], gw['plane_bytes'], (block[0] // 32) * gw['nks'] * 1024
		planes = _filled((total + 1024, ), 0x5A, torch.uint8)
		exps = _filled((rp + 1, ), EXP_SENTINEL, torch.int32)
		fix = _filled((rp + 1, k1.FIX_STRIDE), float('nan'), t64)
		if chunks:
			_lib.check(lib.nrm_residualize_q_chunked(xd.data_ptr(), code, rows, n, xd.stride(0), ptr(cd), nc, kp, ptr(dd), int(rank), rp, ss.data_ptr(), ns,
													 planes.data_ptr(), exps.data_ptr(), g['cks'], ptr(cm), fix.data_ptr(), st))
		else:
			_lib.check(lib.nrm_residualize_q(xd.data_ptr(), code, rows, n, xd.stride(0), ptr(cd), nc, kp, ptr(dd), int(rank), ptr(out), kp, rp, ss.data_ptr(),
											 ptr(coef), ns, planes.data_ptr() + first, exps.data_ptr(), pitch, ptr(cm), fix.data_ptr(), st))
		torch.cuda.synchronize()
		dev.update(geo=g, planes=planes.cpu().numpy().view(np.int8), exps=exps.cpu().numpy(), fix=fix.cpu().numpy(), pitch=pitch, first=first)
	torch.cuda.synchronize()
	dev.update(out=None if out is None else out.cpu().numpy(), ss=ss.cpu().numpy(), coef=None if coef is None else coef.cpu().numpy())
	# the inputs are intact, padding included
	assert torch.equal(xd.cpu(), torch.from_numpy(np.ascontiguousarray(x))) and (x_all[:, n:] == SENTINEL).all()
	return dev


def note(name, w, case):
	print('%-8s %-60s worst error / bound %.3g at %s' % (name, w.what, w.ratio, w.where))
	if w.ratio > WORST.get(name, (-1.0, ''))[0]:
		WORST[name] = (w.ratio, case)


def decode(dev):
	"""The digits of a direct call, decoded as far as live rows reach (whole 32-row blocks); the blocks after them must be all-zero bytes."""
	g, ns, rp = dev['geo'], dev['ns'], dev['rows_pad']
	buf = dev['planes']
	guard = buf[-1024:]
	assert (guard == 0x5A).all(), 'bytes written past the end of the planes'
	if dev['pitch']:
		return k1.decode_planes(buf, ns, rp, g['nks'], plane_pitch=dev['pitch'], offset=dev['first']), rp
	if g['nchunks'] > 1 or rp * g['nks'] * 32 <= (1 << 22):
		return k1.decode_planes(buf, ns, rp, g['nchunks'] * g['cks'], g['cks']), rp
	nb = k1.round_up(dev['rows'], 32)
	img = buf[:g['total']].reshape(ns, rp // 32, g['nks'] * 1024)
	assert not img[:, nb // 32:].any(), 'digits: padding rows (blocks past the live rows)'
	return k1.decode_planes(buf, ns, nb, g['nks'], plane_pitch=g['plane_bytes']), nb


def check(dev, ref, kind, case, out_of=None):
	"""Every comparator on the outputs of one call; prints, records and asserts.  out_of: the call whose fp64 `out` the digits are held to when this one
	kept none (same input: the bit-identity of the two calls' digits is then part of the claim)."""
	rows, n, rp, ns = dev['rows'], dev['n'], dev['rows_pad'], dev['ns']
	cnt = k1.counts(kind, n, ref['nc'], ref['active'])
	ws = {}
	out = dev['out']
	if out is not None:
		assert np.isnan(out[rp:]).all(), 'out: written past rows_pad'
		ws['out'] = k1.compare_out(out[:rp], ref, cnt)
	assert np.isnan(dev['ss'][rp:]).all(), 'ss: written past rows_pad'
	ws['ss'] = k1.compare_ss(dev['ss'][:rp], ref, cnt)
	if dev['coef'] is not None:
		if ref['active']:
			ws['coef'] = k1.compare_coef(dev['coef'], ref, cnt)
		else:
			assert (dev['coef'] == 0).all(), 'coef: written without active covariates'
	if ns:
		assert dev['exps'][rp] == EXP_SENTINEL and np.isnan(dev['fix'][rp:]).all(), 'exps / fix: written past rows_pad'
		exps = dev['exps'][:rp]
		assert (exps != EXP_SENTINEL).all() and (np.abs(exps.astype(np.int64)) < 4096).all(), 'exps: a row without an exponent'
		d, nb = decode(dev)
		src = out[:rp] if out is not None else out_of
		ws['digits'] = k1.compare_digits(d, src[:nb], exps[:nb], rows, n, ns)
		ws['exps'] = k1.compare_exps(exps, None if out is None else out[:rp], ref, cnt, ns)
		assert not dev['fix'][nb:rp].any()
		ws['fix'] = k1.compare_fix(dev['fix'][:nb], d, exps[:nb], dev['ss'][:nb], n, ns, rows)
	for name, w in ws.items():
		note(name, w, case)
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (case, bad)
	return ws


# ---- the sweep over cells, rows, covariates, types and NS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', k1.grid(), ids=k1.case_id)
def test_k1_grid_against_longdouble(case):
	"""The vector kernel on 16-cell padded pitches (so that cell counts with a ragged last group of four reach it), then the same rows through
	Engine.residualize as the library's callers place them (contiguous: an odd cell count goes to the scalar kernel and the stand-alone quantiser)."""
	torch, _lib, eng = _env()
	rows, n, cov, dtype, ns = case
	x, C = k1.case_inputs(case)
	C64, dci, rank = k1.prepare(C)
	ref = k1.reference(x, C64, dci, rank)
	cid = k1.case_id(case)
	print(k1.instantiation(dtype, n, C64.shape[0], rank, ns))
	check(run_k1(x, C64, dci, rank, ns), ref, 'v4', cid)
	if n > 4096:
		return
	d_c, d_dci = eng.covariates(C64, dci)
	xd = torch.from_numpy(x).cuda()
	r = eng.residualize(xd, d_c, d_dci, rank, want_coef=True, nslices=ns, keep_fp64=True)
	aligned = (n * x.dtype.itemsize) % 16 == 0  # contiguous rows on 16-byte boundaries (the covariates' 8 n bytes then are as well): the vector kernel
	fused = bool(ns) and eng.k1_quantises(xd, d_c)
	assert fused == (bool(ns) and aligned)
	dev = dict(rows=rows, n=n, rows_pad=r.rows_pad, ns=ns if fused else 0, kp=r.k_pad, out=np.vstack([r.data.cpu().numpy(), np.full((1, r.k_pad), np.nan)]),
			   ss=np.append(r.ss.cpu().numpy(), np.nan), coef=None if r.coef is None or not C64.shape[0] else r.coef.cpu().numpy())
	assert (r.rows_pad, r.k_pad) == (k1.round_up(rows, 128), k1.round_up(n, 16))
	if fused:
		g = k1.geometry(n, r.rows_pad, ns)
		assert r.digits.planes.numel() == g['total']
		dev.update(geo=g, planes=np.append(r.digits.planes.cpu().numpy().view(np.int8), np.full(1024, 0x5A, dtype=np.int8)), pitch=0, first=0,
				   exps=np.append(r.digits.exps.cpu().numpy(), np.int32(EXP_SENTINEL)), fix=np.vstack([r.fix.cpu().numpy(), np.full((1, k1.FIX_STRIDE), np.nan)]))
	check(dev, ref, 'v4' if aligned else 'scalar', cid + ' (engine)')


@pytest.mark.parametrize('case', k1.scalar_cases(), ids=lambda c: 'r%d-n%d-c%s-%s' % (c[0], c[1], c[2], c[3][5:]))
def test_k1_scalar_fallback_against_longdouble(case):
	"""k_residualize<T>: an odd row pitch breaks the 16-byte alignment.  With digits asked for, the same call returns the library's error and no result."""
	torch, _lib, eng = _env()
	x, C = k1.scalar_inputs(case)
	C64, dci, rank = k1.prepare(C)
	ref = k1.reference(x, C64, dci, rank)
	check(run_k1(x, C64, dci, rank, 0, misalign=True), ref, 'scalar', 'scalar r%d-n%d-c%s-%s' % case)
	with pytest.raises(ValueError, match='16-byte aligned rows'):
		run_k1(x, C64, dci, rank, 6, misalign=True)


# ---- the exponent ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ns', [6, 5])
def test_k1_exponent_paths(ns):
	"""k1_longdouble.exponent_rows: both properties on every row, and WHICH exponent each group of four took.  The tight rows are scaled so that the bound's
	exponent is one above that of the true maximum: rows 0-3 carry the bound's (accepted without a sweep), their likes beside a loose row (8, 10, 11) and
	beside the explained and the zero row (12, 15) carry the true maximum's, and so does every row when the covariates' maxima are absent."""
	torch, _lib, eng = _env()
	x, C, kind = k1.exponent_rows()
	C64, dci, rank = k1.prepare(C)
	ref = k1.reference(x, C64, dci, rank)
	for cmax in (True, False):
		dev = run_k1(x, C64, dci, rank, ns, cmax=cmax)
		check(dev, ref, 'v4', 'exponent rows ns%d cmax %s' % (ns, cmax))
		_, true_sh = model.quantise(dev['out'][:16], ns)  # the exponent of K1's own largest |out|
		got = dev['exps'][:16].astype(np.int64)
		want = true_sh + (np.arange(16) < 4) if cmax else true_sh
		print('exps - exponent of the true maximum:', got - true_sh)
		assert np.array_equal(got, want), (cmax, got - true_sh)
		assert got[14] == -(8 * ns - 2) and dev['ss'][14] == 0 and dev['ss'][13] < 1e-24 * float(ref['raw'][13])
	# the same through the Engine: maxima recorded by Engine.covariates, absent for covariates uploaded outside it
	x, C, kind = k1.exponent_rows(2052)  # (an even cell count: the Engine's contiguous rows and covariates stay 16-byte aligned)
	C64, dci, rank = k1.prepare(C)
	xd = torch.from_numpy(x).cuda()
	for cmax in (True, False):
		d_c, d_dci = eng.covariates(C64, dci)
		if not cmax:
			d_c = eng.upload(C64)
		assert (eng.cmax_ptr(d_c) != 0) == cmax
		r = eng.residualize(xd, d_c, d_dci, rank, nslices=ns, keep_fp64=True)
		_, true_sh = model.quantise(r.data.cpu().numpy()[:16], ns)
		assert np.array_equal(r.digits.exps.cpu().numpy()[:16].astype(np.int64), true_sh + (np.arange(16) < 4) if cmax else true_sh)


# ---- the same bits in every form ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('ns', [6, 5])
def test_k1_same_bits_across_forms(dtype, ns):
	"""ss, exps, the digits and the row records of one input are identical with and without the fp64 output, in the whole and the chunked layout (1, 2 and 3
	chunks of 2050 cells = 65 k-steps: ragged last chunks), and from call to call; `out` is the same with and without digits."""
	torch, _lib, eng = _env()
	case = (33, 2050, 2, dtype, ns)  # (an even cell count: the Engine's contiguous covariates stay 16-byte aligned)
	x, C = k1.case_inputs(case)
	C64, dci, rank = k1.prepare(C)
	ref = k1.reference(x, C64, dci, rank)
	d_c, d_dci = eng.covariates(C64, dci)
	xd, _ = _place(x, 2064)
	full = eng.residualize(xd, d_c, d_dci, rank, nslices=ns, keep_fp64=True)
	g = k1.geometry(2050, 128, ns)
	pack = lambda r: dict(rows=33, n=2050, rows_pad=128, ns=ns, kp=2064, geo=g, pitch=0, first=0, coef=None, out=None, ss=np.append(r.ss.cpu().numpy(), np.nan),
						  planes=np.append(r.digits.planes.cpu().numpy().view(np.int8), np.full(1024, 0x5A, dtype=np.int8)),
						  exps=np.append(r.digits.exps.cpu().numpy(), np.int32(EXP_SENTINEL)), fix=np.vstack([r.fix.cpu().numpy(), np.full((1, k1.FIX_STRIDE), np.nan)]))
	base = pack(full)
	base['out'] = np.vstack([full.data.cpu().numpy(), np.full((1, 2064), np.nan)])
	check(base, ref, 'v4', 'forms %s ns%d' % (dtype, ns))
	same = lambda r: (torch.equal(r.ss, full.ss) and torch.equal(r.digits.exps, full.digits.exps) and torch.equal(r.fix, full.fix))
	lean = eng.residualize(xd, d_c, d_dci, rank, nslices=ns, keep_fp64=False)
	assert lean.data is None and same(lean) and torch.equal(lean.digits.planes, full.digits.planes)
	check(pack(lean), ref, 'v4', 'forms %s ns%d keep_fp64=False' % (dtype, ns), out_of=base['out'][:128])
	again = eng.residualize(xd, d_c, d_dci, rank, nslices=ns, keep_fp64=True)
	assert same(again) and torch.equal(again.digits.planes, full.digits.planes) and torch.equal(again.data, full.data)
	plain = eng.residualize(xd, d_c, d_dci, rank, nslices=0)
	assert torch.equal(plain.data, full.data) and torch.equal(plain.ss, full.ss)
	d_full = k1.decode_planes(base['planes'], ns, 128, g['nks'])
	for chunks in (1, 2, 3):
		ch = eng.residualize_chunked(xd, d_c, d_dci, rank, 128, ns, chunks)
		gc = k1.geometry(2050, 128, ns, chunks)
		assert ch.digits.cks == gc['cks'] and len(ch.digits.chunks) == gc['nchunks'] == chunks and ch.digits.planes.numel() == gc['total'] and same(ch)
		d = k1.decode_planes(ch.digits.planes.cpu().numpy(), ns, 128, gc['nchunks'] * gc['cks'], gc['cks'])
		assert np.array_equal(d[:, :, :g['nks'] * 32], d_full) and not d[:, :, g['nks'] * 32:].any(), chunks
		dev = run_k1(x, C64, dci, rank, ns, keep=False, chunks=chunks)  # (the direct entry into sentinel-filled buffers: every byte of every chunk is written)
		assert np.array_equal(dev['planes'][:gc['total']], ch.digits.planes.cpu().numpy().view(np.int8))
		check(dev, ref, 'v4', 'forms %s ns%d %d chunks' % (dtype, ns, chunks), out_of=base['out'][:128])


@pytest.mark.parametrize('dtype,ns', [('float32', 6), ('float64', 5)])
def test_k1_row_block_equals_the_rows_alone(dtype, ns):
	"""Rows 128-199 of a 200-row matrix: as a view of the whole (Engine.row_block), written on their own into their block of a larger plane buffer through the
	plane pitch (what the resident coex paths do), and quantised alone -- the same digits, exponents, sums of squares and records; the bytes of the larger
	buffer outside the block are not touched."""
	torch, _lib, eng = _env()
	n = 1026
	x, C = k1.case_inputs((200, n, 2, dtype, ns))
	C64, dci, rank = k1.prepare(C)
	d_c, d_dci = eng.covariates(C64, dci)
	xd, _ = _place(x, 1040)
	whole = eng.residualize(xd, d_c, d_dci, rank, nslices=ns, keep_fp64=False)
	alone = eng.residualize(xd[128:], d_c, d_dci, rank, nslices=ns, keep_fp64=True)
	assert whole.rows_pad == 256 and alone.rows_pad == 128
	blk = eng.row_block(whole, 128, 256)
	g, gw = k1.geometry(n, 128, ns), k1.geometry(n, 256, ns)
	assert blk.rows == 72 and blk.digits.pitch == gw['plane_bytes']
	d_alone = k1.decode_planes(alone.digits.planes.cpu().numpy(), ns, 128, g['nks'])
	d_blk = k1.decode_planes(blk.digits.planes.cpu().numpy(), ns, 128, g['nks'], plane_pitch=blk.digits.pitch)
	assert np.array_equal(d_blk, d_alone)
	assert torch.equal(blk.digits.exps, alone.digits.exps) and torch.equal(blk.ss, alone.ss) and torch.equal(blk.fix, alone.fix)
	ref = k1.reference(x[128:], C64, dci, rank)
	dev = run_k1(x[128:], C64, dci, rank, ns, block=(128, 384))
	check(dev, ref, 'v4', 'row block %s ns%d' % (dtype, ns))
	assert np.array_equal(k1.decode_planes(dev['planes'], ns, 128, g['nks'], plane_pitch=dev['pitch'], offset=dev['first']), d_alone)
	assert np.array_equal(dev['exps'][:128], alone.digits.exps.cpu().numpy()) and np.array_equal(dev['ss'][:128], alone.ss.cpu().numpy())
	assert np.array_equal(dev['fix'][:128], alone.fix.cpu().numpy()) and np.array_equal(dev['out'][:128], alone.data.cpu().numpy())
	g3 = k1.geometry(n, 384, ns)
	img = dev['planes'][:g3['total']].reshape(ns, 384 // 32, g3['nks'] * 1024)
	assert (img[:, :4] == 0x5A).all() and (img[:, 8:] == 0x5A).all() and (img[:, 4:8] != 0x5A).any()


@pytest.mark.parametrize('dtype,ns', [('float32', 6), ('float64', 5)])
def test_k1_block_by_block_into_an_empty_operand_equals_one_call(dtype, ns):
	"""The same 200 rows x 1026 cells as Engine.empty_operand (256 rows) filled by two Engine.residualize_into calls -- rows 0-127, then the ragged block
	128-199 at a non-zero row-group offset, both through the whole operand's plane pitch -- against one Engine.residualize call: planes, exps, ss and
	fix bit for bit, padding rows included (every byte of the sentinel-filled operand is written: K1 writes all rows_pad rows of a call)."""
	torch, _lib, eng = _env()
	n = 1026
	x, C = k1.case_inputs((200, n, 2, dtype, ns))
	C64, dci, rank = k1.prepare(C)
	d_c, d_dci = eng.covariates(C64, dci)
	xd, _ = _place(x, 1040)
	once = eng.residualize(xd, d_c, d_dci, rank, nslices=ns, keep_fp64=False)
	whole = eng.empty_operand(200, n, ns)
	q = whole.digits
	gw = k1.geometry(n, 256, ns)
	assert (whole.rows, whole.n, whole.rows_pad, whole.k_pad, whole.data, whole.coef) == (200, n, 256, 1040, None, None)
	assert (q.planes.numel(), q.plane_bytes, q.pitch, q.nslices, q.cks) == (gw['total'], gw['plane_bytes'], 0, ns, None)
	q.planes.fill_(0x5A), q.exps.fill_(EXP_SENTINEL), q.fix.fill_(float('nan')), whole.ss.fill_(float('nan'))
	eng.residualize_into(whole, 0, xd[:128], d_c, d_dci, rank)
	img = q.planes.cpu().numpy().reshape(ns, 256 // 32, gw['nks'] * 1024)
	assert (img[:, 4:] == 0x5A).all() and (q.exps[128:] == EXP_SENTINEL).all() and torch.isnan(whole.ss[128:]).all() and torch.isnan(q.fix[128:]).all(), 'written outside the block'
	eng.residualize_into(whole, 128, xd[128:], d_c, d_dci, rank)
	assert torch.equal(q.planes, once.digits.planes) and torch.equal(q.exps, once.digits.exps) and torch.equal(whole.ss, once.ss) and torch.equal(q.fix, once.digits.fix)
	assert torch.equal(whole.fix, once.fix)


# ---- the cell-parallel variant ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,n,dtype,const_last', [(r, n, t, cl) for r in (1, 5, 32) for n in (1, 1023, 1025, 3000) for t, cl in (('float64', 1), ('float32', 0))] +
						 [(5, 3000, 'float64', 0)])
def test_k1_wide_against_longdouble(rows, n, dtype, const_last):
	"""nrm_residualize_wide (k_residualize_wide + k_rw_sum) given the same ga: out on all (rows, ldo) elements, ss, coef; a copy of a covariate and a constant
	row beside the intercept come back cleared with ss == 0, the row that keeps 1e-18 of its norm does not (k1_longdouble.wide_rows)."""
	torch, _lib, eng = _env()
	lib = eng.lib
	x, C = k1.wide_rows(rows, n, dtype, const_last)
	C64, dci, rank = k1.prepare(C)
	nc = C64.shape[0]
	ga, a = k1.wide_products(x, C64, const_last)
	ref = k1.reference(x, C64, dci, rank, a=a)
	ldo = k1.round_up(n, 128)
	cnt = k1.counts('wide', n, nc, ref['active'], ldo=ldo)
	cleared = k1.clear_expected(ref, cnt) == 1
	xd, x_all = _place(x, n + 3)
	cd, _ = _place(C64, n + 1)
	out = _filled((rows + 1, ldo), float('nan'), torch.float64)
	ss = _filled((rows + 1, ), float('nan'), torch.float64)
	coef = _filled((rows, nc), float('nan'), torch.float64)
	work = _filled((64 * ((ldo + 1023) // 1024) + 1, ), float('nan'), torch.float64)
	gd, dd = torch.from_numpy(ga).cuda(), torch.from_numpy(np.ascontiguousarray(dci)).cuda()
	_lib.check(lib.nrm_residualize_wide(xd.data_ptr(), _lib.NRM_F64 if dtype == 'float64' else _lib.NRM_F32, rows, n, xd.stride(0), cd.data_ptr(), nc, cd.stride(0),
										gd.data_ptr(), dd.data_ptr(), int(rank),
										out.data_ptr(), ldo, ss.data_ptr(), coef.data_ptr(), work.data_ptr(), const_last, eng._stream()))
	torch.cuda.synchronize()
	out, ss, coef, work = out.cpu().numpy(), ss.cpu().numpy(), coef.cpu().numpy(), work.cpu().numpy()
	assert np.isnan(out[rows:]).all() and np.isnan(ss[rows:]).all() and np.isnan(work[-1]), 'written past the end'
	case = 'wide r%d-n%d-%s-cl%d' % (rows, n, dtype[5:], const_last)
	ws = dict(out=k1.compare_out(out[:rows], ref, cnt, cleared), ss=k1.compare_ss(ss[:rows], ref, cnt, cleared), coef=k1.compare_coef(coef, ref, cnt))
	for name, w in ws.items():
		note('wide ' + name, w, case)
	print('cleared rows:', np.nonzero(cleared)[0], ' ss / |x|^2:', ss[:rows] / np.asarray(ref['raw'], dtype=np.float64))
	assert all(w.ratio <= 1 for w in ws.values()), ws
	assert (ss[:rows][~cleared] > 0).all()


def test_k1_zz_worst_ratios_of_this_run():
	"""The table the next K1 rewrite holds itself to: the worst error-to-bound ratio per output over the tests of this file that ran before this one."""
	for name in sorted(WORST):
		print('%-10s worst error / bound %.3g   (%s)' % ((name, ) + WORST[name]))
	assert all(v[0] <= 1 for v in WORST.values())
