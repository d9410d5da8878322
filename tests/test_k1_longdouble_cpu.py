"""CPU: the K1 reference and comparators of tests/k1_longdouble.py can fail, and accept what they should.

The comparators are fed an fp64 numpy EMULATION of what K1 writes -- out, ss, coef, exps, the row records and the plane buffer, laid out byte by byte with the
address arithmetic of k_residualize_v4 (not with the decoder's reshapes) -- at every shape the GPU tests use: they must accept it.  Then nine mutations, each
a way a rewritten K1 could be subtly wrong, are made to the EMULATED outputs (never to the library), and the comparator that is responsible for that output
must reject each.  Last, the designated rows of the exponent and clear-rule tests are shown to lie a factor 100 from every threshold by the reference alone,
and the reference is held to the oracle."""
import numpy as np
import pytest

import k1_longdouble as k1
from k1_longdouble import model


# ---- emulation -----------------------------------------------------------------------------------------------------------------------------------------------
def write_planes(buf, d, rows_pad, cks, plane_bytes, chunk_bytes, base=0, shift_chunk=None):
	"""Digits d (ns, rows_pad, cells) into buf at the byte addresses k_residualize_v4 computes: image (row >> 5, k-step), 32 bytes per row, half (kk >> 4) ^ flip.
	shift_chunk: (chunk, bytes) writes that chunk at a wrong offset (a mutation)."""
	ns, _, cells = d.shape
	r, k = np.arange(rows_pad)[:, None], np.arange(cells)[None, :]
	rr, kk, ks_all = r & 31, k & 31, k >> 5
	chunk = ks_all // cks
	ks = ks_all - chunk * cks + chunk * (chunk_bytes >> 10)
	off = base + (r >> 5) * cks * 1024 + 2 * rr * 16 + ks * 1024 + (((kk >> 4) ^ ((rr >> 3) & 1)) << 4) + (kk & 15)
	if shift_chunk is not None:
		off = off + np.where(chunk == shift_chunk[0], shift_chunk[1], 0)
	for s in range(ns):
		buf[off + s * plane_bytes] = d[s].astype(np.int8)


def emulate(x, C, dci, rank, rows_pad, ns, chunks=0, a=None, b_swap=None, ldo=None):
	"""What K1 writes for these inputs, in fp64 numpy (BLAS order: well inside the worst-case bounds).  The exponent is that of the row's true maximum.
	a: products to use in place of x C^T (mutation 1); b_swap: (i, j) residualises row i with row j's coefficients (mutation 2)."""
	x64 = np.asarray(x, dtype=np.float64)
	rows, n = x64.shape
	nc = C.shape[0]
	ldo = k1.round_up(n, 16) if ldo is None else ldo
	active = rank > 0 and nc > 0
	b = np.zeros((rows, nc))
	res = x64.copy()
	if active:
		b = (x64 @ C.T if a is None else a) @ np.asarray(dci).reshape(nc, nc).T
		bb = b.copy()
		if b_swap:
			bb[b_swap[0]] = b[b_swap[1]]
		res = x64 - bb @ C
	out = np.zeros((rows_pad, ldo))
	out[:rows, :n] = res
	e = dict(out=out, ss=(out * out).sum(axis=1), coef=b, rows=rows, n=n, rows_pad=rows_pad, ns=ns)
	if ns:
		g = k1.geometry(n, rows_pad, ns, chunks)
		cells = g['nchunks'] * g['cks'] * 32
		o = np.zeros((rows_pad, cells))
		o[:, :min(ldo, cells)] = out[:, :min(ldo, cells)]
		q, sh = model.quantise(o, ns)
		d = np.stack(model.digits(q, ns))
		buf = np.zeros(g['total'], dtype=np.int8)
		write_planes(buf, d, rows_pad, g['cks'], g['plane_bytes'], g['chunk_bytes'])
		fix = np.zeros((rows_pad, k1.FIX_STRIDE))
		for i in range(rows):
			st = model.row_stats([t[i, :n] for t in d], q[i, :n], sh[i], n, ns)
			fix[i, :ns - 1] = st['u']
			fix[i, 5:8] = st['c'], st['g'], np.ldexp(2 * st['g'], 8 * ns - 2)
		e.update(geo=g, exps=sh.astype(np.int32), planes=buf, fix=fix, d=d, q=q)
	return e


def judge(e, ref, cnt):
	"""Every comparator on one set of (emulated) outputs: {name: Worst}."""
	w = dict(out=k1.compare_out(e['out'], ref, cnt), ss=k1.compare_ss(e['ss'], ref, cnt), coef=k1.compare_coef(e['coef'], ref, cnt))
	if e['ns']:
		g = e['geo']
		d = k1.decode_planes(e['planes'], e['ns'], e['rows_pad'], g['nchunks'] * g['cks'], g['cks'])
		w['digits'] = k1.compare_digits(d, e['out'], e['exps'], e['rows'], e['n'], e['ns'])
		w['exps'] = k1.compare_exps(e['exps'], e['out'], ref, cnt, e['ns'])
		w['fix'] = k1.compare_fix(e['fix'], d, e['exps'], e['ss'], e['n'], e['ns'], e['rows'])
	return w


def accepted(w):
	return all(v.ratio <= 1 for v in w.values())


def setup(x, C, rows_pad=128, ns=6, chunks=0, kind='v4', **ka):
	C64, dci, rank = k1.prepare(C)
	ref = k1.reference(x, C64, dci, rank)
	cnt = k1.counts(kind, x.shape[1], C64.shape[0], ref['active'])
	return emulate(x, C64, dci, rank, rows_pad, ns, chunks, **ka), ref, cnt, (C64, dci, rank)


# ---- acceptance at every shape of the GPU tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', k1.grid(), ids=k1.case_id)
def test_comparators_accept_the_emulation_at_every_grid_shape(case):
	x, C = k1.case_inputs(case)
	e, ref, cnt, _ = setup(x, C, k1.round_up(case[0], 128), case[4])
	w = judge(e, ref, cnt)
	assert accepted(w), w
	# the scalar fallback's constants accept the same numbers
	cnt = k1.counts('scalar', x.shape[1], C.shape[0], ref['active'])
	assert k1.compare_out(e['out'], ref, cnt).ratio <= 1 and k1.compare_ss(e['ss'], ref, cnt).ratio <= 1 and k1.compare_coef(e['coef'], ref, cnt).ratio <= 1


def test_every_instantiation_has_a_case():
	"""From the launcher's conditions (k1_longdouble.instantiation), not by assumption: the grid and the scalar cases launch every kernel it can reach."""
	first = {}
	for c in k1.grid():
		C64, dci, rank = k1.prepare(k1.case_inputs(c)[1])
		first.setdefault(k1.instantiation(c[3], c[1], C64.shape[0], rank, c[4]), 'grid ' + k1.case_id(c))
	for c in k1.scalar_cases():
		first.setdefault(k1.instantiation(c[3], c[1], 0, 0, 0, vec=False), 'scalar r%d-n%d-c%s-%s' % (c[0], c[1], c[2], c[3][5:]))
	assert set(first) == k1.all_instantiations(), sorted(k1.all_instantiations() ^ set(first))
	for name in sorted(first):  # (pytest -rP shows the table)
		print('%-42s %s' % (name, first[name]))


@pytest.mark.parametrize('case', k1.scalar_cases(), ids=lambda c: 'r%d-n%d-c%s-%s' % (c[0], c[1], c[2], c[3][5:]))
def test_comparators_accept_the_emulation_at_every_scalar_shape(case):
	x, C = k1.scalar_inputs(case)
	e, ref, cnt, _ = setup(x, C, k1.round_up(case[0], 4), 0, kind='scalar')
	assert accepted(judge(e, ref, cnt))


@pytest.mark.parametrize('chunks', [1, 2, 3])
@pytest.mark.parametrize('ns', [5, 6])
def test_comparators_accept_the_chunked_layout(chunks, ns):
	"""2050 cells are 65 k-steps: two chunks of 33 (the last one ragged: 32 + a zero image), three of 22 (the last one 21 + one)."""
	x, C = k1.case_inputs((33, 2050, 2, 'float64', ns))
	e, ref, cnt, _ = setup(x, C, 128, ns, chunks)
	assert e['geo']['nchunks'] == chunks and e['geo']['cks'] * chunks > e['geo']['nks'] - (chunks == 1)
	assert accepted(judge(e, ref, cnt))


def test_decoder_reads_a_block_of_a_larger_matrix():
	"""Rows 128-255 of a 384-row matrix, written with the plane pitch of the whole: the decoder finds them through (pitch, offset), and the same bytes decoded as
	the whole matrix carry them in rows 128-255."""
	ns, n = 6, 1026
	x, C = k1.case_inputs((200, n, 2, 'float64', ns))
	e, ref, cnt, _ = setup(x, C, 256, ns)
	g, gw = e['geo'], k1.geometry(n, 384, ns)
	whole = np.zeros(gw['total'], dtype=np.int8)
	blk = e['d'][:, 128:256]
	first = (128 // 32) * gw['nks'] * 1024
	write_planes(whole, blk, 128, gw['cks'], gw['plane_bytes'], 0, base=first)
	assert np.array_equal(k1.decode_planes(whole, ns, 128, gw['nks'], plane_pitch=gw['plane_bytes'], offset=first), blk)
	full = k1.decode_planes(whole, ns, 384, gw['nks'])
	assert np.array_equal(full[:, 128:256], blk) and not full[:, :128].any() and not full[:, 256:].any()
	assert np.array_equal(k1.decode_planes(e['planes'], ns, 256, g['nks']), e['d'])


@pytest.mark.parametrize('n', [2051, 2052])
def test_exponent_rows_keep_their_margin_and_are_accepted(n):
	"""Every designated row of the exponent test is decided by the reference alone with a factor MARGIN to spare.  K1 sweeps a row unless share > 1 AND
	loose <= 1 (k1_longdouble.margins): 'tight' rows need share >= MARGIN and loose <= 1 / MARGIN, the others loose >= MARGIN or share <= 1 / MARGIN."""
	x, C, kind = k1.exponent_rows(n)
	e, ref, cnt, (C64, dci, rank) = setup(x, C)
	loose, share = k1.margins(ref, np.abs(C64).max(axis=1))
	for i, kd in enumerate(kind):
		if kd == 'tight':
			assert share[i] >= k1.MARGIN and loose[i] <= 1 / k1.MARGIN, (i, loose[i], share[i])
			assert abs(ref['est'][i] - ref['ss'][i]) <= 1e-6 * ref['ss'][i]  # the estimate the kernel decides with IS the sum of squares
		elif kd == 'zero':
			assert ref['raw'][i] == 0
		else:
			assert loose[i] >= k1.MARGIN or share[i] <= 1 / k1.MARGIN, (i, kd, loose[i], share[i])
	assert loose[13] < 0 or share[13] <= 1 / k1.MARGIN  # the explained row: nothing of |x|^2 is left
	# 1 lies between a tight row's largest |residual| and its bound, 1e-5 from either, a hundred million times their rounding errors (1e-13)
	m = ref['xmax'] + (np.abs(ref['b']) * np.abs(C64).max(axis=1)[None, :]).sum(axis=1)
	tight = np.array([kd == 'tight' for kd in kind])
	assert (ref["max"][tight] < 1 - 1e-5).all() and (m[tight] > 1 + 1e-5).all() and (m[tight] < 2).all()
	assert accepted(judge(e, ref, cnt))
	# an emulation that takes the accepted bound for the tight rows (one bit looser at most) passes as well; two bits looser than the rule allows does not
	for extra, ok in ((1, True), (5, False)):
		e2 = dict(e, exps=e['exps'] + np.where(np.arange(128) < 4, extra, 0).astype(np.int32))
		assert (k1.compare_exps(e2['exps'], e2['out'], ref, cnt, 6).ratio <= 1) == ok


@pytest.mark.parametrize('rows,n,dtype,const_last', [(r, n, t, cl) for r in (1, 5, 32) for n in (1, 1023, 1025, 3000) for t, cl in (('float64', 1), ('float32', 0))] +
						 [(5, 3000, 'float64', 0)])
def test_wide_cases_keep_their_margin_and_are_accepted(rows, n, dtype, const_last):
	x, C = k1.wide_rows(rows, n, dtype, const_last)
	C64, dci, rank = k1.prepare(C)
	ga, a = k1.wide_products(x, C64, const_last)
	ref = k1.reference(x, C64, dci, rank, a=a)
	cnt = k1.counts('wide', n, C64.shape[0], ref['active'], ldo=k1.round_up(n, 128))
	clear = k1.clear_expected(ref, cnt)
	assert (clear >= 0).all(), clear
	if rows >= 5 and n >= 1023 and dtype == 'float64':
		assert list(clear[:5]) == [0, 1, 1, 0, 0]
		assert 1e-19 < ref['ss'][3] / ref['raw'][3] < 1e-17  # "a row at 1e-18 of its norm"
	else:
		assert not clear.any() or n == 1  # (one cell: the intercept explains every row)
	e = emulate(x, C64, dci, rank, rows, 0, a=a, ldo=k1.round_up(n, 128))
	cleared = clear == 1
	e['out'][:rows][cleared] = 0
	e['ss'][:rows][cleared] = 0
	assert k1.compare_out(e['out'], ref, cnt, cleared).ratio <= 1 and k1.compare_ss(e['ss'], ref, cnt, cleared).ratio <= 1
	assert k1.compare_coef(e['coef'], ref, cnt).ratio <= 1
	if cleared.any() and n > 1:  # a kernel that does not clear is rejected
		e = emulate(x, C64, dci, rank, rows, 0, a=a, ldo=k1.round_up(n, 128))
		assert k1.compare_out(e['out'], ref, cnt, cleared).ratio > 1 and k1.compare_ss(e['ss'], ref, cnt, cleared).ratio > 1


# ---- the nine mutations --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def base():
	"""33 rows (row 9 has its halves swapped, row 32 opens a second block of 32) x 1027 cells (a tail of 3, 13 padding cells up to ldo = 1040), 2 covariates."""
	x, C = k1.case_inputs((33, 1027, 2, 'float64', 6))
	e, ref, cnt, cov = setup(x, C)
	assert accepted(judge(e, ref, cnt))
	return x, C, e, ref, cnt, cov


def rejected_by(w, name, what=None):
	assert w[name].ratio > 1, (name, w)
	assert what is None or w[name].what.startswith(what), w[name]
	return True


def test_mutation_last_tail_cell_left_out_of_a(base):
	x, C, e, ref, cnt, (C64, dci, rank) = base
	n = x.shape[1]
	assert n % 4
	m = emulate(x, C64, dci, rank, 128, 6, a=x[:, :n - 1] @ C64[:, :n - 1].T)
	assert rejected_by(judge(m, ref, cnt), 'coef', 'coef')


def test_mutation_row_residualised_with_its_neighbours_b(base):
	x, C, e, ref, cnt, (C64, dci, rank) = base
	m = emulate(x, C64, dci, rank, 128, 6, b_swap=(5, 6))
	w = judge(m, ref, cnt)
	assert rejected_by(w, 'out', 'out') and w['out'].where[0] == 5 and w['coef'].ratio <= 1


def test_mutation_one_residual_off_by_64_ulps(base):
	x, C, e, ref, cnt, _ = base
	bound = k1.gamma(cnt['res'], cnt['terms']) * ref['res_abs']
	i, k = np.unravel_index(int(np.argmax(np.abs(ref['res']) / ref['res_abs'])), bound.shape)
	m = dict(e, out=e['out'].copy())
	m['out'][i, k] += 64 * np.spacing(m['out'][i, k])
	w = judge(m, ref, cnt)
	assert rejected_by(w, 'out', 'out') and w['out'].where == (i, k)
	# ... and at EVERY element of the rows without active covariates, where the bound is zero: one ulp is enough
	xi, Ci = k1.case_inputs((5, 1027, 'inactive', 'float32', 6))
	ei, refi, cnti, _ = setup(xi, Ci)
	ei['out'][3, 77] += np.spacing(ei['out'][3, 77])
	assert k1.compare_out(ei['out'], refi, cnti).ratio == np.inf


def test_mutation_ss_summed_over_the_padding_of_a_buffer_that_is_not_zero(base):
	"""The sum of squares taken over ldo cells of a row buffer whose 13 cells past n hold a sentinel of the row's own size."""
	x, C, e, ref, cnt, _ = base
	n, ldo = x.shape[1], e['out'].shape[1]
	assert ldo - n == 13
	rms = np.sqrt(e['ss'][:33] / n)
	m = dict(e, ss=e['ss'].copy())
	m['ss'][:33] += (ldo - n) * (1e-3 * rms)**2  # 1.3e-8 of ss: a hundred thousand times the bound, a hundred times below the suite's 1e-6
	assert rejected_by(judge(m, ref, cnt), 'ss', 'ss')
	m = dict(e, ss=e['ss'].copy())
	m['ss'][40] = 1e-300
	assert rejected_by(judge(m, ref, cnt), 'ss', 'ss: padding row')


def test_mutation_halves_swapped_in_one_row(base):
	x, C, e, ref, cnt, _ = base
	g = e['geo']
	row = 9
	assert (row >> 3) & 1
	m = dict(e, planes=e['planes'].copy())
	img = m['planes'].reshape(6, 128 // 32, g['nks'], 32, 2, 16)
	img[2, 0, :32, row] = img[2, 0, :32, row, ::-1].copy()  # plane 2 only: a change of 2^-30 of the row's scale
	w = judge(m, ref, cnt)
	assert rejected_by(w, 'digits', 'digits: integer') and w['digits'].where[0] == row


def test_mutation_digit_off_by_one_without_carry(base):
	x, C, e, ref, cnt, _ = base
	m = dict(e, planes=e['planes'].copy())
	d0 = e['d'][0]
	i, k = np.argwhere((d0[:33, :1027] == 127))[0]  # rounding up here needs a carry into the next digit
	g = e['geo']
	off = (i >> 5) * g['cks'] * 1024 + 2 * (i & 31) * 16 + (k >> 5) * 1024 + ((((k & 31) >> 4) ^ ((i & 31) >> 3 & 1)) << 4) + (k & 15)
	assert m['planes'][off] == 127
	m['planes'][off] = -128  # 127 + 1 in a byte, the next digit untouched
	w = judge(m, ref, cnt)
	assert rejected_by(w, 'digits', 'digits: integer') and w['digits'].where == (i, k)
	m['planes'][off] = 126  # the lowest digit one short: 2^-46 of the row's scale
	assert rejected_by(judge(m, ref, cnt), 'digits', 'digits: integer')


def test_mutation_exponent_one_too_small(base):
	"""An exponent one below that of the row's maximum: |q| reaches 2^(8 NS - 2), the top digit leaves +-64."""
	x, C, e, ref, cnt, _ = base
	row = 4
	exps = e['exps'].copy()
	exps[row] -= 1
	o = np.zeros((128, e['geo']['nks'] * 32))
	o[:, :e['out'].shape[1]] = e['out']
	q, _ = model.quantise(o, 6, sh=exps.astype(np.int64))
	d = np.stack(model.digits(q, 6))
	assert np.abs(d[5, row]).max() > 64
	buf = np.zeros_like(e['planes'])
	write_planes(buf, d, 128, e['geo']['cks'], e['geo']['plane_bytes'], e['geo']['chunk_bytes'])
	w = judge(dict(e, exps=exps, planes=buf), ref, cnt)
	assert rejected_by(w, 'exps', 'exps: 2^(exps') and w['exps'].where == (row, )
	assert rejected_by(w, 'digits', 'digits: top digit')


def test_mutation_padding_row_with_a_digit(base):
	x, C, e, ref, cnt, _ = base
	for row, k, s in ((33, 0, 0), (127, 1039, 5)):
		m = dict(e, planes=e['planes'].copy())
		d = np.zeros_like(e['d'])
		d[s, row, k] = 1
		buf = np.zeros_like(e['planes'])
		write_planes(buf, d, 128, e['geo']['cks'], e['geo']['plane_bytes'], e['geo']['chunk_bytes'])
		m['planes'] += buf
		w = judge(m, ref, cnt)
		assert rejected_by(w, 'digits', 'digits: padding row') and w['digits'].where[0] == row
	# the same for a padding CELL of a live row (cells 1027 .. 1055 of the planes), for out and for the row records
	m = dict(e, planes=e['planes'].copy())
	d = np.zeros_like(e['d'])
	d[0, 2, 1050] = -1
	buf = np.zeros_like(e['planes'])
	write_planes(buf, d, 128, e['geo']['cks'], e['geo']['plane_bytes'], e['geo']['chunk_bytes'])
	m['planes'] += buf
	assert rejected_by(judge(m, ref, cnt), 'digits', 'digits: padding cell')
	m = dict(e, out=e['out'].copy(), fix=e['fix'].copy())
	m['out'][100, 5] = 1e-200
	m['fix'][64, 6] = 1.0
	w = judge(m, ref, cnt)
	assert rejected_by(w, 'out', 'out: padding row') and rejected_by(w, 'fix', 'fix: padding row')
	m = dict(e, out=e['out'].copy())
	m['out'][0, 1030] = -1e-200
	assert rejected_by(judge(m, ref, cnt), 'out', 'out: padding cell')


def test_mutation_chunk_at_the_wrong_offset(base):
	x, C, e0, ref, cnt, (C64, dci, rank) = base
	e = emulate(x, C64, dci, rank, 128, 6, chunks=3)
	g = e['geo']
	assert g['nchunks'] == 3 and accepted(judge(e, ref, cnt))
	for shift in (1024, -1024, g['plane_bytes']):  # one image late, one early, one plane late
		buf = np.zeros(g['total'] + 2 * g['plane_bytes'], dtype=np.int8)
		write_planes(buf, e['d'], 128, g['cks'], g['plane_bytes'], g['chunk_bytes'], base=g['plane_bytes'], shift_chunk=(1, shift))
		m = dict(e, planes=buf[g['plane_bytes']:g['plane_bytes'] + g['total']].copy())
		w = judge(m, ref, cnt)
		assert rejected_by(w, 'digits'), shift
	# the whole layout's bytes read as chunks are not the same digits either
	m = dict(e, planes=np.concatenate([e0['planes'], np.zeros(g['total'] - e0['planes'].size, dtype=np.int8)]))
	assert rejected_by(judge(m, ref, cnt), 'digits')


def test_row_records_of_a_wrong_row_are_rejected(base):
	x, C, e, ref, cnt, _ = base
	m = dict(e, fix=e['fix'].copy())
	m['fix'][[7, 8]] = m['fix'][[8, 7]]
	assert rejected_by(judge(m, ref, cnt), 'fix', 'fix: digit sums')
	m = dict(e, fix=e['fix'].copy())
	m['fix'][3, 5] *= 1 + 1e-5  # c formed from something else than this row's sum of squares
	assert rejected_by(judge(m, ref, cnt), 'fix', 'fix: c')


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------------------------------
def test_reference_against_the_oracle():
	"""b, the residual variances and -- through the oracle's alpha = b_y - gamma b_x and gamma -- the residuals' inner products, on a well-conditioned case."""
	import oracle
	rng = np.random.default_rng(5)
	n = 300
	x = k1.make_rows(rng, 6, n, 'float64')
	C = k1.make_covariates(rng, 3, n)
	C64, dci, rank = k1.prepare(C)
	ref = k1.reference(x, C64, dci, rank)
	dci_o, rank_o = oracle.inv_rank(np.matmul(C64, C64.T))
	assert rank_o == rank == 3
	_, _, p, gam, alpha, varx, vary = oracle.association_test_1(None, None, x, x, C64, dci_o, rank_o)
	ss = np.asarray(ref['ss'], dtype=np.float64)
	assert np.allclose(ss / n, varx, rtol=1e-12, atol=0)
	dot = np.asarray(ref['res'] @ ref['res'].T, dtype=np.float64)
	g_ref = dot / ss[:, None]  # gamma[i][j] = x~_j . x~_i / (n var_i)
	assert np.allclose(g_ref, gam, rtol=1e-10, atol=1e-13)
	b = np.asarray(ref['b'], dtype=np.float64)
	assert np.allclose(b[None, :, :] - g_ref[:, :, None] * b[:, None, :], alpha, rtol=1e-9, atol=1e-12)
	# and the absolute-value versions dominate what they bound
	assert (ref['a_abs'] >= np.abs(ref['a'])).all() and (ref['b_abs'] >= np.abs(ref['b'])).all() and (ref['res_abs'] >= np.abs(ref['res'])).all()
	assert (ref['ss_abs'] >= ref['ss_cross']).all() and (ref['ss_cross'] >= ref['ss']).all()
