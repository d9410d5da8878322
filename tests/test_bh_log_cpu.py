"""The ln form of bh and binnet (logp=True, p_kind = 1) without a device: the numpy restatement of the device algorithm
(tests/bh_log_numpy.py) against the definitions evaluated in longdouble -- integer stages exactly, ln q within the derived bound 2^-46 + 2^-52 |ln q| (+ 2^-24 |ln q|
for fp32) --, against the linear form where that can tell the P-values apart, and on the stored fixtures (G8_binnet, G25_logp_case); the host numpy form
_bh_host_log, weighted too; invalid entries; the new entries in header, ctypes table and library; the command line's --logp."""
import inspect
import os
import re

import numpy as np
import pytest

import bh_log_numpy as bl
import oracle
from normalisr_amd import _lib
from normalisr_amd import binnet as nb

TILE = 4096
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = {'nrm_bh_pk': 'nrm_bh', 'nrm_bh_host_pk': 'nrm_bh_host', 'nrm_binnet_pk': 'nrm_binnet', 'nrm_binnet_rows_pk': 'nrm_binnet_rows', 'nrm_binnet_host_pk': 'nrm_binnet_host'}


def same_bytes(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_entries_are_declared_exported_and_shaped_like_their_parents():
	hdr = open(os.path.join(HERE, '..', 'include', 'normalisr_hip.h')).read()
	lib = _lib.load()
	for new, old in ENTRIES.items():
		assert re.search(r'\b%s\(' % new, hdr) and new in _lib.exported_symbols() and hasattr(lib, new), new
		a, b = list(_lib._SIGNATURES[new][0]), list(_lib._SIGNATURES[old][0])
		# the parent's arguments with one int for p_kind, before the stream where there is one, else at the end
		assert (a[:-2] + a[-1:] == b and a[-2] is _lib._i32) if new in ('nrm_bh_pk', 'nrm_binnet_pk', 'nrm_binnet_rows_pk') else (a[:-1] == b and a[-1] is _lib._i32), new
	assert int(lib.nrm_bh_tile()) == TILE
	# p_kind is 0 or 1, checked before anything else
	assert lib.nrm_bh_pk(1, _lib.NRM_F64, 1, 8, 8, 1, 8, 1, 0, 1, 2, None) == _lib.NRM_E_ARG
	assert lib.nrm_binnet_rows_pk(1, _lib.NRM_F64, 1, 8, 8, 0, 0.1, 1, 8, 1, 1, -1, None) == _lib.NRM_E_ARG
	assert lib.nrm_bh_pk(None, _lib.NRM_F64, 1, 8, 8, None, 8, None, 0, None, 1, None) == _lib.NRM_E_ARG  # null pointers, as the parent
	for f in (nb.bh, nb.binnet):
		assert inspect.signature(f).parameters['logp'].default is False and 'logarithms' in f.__doc__ and 'logp=True' in f.__doc__


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', bl.sizes(TILE))
def test_restatement_against_longdouble(n, dtype):
	worst = (0.0, 0.0, None)
	for name, lnp in bl.cases(n, dtype, TILE).items():
		assert lnp.dtype == dtype and lnp.shape == (n, ) and (lnp <= 0).all(), name
		st = bl.stages(lnp)
		want, c = bl.exact(lnp)
		# integer stages: exactly
		assert np.array_equal(st['sorted'], np.sort(bl.keys(lnp))) and (np.diff(st['sorted'].astype(np.float64)) >= 0).all()
		assert np.array_equal(np.argsort(st['keys'], kind='stable'), np.argsort(lnp + dtype(0), kind='stable')), ('key order is ln P order', name, n)
		at = np.searchsorted(st['sorted'], st['keys'], side='left')
		assert np.array_equal(st['c'][at], c) and st['c'][-1] == n, ('c', name, n)
		assert np.array_equal(bl.values(st['keys'], dtype), lnp.astype(np.float64) + 0.0)
		# ln q: within the bound, against the definition; the host form as well
		for got in (st['out'], nb.bh(lnp, logp=True), nb.bh(lnp, on_device=False, logp=True)):
			assert got.dtype == dtype and got.shape == (n, )
			ex, err = bl.excess(got, want, dtype)
			if ex > worst[0]:
				worst = (ex, err, name)
			assert ex <= 1.0, (name, n, ex, err)
		out = st['out']
		assert (out[np.isneginf(lnp)] == -np.inf).all() and np.isfinite(out[np.isfinite(lnp)]).all() and (out <= 0).all()
		order = np.argsort(lnp, kind='stable')
		assert (out[order][1:] >= out[order][:-1]).all(), ('non-decreasing in the input', name, n)
		_, inv = np.unique(lnp + dtype(0), return_inverse=True)
		first = np.zeros(inv.max() + 1, dtype=np.int64)
		first[inv[::-1]] = np.arange(n)[::-1]
		assert same_bytes(out, out[first[inv]]), ('equal entries, equal bytes', name, n)
		top = lnp == lnp.max()
		assert same_bytes(out[top], (lnp[top] + dtype(0))), ('c = N leaves u itself', name, n)
	print('n = {} {}: largest |delta ln q| / bound = {:.3f} ({:.3e} absolute, {})'.format(n, np.dtype(dtype).name, *worst))


def test_tie_families_lie_where_they_claim():
	n = 3 * TILE + 17
	for dtype in bl.DTYPES:
		c = bl.cases(n, dtype, TILE)
		for name, (lo, hi) in bl.TIE_GROUPS(TILE).items():
			s = np.sort(c[name])
			assert (s[lo:hi] == s[lo]).all() and s[lo - 1] < s[lo] < s[hi] and np.unique(s).size == n - (hi - lo) + 1
		for b in range(np.dtype(dtype).itemsize):
			k = bl.keys(c['byte{}'.format(b)])
			mask = ~(bl.KEY[np.dtype(dtype)](0xff) << bl.KEY[np.dtype(dtype)](8 * b))
			assert np.unique(k & mask).size == 1 and np.unique(k).size > 32
		t = c['ties']
		assert np.isneginf(t).any() and (t == 0).any() and np.signbit(t[t == 0]).any() and not np.signbit(t[t == 0]).all()
		assert c['loguniform'].min() < -8e6 and c['loguniform'].max() > -1e-5


def test_against_the_linear_form_where_p_values_are_far_apart():
	"""ln P = -k 2^-6 for distinct integers k, with repeats: neighbouring P-values differ by a factor e^(1/64), so the linear form sees the same ties and the same
	counts wherever P is a normal number, and exp(ln q) equals its q to 1e-12 relative wherever q >= 1e-300."""
	rng = np.random.default_rng(17)
	k = rng.choice(60000, 3000, replace=False)
	k = np.concatenate([k, rng.choice(k, 2000), [0, 0]])
	lnp = -(k.astype(np.float64)) / 64
	q = oracle.bh(np.exp(lnp))
	for got in (bl.bh(lnp), nb.bh(lnp, logp=True)):
		m = q >= 1e-300
		assert m.sum() > 3000 and (~m).sum() > 100
		rel = np.abs(np.exp(got[m]) / q[m] - 1)
		print('exp(ln q) against the linear q: largest relative difference {:.3e}'.format(rel.max()))
		assert rel.max() <= 1e-12
		assert np.isfinite(got).all() and (got[~m] < np.log(1e-300) + 1e-9).all()


G8 = (('p', (('net_q5', 0.05), ('net_q20', 0.2), ('net_q50', 0.5))), ('p32', (('net32_q5', 0.05), ('net32_q30', 0.3))), ('pt', (('nett_q10', 0.1), ('nett_q25', 0.25))))
G25_EDGES = ((0.01, 28), (0.05, 34), (0.2, 54))


def test_ln_binnet_reproduces_the_stored_networks(golden):
	g = golden('G8_binnet')
	closest = np.inf
	for src, nets in G8:
		with np.errstate(divide='ignore'):
			lnp = np.log(g[src].astype(np.float64))
		assert np.isneginf(np.diag(lnp)).all()
		for name, q in nets:
			for dtype in bl.DTYPES:
				net, margin = bl.binnet(lnp.astype(dtype), q)
				assert net.shape == g[name].shape and np.array_equal(net, g[name]) and not net.diagonal().any(), (name, np.dtype(dtype).name)  # every row
				if dtype == np.float64:
					closest = min(closest, margin)
	print('G8: the closest pre-minimum ln q to ln qcut: {:.3e}'.format(closest))
	assert closest >= 1.9e-5
	c = golden('G25_logp_case')
	lnp = c['lnp_coex']
	closest = np.inf
	for q, edges in G25_EDGES:
		net, margin = bl.binnet(lnp, q)
		closest = min(closest, margin)
		assert int(net.sum()) == edges and np.array_equal(net, oracle.binnet(np.exp(lnp), q)), q
		assert np.array_equal(bl.binnet(lnp.astype(np.float32), q)[0], net)
	print('G25: the closest pre-minimum ln q to ln qcut: {:.3e}'.format(closest))
	assert closest >= 0.03  # (0.0348 over the three cutoffs and every row and distinct value; ten orders of magnitude above the arithmetic's error either way)


def test_ln_q_of_the_stored_de_case_is_finite_where_q_is_zero(golden):
	lnp = golden('G25_logp_case')['lnp_de'].ravel()
	q = oracle.bh(np.exp(lnp))
	zero = q == 0
	assert zero.sum() == 1
	for got in (bl.bh(lnp), nb.bh(lnp, logp=True)):
		assert np.isfinite(got).all() and -1560 < got[zero][0] < -1545
		err = np.abs(got[~zero] - np.log(q[~zero]))
		print('ln q against ln of the linear q: largest difference {:.3e}; ln q where q = 0: {:.4f}'.format(err.max(), got[zero][0]))
		assert err.max() <= 1e-14


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
def test_seeded_rows_of_every_policy_keep_clear_of_the_cutoff(dtype):
	"""What tests/test_gpu_binnet_log.py compares the device with: on these rows the restatement's closest |ln q - ln qcut| exceeds 1e-9 (the device's logarithms may
	differ from numpy's in the last place: 1e-15), so no row is left out there."""
	for ng in bl.ROW_WIDTHS[np.dtype(dtype)]:
		lnp, row0 = bl.rows_case(ng, dtype)
		assert lnp.shape == (3, ng) and lnp.dtype == dtype and np.isneginf(lnp[np.arange(3), row0 + np.arange(3)]).all() and (lnp <= 0).all()
		assert lnp[np.isfinite(lnp)].min() < -5e3 and (lnp == 0).any() and np.isneginf(lnp).sum() > 3
		net, margin = bl.binnet(lnp, bl.ROWS_QCUT, row0=row0)
		print('ng = {} {}: margin {:.3e}, {} edges'.format(ng, np.dtype(dtype).name, margin, int(net.sum())))
		assert margin > 1e-9 and 0 < net.sum() < net.size - 3 and not net[np.arange(3), row0 + np.arange(3)].any()


def test_invalid_entries_and_the_linear_assertions():
	good = np.array([-np.inf, -9e6, -1.5, -1.5, 0.0, -0.0])
	assert nb._lnp_within(good) and np.isneginf(nb.bh(good, logp=True)[0])
	for bad in (np.nan, 1e-300, np.inf):
		for dtype in (np.float64, np.float32):
			x = good.astype(dtype)
			x[2] = bad
			if x[2] == 0:
				continue  # (1e-300 is 0 in fp32: a valid entry)
			assert not nb._lnp_within(x)
			with pytest.raises(AssertionError):
				nb.bh(x, logp=True)
			with pytest.raises(AssertionError):
				nb.bh(x, weight=np.ones(x.size), logp=True)
	# ln P without logp=True is still refused by the linear assertion
	with pytest.raises(AssertionError):
		nb.bh(good)
	with pytest.raises(AssertionError):
		nb.bh(good[1:])
	with pytest.raises(AssertionError):
		nb.bh(np.zeros((2, 2)), logp=True)  # the host path keeps the 1-D assertion
	with pytest.raises(AssertionError):
		nb.bh(np.array([0, -1, -1]), logp=True)  # integers are no ln P
	# binnet checks its arguments before any device call, with and without logp
	for ka in ({}, {'logp': True}):
		with pytest.raises(ValueError):
			nb.binnet(np.zeros((3, 4)), 0.1, **ka)
		with pytest.raises(ValueError):
			nb.binnet(np.zeros((3, 3)), 1.0, **ka)


def test_identical_entries_warn(caplog):
	import logging
	with caplog.at_level(logging.WARNING):
		out = nb.bh(np.full(5, -2.5), logp=True)
	assert 'Identical p-value in all entries.' in caplog.text and same_bytes(out, np.full(5, -2.5))
	caplog.clear()
	with caplog.at_level(logging.WARNING):
		nb.bh(np.array([0.0, -0.0]), logp=True)
	assert 'Identical p-value in all entries.' in caplog.text  # both zeros are ln 1


def test_weighted_host_form_against_longdouble():
	rng = np.random.default_rng(23)
	lnp = -np.round(10.0 ** rng.uniform(-2, 3.5, 400), 1)
	lnp[:3] = -np.inf
	lnp[3:6] = 0.0
	w = rng.random(400) + 0.1
	w[0] = 0.0
	for dtype in bl.DTYPES:
		x = lnp.astype(dtype)
		got = nb.bh(x, weight=w, logp=True)
		u, ids = np.unique(x.astype(np.longdouble), return_inverse=True)
		cw = np.zeros(u.size, dtype=np.longdouble)
		np.add.at(cw, ids, w.astype(np.longdouble))
		cw = np.cumsum(cw)
		lq = u - np.log(cw / cw[-1])
		lq = np.where(lq < 0, lq, np.longdouble(0))
		lq = np.minimum.accumulate(lq[::-1])[::-1][ids]
		assert got.dtype == dtype and (got[:3] == -np.inf).all()
		ex, err = bl.excess(got, lq, dtype)
		print('weighted, {}: largest |delta ln q| / bound = {:.3f} ({:.3e})'.format(np.dtype(dtype).name, ex, err))
		assert ex <= 1.0
		# unit weights: the unweighted form
		ex, _ = bl.excess(nb.bh(x, weight=np.ones(400), logp=True), bl.exact(x)[0], dtype)
		assert ex <= 1.0
	# against the linear weighted form where P is a normal number
	x = -rng.choice(2000, 300).astype(np.float64) / 8
	q = oracle.bh(np.exp(x), weight=w[:300])
	assert np.abs(np.exp(nb.bh(x, weight=w[:300], logp=True)) / q - 1).max() < 1e-12


def test_cli_takes_logp():
	from normalisr_amd.__main__ import build_parser
	from normalisr_amd import run
	p = build_parser()
	a = vars(p.parse_args(['bh', 'p.tsv', 'q.tsv', '--logp']))
	assert a['cmd'] == 'bh' and a['logp'] is True and vars(p.parse_args(['bh', 'p.tsv', 'q.tsv']))['logp'] is None
	a = vars(p.parse_args(['binnet', 'p.tsv', 'n.tsv', '0.05', '--logp']))
	assert a['cmd'] == 'binnet' and a['logp'] is True and a['qcut'] == 0.05 and vars(p.parse_args(['binnet', 'p.tsv', 'n.tsv', '0.05']))['logp'] is None
	for cmd in ('bh', 'binnet'):
		assert run.COMMANDS[cmd]['options']['logp'] == ('logp', bool)


def test_text_input_reads_minus_inf(tmp_path):
	"""What `coex --logp` writes on the diagonal, -INF, reads back as -inf: the text route of `normalisr binnet --logp`."""
	from normalisr_amd import run
	a = np.array([[-np.inf, -12.5, -0.0], [-12.5, -np.inf, -745.25], [0.0, -745.25, -np.inf]])
	f = str(tmp_path / 'lnp.tsv')
	run.file_write_tsv(f, a)
	assert b'-INF' in open(f, 'rb').read()
	assert np.array_equal(run.file_read_tsv(f), a)
