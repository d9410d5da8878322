"""The ln form of bh on the device (binnet.bh(..., logp=True); nrm_bh_pk with p_kind = 1, csrc/nrm_bh.hip) against the numpy restatement
(tests/bh_log_numpy.py) and the definition in longdouble.  The integer stages a finished call leaves in its workspace (nrm_bh_layout: sorted keys, c) match the
restatement in bytes; ln q per sorted position and the output lie within the derived bound 2^-46 + 2^-52 |ln q| (+ 2^-24 |ln q| for fp32) of the longdouble value
-- the device's logarithm may differ from numpy's in the last place, so ln q is not compared in bytes --; equal entries get equal bytes.  Pitched, in-place and
unaligned calls; invalid entries; the numpy and whole-problem-entry routes; the command line in a child that cannot import torch; a captured graph replayed over
rewritten input."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import bh_log_numpy as bl
from normalisr_amd import _lib
from normalisr_amd import binnet as nb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WARNING = 'Identical p-value in all entries.'
_REF = {}


def _engine():
	from normalisr_amd import engine
	return engine.get_engine()


def tile():
	return int(_lib.load().nrm_bh_tile())


def same_bytes(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def reference(n, dtype, name, lnp):
	"""(ln q in longdouble by the definition, the restatement's stages) of a generator case, computed once per session."""
	key = (n, np.dtype(dtype).name, name)
	if key not in _REF:
		want = bl.exact(lnp)[0]
		want.setflags(write=False)
		_REF[key] = (want, bl.stages(lnp))
	return _REF[key]


def call(eng, d_p, rows, cols, ldp, d_q, ldq, stream=None, p_kind=1):
	"""nrm_bh_pk with a workspace and flags of the test's own -> (workspace, flags), nothing synchronised."""
	torch, lib = eng.torch, eng.lib
	code = _lib.NRM_F64 if d_p.dtype == torch.float64 else _lib.NRM_F32
	nbytes = int(lib.nrm_bh_workspace_bytes(rows * cols, code))
	assert nbytes > 0
	work = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
	flags = torch.full((2, ), -1, dtype=torch.int32, device=eng.device)
	_lib.check(lib.nrm_bh_pk(d_p.data_ptr(), code, rows, cols, ldp, d_q.data_ptr(), ldq, work.data_ptr(), nbytes, flags.data_ptr(), p_kind,
							 eng._stream() if stream is None else stream))
	return work, flags


def left_in_workspace(eng, work, n, dtype):
	dt = np.dtype(dtype)
	off = (ctypes.c_int64 * 4)()
	_lib.check(eng.lib.nrm_bh_layout(n, _lib.NRM_F64 if dt == np.float64 else _lib.NRM_F32, off))
	w = work.cpu().numpy()
	return (w[off[0]:off[0] + n * dt.itemsize].view(bl.KEY[dt]), w[off[1]:off[1] + 4 * n].view(np.uint32), w[off[2]:off[2] + n * dt.itemsize].view(dt))


def within(got, want, dtype, what, worst):
	ex, err = bl.excess(got, want, dtype)
	if ex > worst[0]:
		worst[:] = [ex, err, what]
	assert ex <= 1.0, (what, ex, err)


def equal_entries_equal_bytes(lnp, out):
	_, inv = np.unique(lnp + lnp.dtype.type(0), return_inverse=True)
	first = np.zeros(inv.max() + 1, dtype=np.int64)
	first[inv[::-1]] = np.arange(lnp.size)[::-1]
	return same_bytes(out, out[first[inv]])


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', bl.sizes(4096))
def test_ln_bh_stage_by_stage(n, dtype, caplog):
	eng = _engine()
	torch = eng.torch
	T = tile()
	assert n in bl.sizes(T)
	worst = [0.0, 0.0, None]
	for name, lnp in bl.cases(n, dtype, T).items():
		want, st = reference(n, dtype, name, lnp)
		d_p = eng.upload(lnp)
		caplog.clear()
		with caplog.at_level(logging.WARNING):
			q = nb.bh(d_p, logp=True)
		assert q.is_cuda and q.dtype == d_p.dtype and q.shape == d_p.shape and same_bytes(eng.download(d_p), lnp)
		identical = np.unique(bl.keys(lnp)).size == 1
		assert (WARNING in caplog.text) == identical, (name, n)
		out = torch.empty_like(d_p)
		work, flags = call(eng, d_p, 1, n, n, out, n)
		assert flags.tolist() == [0, 0 if identical else 1], (name, n)
		skeys, c, qs = left_in_workspace(eng, work, n, dtype)
		assert np.array_equal(skeys, st['sorted']), ('sorted keys', name, n)
		assert np.array_equal(c, st['c']), ('c', name, n)
		within(qs, np.sort(want), dtype, ('ln q per sorted position', name, n), worst)  # (ln q is non-decreasing in ln P: the sorted positions hold the sorted values)
		assert (qs[1:] >= qs[:-1]).all(), ('suffix minimum', name, n)
		got = out.cpu().numpy()
		within(got, want, dtype, ('look-up', name, n), worst)
		assert same_bytes(got, qs[np.searchsorted(st['sorted'], st['keys'], side='left')]), ('look-up', name, n)
		assert same_bytes(q.cpu().numpy(), got), (name, n)
		assert equal_entries_equal_bytes(lnp, got), (name, n)
		assert (got[np.isneginf(lnp)] == -np.inf).all() and np.isfinite(got[np.isfinite(lnp)]).all() and (got <= 0).all()
		top = lnp == lnp.max()
		assert same_bytes(got[top], lnp[top] + dtype(0)), ('c = N leaves u itself', name, n)
	print('n = {} {}: largest |delta ln q| / bound = {:.3f} ({:.3e} absolute, {})'.format(n, np.dtype(dtype).name, *worst))


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
def test_ln_bh_pitched_in_place_unaligned_and_repeated(dtype):
	eng = _engine()
	rows, cols, ld = 37, 333, 350  # 12 321 entries: more than three tiles
	rng = np.random.default_rng(5)
	wide = (-10.0 ** rng.uniform(-3, 3, (rows, ld))).astype(dtype)
	wide[:, 5:5 + cols] = np.round(wide[:, 5:5 + cols], 1)  # heavy ties, zeros among them
	wide[3, 7] = -np.inf
	lnp = np.ascontiguousarray(wide[:, 5:5 + cols])
	want = bl.exact(lnp.ravel())[0].reshape(rows, cols)
	d_wide = eng.upload(wide)
	d_p = d_wide[:, 5:5 + cols]
	assert d_p.stride(0) == ld and d_p.data_ptr() % 16 != 0
	q = nb.bh(d_p, logp=True)
	ref = q.cpu().numpy()
	assert q.shape == (rows, cols) and bl.excess(ref, want, dtype)[0] <= 1.0 and equal_entries_equal_bytes(lnp.ravel(), ref.ravel())
	assert same_bytes(nb.bh(d_p, logp=True).cpu().numpy(), ref)  # twice: the same bytes
	assert same_bytes(d_wide.cpu().numpy(), wide)  # the input is left alone
	flat = eng.upload(np.concatenate([[-0.5], lnp.ravel()]).astype(dtype))
	assert flat[1:].data_ptr() % 16 != 0
	for t in (eng.upload(lnp), eng.upload(lnp.ravel()), flat[1:]):
		assert same_bytes(nb.bh(t, logp=True).cpu().numpy().ravel(), ref.ravel())  # the vector loads and the element loads: the same bytes
	work, flags = call(eng, d_p, rows, cols, ld, d_p, ld)  # in place, pitched: the columns outside the slice keep their bytes
	expect = wide.copy()
	expect[:, 5:5 + cols] = ref
	assert flags.tolist() == [0, 1] and same_bytes(d_wide.cpu().numpy(), expect)
	d_c = eng.upload(lnp)
	work, flags = call(eng, d_c, rows, cols, cols, d_c, cols)  # in place, contiguous
	assert same_bytes(d_c.cpu().numpy(), ref)
	assert eng.lib.nrm_bh_pk(d_p.data_ptr(), _lib.NRM_F64, rows, cols, ld, d_p.data_ptr(), cols, work.data_ptr(), work.numel(), flags.data_ptr(), 1, None) == _lib.NRM_E_ARG


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
def test_ln_bh_invalid_entries_raise_and_leave_nothing_behind(dtype):
	eng = _engine()
	n = 3 * tile() + 17
	lnp = bl.cases(n, dtype, tile())['loguniform']
	ref = nb.bh(eng.upload(lnp), logp=True).cpu().numpy()
	for bad in (np.nan, 1e-30, np.inf):
		for pos in (0, n - 1, n // 2 + 1):
			x = lnp.copy()
			x[pos] = bad
			with pytest.raises(AssertionError):
				nb.bh(eng.upload(x), logp=True)
			with pytest.raises(AssertionError):
				nb.bh(x, on_device=True, logp=True)
		assert same_bytes(nb.bh(eng.upload(lnp), logp=True).cpu().numpy(), ref), bad
	# ln P without logp=True is refused by the linear form's assertion, on every route; P-values above 0 are refused by the ln form
	with pytest.raises(AssertionError):
		nb.bh(eng.upload(lnp))
	with pytest.raises(AssertionError):
		nb.bh(lnp, on_device=True)
	with pytest.raises(AssertionError):
		nb.bh(eng.upload(np.exp(lnp.astype(np.float64)).astype(dtype) + dtype(0.25)), logp=True)


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
def test_ln_bh_numpy_on_device_and_host_entry_routes(dtype, monkeypatch, caplog):
	eng = _engine()
	T = tile()
	n = 3 * T + 17
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	for name in ('ties', 'tie_whole_tiles', 'identical'):
		lnp = bl.cases(n, dtype, T)[name]
		want, _ = reference(n, dtype, name, lnp)
		ref = nb.bh(eng.upload(lnp), logp=True).cpu().numpy()
		assert bl.excess(ref, want, dtype)[0] <= 1.0
		for entry in (None, '1'):
			if entry:
				monkeypatch.setenv('NRM_HOST_ENTRY', entry)
			caplog.clear()
			with caplog.at_level(logging.WARNING):
				q = nb.bh(lnp, on_device=True, logp=True)
				q2 = nb.bh(lnp.reshape(-1, 1), on_device=True, logp=True)
			assert isinstance(q, np.ndarray) and same_bytes(q, ref) and same_bytes(q2, ref.reshape(-1, 1)), (name, entry)
			assert (WARNING in caplog.text) == (name == 'identical')
			monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
		assert bl.excess(nb.bh(lnp, logp=True), want, dtype)[0] <= 1.0  # the host numpy form
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	bad = lnp.copy()
	bad[7] = 1.5
	with pytest.raises(AssertionError, match='ln P-values must be <= 0'):
		nb.bh(bad, on_device=True, logp=True)
	monkeypatch.delenv('NRM_HOST_ENTRY')


def test_ln_bh_with_weights_goes_through_the_host():
	eng = _engine()
	rng = np.random.default_rng(3)
	lnp = -np.round(10.0 ** rng.uniform(-2, 3, (9, 41)), 1)
	w = rng.random((9, 41)) + 0.1
	q = nb.bh(eng.upload(lnp), weight=eng.upload(w), logp=True)
	assert q.is_cuda and q.shape == (9, 41) and same_bytes(q.cpu().numpy().ravel(), nb.bh(lnp.ravel(), weight=w.ravel(), logp=True))


def test_ln_bh_cli_in_a_child_that_cannot_import_torch(tmp_path):
	from normalisr_amd import run
	eng = _engine()
	rng = np.random.default_rng(11)
	m64 = -np.round(10.0 ** rng.uniform(-2, 4, (23, 57)), 2)
	m64[2, 3] = -np.inf  # written as -INF
	m32 = (-10.0 ** rng.uniform(-3, 6, (5, 1000))).astype(np.float32)
	files, args = {}, []
	for stem, m, ext in (('a', m64, '.npy'), ('b', m32, '.npy'), ('c', m64, '.tsv'), ('d', m64[3], '.tsv.gz')):
		files[stem] = (str(tmp_path / (stem + '_p' + ext)), str(tmp_path / (stem + '_q' + ext)))
		run.file_write_tsv(files[stem][0], m)
		args += ['bh', files[stem][0], files[stem][1], '-']
	env = {k: v for k, v in os.environ.items() if k != 'NRM_HOST_ENTRY'}
	r = subprocess.run([sys.executable, os.path.join(HERE, 'bh_log_cli_child.py')] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
	assert r.returncode == 0 and 'child ok' in r.stdout, r.stdout[-3000:]
	for stem in files:
		pin, got = run.file_read_tsv(files[stem][0]), run.file_read_tsv(files[stem][1])  # (text: ln P as the command read it, %.8G)
		want = nb.bh(eng.upload(pin.ravel()), logp=True).cpu().numpy().reshape(pin.shape)
		assert bl.excess(want, bl.exact(pin.ravel())[0], pin.dtype)[0] <= 1.0
		if files[stem][1].endswith('.npy'):
			assert same_bytes(got, want), stem
		else:
			text = str(tmp_path / (stem + '_want' + os.path.splitext(files[stem][1])[1].replace('.gz', '.tsv')))
			run.file_write_tsv(text, want)
			assert got.shape == want.shape and same_bytes(got, run.file_read_tsv(text)), stem
	assert np.isneginf(run.file_read_tsv(files['c'][1])[2, 3])


def test_ln_bh_captured_in_a_graph_follows_rewritten_input():
	"""nrm_bh_pk with p_kind = 1 recorded into a graph on a side stream, replayed twice with the input rewritten in place in between: the launch sequence depends on
	(N, dtype, p_kind) only and nothing is read back."""
	eng = _engine()
	torch = eng.torch
	T = tile()
	n = 3 * T + 17
	for dtype in bl.DTYPES:
		c = bl.cases(n, dtype, T)
		d_p = eng.upload(c['uniform'])
		out = torch.empty_like(d_p)
		side = torch.cuda.Stream(device=eng.device)
		side.wait_stream(torch.cuda.current_stream(eng.device))
		with torch.cuda.stream(side):
			work, flags = call(eng, d_p, 1, n, n, out, n, stream=side.cuda_stream)  # (warm-up: the kernels' code objects are loaded)
			side.synchronize()
			assert bl.excess(out.cpu().numpy(), reference(n, dtype, 'uniform', c['uniform'])[0], dtype)[0] <= 1.0
			code = _lib.NRM_F64 if dtype == np.float64 else _lib.NRM_F32
			g = torch.cuda.CUDAGraph()
			with torch.cuda.graph(g, stream=side):
				_lib.check(eng.lib.nrm_bh_pk(d_p.data_ptr(), code, 1, n, n, out.data_ptr(), n, work.data_ptr(), work.numel(), flags.data_ptr(), 1,
											 torch.cuda.current_stream(eng.device).cuda_stream))
		torch.cuda.synchronize()
		for name in ('tie_whole_tiles', 'ties'):
			d_p.copy_(torch.from_numpy(c[name]))
			out.zero_()
			torch.cuda.synchronize()
			g.replay()
			torch.cuda.synchronize()
			got = out.cpu().numpy()
			assert bl.excess(got, reference(n, dtype, name, c[name])[0], dtype)[0] <= 1.0, (name, np.dtype(dtype).name)
			assert same_bytes(got, nb.bh(eng.upload(c[name]), logp=True).cpu().numpy()) and flags.tolist() == [0, 1]
		del g
