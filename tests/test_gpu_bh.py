"""bh on the device (normalisr_amd/binnet.py: bh; csrc/nrm_bh.hip) against the reference's steps (oracle.bh, binnet.py:77-131).  Every comparison is bit for bit: the
contract has one division per step in the input's dtype and an exact minimum.  The final answer for every (N, family, dtype) of tests/bh_numpy.py, and the stages a
finished call leaves in its workspace (nrm_bh_layout: sorted keys, c, q per sorted position) against the numpy restatement, so that a wrong answer names its stage;
pitched and in-place calls; invalid entries at the first, last and a middle position; the numpy and whole-problem-entry routes; the command line in a child that
cannot import torch; weights through the documented download; nrm_bh captured into a graph and replayed over rewritten input."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import bh_numpy
import oracle
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


def reference(n, dtype, name, pv):
	"""oracle.bh of a generator case, computed once per session."""
	key = (n, np.dtype(dtype).name, name)
	if key not in _REF:
		_REF[key] = oracle.bh(pv)
		_REF[key].setflags(write=False)
	return _REF[key]


def call(eng, d_p, rows, cols, ldp, d_q, ldq, stream=None):
	"""nrm_bh with a workspace and flags of the test's own -> (workspace, flags), nothing synchronised."""
	torch, lib = eng.torch, eng.lib
	code = _lib.NRM_F64 if d_p.dtype == torch.float64 else _lib.NRM_F32
	nbytes = int(lib.nrm_bh_workspace_bytes(rows * cols, code))
	assert nbytes > 0
	work = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
	flags = torch.full((2, ), -1, dtype=torch.int32, device=eng.device)
	_lib.check(lib.nrm_bh(d_p.data_ptr(), code, rows, cols, ldp, d_q.data_ptr(), ldq, work.data_ptr(), nbytes, flags.data_ptr(), eng._stream() if stream is None else stream))
	return work, flags


def left_in_workspace(eng, work, n, dtype):
	"""(sorted keys, c, q per sorted position) as nrm_bh_layout places them."""
	dt = np.dtype(dtype)
	off = (ctypes.c_int64 * 4)()
	_lib.check(eng.lib.nrm_bh_layout(n, _lib.NRM_F64 if dt == np.float64 else _lib.NRM_F32, off))
	assert off[3] == 0
	w = work.cpu().numpy()
	return (w[off[0]:off[0] + n * dt.itemsize].view(bh_numpy.KEY[dt]), w[off[1]:off[1] + 4 * n].view(np.uint32), w[off[2]:off[2] + n * dt.itemsize].view(dt))


@pytest.mark.parametrize('dtype', bh_numpy.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', bh_numpy.sizes(4096))
def test_bh_tensor_equals_reference_bit_for_bit_stage_by_stage(n, dtype, caplog):
	eng = _engine()
	torch = eng.torch
	T = tile()
	assert n in bh_numpy.sizes(T)  # (the sizes are laid around the tile this build reports)
	for name, pv in bh_numpy.cases(n, dtype, T).items():
		ref = reference(n, dtype, name, pv)
		d_p = eng.upload(pv)
		caplog.clear()
		with caplog.at_level(logging.WARNING):
			q = nb.bh(d_p)
		assert q.is_cuda and q.dtype == d_p.dtype and q.shape == d_p.shape and same_bytes(eng.download(d_p), pv)
		identical = np.unique(bh_numpy.keys(pv)).size == 1
		assert (WARNING in caplog.text) == identical, (name, n)
		# the stages first: a wrong final answer then names the stage that broke
		st = bh_numpy.stages(pv)
		out = torch.empty_like(d_p)
		work, flags = call(eng, d_p, 1, n, n, out, n)
		assert flags.tolist() == [0, 0 if identical else 1], (name, n)
		skeys, c, qs = left_in_workspace(eng, work, n, dtype)
		assert np.array_equal(skeys, np.sort(bh_numpy.keys(pv))), ('sorted keys', name, n)
		assert np.array_equal(c, st['c']), ('c', name, n)
		assert same_bytes(qs, st['q']), ('q per sorted position', name, n)
		assert same_bytes(out.cpu().numpy(), ref), ('look-up', name, n)
		assert same_bytes(q.cpu().numpy(), ref), (name, n)


@pytest.mark.parametrize('dtype', bh_numpy.DTYPES, ids=lambda d: np.dtype(d).name)
def test_bh_pitched_in_place_unaligned_and_repeated(dtype):
	eng = _engine()
	torch = eng.torch
	rows, cols, ld = 37, 333, 350  # 12 321 entries: more than three tiles
	rng = np.random.default_rng(5)
	wide = rng.random((rows, ld)).astype(dtype)
	wide[:, 5:5 + cols] = np.round(wide[:, 5:5 + cols], 2)  # heavy ties
	pv = np.ascontiguousarray(wide[:, 5:5 + cols])
	ref = oracle.bh(pv.ravel()).reshape(rows, cols)
	d_wide = eng.upload(wide)
	d_p = d_wide[:, 5:5 + cols]  # a column slice of a wider result: pitch 350, rows not 16-byte aligned
	assert d_p.stride(0) == ld and d_p.data_ptr() % 16 != 0
	q = nb.bh(d_p)
	assert q.shape == (rows, cols) and same_bytes(q.cpu().numpy(), ref)
	assert same_bytes(nb.bh(d_p).cpu().numpy(), q.cpu().numpy())  # twice: the same bytes
	assert same_bytes(d_wide.cpu().numpy(), wide)  # the input is left alone
	# a contiguous 2-D tensor, a 1-D one, and a 1-D one that starts off a 16-byte boundary (the element loads)
	flat = eng.upload(np.concatenate([[0.5], pv.ravel()]).astype(dtype))
	assert flat[1:].data_ptr() % 16 != 0
	for t in (eng.upload(pv), eng.upload(pv.ravel()), flat[1:]):
		assert same_bytes(nb.bh(t).cpu().numpy().ravel(), ref.ravel())
	# in place, pitched: the columns outside the slice keep their bytes
	work, flags = call(eng, d_p, rows, cols, ld, d_p, ld)
	got = d_wide.cpu().numpy()
	want = wide.copy()
	want[:, 5:5 + cols] = ref
	assert flags.tolist() == [0, 1] and same_bytes(got, want)
	# in place, contiguous
	d_c = eng.upload(pv)
	work, flags = call(eng, d_c, rows, cols, cols, d_c, cols)
	assert same_bytes(d_c.cpu().numpy(), ref)
	# unequal pitches in place are refused before anything is queued
	assert eng.lib.nrm_bh(d_p.data_ptr(), _lib.NRM_F64, rows, cols, ld, d_p.data_ptr(), cols, work.data_ptr(), work.numel(), flags.data_ptr(), None) == _lib.NRM_E_ARG


@pytest.mark.parametrize('dtype', bh_numpy.DTYPES, ids=lambda d: np.dtype(d).name)
def test_bh_invalid_entries_raise_and_leave_nothing_behind(dtype):
	eng = _engine()
	n = 3 * tile() + 17
	pv = bh_numpy.cases(n, dtype, tile())['loguniform']
	ref = reference(n, dtype, 'loguniform', pv)
	one = np.dtype(dtype).type(1)
	for bad in (np.nan, np.inf, -1e-3, np.nextafter(one, one * 2)):
		for pos in (0, n - 1, n // 2 + 1):
			x = pv.copy()
			x[pos] = bad
			with pytest.raises(AssertionError):
				nb.bh(eng.upload(x))
			with pytest.raises(AssertionError):
				nb.bh(x, on_device=True)
		assert same_bytes(nb.bh(eng.upload(pv)).cpu().numpy(), ref), bad  # a valid call afterwards: flags cleared, nothing left in the workspace


@pytest.mark.parametrize('dtype', bh_numpy.DTYPES, ids=lambda d: np.dtype(d).name)
def test_bh_numpy_on_device_and_host_entry_routes(dtype, monkeypatch, caplog):
	T = tile()
	n = 3 * T + 17
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	for name in ('ties', 'tie_whole_tiles', 'identical'):
		pv = bh_numpy.cases(n, dtype, T)[name]
		ref = reference(n, dtype, name, pv)
		for entry in (None, '1'):
			if entry:
				monkeypatch.setenv('NRM_HOST_ENTRY', entry)
			caplog.clear()
			with caplog.at_level(logging.WARNING):
				q = nb.bh(pv, on_device=True)
				q2 = nb.bh(pv.reshape(-1, 1), on_device=True)
			assert isinstance(q, np.ndarray) and same_bytes(q, ref) and same_bytes(q2, ref.reshape(-1, 1)), (name, entry)
			assert (WARNING in caplog.text) == (name == 'identical')
			monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	bad = pv.copy()
	bad[7] = 1.5
	with pytest.raises(AssertionError, match='P-values must be finite'):
		nb.bh(bad, on_device=True)
	monkeypatch.delenv('NRM_HOST_ENTRY')


def test_bh_with_weights_goes_through_the_host():
	eng = _engine()
	rng = np.random.default_rng(3)
	pv = np.round(rng.random((9, 41)), 2)
	w = rng.random((9, 41)) + 0.1
	q = nb.bh(eng.upload(pv), weight=eng.upload(w))
	assert q.is_cuda and q.shape == (9, 41) and same_bytes(q.cpu().numpy().ravel(), nb.bh(pv.ravel(), weight=w.ravel()))
	q = nb.bh(eng.upload(pv.ravel()), weight=w.ravel())
	assert same_bytes(q.cpu().numpy(), nb.bh(pv.ravel(), weight=w.ravel()))
	with pytest.raises(TypeError):
		nb.bh(eng.upload(np.array([0, 1, 1])))  # an integer tensor: what the host path raises


def test_bh_cli_in_a_child_that_cannot_import_torch(tmp_path):
	from normalisr_amd import run
	rng = np.random.default_rng(11)
	m64 = np.round(10.0 ** (-6 * rng.random((23, 57))), 4)
	m32 = rng.random((5, 1000)).astype(np.float32)
	files = {}
	for stem, m, ext in (('a', m64, '.npy'), ('b', m32, '.npy'), ('c', m64, '.tsv'), ('d', m64[3], '.tsv.gz')):
		files[stem] = (str(tmp_path / (stem + '_p' + ext)), str(tmp_path / (stem + '_q' + ext)))
		run.file_write_tsv(files[stem][0], m)
	args = [f for pair in files.values() for f in pair]
	env = {k: v for k, v in os.environ.items() if k != 'NRM_HOST_ENTRY'}
	r = subprocess.run([sys.executable, os.path.join(HERE, 'bh_cli_child.py')] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
	assert r.returncode == 0 and 'child ok' in r.stdout, r.stdout[-3000:]
	for stem in files:
		pin, got = run.file_read_tsv(files[stem][0]), run.file_read_tsv(files[stem][1])  # (text: the P-values as the command read them, %.8G)
		want = nb.bh(pin.ravel()).reshape(pin.shape)
		if files[stem][1].endswith('.npy'):
			assert same_bytes(got, want), stem
		else:
			text = str(tmp_path / (stem + '_want' + os.path.splitext(files[stem][1])[1].replace('.gz', '.tsv')))
			run.file_write_tsv(text, want)
			assert got.shape == want.shape and same_bytes(got, run.file_read_tsv(text)), stem


def test_bh_captured_in_a_graph_follows_rewritten_input():
	"""nrm_bh recorded into a graph on a side stream, replayed twice with the input rewritten in place in between: the launch sequence holds no host-side decision
	and no read-back (either would end the capture with an error)."""
	eng = _engine()
	torch = eng.torch
	T = tile()
	n = 3 * T + 17
	for dtype in bh_numpy.DTYPES:
		c = bh_numpy.cases(n, dtype, T)
		first, second, third = c['uniform'], c['tie_whole_tiles'], c['ties']
		d_p = eng.upload(first)
		out = torch.empty_like(d_p)
		side = torch.cuda.Stream(device=eng.device)
		side.wait_stream(torch.cuda.current_stream(eng.device))
		with torch.cuda.stream(side):
			work, flags = call(eng, d_p, 1, n, n, out, n, stream=side.cuda_stream)  # (warm-up: the kernels' code objects are loaded)
			side.synchronize()
			assert same_bytes(out.cpu().numpy(), reference(n, dtype, 'uniform', first))
			code = _lib.NRM_F64 if dtype == np.float64 else _lib.NRM_F32
			g = torch.cuda.CUDAGraph()
			with torch.cuda.graph(g, stream=side):
				_lib.check(eng.lib.nrm_bh(d_p.data_ptr(), code, 1, n, n, out.data_ptr(), n, work.data_ptr(), work.numel(), flags.data_ptr(), torch.cuda.current_stream(eng.device).cuda_stream))
		torch.cuda.synchronize()
		for name, pv in (('tie_whole_tiles', second), ('ties', third)):
			d_p.copy_(torch.from_numpy(pv))
			out.zero_()
			torch.cuda.synchronize()
			g.replay()
			torch.cuda.synchronize()
			assert same_bytes(out.cpu().numpy(), reference(n, dtype, name, pv)), (name, np.dtype(dtype).name)
			assert flags.tolist() == [0, 1]
		del g
