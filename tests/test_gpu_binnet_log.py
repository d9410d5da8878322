"""The ln form of binnet on the device (binnet.binnet(..., logp=True); nrm_binnet_pk / nrm_binnet_rows_pk / nrm_binnet_host_pk with p_kind = 1, csrc/nrm_binnet.hip;
DESIGN.md section 4g): the stored networks of G8_binnet and G25_logp_case from ln P on every route, coex(logp=True) fed straight into binnet(logp=True) in HBM,
every row policy of the dispatch at the smallest width that reaches it against the numpy restatement (tests/bh_log_numpy.py; tests/test_bh_log_cpu.py asserts
that those rows keep 1e-9 clear of the cutoff, so every row is compared), invalid entries, and the command line in a child that cannot import torch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bh_log_numpy as bl
from conftest import GOLDEN
from normalisr_amd import _lib
from normalisr_amd import binnet as nb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G8 = (('p', (('net_q5', 0.05), ('net_q20', 0.2), ('net_q50', 0.5))), ('p32', (('net32_q5', 0.05), ('net32_q30', 0.3))), ('pt', (('nett_q10', 0.1), ('nett_q25', 0.25))))
G25_EDGES = ((0.01, 28), (0.05, 34), (0.2, 54))


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd import engine
	return engine.get_engine()


def routes(eng, lnp, q, monkeypatch):
	"""binnet(logp=True) of one matrix: tensor in and tensor out, numpy, the torch-free host entry."""
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	d = nb.binnet(eng.upload(lnp), q, logp=True)
	assert d.is_cuda and d.dtype == eng.torch.bool
	h = nb.binnet(lnp, q, logp=True)
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	e = nb.binnet(lnp, q, logp=True)
	monkeypatch.delenv('NRM_HOST_ENTRY')
	assert h.dtype == np.bool_ and e.dtype == np.bool_
	return d.cpu().numpy(), h, e


def test_stored_networks_from_ln_p(eng, monkeypatch):
	g = np.load(os.path.join(GOLDEN, 'G8_binnet.npz'))
	for src, nets in G8:
		with np.errstate(divide='ignore'):
			lnp = np.log(g[src].astype(np.float64))
		for name, q in nets:
			for dtype in bl.DTYPES:
				for net in routes(eng, lnp.astype(dtype), q, monkeypatch):
					assert np.array_equal(net, g[name]) and not net.diagonal().any(), (name, np.dtype(dtype).name)
	c = np.load(os.path.join(GOLDEN, 'G25_logp_case.npz'))
	for q, edges in G25_EDGES:
		want = bl.binnet(c['lnp_coex'], q)[0]
		assert int(want.sum()) == edges
		for dtype in bl.DTYPES:
			for net in routes(eng, c['lnp_coex'].astype(dtype), q, monkeypatch):
				assert np.array_equal(net, want), (q, np.dtype(dtype).name)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_coex_logp_into_binnet_logp_stays_in_hbm(eng, dtype):
	from normalisr_amd import coex as mcoex
	c = np.load(os.path.join(GOLDEN, 'G25_logp_case.npz'))
	dt, dc = np.ascontiguousarray(c['dt'], dtype=dtype), np.ascontiguousarray(c['dc'])
	lnp = mcoex.coex(dt, dc, logp=True, device_out=True)[0]
	p = mcoex.coex(dt, dc, device_out=True)[0]
	assert lnp.is_cuda and p.is_cuda
	for q, edges in G25_EDGES:
		a, b = nb.binnet(lnp, q, logp=True), nb.binnet(p, q)
		assert a.is_cuda and eng.torch.equal(a, b) and int(a.sum().item()) == edges, q
	# the ln P matrix without logp=True is refused by the linear form's assertion, a P-value matrix is refused by the ln form's (its off-diagonal entries are > 0)
	with pytest.raises(AssertionError):
		nb.binnet(lnp, 0.05)
	with pytest.raises(AssertionError):
		nb.binnet(p, 0.05, logp=True)


def rows_call(eng, d_p, ng, row0, q, p_kind=1):
	torch = eng.torch
	rows = d_p.shape[0]
	out = torch.full((rows, ng), 7, dtype=torch.uint8, device=eng.device)
	total = torch.full((1, ), -1, dtype=torch.int64, device=eng.device)
	flags = torch.zeros(2, dtype=torch.int32, device=eng.device)
	_lib.check(eng.lib.nrm_binnet_rows_pk(d_p.data_ptr(), _lib.NRM_F64 if d_p.dtype == torch.float64 else _lib.NRM_F32, rows, ng, d_p.stride(0), row0, float(q),
										  out.data_ptr(), out.stride(0), total.data_ptr(), flags.data_ptr(), p_kind, eng._stream()))
	torch.cuda.synchronize()
	return out.cpu().numpy(), int(total.item()), flags.tolist()


@pytest.mark.parametrize('dtype', bl.DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_row_policy_against_the_restatement(eng, dtype):
	for ng in bl.ROW_WIDTHS[np.dtype(dtype)]:
		lnp, row0 = bl.rows_case(ng, dtype)
		want, margin = bl.binnet(lnp, bl.ROWS_QCUT, row0=row0)
		assert margin > 1e-9
		got, total, flags = rows_call(eng, eng.upload(lnp), ng, row0, bl.ROWS_QCUT)
		assert set(np.unique(got)) <= {0, 1} and flags[0] == 0, ng
		bad = np.flatnonzero((got.view(np.bool_) != want).any(axis=1))
		assert bad.size == 0, (ng, np.dtype(dtype).name, bad, (got.view(np.bool_) != want).sum(axis=1))  # every row
		assert total == int(want.sum()), ng
		# a row without an edge (ln P = 0 throughout), a row of exact zeros (every entry an edge) and an invalid row, through the same policy
		x = lnp.copy()
		x[0] = 0.0
		x[1] = -np.inf
		x[2, 5] = np.nan
		got, total, flags = rows_call(eng, eng.upload(x), ng, row0, bl.ROWS_QCUT)
		assert not got[0].any() and got[1].sum() == ng - 1 and got[1, row0 + 1] == 0 and flags[0] == 1, ng


def test_invalid_entries_raise_on_every_route(eng, monkeypatch):
	c = np.load(os.path.join(GOLDEN, 'G25_logp_case.npz'))
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	for bad in (np.nan, 1e-300, np.inf):
		x = c['lnp_coex'].copy()
		x[3, 60] = bad
		with pytest.raises(AssertionError):
			nb.binnet(eng.upload(x), 0.05, logp=True)
		with pytest.raises(AssertionError):
			nb.binnet(x, 0.05, logp=True)
		monkeypatch.setenv('NRM_HOST_ENTRY', '1')
		with pytest.raises(AssertionError, match='ln P-values must be <= 0'):
			nb.binnet(x, 0.05, logp=True)
		monkeypatch.delenv('NRM_HOST_ENTRY')
	with pytest.raises(AssertionError):
		nb.binnet(c['lnp_coex'], 0.05)  # ln P without logp=True
	with pytest.raises(RuntimeError, match='Empty binary network'):
		nb.binnet(np.zeros((5, 5)), 0.05, logp=True)  # P = 1 throughout


def test_binnet_logp_cli_in_a_child_that_cannot_import_torch(tmp_path):
	from normalisr_amd import run
	c = np.load(os.path.join(GOLDEN, 'G25_logp_case.npz'))
	files, args = {}, []
	for stem, ext in (('a', '.npy'), ('b', '.tsv')):
		files[stem] = (str(tmp_path / (stem + '_lnp' + ext)), str(tmp_path / (stem + '_net' + ext)))
		run.file_write_tsv(files[stem][0], c['lnp_coex'])  # (text: -INF on the diagonal)
		args += ['binnet', files[stem][0], files[stem][1], '0.05']
	assert b'-INF' in open(files['b'][0], 'rb').read()
	env = {k: v for k, v in os.environ.items() if k != 'NRM_HOST_ENTRY'}
	r = subprocess.run([sys.executable, os.path.join(HERE, 'bh_log_cli_child.py')] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
	assert r.returncode == 0 and 'child ok' in r.stdout, r.stdout[-3000:]
	want = bl.binnet(c['lnp_coex'], 0.05)[0]
	for stem in files:
		got = run.file_read_tsv(files[stem][1])
		assert got.shape == want.shape and np.array_equal(got != 0, want) and int(want.sum()) == 34, stem
