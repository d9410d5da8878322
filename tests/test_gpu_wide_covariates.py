"""GPU: compute_var and normvar with 64 to 1024 covariates (csrc/nrm_fitvar.hip's WIDE instantiations, csrc/nrm_normvar_wide.hip) against what the reference
returned for G22 (tests/golden/make_g22.py), the oracle and the numpy restatements (tests/front_numpy.py, tests/normvar_wide_numpy.py).  Every test here raises
NotImplementedError (or misses a symbol) on a library without the feature.  Bounds: fp64 results close(1e-9, floor=1); fp32 input within 1e-6 of the result's
scale; the Cholesky kernel alone within Cholesky's backward-error bound 4 r^2 u; pair products, repeated runs and every block / panel setting: equal bits."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import front_numpy
import normvar_wide_numpy as wide
from conftest import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('A', 'B', 'C')
# (nv_panel_rows, nv_gene_block) per case: at least three panels and three gene blocks, the last ones ragged, panels starting in the middle of a triangle row
SMALL = {'A': (2000, 10), 'B': (30000, 3), 'C': (1000, 6)}


def close(a, b, rtol=1e-9, floor=1.0):
	return relerr(a, b, floor) < rtol


def p_close(p, ref, rtol=1e-6):
	p, ref = np.asarray(p, dtype=np.float64), np.asarray(ref, dtype=np.float64)
	normal = ref >= 1e-290
	return (relerr(p[normal], ref[normal]) < rtol if normal.any() else True) and np.all(np.abs(p[~normal] - ref[~normal]) <= 1e-307)


@pytest.fixture(scope='module')
def norm():
	import normalisr_amd.normalisr as norm
	return norm


@pytest.fixture(scope='module')
def torch():
	import torch
	return torch


@pytest.fixture(scope='module')
def g22(golden):
	g = golden('G22_wide_covariates')
	return {c: {k: g['%s_%s' % (c, k)] for k in ('dt', 'dc', 'wt', 'w1', 'w3', 'nv', 'dcn', 'ranks')} for c in CASES}


def _covariates(rng, nc, n):
	"""nc rows on n cells through the package's normcov: 64 and 65 continuous of full rank; 131 one-hot (60 + 40 + 27 levels) + 3 continuous + the intercept, rank 129."""
	from normalisr_amd.norm import normcov
	if nc == 131:
		rows = []
		for lv in (60, 40, 27):
			f = rng.integers(0, lv, n)
			f[:lv] = np.arange(lv)
			rows.append((f[rng.permutation(n)][None, :] == np.arange(lv)[:, None]).astype(float))
		raw = np.concatenate(rows + [np.array([rng.normal(0, 1, n), rng.normal(100, 30, n), rng.normal(0.05, 0.01, n)])])
	else:
		raw = rng.normal(0, 1, (nc - 1, n)) * 10.0**rng.integers(-2, 3, nc - 1)[:, None]
	dc = normcov(raw)
	assert dc.shape == (nc, n)
	return dc


@pytest.fixture(scope='module')
def small_cases():
	"""13 genes x 403 cells (rows no multiple of the 4-gene workgroups, cells no multiple of 4: the unaligned loads) for 63, 64, 65 and 131 covariates, with
	the restatement's weights for stepmax 1 and 3 -- computed once."""
	rng = np.random.default_rng(2220)
	out = {}
	for nc in (63, 64, 65, 131):
		dc = _covariates(rng, nc, 403)
		cell = np.exp(0.3 * rng.normal(0, 1, 403))
		dt = (rng.normal(0, 1, (13, 403)) * cell + rng.normal(0, 0.3, (13, nc)) @ dc / np.sqrt(nc / 8) + 3.0).astype(np.float32)
		out[nc] = (dt, dc, {s: front_numpy.compute_var(dt.astype(np.float64), dc, stepmax=s) for s in (1, 3)})
	return out


@pytest.mark.parametrize('nc', (64, 65, 131))
def test_compute_var_past_the_static_table(norm, torch, small_cases, nc):
	dt32, dc, ref = small_cases[nc]
	for dt in (dt32, dt32.astype(np.float64)):
		for src in (dt, torch.as_tensor(dt).cuda()):
			for steps in (1, 3):
				w = norm.compute_var(src, dc, stepmax=steps)
				print(nc, dt.dtype, type(src).__name__, steps, relerr(w, ref[steps], 1.0))
				assert close(w, ref[steps]) and w.min() == 1.0
				assert np.array_equal(w, norm.compute_var(src, dc, stepmax=steps))  # the same bits run to run


def test_compute_var_g22_against_the_reference(norm, torch, g22):
	for case in CASES:  # 113 (700 cells: 16-byte aligned rows), 384 and 70 covariates
		d = g22[case]
		for src in (d['dt'], d['dt'].astype(np.float64), torch.as_tensor(d['dt']).cuda()):
			for steps, key in ((1, 'w1'), (3, 'w3')):
				w = norm.compute_var(src, d['dc'], stepmax=steps)
				print(case, steps, relerr(w, d[key], 1.0))
				assert close(w, d[key])
		assert np.array_equal(norm.compute_var(d['dt'], d['dc'], stepmax=3), norm.compute_var(d['dt'], d['dc'], stepmax=3))


def test_compute_var_up_to_63_covariates_as_before(norm, torch, golden, small_cases):
	"""The instantiations for up to 63 covariates are the ones the library had: G18's chain value as tests/test_gpu_front.py holds it, and 63 covariates beside 64."""
	g, h = golden('G18_front'), golden('G18_front_chain')
	assert close(norm.compute_var(g['lcpm'], h['normcov_c']), h['w1'])
	dt32, dc, ref = small_cases[63]
	for steps in (1, 3):
		w = norm.compute_var(dt32, dc, stepmax=steps)
		assert close(w, ref[steps]) and np.array_equal(w, norm.compute_var(torch.as_tensor(dt32).cuda(), dc, stepmax=steps))


def _settings(monkeypatch, case, small):
	if small:
		monkeypatch.setenv('NRM_DEBUG', 'nv_panel_rows=%d,nv_gene_block=%d' % SMALL[case])
	else:
		monkeypatch.delenv('NRM_DEBUG', raising=False)


@pytest.mark.parametrize('case', CASES)
def test_normvar_g22_against_the_reference(norm, torch, g22, monkeypatch, case):
	from normalisr_amd import engine
	d = g22[case]
	dt64 = d['dt'].astype(np.float64)
	scale = np.abs(d['nv']).max()
	got = {}
	for small in (False, True):
		_settings(monkeypatch, case, small)
		for name, src in (('f64', dt64), ('f32', d['dt']), ('dev', torch.as_tensor(dt64).cuda())):
			for rep in range(2):
				got[small, name, rep] = norm.normvar(src, d['dc'], d['w3'], d['wt'])
			last = engine.get_engine()._normvar_wide_last
			npair = last['rank'] * (last['rank'] + 1) // 2
			assert last['rank'] == d['ranks'][0] and (last['status'].cpu().numpy() == 0).all()
			if small:
				assert -(-npair // last['panel_rows']) >= 3 and npair % last['panel_rows'] and -(-dt64.shape[0] // last['gene_block']) >= 3 and dt64.shape[0] % last['gene_block']
	ref = got[False, 'f64', 0]
	print(case, 'fp64', relerr(ref[0], d['nv'], 1.0), 'fp32', np.abs(got[False, 'f32', 0][0] - d['nv']).max() / scale)
	assert ref[0].dtype == np.float64 and close(ref[0], d['nv']) and close(ref[1], d['dcn'])
	for g in (0, 2):  # the gene with wt = 0; the gene whose covariate effects explain 99 % of its variance (the cancellation in s2 - a . b)
		assert close(ref[0][g], d['nv'][g])
	assert d['wt'][0] == 0
	for (small, name, rep), v in got.items():
		base = got[False, name, 0]
		assert np.array_equal(v[0], base[0]) and np.array_equal(v[1], base[1]), (small, name, rep)  # every setting, every run: the same bits
	assert np.array_equal(got[False, 'dev', 0][0], ref[0])
	f32 = got[False, 'f32', 0][0]
	assert f32.dtype == np.float64 and np.abs(f32 - d['nv']).max() <= 1e-6 * scale  # (the covariates are fp64: the result type is fp64; the input is fp32)
	o32 = norm.normvar(d['dt'], d['dc'].astype(np.float32), d['w3'].astype(np.float32), d['wt'].astype(np.float32))[0]
	assert o32.dtype == np.float32 and np.abs(o32 - d['nv']).max() <= 1e-6 * scale * 4  # fp32 covariates and weights: their rounding (6e-8 each) reaches the result too


def test_normvar_options_against_the_oracle(norm, torch, g22, monkeypatch):
	import oracle
	d = g22['A']
	dt = d['dt'].astype(np.float64)
	rng = np.random.default_rng(2221)
	dextra = rng.normal(size=(2, dt.shape[1]))
	for small in (False, True):
		_settings(monkeypatch, 'A', small)
		for ka in (dict(keepvar=False), dict(normmean=True), dict(cat=0), dict(cat=2), dict(cat=1, dextra=dextra), dict(keepvar=False, normmean=True, cat=2)):
			got = norm.normvar(dt, d['dc'], d['w3'], d['wt'], **ka)
			ref = oracle.normvar(dt, d['dc'], d['w3'], d['wt'], **ka)
			assert len(got) == len(ref)
			for a, b in zip(got, ref):
				assert close(a, b), ka
	monkeypatch.delenv('NRM_DEBUG', raising=False)
	nv = norm.normvar(torch.as_tensor(dt).cuda(), d['dc'], d['w3'], d['wt'], device_out=True)
	assert nv[0].is_cuda and close(nv[0].cpu().numpy(), d['nv'])
	p, dot, var = norm.coex(nv[0], nv[1])
	po, do, vo = oracle.coex(d['nv'], d['dcn'])
	host = lambda a: a.cpu().numpy() if hasattr(a, 'is_cuda') else a
	assert p_close(host(p), po) and close(host(var), vo)


def test_normvar_plan_falls_back_to_the_public_call(norm, torch, g22):
	from normalisr_amd.norm import NormvarPlan
	d = g22['C']
	plan = NormvarPlan(torch.as_tensor(d['dt'].astype(np.float64)).cuda(), d['dc'], d['w3'], d['wt'])
	assert not plan.lean
	plan.step()
	assert close(plan.results()[0], d['nv'])


def test_normvar_without_a_certificate_takes_the_reference_path(norm, g22, caplog):
	import oracle
	d = g22['C']
	rng = np.random.default_rng(2222)
	dc = np.vstack([d['dc'], d['dc'][3] + 1e-4 * rng.normal(size=d['dc'].shape[1])])  # an eigenvalue inside the forbidden band (tests/test_wide_covariates_cpu.py)
	dt = d['dt'][:4].astype(np.float64)
	with caplog.at_level(logging.WARNING):
		got = norm.normvar(dt, dc, d['w3'], d['wt'][:4])
	assert any('without a rank certificate' in r.getMessage() for r in caplog.records)
	ref = oracle.normvar(dt, dc, d['w3'], d['wt'][:4])
	assert close(got[0], ref[0]) and close(got[1], ref[1])


def _dev(torch, a):
	return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('r', (1, 2, 63, 64, 65, 130, 377))
def test_cholesky_kernel_alone(torch, r):
	"""nrm_normvar_chol on seeded positive definite stacks of three, condition 1 and 1e4: the normwise residual |M b - a|_inf / (|M|_inf |b|_inf), in extended
	precision, within 4 r^2 u (Higham, Accuracy and Stability, Thm 10.4, normwise); an indefinite matrix sets its status and counter and leaves its neighbours alone."""
	from normalisr_amd import _lib
	lib = _lib.load()
	rng = np.random.default_rng(2230 + r)
	iu = np.triu_indices(r)
	u = 2.0**-53
	stream = torch.cuda.current_stream().cuda_stream

	def solve(ms, a):
		d_m, d_a = _dev(torch, np.stack([m[iu] for m in ms])), _dev(torch, a)
		d_b, d_sc = torch.full((3, r), np.nan, dtype=torch.float64, device='cuda'), torch.full((3, ), np.nan, dtype=torch.float64, device='cuda')
		status, flags = torch.full((3, ), -1, dtype=torch.int32, device='cuda'), torch.zeros((4, ), dtype=torch.int32, device='cuda')
		_lib.check(lib.nrm_normvar_chol(d_m.data_ptr(), d_m.stride(0), d_a.data_ptr(), d_a.stride(0), 3, r, None, None, None, 0, 0, d_b.data_ptr(), d_sc.data_ptr(),
										status.data_ptr(), flags.data_ptr(), stream))
		torch.cuda.synchronize()
		return d_b.cpu().numpy(), d_sc.cpu().numpy(), status.cpu().numpy(), flags.cpu().numpy()

	def residual(m, b, a):
		ml, bl = m.astype(np.longdouble), b.astype(np.longdouble)
		return float(np.abs(ml @ bl - a).max() / (np.abs(ml).sum(axis=1).max() * np.abs(bl).max()))

	for cond in (1.0, 1e4):
		ms = []
		for _ in range(3):
			q = np.linalg.qr(rng.normal(size=(r, r)))[0]
			lam = np.exp(-np.log(cond) * rng.permutation(r) / max(r - 1, 1)) * rng.uniform(0.5, 2.0)
			m = (q * lam) @ q.T
			ms.append((m + m.T) / 2)
		a = rng.normal(size=(3, r))
		b, sc, status, flags = solve(ms, a)
		worst = max(residual(ms[g], b[g], a[g]) for g in range(3))
		print('r', r, 'cond', cond, 'residual', worst, 'bound', 4 * r * r * u)
		assert (status == 0).all() and (flags == 0).all() and (sc == 1.0).all() and np.isfinite(b).all()
		assert worst <= 4 * r * r * u
		b2 = solve(ms, a)[0]
		assert np.array_equal(b, b2)
		if r > 1:
			q = np.linalg.qr(rng.normal(size=(r, r)))[0]
			lam = np.ones(r)
			lam[r // 2] = -0.5
			bad = (q * lam) @ q.T
			bb, bsc, bstatus, bflags = solve([ms[0], (bad + bad.T) / 2, ms[2]], a)
			assert list(bstatus) == [0, 1, 0] and bflags[0] == 1 and bflags[1] == 0
			assert (bb[1] == 0).all() and bsc[1] == 0 and np.array_equal(bb[0], b[0]) and np.array_equal(bb[2], b[2])
	nan = ms[1].copy()
	nan[0, r - 1] = nan[r - 1, 0] = np.nan
	_, _, nstatus, nflags = solve([ms[0], nan, ms[2]], a)
	assert nstatus[0] == 0 and nstatus[2] == 0 and nstatus[1] in (1, 2) and nflags[0] + nflags[1] == 1


def test_pair_products_kernel(torch):
	"""nrm_normvar_pairs: rows [pair0, pair0 + count) of the pair products in numpy's triu order, bit for bit; panels that start in the middle of a row of the
	triangle, a cell count off the tile size, zeros in the padding rows and cells."""
	from normalisr_amd import _lib
	lib = _lib.load()
	rng = np.random.default_rng(2240)
	stream = torch.cuda.current_stream().cuda_stream
	for r, n, ldb in ((37, 403, 416), (1, 5, 16), (130, 1031, 1040)):
		b = np.zeros((r, ldb))
		b[:, :n] = rng.normal(size=(r, n))
		d_b = _dev(torch, b)
		iu = np.triu_indices(r)
		npair = len(iu[0])
		full = b[iu[0]] * b[iu[1]]
		for pair0, count, rows_pad in ((0, npair, npair), (npair // 3 + 1, npair // 2, npair // 2 + 77), (npair - 1, 1, 128), (5 % npair, 0, 16)):
			ldp = ldb + 16
			d_p = torch.full((rows_pad, ldp), np.nan, dtype=torch.float64, device='cuda')
			_lib.check(lib.nrm_normvar_pairs(d_b.data_ptr(), r, n, ldb, pair0, count, d_p.data_ptr(), rows_pad, ldp, stream))
			p = d_p.cpu().numpy()
			assert np.array_equal(p[:count, :n], full[pair0:pair0 + count, :n]) and (p[count:] == 0).all() and (p[:, n:] == 0).all()
	with pytest.raises(ValueError):
		_lib.check(lib.nrm_normvar_pairs(d_b.data_ptr(), r, n, ldb, npair - 3, 4, d_p.data_ptr(), rows_pad, ldp, stream))


def test_cli_fitvar_normvar_wide_covariates(g22, tmp_path):
	"""`normalisr fitvar` then `normalisr normvar` on case A's files, each its own process; outputs carry 8 significant digits: close(1e-6, floor=1)."""
	d = g22['A']
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('lcpm.tsv'), d['dt'].astype(np.float64), fmt='%.17G', delimiter='\t')
	np.savetxt(f('cov.tsv'), d['dc'], fmt='%.17G', delimiter='\t')
	np.savetxt(f('w3.tsv'), d['w3'][None, :], fmt='%.17G', delimiter='\t')
	np.savetxt(f('wt.tsv'), d['wt'][None, :], fmt='%.17G', delimiter='\t')
	env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
	env.pop('NRM_DEBUG', None)

	def run(*args):
		r = subprocess.run([sys.executable, '-m', 'normalisr_amd'] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
		assert r.returncode == 0, r.stderr[-3000:]
	run('fitvar', f('lcpm.tsv'), f('cov.tsv'), f('w.tsv'))
	run('normvar', f('lcpm.tsv'), f('w3.tsv'), f('cov.tsv'), f('wt.tsv'), f('exp.tsv'), f('ecov.tsv'))
	load = lambda name: np.loadtxt(f(name), delimiter='\t', ndmin=2)
	near = lambda a, b: close(a, b, 1e-6, floor=1.0)
	print('w', relerr(load('w.tsv').ravel(), d['w1'], 1.0), 'exp', relerr(load('exp.tsv'), d['nv'], 1.0))
	assert near(load('w.tsv').ravel(), d['w1']) and near(load('exp.tsv'), d['nv']) and near(load('ecov.tsv'), d['dcn'])
