"""GPU checks of the top-PC covariate (normalisr_amd/gocovt.py, csrc/nrm_pc.hip): the degree kernel alone against net.sum(axis=1), principal_genes and pccovt
against what the reference returned (golden G21), pccovt against the numpy restatement of tests/pc_numpy.py in longdouble on the shapes where the kernels can go
wrong, the same bits from call to call, relations that need no reference, the iteration cap, one resident level coex -> binnet -> principal_genes -> pccovt ->
coex against the same chain through numpy, and the two sub-commands as child processes.

The allowance of a case against longdouble is 10 x the distance of the restatement in float64 from the restatement in longdouble on that case, not below
64 m u (u = 2^-53: the stop rule of the power iteration, residual <= 16 m u lambda, leaves the component within 16 m u / (1 - (sigma_2 / sigma_1)^2) of the
exact one, which is 44 m u at sigma_2 / sigma_1 = 0.8) and not above 1e-10, relative to max |score|: the form DESIGN.md section 6f uses for compute_var."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import pc_numpy
from pc_numpy import g21_case, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = 2.0**-53
M_SIZES = (2, 7, 33, 40, 260)  # no multiples of K2's 32-row tile; 260 exceeds one workgroup's share of genes in the score pass
N_SIZES = (96, 257, 1001, 2049)  # ragged in 4 and in 16; 96 is narrower than one workgroup of the score pass, so the genes are split
_REFS = {}
WORST = {'ratio': 0.0, 'case': None}


@pytest.fixture(scope='module', autouse=True)
def worst_ratio_report():
	"""After the module's tests: prints the worst error / allowance they met against longdouble (the figure DESIGN.md section 6i records; shown with -s)."""
	yield
	print('worst error / allowance against longdouble: {:.3g} ({})'.format(WORST['ratio'], WORST['case']))


def covariates(rng, n):
	"""As normcov builds them: 4 one-hot batches, 3 standardised continuous covariates, the intercept (rank 7 of 8)."""
	batch = rng.integers(0, 4, n)
	batch[:4] = np.arange(4)
	cont = rng.normal(size=(3, n)) * np.array([[1.0], [30.0], [0.01]]) + np.array([[0.0], [100.0], [0.05]])
	cont = (cont - cont.mean(axis=1, keepdims=True)) / cont.std(axis=1, keepdims=True)
	return np.concatenate([(batch[None, :] == np.arange(4)[:, None]).astype(float), cont, np.ones((1, n))])


def expression(rng, nt, n, dc, strength=0.7, second=0.0, signs=None, shift=2.0):
	"""fp32-representable rows: noise + a common factor of mixed sign (+ a second one) + covariate effects + a mean."""
	load = (rng.choice([-1.0, 1.0], nt) if signs is None else signs) * (rng.uniform(0.6, 1.4, nt) if signs is None else 1.0)
	x = rng.normal(size=(nt, n)) + strength * load[:, None] * rng.normal(size=n)[None, :]
	if second:
		x += second * rng.choice([-1.0, 1.0], nt)[:, None] * rng.normal(size=n)[None, :]
	x += rng.normal(0, 0.5, (nt, dc.shape[0])) @ dc
	return (x + shift).astype(np.float32)


def reference(key, dt, dc, idx, condcov=True):
	"""The longdouble restatement of a case, computed once and shared: (score as float64, allowance, argmax |loading|, sigma_2 / sigma_1)."""
	if key not in _REFS:
		ld, v, lam, z = pc_numpy.pccovt(dt, dc, idx, condcov=condcov, ft=np.longdouble, return_all=True)
		f64 = pc_numpy.pccovt(dt, dc, idx, condcov=condcov, ft=np.float64)
		scale = float(np.abs(ld).max())
		dist = float(np.abs(f64.astype(np.longdouble) - ld).max()) / scale if scale > 0 else 0.0
		m = len(idx)
		_REFS[key] = (ld.astype(np.float64), min(max(10 * dist, 64 * m * UNIT), 1e-10), int(np.argmax(np.abs(v))), pc_numpy.singular_ratio(z))
	return _REFS[key]


def held(case, got, ref, bound):
	err = rel(got, ref)
	if bound > 0 and err / bound > WORST['ratio']:
		WORST['ratio'], WORST['case'] = err / bound, case
	print('{}: error {:.3g} of allowance {:.3g}'.format(case, err, bound))
	assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and err <= bound, (case, err, bound)


def on_device(a, pad=0):
	"""A torch CUDA tensor holding a; pad > 0: a view of a wider buffer (a pitch larger than the row)."""
	import torch
	t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
	if pad:
		wide = torch.full((a.shape[0], a.shape[1] + pad), float('nan'), dtype=t.dtype, device='cuda')
		wide[:, :a.shape[1]] = t
		t = wide[:, :a.shape[1]]
		assert t.stride(0) == a.shape[1] + pad and not t.is_contiguous()
	return t


# ---- the degree kernel ------------------------------------------------------------------------------------------------------------------------------------------

def _network(rng, ng):
	net = rng.random((ng, ng)) < 0.3
	if ng > 2:
		net[ng // 2, :] = False  # an all-False row
		net[ng // 3, :] = True  # an all-True row
	return net


@pytest.mark.parametrize('ng', [15, 16, 17, 97, 1030])
def test_net_degree_kernel_is_exact(ng):
	import torch
	from normalisr_amd import gocovt
	rng = np.random.default_rng(ng)
	net = _network(rng, ng)
	want = net.sum(axis=1).astype(np.int64)
	got = gocovt.net_degree(net)
	assert got.dtype == np.int64 and np.array_equal(got, want)
	assert np.array_equal(gocovt.net_degree(net.astype(np.uint8) * 255), want)  # any non-zero byte counts once
	mixed = np.where(net, rng.integers(1, 256, net.shape), 0).astype(np.uint8)
	assert np.array_equal(gocovt.net_degree(mixed), want)
	for pitch, offset in ((ng, 0), (ng + 3, 0), (ng, 1), (ng + 3, 1)):  # the rows' alignment changes from row to row; a base one byte past an aligned address
		buf = torch.full((offset + ng * pitch + 16, ), 1, dtype=torch.uint8, device='cuda')  # (padding of ones: a byte read past a row would be counted)
		view = buf[offset:offset + ng * pitch].view(ng, pitch)[:, :ng]
		view.copy_(torch.from_numpy(mixed).cuda())
		assert view.data_ptr() % 16 == offset and view.stride(0) == pitch
		deg = gocovt.net_degree(view, device_out=True)
		assert deg.is_cuda and deg.dtype == torch.int64 and np.array_equal(deg.cpu().numpy(), want), (pitch, offset)
		assert np.array_equal(gocovt.net_degree(view != 0), want)  # a bool tensor, as binnet returns


def test_net_degree_of_one_gene_through_the_entry():
	import torch
	from normalisr_amd import _lib, engine
	eng = engine.get_engine()
	for value in (0, 1, 255):
		net = torch.full((1, ), value, dtype=torch.uint8, device='cuda')
		deg = torch.full((1, ), -7, dtype=torch.int64, device='cuda')
		_lib.check(eng.lib.nrm_net_degree(net.data_ptr(), 1, 1, deg.data_ptr(), eng._stream()))
		assert int(deg.cpu()[0]) == (1 if value else 0)


# ---- against the reference (golden G21) ------------------------------------------------------------------------------------------------------------------------------

def test_principal_genes_match_the_reference(golden):
	import torch
	from normalisr_amd import gocovt
	g = golden('G21_pccovt')
	net = g['net']
	dev = torch.from_numpy(net).cuda()
	for n in (5, 20, 60):
		want = g['principal_%d' % n]
		got = gocovt.principal_genes(net, n=n)
		assert got.dtype == np.int64 and np.array_equal(got, want)
		assert np.array_equal(gocovt.principal_genes(dev, n=n), want)
		assert np.array_equal(gocovt.principal_genes(dev.to(torch.uint8), n=n), want)
		t = gocovt.principal_genes(dev, n=n, device_out=True)
		assert t.is_cuda and t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), want)
	with pytest.raises(RuntimeError, match='Not enough principal genes'):
		gocovt.principal_genes(np.zeros((9, 9), dtype=bool), n=3)


@pytest.mark.parametrize('name', ['c1', 'c2', 'c3', 'c4', 'c5'])
def test_pccovt_matches_the_reference(golden, name):
	from normalisr_amd import gocovt
	g = golden('G21_pccovt')
	dt, dc, namet, genes, idx, cond, want = g21_case(g, name)
	tol = 1e-6 if name == 'c5' else 1e-9
	got = gocovt.pccovt(dt, dc, namet, genes, condcov=cond)
	assert got.shape == want.shape and got.dtype == want.dtype
	assert np.array_equal(got[:-1], dc) and got[:-1].tobytes() == dc.tobytes()  # the first nc rows are dc, bit for bit
	err = rel(got[-1], want[-1])
	print(name, 'against the reference: %.3g' % err)
	assert err < tol
	# the resident form: integer rows of a tensor in HBM, fp32 input as well (every input of G21 is exact in fp32)
	for t in (on_device(dt), on_device(dt.astype(np.float32), pad=3)):
		res, info = gocovt.pccovt(t, dc, None, idx, condcov=cond, return_info=True)
		assert res.dtype == (want.dtype if str(t.dtype) == 'torch.float64' or cond else np.result_type(dc.dtype, np.float32))
		# (fp32 rows that are only centred -- no conditioning, or no covariate to condition on -- give an fp32 score, as in the reference: the fp32 bound)
		fp32_score = str(t.dtype) == 'torch.float32' and not (cond and dc.shape[0] > 0)
		assert rel(res[-1], want[-1]) < (1e-6 if fp32_score else tol) and info['converged'] and info['iterations'] % 16 == 0 and info['iterations'] <= 4096
	out = gocovt.pccovt(on_device(dt), dc, None, idx, condcov=cond, device_out=True)
	assert out.is_cuda and tuple(out.shape) == want.shape and np.array_equal(out.cpu().numpy(), got)


# ---- against the restatement in longdouble -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', N_SIZES)
@pytest.mark.parametrize('m', M_SIZES)
def test_pccovt_against_longdouble_on_kernel_shapes(m, n):
	from normalisr_amd import gocovt
	rng = np.random.default_rng(1000 * m + n)
	nt = m + 5
	dc = covariates(rng, n)
	# (two genes carry loadings of EQUAL magnitude, (1, +-1) / sqrt 2, whatever the data: with opposite signs rounding alone would pick the positive one)
	dt32 = expression(rng, nt, n, dc, signs=np.ones(nt) if m == 2 else None)
	idx = rng.permutation(nt)[:m].astype(np.int64)
	ref, bound, top, ratio = reference(('shape', m, n), dt32.astype(np.float64), dc, idx)
	for dtype in (np.float32, np.float64):
		x = dt32.astype(dtype)
		for form, arg in (('numpy', x), ('device', on_device(x)), ('pitch', on_device(x, pad=5))):
			got, info = gocovt.pccovt(arg, dc, None, idx, return_info=True)
			assert got.dtype == np.float64 and got.shape == (9, n) and np.array_equal(got[:-1], dc)
			held('m {} n {} {} {} (sigma2/sigma1 {:.2f})'.format(m, n, np.dtype(dtype).name, form, ratio), got[-1], ref, bound)
			assert float(got[-1] @ ref) > 0 and (m <= 2 or info['top'] == top) and info['converged']  # the sign rule: argmax |loading| is positive


def _special(kind):
	"""(dt32, dc, idx, condcov) of the additional cases."""
	rng = np.random.default_rng({'repeat': 1, 'alternating': 2, 'close': 3, 'one': 5}[kind])
	n = 517
	dc = covariates(rng, n)
	if kind == 'repeat':  # gene indices unsorted and with one repeat
		return expression(rng, 30, n, dc), dc, np.array([17, 3, 29, 8, 3, 0, 21, 11, 12], dtype=np.int64), True
	if kind == 'alternating':  # loadings +-1 in turn: they add up to zero, a constant start vector would be orthogonal to the component
		return expression(rng, 24, n, dc, strength=1.0, signs=np.where(np.arange(24) % 2, -1.0, 1.0)), dc, np.arange(24, dtype=np.int64), True
	if kind == 'close':  # sigma_2 / sigma_1 about 0.8
		return expression(rng, 40, n, dc, strength=0.62, second=0.45), dc, np.arange(40, dtype=np.int64), True
	return expression(rng, 12, n, dc), dc, np.array([7], dtype=np.int64), True  # m == 1


@pytest.mark.parametrize('kind', ['repeat', 'alternating', 'close', 'one'])
def test_pccovt_against_longdouble_on_special_cases(kind):
	from normalisr_amd import gocovt
	dt32, dc, idx, cond = _special(kind)
	ref, bound, top, ratio = reference(('special', kind), dt32.astype(np.float64), dc, idx, cond)
	if kind == 'close':
		assert 0.72 < ratio < 0.88, ratio
	for dtype in (np.float32, np.float64):
		got, info = gocovt.pccovt(dt32.astype(dtype), dc, None, idx, condcov=cond, return_info=True)
		held('{} {} (sigma2/sigma1 {:.2f}, {} iterations)'.format(kind, np.dtype(dtype).name, ratio, info['iterations']), got[-1], ref, bound)
		assert float(got[-1] @ ref) > 0 and info['converged']
		if kind != 'repeat':  # (the two copies of a repeated row carry the same loading: either may be the first of equals)
			assert info['top'] == top and info['sign'] in (1, -1)
	if kind == 'one':  # the standardised row, loading +1
		row = dt32[idx[0]].astype(np.float64)
		assert info['sign'] == 1 and info['top'] == 0 and abs(float((got[-1]**2).mean()) - 1) < 1e-12 and abs(float(got[-1].mean())) < 1e-12
		names = ['g%d' % i for i in range(12)]
		assert np.array_equal(gocovt.pccovt(dt32, dc, names, ['g7']), got)  # (through the names: the same call)
		plain = gocovt.pccovt(row[None, :], dc[:0], None, [0])
		want = (row - row.mean()) / np.sqrt(((row - row.mean())**2).mean())
		assert plain.shape == (1, len(row)) and rel(plain[0], want) < 64 * UNIT * 8


def test_zero_row_without_conditioning():
	"""A row of exact zeros stays zero after centring: a = 1e200 beside G = 0.  The result is that of the call without the row; nothing is NaN."""
	from normalisr_amd import gocovt
	dt32, dc, idx, _ = _special('repeat')
	x = dt32.astype(np.float64)[np.unique(idx)]
	m = x.shape[0]
	ref, bound, top, ratio = reference(('zero', ), x, dc, np.arange(m), False)
	z = np.concatenate([x[:3], np.zeros((1, x.shape[1])), x[3:]])
	for arg, rows in ((x, np.arange(m)), (z, np.arange(m + 1))):
		for dtype in (np.float32, np.float64):
			got = gocovt.pccovt(arg.astype(dtype), dc, None, rows, condcov=False)
			assert got.dtype == np.result_type(np.float64, dtype) and np.isfinite(got).all()
			if dtype == np.float64:
				held('zero row: {} rows'.format(len(rows)), got[-1], ref, bound)
			else:
				assert rel(got[-1], ref) < 1e-6
	only = gocovt.pccovt(np.zeros((2, 50)), np.zeros((0, 50)), None, [0, 1], condcov=False)
	assert only.shape == (1, 50) and (only == 0).all()  # every chosen row zero: a zero covariate, no NaN and no warning


# ---- the same bits, relations, the cap -----------------------------------------------------------------------------------------------------------------------------

def test_same_bits_from_call_to_call():
	from normalisr_amd import gocovt
	dt32, dc, idx, _ = _special('close')
	a = gocovt.pccovt(dt32, dc, None, idx)
	b = gocovt.pccovt(dt32, dc, None, idx)
	other, dco, idxo, _ = _special('repeat')
	gocovt.pccovt(other[:, :300], dco[:, :300], None, idxo)  # a call of another shape in between
	c = gocovt.pccovt(on_device(dt32), dc, None, idx)
	assert a.tobytes() == b.tobytes() == c.tobytes()
	rng = np.random.default_rng(8)
	big = expression(rng, 265, 96, covariates(rng, 96))  # (the genes split over workgroups in the score pass)
	rows = np.arange(260)
	assert gocovt.pccovt(big, np.zeros((0, 96)), None, rows).tobytes() == gocovt.pccovt(big, np.zeros((0, 96)), None, rows).tobytes()


def test_relations_that_need_no_reference():
	from normalisr_amd import gocovt
	dt32, dc, idx, _ = _special('repeat')
	idx = np.unique(idx)
	x = dt32.astype(np.float64)
	_, bound, _, _ = reference(('relations', ), x, dc, idx)
	base = gocovt.pccovt(x, dc, None, idx)[-1]
	rng = np.random.default_rng(4)
	held('genes permuted', gocovt.pccovt(x, dc, None, rng.permutation(idx))[-1], base, bound)
	perm = rng.permutation(x.shape[1])
	held('cells permuted', gocovt.pccovt(x[:, perm], dc[:, perm], None, idx)[-1], base[perm], bound)
	scaled = x.copy()
	scaled[idx[2]] *= 1e6
	held('a row rescaled by 1e6', gocovt.pccovt(scaled, dc, None, idx)[-1], base, bound)
	more = np.concatenate([dc, (0.5 * dc[4] - 2.0 * dc[5] + dc[0])[None, :]])
	got = gocovt.pccovt(x, more, None, idx)
	assert got.shape == (dc.shape[0] + 2, x.shape[1]) and np.array_equal(got[:-1], more)
	held('a dependent covariate row added', got[-1], base, bound)


def test_iteration_cap_warns_and_returns_finite_values():
	from normalisr_amd import gocovt
	dt32, dc, idx, _ = _special('close')
	with pytest.warns(RuntimeWarning, match='top principal component not separated'):
		got, info = gocovt.pccovt(dt32, dc, None, idx, max_iter=1, return_info=True)
	assert info['iterations'] == 1 and not info['converged'] and np.isfinite(got).all() and got.shape == (dc.shape[0] + 1, dt32.shape[1])
	with warnings.catch_warnings():
		warnings.simplefilter('error', RuntimeWarning)
		_, info = gocovt.pccovt(dt32, dc, None, idx, return_info=True)  # the default cap: converged, no warning
	assert info['converged'] and 16 <= info['iterations'] <= 4096 and info['residual'] <= 16 * len(idx) * UNIT * info['eigenvalue']


# ---- one resident level ----------------------------------------------------------------------------------------------------------------------------------------------

def test_resident_level_matches_the_chain_through_numpy():
	"""coex(device_out=True) -> binnet -> principal_genes -> pccovt(namet=None, a tensor in HBM) -> coex with the new covariates: one level of the loop of
	examples/GSE123139/code/cmd_coex.sh:37-46 without leaving HBM, against the same chain through numpy arrays."""
	from conftest import relerr
	from normalisr_amd import gocovt
	from normalisr_amd.binnet import binnet
	from normalisr_amd.coex import coex
	rng = np.random.default_rng(12)
	n, nt = 600, 80
	dc = covariates(rng, n)
	dt = expression(rng, nt, n, dc, strength=0.35).astype(np.float64)
	dt[:30] += 0.8 * rng.normal(size=n)[None, :] * rng.uniform(0.5, 1.5, 30)[:, None]  # a pathway that dominates the network
	dev = on_device(dt)
	p_dev = coex(dev, dc, device_out=True)[0]
	net_dev = binnet(p_dev, 0.05)
	assert net_dev.is_cuda
	genes_dev = gocovt.principal_genes(net_dev, n=20, device_out=True)
	cov_dev = gocovt.pccovt(dev, dc, None, genes_dev)
	p2_dev = coex(dev, cov_dev, device_out=True)[0].cpu().numpy()
	p_np = coex(dt, dc)[0]
	net_np = binnet(p_np, 0.05)
	genes_np = gocovt.principal_genes(net_np, n=20)
	cov_np = gocovt.pccovt(dt, dc, None, genes_np)
	p2_np = coex(dt, cov_np)[0]
	assert np.array_equal(net_dev.cpu().numpy(), net_np) and np.array_equal(genes_dev.cpu().numpy(), genes_np) and 20 <= len(genes_np) < nt
	assert cov_dev.shape == (dc.shape[0] + 1, n) and rel(cov_dev[-1], cov_np[-1]) < 1e-10
	assert relerr(p2_dev, p2_np, atol=1e-290) < 1e-6


# ---- the command line (child processes) ---------------------------------------------------------------------------------------------------------------------------

def test_cli_principal_and_pccovt(golden, tmp_path):
	"""`normalisr principal` and `normalisr pccovt` as child processes on text files written from G21, against the API on the same files read back."""
	from normalisr_amd import gocovt, run
	g = golden('G21_pccovt')
	f = lambda name: str(tmp_path / name)
	env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))

	def cli(*args):
		r = subprocess.run([sys.executable, '-m', 'normalisr_amd'] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
		assert r.returncode == 0, r.stderr[-3000:]

	names = lambda name: [v.strip() for v in open(f(name)) if v.strip()]
	np.savetxt(f('net.tsv'), g['net'].astype('u1'), delimiter='\t', fmt='%i')
	run.file_write_txtlist(f('net_genes.txt'), [str(v) for v in g['net_names']])
	cli('principal', f('net.tsv'), f('net_genes.txt'), f('master.txt'), '-n', '20')
	assert names('master.txt') == [str(v) for v in g['principal_names_20']] == [str(v) for v in g['net_names'][gocovt.principal_genes(g['net'], n=20)]]
	dt, dc, namet, genes, idx, cond, want = g21_case(g, 'c1')
	namet = ['G%04d' % i for i in range(len(namet))]  # (unique names in the files; the rows are those of the fixture)
	pathway = [namet[i] for i in idx]
	run.file_write_tsv(f('exp.tsv'), dt)
	run.file_write_tsv(f('cov.tsv'), dc)
	run.file_write_txtlist(f('genes.txt'), namet)
	run.file_write_txtlist(f('pathway.txt'), pathway)
	dt8, dc8 = run.file_read_tsv(f('exp.tsv')), run.file_read_tsv(f('cov.tsv'))  # what the text keeps: 8 digits
	for flags, cnd in (([], True), (['--nocond'], False)):
		cli('pccovt', f('exp.tsv'), f('cov.tsv'), f('genes.txt'), f('pathway.txt'), f('cov_out.tsv'), *flags)
		got = run.file_read_tsv(f('cov_out.tsv'))
		api = gocovt.pccovt(dt8, dc8, namet, pathway, condcov=cnd)
		assert got.shape == api.shape == (dc.shape[0] + 1, dt.shape[1])
		assert np.abs(got - api).max() <= 1e-7 * np.abs(api).max()  # '%.8G': eight significant digits
		if cnd:
			assert rel(got[-1], want[-1]) < 1e-5  # (and the reference's result, to what the rounded inputs allow)

