"""logp=True on the GPU: ln P from the single=0 sweeps, finite where P underflows to 0.

The function alone against exact values (G25_logp_grid, tests/golden/make_g25.py), its agreement with the linear function, one stored problem
(G25_logp_case) through every route that reaches a sweep, and larger problems built from that problem's rows for the routes and kernels that only
run on more than one block row."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# Largest |d ln P| / (1 + |ln P|) of nrm_logpvalue against the exact values of G25_logp_grid, measured on an MI355X: 1.03e-13, at dof 16 and
# R^2 = 0.7768 (a = 8, where the series in 1 / alpha is at its worst, as for the linear function: 1.7e-13 on G12); from dof 30 on it is below
# 1.2e-15.  The bound is twice the figure, rounded up to one digit; it has to stay below 1e-9 whatever is measured.
FUNCTION_BOUND = 3e-13


@pytest.fixture(scope='module')
def eng():
	from normalisr_amd import engine
	return engine.get_engine()


@pytest.fixture(scope='module')
def case():
	return {k: v for k, v in np.load(os.path.join(GOLDEN, 'G25_logp_case.npz')).items()}


def _from_r2(eng, entry, r2, dof):
	import torch
	from normalisr_amd import _lib
	d_r2 = torch.from_numpy(np.ascontiguousarray(r2, dtype=np.float64)).cuda()
	out = torch.empty_like(d_r2)
	_lib.check(getattr(eng.lib, entry)(d_r2.data_ptr(), r2.size, float(dof), out.data_ptr(), 0))
	torch.cuda.synchronize()
	return out.cpu().numpy()


def test_logpvalue_function_against_exact_values(eng):
	g = np.load(os.path.join(GOLDEN, 'G25_logp_grid.npz'))
	assert FUNCTION_BOUND < 1e-9
	worst = (0.0, None)
	for dof in np.unique(g['dof']):
		m = g['dof'] == dof
		r2, ref = g['r2'][m], g['lnp'][m]
		got = _from_r2(eng, 'nrm_logpvalues_from_r2', r2, dof)
		assert np.isfinite(got).all() and (got <= 0).all(), dof
		err = np.abs(got - ref) / (1 + np.abs(ref))
		k = int(np.argmax(err))
		print('dof %g: max |d ln P| / (1 + |ln P|) = %.3g at R^2 = %.17g (ln P = %.17g)' % (dof, err[k], r2[k], ref[k]))
		if err[k] > worst[0]:
			worst = (float(err[k]), (float(dof), float(r2[k])))
	print('nrm_logpvalue against G25_logp_grid: worst %.3g at (dof, R^2) = %s' % worst)
	assert worst[0] <= FUNCTION_BOUND, worst


def test_logpvalue_edges(eng):
	r2 = np.array([0.0, -1e-3, 1e-300, 5e-324, 1.0, 1.0 + 1e-9, 2.0, np.nan, np.inf, 1.0 - 2.0**-53])
	for dof in (11.0, 2095.0, 499996.0):  # (dof 11: no fast path at all)
		got = _from_r2(eng, 'nrm_logpvalues_from_r2', r2, dof)
		assert (got[:4] == 0).all()  # x = fl(1 - R^2) >= 1: P = 1
		assert np.isneginf(got[4:7]).all()  # x <= 0: the linear path's exact 0
		assert np.isnan(got[7]) and np.isneginf(got[8])  # NaN propagates; R^2 = inf is x = -inf <= 0 (the sweeps count it as non-finite input)
		assert np.isfinite(got[9]) and got[9] < -150  # x = 2^-53, the smallest positive x there is: about (dof / 2) ln x


def test_logpvalue_agrees_with_the_linear_function(eng):
	g = np.load(os.path.join(GOLDEN, 'G25_logp_grid.npz'))
	seen = 0
	for dof in np.unique(g['dof']):
		m = g['dof'] == dof
		r2 = g['r2'][m]
		lnp = _from_r2(eng, 'nrm_logpvalues_from_r2', r2, dof)
		p = _from_r2(eng, 'nrm_pvalues_from_r2', r2, dof)
		ok = p >= 1e-300
		seen += int(ok.sum())
		err = np.abs(lnp[ok] - np.log(p[ok])) / (1 + np.abs(lnp[ok]))
		k = int(np.argmax(err))
		print('dof %g: max |ln P - ln(nrm_pvalue)| / (1 + |ln P|) = %.3g at R^2 = %.17g' % (dof, err[k], r2[ok][k]))
		assert (err <= 2 * FUNCTION_BOUND).all(), (dof, r2[ok][k], err[k])
		assert (p[~ok] < 1e-300).all() and np.isfinite(lnp[~ok]).all()  # where P leaves the double range ln P goes on
	assert seen > 300


# ---- the stored problem through every route ---------------------------------------------------------------------------------------------------------------
def _bound(ref, dtype):
	"""|d ln P| <= 1e-6 max(1, |ln P|), plus one rounding of the output dtype for fp32."""
	return 1e-6 * np.maximum(1, np.abs(ref)) + (2.0**-24 * np.abs(ref) if np.dtype(dtype) == np.float32 else 0)


def _host(a):
	return a.cpu().numpy() if hasattr(a, 'is_cuda') else np.asarray(a)


def _route_env(monkeypatch, eng, route, n):
	from normalisr_amd import _lib
	for k in ('NRM_GRAM', 'NRM_DE_PATH', 'NRM_DE_SPARSE', 'NRM_DEBUG', 'NRM_HOST_ENTRY', 'NRM_PIPELINE'):
		monkeypatch.delenv(k, raising=False)
	if 'f64' in route:
		monkeypatch.setenv('NRM_GRAM', 'f64')
	if 'general' in route or 'sparse' in route or 'chunked' in route:
		monkeypatch.setenv('NRM_DE_PATH', 'general')
		monkeypatch.setenv('NRM_DEBUG', 'de_path=general')
	if 'sparse' in route:
		monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	if 'chunked' in route:
		monkeypatch.setattr(eng, 'CHUNK_BYTES', 32 * n * 4, raising=False)
	if 'host' in route:
		monkeypatch.setenv('NRM_HOST_ENTRY', '1')
		assert _lib.host_entry_preferred()


def _inputs(case, route, dtype):
	n = int(case['cut']) if 'cut' in route else case['dt'].shape[1]
	dt = np.ascontiguousarray(case['dt'][:, :n], dtype=dtype)
	dc = np.ascontiguousarray(case['dc'][:, :n])
	dg = np.ascontiguousarray(case['dg'][:, :n], dtype=dtype)
	return dt, dc, dg, n


# (route, device_out): device_out returns torch tensors, so it is no keyword of the torch-free entry
COEX_ROUTES = [(r, d) for r in ('default', 'f64', 'cut') for d in (False, True)] + [(r, False) for r in ('host', 'host-f64', 'host-cut')]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('route,device_out', COEX_ROUTES)
def test_case_coex(case, eng, monkeypatch, route, dtype, device_out):
	from normalisr_amd import coex as mcoex
	dt, dc, _, n = _inputs(case, route, dtype)
	_route_env(monkeypatch, eng, route, n)
	ref = case['lnp_coex_cut' if 'cut' in route else 'lnp_coex']
	lnp, dot, var = mcoex.coex(dt, dc, logp=True, device_out=device_out)
	if device_out:
		assert lnp.is_cuda and dot.is_cuda
	p0, dot0, var0 = mcoex.coex(dt, dc, device_out=device_out)
	lnp, dot, p0, dot0 = _host(lnp), _host(dot), _host(p0), _host(dot0)
	assert lnp.dtype == np.dtype(dtype) and lnp.shape == (70, 70)
	# everything else is the same bytes as without logp
	assert dot.tobytes() == dot0.tobytes() and np.asarray(var).tobytes() == np.asarray(var0).tobytes()
	assert lnp.tobytes() == lnp.T.copy().tobytes() and np.isneginf(np.diag(lnp)).all() and (np.diag(p0) == 0).all()
	i, j = (int(v) for v in case['dup'])
	keep = ~np.eye(70, dtype=bool)
	keep[i, j] = keep[j, i] = False  # R^2 = 1 up to rounding: rounding decides between -inf and a large negative number
	err = np.abs(lnp[keep].astype(np.float64) - ref[keep])
	ratio = err / _bound(ref[keep], dtype)
	print('coex %s %s: worst |d ln P| / bound = %.3g; duplicate pair ln P = %r; guard %s' % (route, np.dtype(dtype).name, ratio.max(), float(lnp[i, j]),
																					 None if 'host' in route else eng.last_guard))
	assert not np.isnan(lnp).any() and np.isfinite(lnp[keep]).all() and (lnp[keep] <= 0).all()
	assert (ratio <= 1).all(), (route, ratio.max(), np.argwhere(keep)[np.argmax(ratio)])
	assert lnp[i, j] <= case['lnp_dup_bound'][1 if 'cut' in route else 0] and lnp[i, j] == lnp[j, i]
	# and the linear call is what it is there for: where P is representable it is exp(ln P); the planted pairs are exact zeros that ln P tells apart
	rep = keep & (ref > -80)
	assert np.allclose(np.exp(lnp[rep].astype(np.float64)), p0[rep], rtol=1e-4 if np.dtype(dtype) == np.float32 else 1e-5, atol=0)
	if 'cut' not in route:
		(a0, b0), (a1, b1) = case['planted_pairs'][:2]
		assert p0[a0, b0] == 0 and p0[a1, b1] == 0 and np.isfinite(lnp[a0, b0]) and lnp[a1, b1] < lnp[a0, b0] < -745


# (route, device_out): the results stay in HBM on the general and the sparse-design routes of the torch engine only
DE_ROUTES = ([(r, False) for r in ('streaming', 'general', 'general-f64', 'sparse', 'chunked', 'cut', 'cut-general', 'host', 'host-general', 'host-sparse', 'host-cut')] +
			 [(r, True) for r in ('general', 'general-f64', 'sparse', 'cut-general')])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('route,device_out', DE_ROUTES)
def test_case_de(case, eng, monkeypatch, route, dtype, device_out):
	from normalisr_amd.association import association_tests
	from normalisr_amd import de as mde
	dt, dc, dg, n = _inputs(case, route, dtype)
	_route_env(monkeypatch, eng, route, n)
	ref = case['lnp_de_cut' if 'cut' in route else 'lnp_de']
	if device_out:  # (de() returns numpy; the resident form is association_tests')
		call = lambda **ka: association_tests(dg, dt, dc, return_dot=False, device_out=True, **ka)
	else:
		call = lambda **ka: mde.de(dg, dt, dc, **ka)
	res, res0 = call(logp=True), call()
	lnp, p0 = _host(res[0]).astype(np.float64), _host(res0[0]).astype(np.float64)
	assert _host(res[0]).dtype == np.dtype(dtype) and lnp.shape == (5, 70)
	for a, b in zip(res[1:], res0[1:]):  # log fold change, alpha, the variances: the same bytes
		assert (a is None and b is None) or _host(a).tobytes() == _host(b).tobytes()
	if not device_out and 'host' not in route:
		path = getattr(eng._tls, 'path', '') or ''
		want = dict(streaming='streaming', cut='streaming', sparse='sparse-design', chunked='uploaded in chunks').get(route)
		assert want is None or want in path, (route, path)
	ratio = np.abs(lnp - ref) / _bound(ref, dtype)
	print('de %s %s: worst |d ln P| / bound = %.3g at %s' % (route, np.dtype(dtype).name, ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape)))
	assert np.isfinite(lnp).all() and (lnp <= 0).all()
	assert (ratio <= 1).all(), (route, ratio.max())
	rep = ref > -80
	assert np.allclose(np.exp(lnp[rep]), p0[rep], rtol=1e-4 if np.dtype(dtype) == np.float32 else 1e-5, atol=0)
	if 'cut' not in route:
		assert (p0[ref < -760] == 0).all() and (ref < -760).any()


def test_case_de_untested_rows_come_back_as_ln_one(case, monkeypatch, eng):
	from normalisr_amd import de as mde
	dt, dc, dg, n = _inputs(case, 'streaming', np.float32)
	_route_env(monkeypatch, eng, 'streaming', n)
	dg2 = np.concatenate([dg[:2], np.ones((1, n), dtype=np.float32), dg[2:]])  # a single-valued row is not tested: P = 1 (de.py:107-122)
	lnp = mde.de(dg2, dt, dc, logp=True)[0]
	p = mde.de(dg2, dt, dc)[0]
	assert (lnp[2] == 0).all() and (p[2] == 1).all() and np.array_equal(np.delete(lnp, 2, axis=0), mde.de(dg, dt, dc, logp=True)[0])


def test_cli_logp_writes_ln_p(case, tmp_path, monkeypatch, eng):
	"""`normalisr coex --logp` / `de --logp` through the command line's own route (the torch-free entry): ln P in pv_out, -INF on coex's diagonal."""
	from normalisr_amd.__main__ import main
	from normalisr_amd import run
	dt, dc, dg, n = _inputs(case, 'host', np.float64)
	_route_env(monkeypatch, eng, 'host', n)
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)  # (run() prefers the entries by itself)
	f = {k: str(tmp_path / (k + '.tsv')) for k in ('dt', 'dc', 'dg', 'pv', 'pv_de', 'lfc')}
	for k, v in (('dt', dt), ('dc', dc), ('dg', dg)):
		run.file_write_tsv(f[k], v)
	assert main(['coex', f['dt'], f['dc'], f['pv'], '--logp']) == 0
	assert main(['de', f['dg'], f['dt'], f['dc'], f['pv_de'], f['lfc'], '--logp']) == 0
	text = open(f['pv']).read()
	assert text.split('\t', 1)[0] == '-INF'
	got, got_de = run.file_read_tsv(f['pv']), run.file_read_tsv(f['pv_de'])
	i, j = (int(v) for v in case['dup'])
	keep = ~np.eye(70, dtype=bool)
	keep[i, j] = keep[j, i] = False
	text_digits = 1e-7  # ('%.8G': eight significant digits)
	assert (np.abs(got[keep] - case['lnp_coex'][keep]) <= _bound(case['lnp_coex'][keep], np.float64) + text_digits * np.abs(case['lnp_coex'][keep])).all()
	assert (np.abs(got_de - case['lnp_de']) <= _bound(case['lnp_de'], np.float64) + text_digits * np.abs(case['lnp_de'])).all()


# ---- more than one block row ------------------------------------------------------------------------------------------------------------------------------
def _rows_from_case(case, rows):
	"""`rows` gene rows built from the stored genes (without the duplicate and the gene all but collinear with another): the genes themselves, then fixed
	mixtures of two of them -- pairs with every R^2 from 0 to near 1, no two rows equal or proportional (the constant gene, all zero, is a row but no part of a
	mixture: a mixture with it would be a multiple of the other gene, R^2 = 1 up to rounding)."""
	drop = [int(case['planted_pairs'][2][1]), int(case['dup'][1])]
	base = np.delete(case['dt'], drop, axis=0)
	mix = np.delete(case['dt'], drop + [int(case['constant'])], axis=0)
	nb, nm = base.shape[0], mix.shape[0]
	out = [base[k] for k in range(min(rows, nb))]
	for k in range(rows - len(out)):
		i = k % nm
		j = (i + 1 + k // nm) % nm  # (every mixture from another pair of genes: no two of them all but collinear)
		w = np.float32(0.3 + 0.4 * ((k * 37) % 101) / 101)
		out.append(w * mix[i] + (np.float32(1) - w) * mix[j])
	return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def _check_against_linear(lnp, p0, dtype):
	"""ln P of a coex call against the linear call on the same input: exp(ln P) = P where P is representable, finite and below the underflow where it is not."""
	ng = lnp.shape[0]
	lnp, p0 = lnp.astype(np.float64), p0.astype(np.float64)
	off = ~np.eye(ng, dtype=bool)
	assert lnp.tobytes() == lnp.T.copy().tobytes() and np.isneginf(np.diag(lnp)).all()
	assert np.isfinite(lnp[off]).all() and (lnp[off] <= 0).all()
	tiny = np.finfo(dtype).tiny
	rep = off & (p0 >= tiny)
	# fp64: the two calls may take their Gram products from different engines, each within the relative 1e-6 of the parity contract; fp32: one rounding of
	# ln P in the output dtype is a relative |ln P| 2^-24 <= 88 x 6e-8 of a normal P
	assert np.allclose(np.exp(lnp[rep]), p0[rep], rtol=1e-5 if np.dtype(dtype) == np.float32 else 1e-6, atol=0)
	gone = off & (p0 == 0)
	assert (lnp[gone] < np.log(tiny) + 1).all()
	return int(rep.sum()), int(gone.sum())


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_second_coex_case_three_block_rows(case, eng, monkeypatch, dtype):
	"""130 genes: three block rows of 64, the last with two rows -- the 32-row pieces of the symmetric sweep and the mirrored writes meet a ragged edge."""
	from normalisr_amd import coex as mcoex
	_route_env(monkeypatch, eng, 'default', 2100)
	dt = _rows_from_case(case, 130).astype(dtype)
	lnp, dot, var = mcoex.coex(dt, case['dc'], logp=True)
	guard = dict(eng.last_guard)
	p0, dot0, var0 = mcoex.coex(dt, case['dc'])
	assert dot.tobytes() == dot0.tobytes() and var.tobytes() == var0.tobytes() and lnp.dtype == np.dtype(dtype)
	rep, gone = _check_against_linear(lnp, p0, dtype)
	print('130 genes %s: %d pairs with a representable P, %d with P = 0; guard %s' % (np.dtype(dtype).name, rep, gone, guard))
	assert rep > 1000 and gone > 50


@pytest.mark.parametrize('out_dtype', [np.float32, np.float64])
def test_band_and_mirror_entries_assemble_the_one_launch_result(case, eng, out_dtype):
	"""Kernel level, 130 genes, ln P: the symmetric problem in one launch (nrm_assoc_sweep_pk) against the same problem assembled the two ways the engine's
	other routes do -- band by band (nrm_assoc_sweep_band_pk in bands of 64 rows: the ragged last band has two rows), and a diagonal block per chunk plus
	nrm_assoc_sweep_mirror_pk on the 2 x 128 rectangle below it (the pipelined coex) -- bit for bit where the same kernel runs, to the function's own
	precision where another one does, and against the non-symmetric kernel."""
	import torch
	from normalisr_amd import _lib
	lib = eng.lib
	ng, n, dof = 130, 2100, 2095.0
	x = torch.from_numpy(_rows_from_case(case, ng)).cuda().double()
	x = x - x.mean(1, keepdim=True)
	mp = 256
	dot = torch.zeros((mp, mp), dtype=torch.float64, device='cuda')
	g = x @ x.T
	dot[:ng, :ng] = torch.triu(g) + torch.triu(g, 1).T  # (a matrix product is not symmetric to the last bit: the rectangle below reads the lower triangle)
	ss = torch.zeros(mp, dtype=torch.float64, device='cuda')
	ss[:ng] = (x * x).sum(1)
	tdt = torch.float32 if out_dtype == np.float32 else torch.float64
	code = _lib.NRM_F32 if out_dtype == np.float32 else _lib.NRM_F64
	esz = np.dtype(out_dtype).itemsize
	s = torch.cuda.current_stream().cuda_stream

	def outputs():
		return (torch.full((ng, ng), 7.0, dtype=tdt, device='cuda'), torch.full((ng, ng), 7.0, dtype=tdt, device='cuda'), torch.zeros(4, dtype=torch.int32, device='cuda'))
	res = {}
	for kind in (0, 1):
		p, st, fl = outputs()
		_lib.check(lib.nrm_assoc_sweep_pk(dot.data_ptr(), mp, ss.data_ptr(), ss.data_ptr(), ng, ng, n, dof, 1, 0, p.data_ptr(), st.data_ptr(), 0, 0, code, ng, fl.data_ptr(),
										  0, 0, 0, 0.0, kind, s))
		res[kind] = (p.cpu().numpy(), st.cpu().numpy(), fl.cpu().numpy())
	whole, stat = res[1][0], res[1][1]
	assert res[0][1].tobytes() == stat.tobytes() and not res[1][2].any()
	_check_against_linear(whole, res[0][0], out_dtype)
	# the non-symmetric kernel (with r and t: k_assoc_sweep) on the same products
	p, st, fl = outputs()
	r, t = torch.empty_like(p), torch.empty_like(p)
	_lib.check(lib.nrm_assoc_sweep_pk(dot.data_ptr(), mp, ss.data_ptr(), ss.data_ptr(), ng, ng, n, dof, 1, 0, p.data_ptr(), st.data_ptr(), r.data_ptr(), t.data_ptr(), code, ng,
									  fl.data_ptr(), 0, 0, 0, 0.0, 1, s))
	assert p.cpu().numpy().tobytes() == whole.tobytes() and st.cpu().numpy().tobytes() == stat.tobytes()
	# band by band
	p, st, fl = outputs()
	for a, b in ((0, 64), (64, 128), (128, 130)):
		_lib.check(lib.nrm_assoc_sweep_band_pk(dot.data_ptr(), mp, ss.data_ptr(), ss.data_ptr(), ng, ng, n, dof, 1, 0, p.data_ptr(), st.data_ptr(), 0, 0, code, ng, fl.data_ptr(),
											   a, b, 0, 0, 0, 0.0, 1, s))
	assert p.cpu().numpy().tobytes() == whole.tobytes() and st.cpu().numpy().tobytes() == stat.tobytes() and not fl.cpu().numpy().any()
	# chunk by chunk: rows [0, 128) with themselves, rows [128, 130) with themselves, and the rectangle rows [128, 130) x columns [0, 128) mirrored
	p, st, fl = outputs()
	for a, b in ((0, 128), (128, 130)):
		sub = dot[a:, a:]
		_lib.check(lib.nrm_assoc_sweep_pk(sub.data_ptr(), mp, ss[a:].data_ptr(), ss[a:].data_ptr(), b - a, b - a, n, dof, 1, 0, p.data_ptr() + (a * ng + a) * esz,
										  st.data_ptr() + (a * ng + a) * esz, 0, 0, code, ng, fl.data_ptr(), 0, 0, 0, 0.0, 1, s))
	rect = dot[128:, :]
	_lib.check(lib.nrm_assoc_sweep_mirror_pk(rect.data_ptr(), mp, ss[128:].data_ptr(), ss.data_ptr(), 2, 128, n, dof, p.data_ptr(), st.data_ptr(), code, ng, 128, 0,
											 fl.data_ptr(), 0, 0, 0, 0.0, 1, s))
	got = p.cpu().numpy()
	assert st.cpu().numpy().tobytes() == stat.tobytes() and not fl.cpu().numpy().any()
	# the two diagonal blocks come from the kernel of the one launch: the same bits.  The rectangle and its mirror image come from another kernel, into which
	# the compiler inlines the function on its own terms (contractions may differ): the same value to twice the function's own bound, and bitwise symmetric
	assert got[:128, :128].tobytes() == whole[:128, :128].tobytes() and got[128:, 128:].tobytes() == whole[128:, 128:].tobytes()
	assert got.tobytes() == got.T.copy().tobytes()
	a64, b64 = got[128:, :128].astype(np.float64), whole[128:, :128].astype(np.float64)
	assert np.isfinite(a64).all() and (np.abs(a64 - b64) <= 2 * FUNCTION_BOUND * (1 + np.abs(b64)) + (2.0**-24 * np.abs(b64) if out_dtype == np.float32 else 0)).all()
	print('mirror rectangle against the one launch: %d of %d entries differ in their bits' % (int((a64 != b64).sum()), a64.size))


def test_guard_in_ln_p_mode_counts_by_relative_ln_p(case, eng):
	"""The integer engine's guard with p_kind 1 at kernel level: row records whose bound is harmless for weak pairs and too large for strong ones.  In P mode
	the strong pairs (P = 0 on the whole interval) are exempt; in ln P mode none is, and a pair counts when the bound exceeds budget x max(1, |ln P|)."""
	import torch
	from normalisr_amd import _lib
	lib = eng.lib
	ng, n, dof = 130, 6000, 5995.0  # (from ~5200 cells on every R^2 >= 1/4 has P = 0)
	g = torch.Generator(device='cuda').manual_seed(5)
	x = torch.randn((ng, n), dtype=torch.float64, device='cuda', generator=g)
	x[64:] += 1.5 * torch.randn((1, n), dtype=torch.float64, device='cuda', generator=g)  # rows 64.. share a factor: R^2 = 0.48 among them
	x = x - x.mean(1, keepdim=True)
	mp = 256
	dot = torch.zeros((mp, mp), dtype=torch.float64, device='cuda')
	dot[:ng, :ng] = x @ x.T
	ss = torch.zeros(mp, dtype=torch.float64, device='cuda')
	ss[:ng] = (x * x).sum(1)
	fix = torch.zeros((mp, 8), dtype=torch.float64, device='cuda')
	fix[:, 6] = 2e-8  # g_i: |delta r| <= g_i + g_j = 4e-8 for every pair, no correction (u = 0, c = 0)
	s = torch.cuda.current_stream().cuda_stream
	r2 = (dot[:ng, :ng]**2 / torch.outer(ss[:ng], ss[:ng])).cpu().numpy()
	off = ~np.eye(ng, dtype=bool)
	budget = 2.5e-7
	hits = {}
	for kind in (0, 1):
		p = torch.empty((ng, ng), dtype=torch.float64, device='cuda')
		st = torch.empty_like(p)
		fl = torch.zeros(4, dtype=torch.int32, device='cuda')
		_lib.check(lib.nrm_assoc_sweep_pk(dot.data_ptr(), mp, ss.data_ptr(), ss.data_ptr(), ng, ng, n, dof, 1, 0, p.data_ptr(), st.data_ptr(), 0, 0, _lib.NRM_F64, ng,
										  fl.data_ptr(), 6, fix.data_ptr(), fix.data_ptr(), budget, kind, s))
		hits[kind] = (int(fl.cpu().numpy()[2]), p.cpu().numpy())
	lnp = hits[1][1]
	# the rule, restated on the host from the same R^2 (upper triangle: every pair is tested once)
	ar = np.sqrt(r2)
	with np.errstate(divide='ignore'):  # (the diagonal, R^2 = 1: no pair)
		bound = 4e-8 * (np.sqrt(dof) + dof * ar) / (1 - r2)**2
	scale = np.maximum(1, np.abs(lnp))
	up = np.triu(off)
	margin = 1e-3  # (|r| comes from a single-precision square root rounded up: pairs this close to the threshold may fall either way)
	sure = int((up & (bound > budget * scale * (1 + margin))).sum())
	maybe = int((up & (bound > budget * scale * (1 - margin))).sum())
	print('guard: P mode %d hits, ln P mode %d hits (host rule: %d..%d)' % (hits[0][0], hits[1][0], sure, maybe))
	assert sure <= hits[1][0] <= maybe and sure > 0
	strong = up & (r2 > 0.25)
	assert (hits[0][1][strong] == 0).all() and np.isfinite(lnp[strong]).all()
	# P mode exempts every strong pair (P = 0 on the whole interval); what it counts are weak pairs only
	weak_sure = int((up & ~strong & (bound > budget * (1 + margin))).sum())
	weak_maybe = int((up & ~strong & (bound > budget * (1 - margin))).sum())
	assert weak_sure <= hits[0][0] <= weak_maybe
	# the strong pairs (bound 6e-4 against 2.5e-7 x |ln P| = 5e-4) are what the two forms disagree about
	assert hits[1][0] - hits[0][0] >= int((strong & (bound > budget * scale * (1 + margin))).sum()) > 1000


# ---- the routes that only run on more than 1024 genes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wide(case, eng):
	"""1100 genes built from the stored rows, and ln P of their coex from the general route on the fp64 Gram kernel (the reference of the routes below)."""
	from normalisr_amd.engine import as_input
	dt = as_input(_rows_from_case(case, 1100))
	dc = case['dc']
	from normalisr_amd.association import _prepare_covariates
	dc64, dci, dcr = _prepare_covariates(dc)
	with eng.forced_f64():
		res = eng.association_single0(dt, None, dc64, dci, dcr, 0, return_dot=True, want_alpha=False, out_dtype=np.float64, device_out=True, logp=True)
	return dict(dt=dt, dc64=dc64, dci=dci, dcr=dcr, lnp=res['p'].cpu().numpy(), stat=res['stat'].cpu().numpy())


@pytest.mark.parametrize('route', ['banded', 'pipelined', 'resident'])
def test_wide_coex_routes(wide, eng, monkeypatch, route):
	import torch
	for k in ('NRM_GRAM', 'NRM_DEBUG', 'NRM_HOST_ENTRY', 'NRM_PIPELINE'):
		monkeypatch.delenv(k, raising=False)
	dt, ng, n = wide['dt'], 1100, 2100
	if route == 'resident':
		d_x = torch.from_numpy(dt).cuda()
		res = eng.coex_blocks_resident(lambda a, b: d_x[a:b].clone(), ng, n, wide['dc64'], wide['dci'], wide['dcr'], 0, np.float32, block_rows=512, logp=True)
		eng.check_flags(res['flags'])
		lin = eng.coex_blocks_resident(lambda a, b: d_x[a:b].clone(), ng, n, wide['dc64'], wide['dci'], wide['dcr'], 0, np.float32, block_rows=512)
		lnp, stat, stat0 = res['p'].cpu().numpy(), res['stat'].cpu().numpy(), lin['stat'].cpu().numpy()
	else:
		# (the pipelined route is the integer engine's: a rerun on the fp64 Gram kernel takes the general one, as it does at full size)
		monkeypatch.setattr(eng, 'coex_pipelined_ok', lambda dx, dc, n_: route == 'pipelined' and eng.gram_slices(n_) > 0)
		monkeypatch.setattr(eng, 'banded_ok', lambda nx, ny, odt: route == 'banded')
		out = []
		for logp in (True, False):
			r = eng.association_single0(dt, None, wide['dc64'], wide['dci'], wide['dcr'], 0, return_dot=True, want_alpha=False, out_dtype=np.float32, logp=logp)
			if not eng.last_guard['fallback']:
				assert ('chunk by chunk' in eng._tls.path) == (route == 'pipelined')
			out.append((np.array(r['p']), np.array(r['stat'])))
		(lnp, stat), (_, stat0) = out
	print('1100 genes, %s: guard %s' % (route, eng.last_guard))
	assert stat.tobytes() == stat0.tobytes() and lnp.dtype == np.float32
	assert lnp.tobytes() == lnp.T.copy().tobytes() and np.isneginf(np.diag(lnp)).all()
	off = ~np.eye(ng, dtype=bool)
	ref = wide['lnp'][off]
	ratio = np.abs(lnp[off].astype(np.float64) - ref) / _bound(ref, np.float32)
	print('1100 genes, %s: worst |d ln P| / bound against the fp64 Gram kernel = %.3g' % (route, ratio.max()))
	assert np.isfinite(lnp[off]).all() and (ratio <= 1).all()
