"""GPU: K3 (csrc/nrm_sweep.hip, csrc/nrm_fix.h, csrc/nrm_pvalue.h) at kernel level -- nrm_assoc_sweep, nrm_assoc_sweep_band, nrm_assoc_sweep_mirror,
nrm_de_small_sweep and nrm_alpha called directly, every output against the reference of tests/k3_reference.py.

What is checked: placement (outputs are pre-filled with NaN, have a pitch 5 elements above the minimum and a 1024-byte tail; `dot` has a pitch of ny + 3 with
NaN in the padding and, for symmetric problems, NaN below the diagonal); on exact problems stat bit for bit against numpy and P bit for bit against
nrm_pvalues_from_r2 at the host's R^2 (the entry G12 pins to mpmath) -- through the straight-line P-value, the slow re-do and every kernel; on real problems
stat, r and t within running-error bounds of the longdouble values; P of a subset (the planted pairs and a spread of ln P) against mpmath at 60 digits
with G12's tolerance; bands and the pipelined assembly bit for bit against one call; flags 0 and 1; the guard's hits and worst estimate within the intervals
the reference derives per pair; the refusals.  tests/test_k3_reference_cpu.py shows that the comparators accept an fp64 emulation of K3 at every shape used
here and reject fourteen mutations of it, and that these cases launch every instantiation of the kernels.

Every test prints its worst error-to-bound ratio per output before it asserts (pytest -rP shows them); the last test prints the table of the run.
Measured on an MI355X: see DESIGN.md section 4, "K3 at kernel level"."""
import functools

import numpy as np
import pytest

import k3_reference as k3

pytestmark = pytest.mark.gpu

WORST = {}  # (kernel, output) -> (ratio, case)
F64, F32 = np.float64, np.float32


@functools.lru_cache(maxsize=None)
def _env():
	import torch
	from normalisr_amd import _lib
	from normalisr_amd import engine
	return torch, _lib, engine.get_engine()


def _dev(a):
	torch, _, _ = _env()
	return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pitched(h, pitch, fill=float('nan')):
	"""The host matrix in HBM with a row pitch of `pitch` elements, the padding filled with NaN: (the view, the allocation)."""
	torch, _, _ = _env()
	whole = torch.full((max(h.shape[0], 1), pitch), fill, dtype=torch.float64, device='cuda')
	view = whole[:h.shape[0], :h.shape[1]]
	view.copy_(torch.from_numpy(np.ascontiguousarray(h)))
	return view, whole


class Out:
	"""A NaN-pre-filled output of `rows` rows at pitch ldo, followed by a 1024-byte tail."""

	def __init__(self, rows, ldo, dtype):
		torch, _, _ = _env()
		self.rows, self.ldo, self.dtype = rows, ldo, np.dtype(dtype)
		self.tail = 1024 // self.dtype.itemsize
		self.t = torch.full((rows * ldo + self.tail, ), float('nan'), dtype=torch.float64 if dtype == F64 else torch.float32, device='cuda')

	def ptr(self, row=0, col=0):
		return self.t.data_ptr() + (row * self.ldo + col) * self.dtype.itemsize

	def get(self):
		"""The (rows, ldo) matrix; the tail must still be NaN."""
		a = self.t.cpu().numpy()
		assert np.isnan(a[self.rows * self.ldo:]).all(), 'written past the end of an output'
		return a[:self.rows * self.ldo].reshape(self.rows, self.ldo)


def _flags(prefill=(0, 0, 0, 0)):
	return _dev(np.array(prefill, dtype=np.int32))


def _records(pb):
	if not pb.ns:
		return None, None
	fx = _dev(pb.fx)
	return fx, fx if pb.sym else _dev(pb.fy)


def _ptr(t):
	return 0 if t is None else t.data_ptr()


def sweep(pb, dtype, stat_kind=0, want_rt=False, budget=0.0, prefill=(0, 0, 0, 0), band=None, outs=None, dot=None, ssx=None, ssy=None, origin=(0, 0), ldo=None):
	"""One nrm_assoc_sweep (band = (row0, row1): nrm_assoc_sweep_band) call on the problem.  outs: write into these (the same outputs again; origin: the
	problem is a block of them).  Returns (outs, flags as numpy)."""
	torch, _lib, eng = _env()
	h = pb.dot if dot is None else dot
	if pb.sym:
		h = np.where(np.tri(pb.nx, k=-1, dtype=bool), np.nan, h)  # nothing below the diagonal may reach a result
	d, _ = _pitched(h, pb.ny + 3)
	sx = _dev(pb.ssx if ssx is None else ssx)
	sy = sx if (pb.sym and ssy is None) else _dev(pb.ssy if ssy is None else ssy)
	fx, fy = _records(pb)
	fl = _flags(prefill)
	if outs is None:
		ldo = ldo or pb.ny + 5
		outs = {k: Out(pb.nx, ldo, dtype) for k in (('p', 'stat', 'r', 't') if want_rt else ('p', 'stat'))}
	o = lambda k: outs[k].ptr(*origin) if k in outs else 0
	code = _lib.NRM_F64 if dtype == F64 else _lib.NRM_F32
	common = (d.data_ptr(), d.stride(0), sx.data_ptr(), sy.data_ptr(), pb.nx, pb.ny, pb.n, float(pb.dof), 1 if pb.sym else 0, stat_kind, o('p'), o('stat'), o('r'), o('t'),
			  code, outs['p'].ldo, fl.data_ptr())
	tail = (pb.ns, _ptr(fx), _ptr(fy), float(budget), eng._stream())
	if band is None:
		rc = eng.lib.nrm_assoc_sweep(*common, *tail)
	else:
		rc = eng.lib.nrm_assoc_sweep_band(*common, band[0], band[1], *tail)
	_lib.check(rc)
	torch.cuda.synchronize()
	return outs, fl.cpu().numpy()


def mirror(pb, dtype, r0, c0, rows, budget=0.0, prefill=(0, 0, 0, 0), outs=None):
	"""nrm_assoc_sweep_mirror of the rectangle problem pb at (r0, c0) of a (rows, rows) result."""
	torch, _lib, eng = _env()
	d, _ = _pitched(pb.dot, pb.ny + 3)
	sx, sy = _dev(pb.ssx), _dev(pb.ssy)
	fx, fy = _records(pb)
	fl = _flags(prefill)
	if outs is None:
		outs = {k: Out(rows, rows + 5, dtype) for k in ('p', 'stat')}
	_lib.check(eng.lib.nrm_assoc_sweep_mirror(d.data_ptr(), d.stride(0), sx.data_ptr(), sy.data_ptr(), pb.nx, pb.ny, pb.n, float(pb.dof), outs['p'].ptr(), outs['stat'].ptr(),
											  _lib.NRM_F64 if dtype == F64 else _lib.NRM_F32, outs['p'].ldo, r0, c0, fl.data_ptr(), pb.ns, _ptr(fx), _ptr(fy), float(budget),
											  eng._stream()))
	torch.cuda.synchronize()
	return outs, fl.cpu().numpy()


def p_device(r2, dof, sym):
	"""nrm_pvalues_from_r2 on the host's R^2: the entry G12 holds to mpmath."""
	torch, _lib, eng = _env()
	d = _dev(np.asarray(r2, dtype=np.float64).ravel())
	p = torch.full_like(d, float('nan'))
	_lib.check(eng.lib.nrm_pvalues_from_r2(d.data_ptr(), d.numel(), float(dof), p.data_ptr(), eng._stream()))
	torch.cuda.synchronize()
	p = p.cpu().numpy().reshape(np.shape(r2))
	if sym:
		p[np.arange(p.shape[0]), np.arange(p.shape[0])] = 0.0
	return p


def logical(outs, nx, ny, origin=(0, 0)):
	"""name -> the (nx, ny) block at origin; everything else of every output must still be NaN."""
	res = {}
	for k, o in outs.items():
		a = o.get()
		m = np.zeros(a.shape, dtype=bool)
		m[origin[0]:origin[0] + nx, origin[1]:origin[1] + ny] = True
		assert np.isnan(a[~m]).all(), '%s: written outside its block' % k
		res[k] = a[origin[0]:origin[0] + nx, origin[1]:origin[1] + ny].copy()
	return res


def note(kernel, ws, case):
	for name, w in ws.items():
		print('%-30s %-16s worst error / bound %.3g at %s  (%s)' % (kernel, name, w.ratio, w.where, w.what))
		if w.ratio > WORST.get((kernel, name), (-1.0, ''))[0]:
			WORST[(kernel, name)] = (w.ratio, case)
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (kernel, case, bad)


def scal_id(s):
	return 'n%d-dof%d' % s


# ---- a, b, c: placement, bits, bounds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('scal', k3.SCALARS, ids=scal_id)
@pytest.mark.parametrize('ng', k3.SYM_NG)
def test_k3_symmetric(ng, scal, exact):
	"""k_assoc_sweep_sym<., 32> (stat_kind 0, no r / t) and k_assoc_sweep<.> with symmetric = 1 (r and t asked for; stat_kind 1): every output of both, and the
	generic kernel's P and covariance equal to the sym kernel's bit for bit."""
	n, dof = scal
	for ns in k3.NSS:
		pb = k3.problem(exact, True, ng, ng, n, dof, ns)
		ref = k3.reference(pb)
		pe = p_device(ref['r2_64'], dof, True) if exact else None
		for dtype in (F64, F32):
			case = 'sym ng%d %s ns%d %s %s' % (ng, scal_id(scal), ns, 'exact' if exact else 'real', dtype.__name__)
			outs, fl = sweep(pb, dtype)
			a = logical(outs, ng, ng)
			print(k3.instantiation('sweep', dtype, 1, 0, False))
			note(k3.instantiation('sweep', dtype, 1, 0, False), k3.judge(a, pb, ref, dtype, 0, pe), case)
			assert (fl == 0).all(), fl
			outs, fl = sweep(pb, dtype, want_rt=True)
			g = logical(outs, ng, ng)
			note(k3.instantiation('sweep', dtype, 1, 0, True), k3.judge(g, pb, ref, dtype, 0, pe), case + ' generic')
			assert (fl == 0).all(), fl
			assert k3.same_bits(g['p'], a['p']).all() and k3.same_bits(g['stat'], a['stat']).all(), 'generic and sym kernel differ'
			outs, fl = sweep(pb, dtype, stat_kind=1)
			g1 = logical(outs, ng, ng)
			ws = k3.judge(g1, pb, ref, dtype, 1, pe)
			ws.pop('stat symmetry')  # (d / vx is not symmetric; its diagonal is still 0)
			assert (np.diagonal(g1['stat']) == 0).all() and k3.same_bits(g1['p'], a['p']).all()
			note(k3.instantiation('sweep', dtype, 1, 1, False), ws, case + ' generic kind 1')
			assert (fl == 0).all(), fl


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('scal', k3.SCALARS, ids=scal_id)
@pytest.mark.parametrize('shape', k3.RECT, ids=lambda s: '%dx%d' % s)
def test_k3_rectangular(shape, scal, exact):
	"""k_assoc_sweep<.> with symmetric = 0: both stat kinds, r and t absent and present."""
	n, dof = scal
	nx, ny = shape
	for ns in k3.NSS:
		pb = k3.problem(exact, False, nx, ny, n, dof, ns)
		ref = k3.reference(pb)
		pe = p_device(ref['r2_64'], dof, False) if exact else None
		for dtype in (F64, F32):
			case = 'rect %dx%d %s ns%d %s %s' % (nx, ny, scal_id(scal), ns, 'exact' if exact else 'real', dtype.__name__)
			kernel = k3.instantiation('sweep', dtype)
			per = {}
			for kind, rt in ((0, False), (1, True)):
				outs, fl = sweep(pb, dtype, stat_kind=kind, want_rt=rt)
				per[kind] = logical(outs, nx, ny)
				note(kernel, k3.judge(per[kind], pb, ref, dtype, kind, pe), case + ' kind %d' % kind)
				assert (fl == 0).all(), fl
			assert k3.same_bits(per[0]['p'], per[1]['p']).all()
			if exact and dtype == F64:
				p64, s64 = per[0]['p'], per[1]
			if exact and dtype == F32:  # each fp32 output is np.float32 of the fp64 one
				assert k3.same_bits(per[0]['p'], p64.astype(F32)).all()
				assert all(k3.same_bits(per[1][k], s64[k].astype(F32)).all() for k in ('stat', 'r', 't'))


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('scal', k3.SCALARS, ids=scal_id)
@pytest.mark.parametrize('shape', k3.MIRROR, ids=lambda s: '%dx%d-r%d-c%d' % s)
def test_k3_mirror(shape, scal, exact):
	"""k_assoc_sweep_mirror<.>: the rectangle at (r0, c0) and its transpose at (c0, r0) of a larger result, bit for bit the same; nothing else is written."""
	n, dof = scal
	mx, my, r0, c0 = shape
	rows = r0 + mx
	for ns in k3.NSS:
		pb = k3.problem(exact, False, mx, my, n, dof, ns)
		ref = k3.reference(pb)
		pe = p_device(ref['r2_64'], dof, False) if exact else None
		for dtype in (F64, F32):
			case = 'mirror %s %s ns%d %s %s' % (shape, scal_id(scal), ns, 'exact' if exact else 'real', dtype.__name__)
			outs, fl = mirror(pb, dtype, r0, c0, rows)
			a, b = {}, {}
			for k, o in outs.items():
				h = o.get()
				m = np.zeros(h.shape, dtype=bool)
				m[r0:r0 + mx, c0:c0 + my] = True
				m[c0:c0 + my, r0:r0 + mx] = True
				assert np.isnan(h[~m]).all(), '%s: written outside the two rectangles' % k
				a[k], b[k] = h[r0:r0 + mx, c0:c0 + my].copy(), h[c0:c0 + my, r0:r0 + mx].T.copy()
				assert k3.same_bits(a[k], b[k]).all(), '%s: the mirrored rectangle differs' % k
			note(k3.instantiation('mirror', dtype), k3.judge(a, pb, ref, dtype, 0, pe), case)
			assert (fl == 0).all(), fl
			if exact and dtype == F64:
				a64 = a
			if exact and dtype == F32:
				assert all(k3.same_bits(a[k], a64[k].astype(F32)).all() for k in a)


@pytest.mark.parametrize('scal', k3.SCALARS, ids=scal_id)
def test_k3_fp32_outputs_are_the_fp64_ones_rounded(scal):
	"""Exact problems through the symmetric kernels: each fp32 output equals np.float32 of the fp64 one, bit for bit."""
	n, dof = scal
	for ns in k3.NSS:
		pb = k3.problem(True, True, 200, 200, n, dof, ns)
		for kw in (dict(), dict(want_rt=True), dict(stat_kind=1, want_rt=True)):
			a64 = logical(sweep(pb, F64, **kw)[0], 200, 200)
			a32 = logical(sweep(pb, F32, **kw)[0], 200, 200)
			for k in a64:
				with np.errstate(over='ignore'):
					assert k3.same_bits(a32[k], a64[k].astype(F32)).all(), (k, kw, ns)


# ---- d: bands and pieces ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('ns', k3.NSS)
def test_k3_bands_add_up_to_one_call(ns, dtype):
	"""nrm_assoc_sweep_band over [0,64) [64,192) [192,200) of ng = 200 into one NaN-filled output: after each call exactly what its comment promises is written
	(sym kernel: the band's rows from column row0 on and their mirror images; generic kernel: the band's rows), and the union is bit for bit the one-call result."""
	ng = 200
	pb = k3.problem(False, True, ng, ng, 4096, 4093, ns)
	for rt in (False, True):
		whole = logical(sweep(pb, dtype, want_rt=rt)[0], ng, ng)
		outs = None
		want = np.zeros((ng, ng), dtype=bool)
		i, j = np.indices((ng, ng))
		for r0, r1 in ((0, 64), (64, 192), (192, 200)):
			outs, fl = sweep(pb, dtype, want_rt=rt, band=(r0, r1), outs=outs)
			assert (fl == 0).all()
			if rt:
				want |= (i >= r0) & (i < r1)
			else:
				want |= ((i >= r0) & (i < r1) & (j >= r0)) | ((j >= r0) & (j < r1) & (i >= r0))
			for k, o in outs.items():
				got = o.get()[:, :ng]
				assert np.array_equal(~np.isnan(got), want), (k, r0, r1, rt)
				assert np.isnan(o.get()[:, ng:]).all()
		assert want.all()
		for k, o in outs.items():
			assert k3.same_bits(o.get()[:, :ng], whole[k]).all(), (k, rt)
	# a band not cut at 64 is refused and writes nothing
	with pytest.raises(ValueError, match='multiples of 64'):
		sweep(pb, dtype, band=(32, 128), outs=outs)
	with pytest.raises(ValueError, match='multiples of 64'):
		sweep(pb, dtype, band=(0, 100), outs=outs)
	for k, o in outs.items():
		assert k3.same_bits(o.get()[:, :ng], whole[k]).all()


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('ns', k3.NSS)
def test_k3_pipelined_assembly_equals_one_call(ns, dtype):
	"""As the pipelined coex assembles its result: per row block a diagonal block by nrm_assoc_sweep on a sub-view of the outputs plus nrm_assoc_sweep_mirror for
	the rectangle to its left.  Exact problem (the mirror kernel takes the correction with the roles of the two genes swapped, which rounds differently on real
	records): bit for bit the one-call result; the parts' hits sum into the whole's interval."""
	ng = 200
	pb, budget, _ = k3.guard_case('sym6-exact') if ns == 6 else (k3.problem(True, True, ng, ng, 4096, 4093, ns), 0.0, None)
	ref = k3.reference(pb)
	whole, fw = sweep(pb, dtype, budget=budget)
	whole = logical(whole, ng, ng)
	outs = {k: Out(ng, ng + 5, dtype) for k in ('p', 'stat')}
	hits = 0
	worst = 0
	for a, b in ((0, 128), (128, 200)):
		_, fl = sweep(pb.sub(a, b, a, b, True), dtype, budget=budget, outs=outs, origin=(a, a))
		hits += fl[2]
		worst = max(worst, fl[3])
		assert fl[0] == 0 and fl[1] == 0
		if a:
			_, fl = mirror(pb.sub(a, b, 0, a, False), dtype, a, 0, ng, budget=budget, outs=outs)
			hits += fl[2]
			worst = max(worst, fl[3])
			assert fl[0] == 0 and fl[1] == 0
	for k, o in outs.items():
		got = o.get()
		assert np.isnan(got[:, ng:]).all()
		assert k3.same_bits(got[:, :ng], whole[k]).all(), k
	if budget:
		g = k3.guard_reference(pb, ref, budget, 'unordered', dtype)
		print('hits: whole %d, parts %d, interval %s; worst bits whole %d parts %d' % (fw[2], hits, g['hits'], fw[3], worst))
		ws = dict(zip(('hits (parts)', 'worst (parts)'), k3.check_guard(np.array([0, 0, hits, worst], dtype=np.int32), 0, g)))
		ws.update(zip(('hits', 'worst'), k3.check_guard(fw, 0, g)))
		note('assembly ' + k3.instantiation('sweep', dtype, 1), ws, 'pipelined ns%d' % ns)


# ---- e: flags 0 and 1 ------------------------------------------------------------------------------------------------------------------------------------------------
def _flag_variants(pb):
	"""name -> (dot, ssx, ssy, flags[0] expected, flags[1] expected); None: the problem's own.  Ordinary data to these kernels: they raise flags."""
	i, j = (3, pb.ny - 1)
	v = {'clean': (None, None, None, False, False)}
	d = pb.dot.copy()
	d[i, j] = np.nan
	v['nan in dot'] = (d, None, None, True, False)
	s = pb.ssy.copy()
	s[pb.ny - 1] = np.inf
	v['inf in ss'] = (None, s, None, True, False) if pb.sym else (None, None, s, True, False)
	if pb.sym:
		d = pb.dot.copy()
		d[np.arange(pb.nx), np.arange(pb.nx)] = np.nan
		v['nan on the diagonal'] = (d, None, None, False, False)
	for name, eps, hit in (('R2 = 1 + 2e-8', 2e-8, True), ('R2 = 1 + 5e-9', 5e-9, False)):
		q = pb.copy()
		q.set_r(i, j, np.sqrt(1 + eps))
		v[name] = (q.dot, None, None, False, hit)
	return v


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('ns', k3.NSS)
def test_k3_flags_0_and_1(ns, dtype):
	"""flags[0] > 0 exactly when an off-diagonal in-range pair has a non-finite d or ss (NaN on a symmetric diagonal does not flag, nor does the NaN that fills
	the pitch padding and the lower triangle of every `dot` here: out-of-range rows of the last tile never flag), flags[1] > 0 exactly when some
	R^2 > 1 + 1e-8."""
	sym = k3.problem(False, True, 130, 130, 4096, 4093, ns, ones=False)
	rect = k3.problem(False, False, 65, 130, 4096, 4093, ns, ones=False)
	for pb, runs in ((sym, (dict(), dict(want_rt=True))), (rect, (dict(), 'mirror'))):
		for name, (dot, ssx, ssy, f0, f1) in _flag_variants(pb).items():
			for kw in runs:
				if kw == 'mirror':
					q = pb.copy()
					q.dot = pb.dot if dot is None else dot
					q.ssy = pb.ssy if ssy is None else ssy
					fl = mirror(q, dtype, 130, 0, 195)[1]
				else:
					fl = sweep(pb, dtype, dot=dot, ssx=ssx, ssy=ssy, **kw)[1]
				print('%-4s %-22s %-18s flags %s' % ('sym' if pb.sym else 'rect', name, kw, fl))
				assert (fl[0] > 0) == f0 and (fl[1] > 0) == f1 and fl[2] == 0 and fl[3] == 0, (name, kw, fl)


# ---- f: the guard ----------------------------------------------------------------------------------------------------------------------------------------------------
PRE = (0, 0, 7, int(np.float32(1e-30).view(np.int32)))


@pytest.mark.parametrize('name', k3.GUARD_CASES)
def test_k3_guard_hits_and_worst(name):
	"""flags[2] minus its pre-fill within the interval of hits, flags[3] within the interval of worst, for every kernel the case's shape reaches."""
	pb, budget, kind = k3.guard_case(name)
	ref = k3.reference(pb)
	for dtype in (F64, F32):
		if kind == 'sym':
			g = k3.guard_reference(pb, ref, budget, 'unordered', dtype)
			fl = sweep(pb, dtype, budget=budget, prefill=PRE)[1]
			print(name, dtype.__name__, 'sym kernel: flags', fl, 'hits interval', g['hits'], 'worst interval', g['worst'])
			note(k3.instantiation('sweep', dtype, 1), dict(zip(('hits', 'worst'), k3.check_guard(fl, PRE[2], g))), name)
			assert fl[0] == 0 and fl[1] == 0
			# the generic kernel visits both triangles and tests the fp64 P-value
			g64 = k3.guard_reference(pb, ref, budget, 'unordered', F64)
			fo = sweep(pb, dtype, budget=budget, prefill=PRE, want_rt=True)[1]
			lo, hi = 2 * g64['hits'][0], 2 * g64['hits'][1]
			print(name, dtype.__name__, 'generic kernel: flags', fo, 'hits interval', (lo, hi))
			go = dict(g64, hits=(lo, hi), worst=k3.guard_reference(pb, ref, budget, 'ordered', F64)['worst'])
			note(k3.instantiation('sweep', dtype, 1, 0, True), dict(zip(('hits', 'worst'), k3.check_guard(fo, PRE[2], go))), name)
			if name == 'exempt':
				assert fl[2] == PRE[2] and fo[2] == PRE[2]
			if name == 'large-g':
				assert fl[2] - PRE[2] >= 1
		else:
			g = k3.guard_reference(pb, ref, budget, 'rect', dtype if kind == 'mirror' else F64)
			if kind == 'mirror':
				fl = mirror(pb, dtype, 130, 0, 200, budget=budget, prefill=PRE)[1]
			else:
				fl = sweep(pb, dtype, budget=budget, prefill=PRE)[1]
			print(name, dtype.__name__, 'flags', fl, 'hits interval', g['hits'], 'worst interval', g['worst'])
			note(k3.instantiation('mirror' if kind == 'mirror' else 'sweep', dtype), dict(zip(('hits', 'worst'), k3.check_guard(fl, PRE[2], g))), name)
			assert fl[0] == 0 and fl[1] == 0


def test_k3_guard_off_and_saturation():
	"""budget = 0 and NS = 0 leave flags[2] and flags[3] untouched; flags[2] pre-filled with 2^30 stays exactly 2^30."""
	pb, budget, _ = k3.guard_case('sym6')
	rect, rbudget, _ = k3.guard_case('rect6')
	for dtype in (F64, F32):
		for kw in (dict(), dict(want_rt=True)):
			assert np.array_equal(sweep(pb, dtype, budget=0.0, prefill=PRE, **kw)[1], PRE)
			fl = sweep(pb, dtype, budget=budget, prefill=(0, 0, 1 << 30, 0), **kw)[1]
			assert fl[2] == 1 << 30 and fl[3] > 0, fl
		assert np.array_equal(mirror(rect, dtype, 130, 0, 200, budget=0.0, prefill=PRE)[1], PRE)
		assert mirror(rect, dtype, 130, 0, 200, budget=rbudget, prefill=(0, 0, 1 << 30, 0))[1][2] == 1 << 30
		p0 = k3.problem(False, True, 200, 200, 4096, 4093, 0)
		assert np.array_equal(sweep(p0, dtype, budget=budget, prefill=PRE)[1], PRE)


# ---- g: the streaming de sweep ---------------------------------------------------------------------------------------------------------------------------------------
def run_de(dp, G, const_last, kind, dtype, want_by, want_rt=True):
	"""One nrm_de_small_sweep call on the raw columns G: (outs as (nx, ny) arrays, ssy, by or None, flags)."""
	torch, _lib, eng = _env()
	nc, nx, ny, n, rank = dp['nc'], dp['nx'], dp['ny'], dp['n'], dp['rank']
	Gd, raw_d, dci_d, ssx_d = _dev(G), _dev(dp['ssraw']), (_dev(dp['dci']) if nc else None), _dev(dp['ssx'])
	outs = {k: Out(nx, ny + 5, dtype) for k in (('p', 'stat', 'r', 't') if want_rt else ('p', 'stat'))}
	o = lambda k: outs[k].ptr() if k in outs else 0
	ssy = torch.full((ny + 128, ), float('nan'), dtype=torch.float64, device='cuda')
	by = torch.full((ny * max(nc, 1) + 128, ), float('nan'), dtype=torch.float64, device='cuda')
	fl = _flags()
	_lib.check(eng.lib.nrm_de_small_sweep(Gd.data_ptr(), raw_d.data_ptr(), _ptr(dci_d), nc, rank, ssx_d.data_ptr(), nx, ny, n, float(dp['dof']), kind, o('p'), o('stat'), o('r'), o('t'),
										  _lib.NRM_F64 if dtype == F64 else _lib.NRM_F32, ny + 5, ssy.data_ptr(), by.data_ptr() if want_by else 0, fl.data_ptr(), const_last,
										  eng._stream()))
	torch.cuda.synchronize()
	ssy_h, by_h = ssy.cpu().numpy(), by.cpu().numpy()
	assert np.isnan(ssy_h[ny:]).all() and np.isnan(by_h[ny * nc if want_by else 0:]).all(), 'ssy / by: written past the end, or by written unasked'
	return logical(outs, nx, ny), ssy_h[:ny], by_h[:ny * nc].reshape(ny, nc) if want_by else None, fl.cpu().numpy()


@pytest.mark.parametrize('scal', [(4096, 4093), (32, 16)], ids=scal_id)
@pytest.mark.parametrize('nc,nx', k3.DE)
def test_k3_de_small_sweep(nc, nx, scal):
	"""k_de_small_sweep<.>: ssy (the clamp at 0 hit on rows 0-3, then the 0 -> n rule), by, and all four outputs against longdouble; const_last 0 and 1 from the
	same ordered G; rank 0 and > 0, with and without by_out; flags as for the other sweeps."""
	n, dof = scal
	ny = k3.DE_NY
	for rank in ((0, ) if nc == 0 else (0, nc)):
		dp = k3.de_problem(nc, nx, n, dof, rank)
		ref = k3.de_reference(dp)
		pb = k3.Problem(sym=False, nx=nx, ny=ny, n=n, dof=float(dof), ns=0, exact=False, plants={'quarter': (0, ny - 1), 'zero': (0, 4)})
		for const_last in ((0, ) if nc == 0 else (0, 1)):
			for dtype in (F64, F32):
				for want_by in ((False, ) if not (rank and nc) else (True, False)):
					for kind in (0, 1):
						a, ssy, by, fl = run_de(dp, k3.de_raw(dp['G'], nc, const_last), const_last, kind, dtype, want_by)
						ws = {k + ' placement': k3.placement(a[k], np.ones((nx, ny), dtype=bool), k) for k in a}
						ws['ssy'] = k3.worst(np.abs(k3.ld(ssy) - ref['ssy']), ref['ssy_bound'], 'ssy')
						assert (ssy[:4] == 0).all(), 'the clamp at 0'
						if want_by:
							ws['by'] = k3.worst(np.abs(k3.ld(by) - ref['by']), ref['by_bound'], 'by')
						ws['stat'] = k3.compare(a['stat'], ref, 'stat%d' % kind, dtype)
						ws['r'] = k3.compare(a['r'], ref, 'r', dtype)
						ws['t'] = k3.compare(a['t'], ref, 't', dtype)
						ws['p mpmath'] = k3.compare_p_subset(a['p'], pb, np.asarray(ref['out']['r2'], dtype=np.float64), dtype, d_r2=ref['bound']['r2'])
						note(k3.instantiation('de', dtype), ws, 'de nc%d nx%d %s rank%d cl%d kind%d' % (nc, nx, scal_id(scal), rank, const_last, kind))
						assert (fl == 0).all(), fl
		# flags as in (e): ordinary data to this kernel too
		for const_last in ((0, ) if nc == 0 else (0, 1)):
			vy6 = float(ref['ssy'][6])
			one = lambda eps: np.sqrt((1 + eps) * (dp['ssx'][0] or n) * vy6)
			for what, row, value, raw5, f0, f1 in (('NaN in G', 5, np.nan, None, True, False), ('R2 = 1 + 2e-8', 6, one(2e-8), None, False, True),
												   ('R2 = 1 + 5e-9', 6, one(5e-9), None, False, False), ('Inf in ssraw', 5, None, np.inf, True, False)):
				G, q = dp['G'].copy(), dict(dp)
				if value is not None:
					G[row, nc] = value
				if raw5 is not None:
					q['ssraw'] = dp['ssraw'].copy()
					q['ssraw'][row] = raw5
				for dtype in (F64, F32):
					fl = run_de(q, k3.de_raw(G, nc, const_last), const_last, 0, dtype, False, want_rt=False)[3]
					print('%-14s const_last %d %s flags %s' % (what, const_last, dtype.__name__, fl))
					assert (fl[0] > 0) == f0 and (fl[1] > 0) == f1, (what, const_last, fl)


# ---- h: alpha --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nc', [1, 3])
@pytest.mark.parametrize('kind', [0, 1])
def test_k3_alpha(kind, nc, dtype):
	"""k_alpha<.,.>: alpha = by - gamma bx from a statistic at a pitch above its row length, against longdouble."""
	torch, _lib, eng = _env()
	rng = np.random.default_rng([kind, nc])
	nx, ny, n = 5, 257, 4096
	stat = rng.normal(size=(nx, ny)).astype(dtype)
	ssx = n * rng.uniform(0.5, 2, nx)
	ssx[1] = 0.0
	bx, by = rng.normal(size=(nx, nc)), rng.normal(size=(ny, nc))
	ref, bound = k3.alpha_reference(stat, kind, ssx, n, bx, by)
	if dtype == F32:
		bound = bound + 2.0**-24 * np.abs(ref) + 2.0**-150
	ldg = ny + 3
	sd = torch.full((nx, ldg), float('nan'), dtype=torch.float64 if dtype == F64 else torch.float32, device='cuda')
	sd[:, :ny].copy_(torch.from_numpy(stat))
	out = torch.full((nx * ny * nc + 256, ), float('nan'), dtype=sd.dtype, device='cuda')
	code = _lib.NRM_F64 if dtype == F64 else _lib.NRM_F32
	ssx_d, bx_d, by_d = _dev(ssx), _dev(bx), _dev(by)
	_lib.check(eng.lib.nrm_alpha(sd.data_ptr(), code, ldg, kind, ssx_d.data_ptr(), n, bx_d.data_ptr(), by_d.data_ptr(), nx, ny, nc, out.data_ptr(), code, eng._stream()))
	torch.cuda.synchronize()
	h = out.cpu().numpy()
	assert np.isnan(h[nx * ny * nc:]).all()
	got = h[:nx * ny * nc].reshape(nx, ny, nc)
	note(k3.instantiation('alpha', dtype), dict(alpha=k3.worst(np.abs(k3.ld(got) - ref), bound, 'alpha')), 'alpha kind%d nc%d' % (kind, nc))


# ---- i: refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_k3_refusals_write_nothing():
	"""A mirror rectangle reaching the diagonal, NS = 4, records without flags, ldo < ny, symmetric with nx != ny: each returns an error and writes nothing
	(a band not cut at 64: test_k3_bands_add_up_to_one_call)."""
	torch, _lib, eng = _env()
	lib = eng.lib
	pb = k3.problem(False, False, 65, 130, 4096, 4093, 6)
	d, _ = _pitched(pb.dot, 133)
	sx, sy, fx, fy = _dev(pb.ssx), _dev(pb.ssy), _dev(pb.fx), _dev(pb.fy)
	outs = {k: Out(200, 205, F64) for k in ('p', 'stat')}
	fl = _flags()
	st = eng._stream()

	def call_sweep(nx=65, ny=130, sym=0, ldo=205, ns=6, flags=fl.data_ptr()):
		return lib.nrm_assoc_sweep(d.data_ptr(), 133, sx.data_ptr(), sy.data_ptr(), nx, ny, 4096, 4093.0, sym, 0, outs['p'].ptr(), outs['stat'].ptr(), 0, 0, _lib.NRM_F64, ldo,
								   flags, ns, fx.data_ptr(), fy.data_ptr(), 0.0, st)

	def call_mirror(r0, c0):
		return lib.nrm_assoc_sweep_mirror(d.data_ptr(), 133, sx.data_ptr(), sy.data_ptr(), 65, 130, 4096, 4093.0, outs['p'].ptr(), outs['stat'].ptr(), _lib.NRM_F64, 205, r0, c0,
										  fl.data_ptr(), 6, fx.data_ptr(), fy.data_ptr(), 0.0, st)

	for what, rc in (('mirror reaching the diagonal', call_mirror(129, 0)), ('mirror above the diagonal', call_mirror(135, 6)), ('NS = 4', call_sweep(ns=4)),
					 ('records without flags', call_sweep(flags=0)), ('ldo < ny', call_sweep(ldo=129)), ('symmetric with nx != ny', call_sweep(sym=1))):
		torch.cuda.synchronize()
		print('%-30s -> %d  %s' % (what, rc, lib.nrm_last_error().decode()))
		assert rc != 0, what
		assert all(np.isnan(o.get()).all() for o in outs.values()) and (fl.cpu().numpy() == 0).all(), what


def test_k3_zz_worst_ratios_of_this_run():
	"""The table the next K3 rewrite holds itself to: the worst error-to-bound ratio per kernel and output over the tests of this file that ran before this one
	in the same process.  It only reports (every ratio is asserted where it is measured, in note()): run alone, or before the others, it prints nothing."""
	for key in sorted(WORST):
		print('%-32s %-16s worst error / bound %.3g   (%s)' % (key + WORST[key]))
	assert all(v[0] <= 1 for v in WORST.values())
