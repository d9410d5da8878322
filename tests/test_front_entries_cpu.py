"""The front-half whole-problem entries (csrc/nrm_host_front.hip) where no GPU is needed: their host arithmetic (csrc/nrm_host_math.h) in a stand-alone program
under g++ -fsanitize=address,undefined against numpy, every argument check before any device call, the imports of a process without torch, and the stability of
the numpy restatement the GPU test compares the 63-covariate compute_var with."""
import subprocess
import sys

import numpy as np
import pytest

import front_entries_child as child
import front_numpy
from cabi_harness import ROOT, build_and_run_host_program, close
from cabi_harness import vp as VP
from normalisr_amd import _lib


def _ulps(a, b):
	"""The largest distance of a from b in units of b's spacing."""
	a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
	return float(np.max(np.abs(a - b) / np.spacing(np.abs(b)))) if a.size else 0.0


def test_front_entry_math_under_address_and_ub_sanitizers(golden, tmp_path):
	"""tests/host/front_entry_math_sanitize.cpp built by g++ with -fsanitize=address,undefined and run directly (nothing loaded into python runs under a
	sanitizer), on inputs made from G18's reads; what it prints against numpy: integers exact, tables within 2 ulp, the pseudo-inverse close(1e-9) after
	multiplying out M M^+ M = M."""
	from scipy.special import digamma
	from normalisr_amd.norm import _pinv_gram_unit_rows
	from normalisr_amd.qc import qc_thresholds
	g, h = golden('G18_front'), golden('G18_front_chain')
	reads = g['reads'].astype(np.int64)
	psi, psi_t0 = digamma(1.0 + np.arange(int(reads.max()) + 1)), float(digamma(float(reads.sum() + 2)))
	total, nnz = reads.sum(axis=0), (reads != 0).sum(axis=0)
	hole = total.copy()
	hole[17] = 0
	c1 = np.vstack([h['normcov_c'], np.ones((1, reads.shape[1]))])  # 9 rows, rank-deficient: normcov_c ends with the ones row already
	rng = np.random.default_rng(11)
	cases = [(g20['a_params'], 300, 517) for g20 in (golden('G20_qc'), )] + [((0.5, 12.000001, 0.02, 60, 24.99, 1.0), 7, 13), ((0, 0, 0, 0, 0, 0), 1, 1),
																				 ((3, 1, 1 / 3, 2, 5, 2 / 7), 185, 374)]
	cases += [(tuple(rng.uniform(0, 50, 2)) + (rng.uniform(0, 1), ) + tuple(rng.uniform(0, 50, 2)) + (rng.uniform(0, 1), ), int(rng.integers(1, 5000)), int(rng.integers(1, 5000)))
			  for _ in range(20)]
	i64, f64 = lambda *v: np.array(v, dtype='<i8').tobytes(), lambda v: np.ascontiguousarray(v, dtype='<f8').tobytes()
	blob = i64(psi.size) + f64([psi_t0]) + f64(psi)
	blob += i64(*reads.shape) + i64(*total) + i64(*nnz) + i64(*reads.shape) + i64(*hole) + i64(*nnz)
	blob += i64(*c1.shape) + f64(c1) + i64(len(cases))
	for p, nt, ns in cases:
		blob += f64(p) + i64(nt, ns)
	src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.txt')
	with open(src, 'wb') as fh:
		fh.write(blob)
	build_and_run_host_program(tmp_path, ['tests/host/front_entry_math_sanitize.cpp'], 'front entry math ok', args=[src, dst], may_skip=True)
	got = {}
	for line in open(dst):
		name, *vals = line.split()
		got.setdefault(name, []).append(vals)
	num = lambda name, i=0: np.array(got[name][i], dtype=np.float64)
	# the tables: psi - psi(t0) is one subtraction (exact), exp within 2 ulp of numpy's, the same expression for unit
	tab = psi - psi_t0
	etab = np.exp(tab)
	assert np.array_equal(num('tab'), tab)
	print('etab ulps', _ulps(num('etab'), etab))
	assert _ulps(num('etab'), etab) <= 2
	unit = ((etab[1:] - etab[0]) / np.arange(1, etab.size)).max()
	mine = num('etab')
	assert num('unit')[0] == ((mine[1:] - mine[0]) / np.arange(1, mine.size)).max() and abs(num('unit')[0] - unit) <= 4 * np.spacing(etab.max())
	# the covariate rows
	assert [int(v[0]) for v in got['cov_stop']] == [-1, 17] and len(got['cov']) == 1
	cov = num('cov').reshape(3, -1)
	t1 = np.log(total)
	assert _ulps(cov[0], t1) <= 2 and np.array_equal(cov[1], reads.shape[0] - nnz) and _ulps(cov[2], t1**2) <= 6  # (the square of a value 2 ulp off: 4, and its own rounding)
	# the pseudo-inverse on unit-length rows
	m = c1 @ c1.T
	mine, ref = num('pinv').reshape(9, 9), _pinv_gram_unit_rows(c1)
	assert int(got['pinv_rank'][0][0]) == np.linalg.matrix_rank(c1) < 9
	assert close(m @ mine @ m, m, 1e-9, floor=1.0) and close(m @ mine @ m, m @ ref @ m, 1e-9, floor=1.0) and close(mine @ m @ mine, mine, 1e-9, floor=np.abs(mine).max())
	# the thresholds
	for vals, (p, nt, ns) in zip(got['thr'], cases):
		assert tuple(int(v) for v in vals) == qc_thresholds(p, nt, ns), (p, nt, ns)
	assert len(got['thr']) == len(cases)


def _codes(calls):
	lib = _lib.load()
	out = []
	for name, args in calls:
		rc = getattr(lib, name)(*args)
		out.append((rc, lib.nrm_last_error().decode()))
	return out


def test_front_entries_check_arguments_before_the_device():
	"""Null pointers, rows or n <= 0, dtype codes, covariate counts, stepmax, eps and QC parameters of the five entries: refused with the status and the words the
	binding turns into the reference's exceptions, on a machine without a GPU."""
	E_ARG, E_UNSUPPORTED = _lib.NRM_E_ARG, _lib.NRM_E_UNSUPPORTED
	x = np.ones((3, 4), dtype=np.int32)
	y, c = np.ones((3, 4)), np.ones((2, 4))
	indptr, indices, data = np.array([0, 1, 2, 3], dtype=np.int64), np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.int32)
	out, cov, zero, info, w, state = np.zeros((3, 4)), np.zeros((3, 4)), np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.int64), np.zeros(4), np.zeros(2)
	gm, cm = np.zeros(3, dtype=np.uint8), np.zeros(4, dtype=np.uint8)
	I32, F64 = _lib.NRM_I32, _lib.NRM_F64

	def lcpm(x=x, dtype=I32, rows=3, n=4, ntot=-1, out=out, odt=F64, zero=zero, info=info):
		return ('nrm_lcpm_host', (VP(x), dtype, rows, n, 1, ntot, VP(out), odt, VP(cov), VP(zero), VP(info)))

	def lcsr(indptr=indptr, indices=indices, data=data, dtype=I32, rows=3, n=4, nnz=3, out=out, odt=F64, info=info):
		return ('nrm_lcpm_csr_host', (VP(indptr), VP(indices), VP(data), dtype, rows, n, nnz, 1, -1, VP(out), odt, VP(cov), VP(zero), VP(info)))

	def cvar(y=y, ydt=F64, rows=3, n=4, c=c, nc=2, stepmax=1, eps=1e-6, w=w, state=state):
		return ('nrm_compute_var_host', (VP(y), ydt, rows, n, VP(c), nc, stepmax, eps, VP(w), VP(state)))

	def qc(x=x, dtype=I32, rows=3, n=4, p=(1, 1, 0.1, 1, 1, 0.1), gm=gm, cm=cm, info=info):
		return ('nrm_qc_reads_host', (VP(x), dtype, rows, n) + tuple(float(v) for v in p) + (VP(gm), VP(cm), VP(info)))

	def qcsr(indptr=indptr, indices=indices, data=data, dtype=I32, rows=3, n=4, nnz=3, p=(1, 1, 0.1, 1, 1, 0.1), gm=gm, info=info):
		return ('nrm_qc_reads_csr_host', (VP(indptr), VP(indices), VP(data), dtype, rows, n, nnz) + tuple(float(v) for v in p) + (VP(gm), VP(cm), VP(info)))

	bad_ptr = np.array([1, 1, 2, 3], dtype=np.int64)
	arg = [lcpm(x=None), lcpm(info=None), lcpm(out=None, zero=None), lcpm(rows=0), lcpm(n=-1), lcpm(dtype=F64), lcpm(dtype=99), lcpm(odt=7), lcpm(ntot=0),
		   lcsr(indptr=None), lcsr(indices=None), lcsr(data=None), lcsr(rows=0), lcsr(n=0), lcsr(nnz=-1), lcsr(n=1 << 31), lcsr(dtype=0), lcsr(odt=16), lcsr(info=None),
		   lcsr(indptr=bad_ptr), lcsr(nnz=2),
		   cvar(y=None), cvar(c=None), cvar(w=None), cvar(state=None), cvar(rows=0), cvar(n=0), cvar(ydt=I32), cvar(stepmax=0), cvar(stepmax=-3), cvar(eps=0.0), cvar(eps=-1.0),
		   cvar(eps=float('nan')), cvar(c=np.array([[1., 2, np.inf, 4], [1, 1, 1, 1]])),
		   qc(x=None), qc(gm=None), qc(cm=None), qc(info=None), qc(rows=0), qc(n=0), qc(dtype=1), qc(p=(-1, 1, 0.1, 1, 1, 0.1)), qc(p=(1, 1, 0.1, 1, -2, 0.1)),
		   qc(p=(1, 1, 1.5, 1, 1, 0.1)), qc(p=(1, 1, 0.1, 1, 1, 2)), qc(p=(float('nan'), 1, 0.1, 1, 1, 0.1)), qc(p=(1e19, 1, 0.1, 1, 1, 0.1)),
		   qcsr(indptr=None), qcsr(data=None), qcsr(rows=-1), qcsr(n=0), qcsr(dtype=3), qcsr(gm=None), qcsr(info=None), qcsr(p=(1, -1, 0.1, 1, 1, 0.1)),
		   qcsr(p=(1, 1, 0.1, 1, 1, 1.01)), qcsr(indptr=bad_ptr)]
	for (rc, msg), (name, _) in zip(_codes(arg), arg):
		assert rc == E_ARG and msg, (name, rc, msg)
	unsupported = [cvar(nc=0), cvar(nc=64), cvar(nc=-1), cvar(nc=1000)]
	for rc, msg in _codes(unsupported):
		assert rc == E_UNSUPPORTED and '63' in msg
	words = [msg for _, msg in _codes([lcpm(rows=0), cvar(eps=0.0), qc(p=(-1, 1, 0.1, 1, 1, 0.1)), qc(p=(1, 1, 1.5, 1, 1, 0.1)), lcsr(nnz=2), cvar(c=np.full((2, 4), np.nan))])]
	assert words == ['reads must not be empty.', 'eps and stepmax must be positive.', 'All parameters must be non-negative.',
									'Proportional parameters must be no greater than 1.', __import__('normalisr_amd.lcpm').lcpm.MALFORMED_CSR,
									'array must not contain infs or NaNs']
	with pytest.raises(NotImplementedError):
		_lib.check(_codes([cvar(nc=64)])[0][0])


def test_front_modules_import_without_torch():
	"""lcpm, norm, qc and run import, and the host-only calls run, in a process where `import torch` fails: normcov, qc_outlier, the four host variables of
	scaling_factor and subset need neither torch nor a device."""
	code = ("import sys\n"
			"sys.modules['torch'] = None\n"
			"sys.path.insert(0, {!r})\n"
			"import numpy as np, scipy.sparse\n"
			"import normalisr_amd.lcpm as lcpm, normalisr_amd.norm as norm, normalisr_amd.qc as qc, normalisr_amd.run\n"
			"rng = np.random.default_rng(0)\n"
			"x = rng.poisson(1.0, (9, 40))\n"
			"x[:, 0] += 1\n"
			"for v in ('logtpropmean', 'logtmeanprop', 'log1-nt0mean'):\n"
			"	assert lcpm.scaling_factor(x + 1 if v == 'logtmeanprop' else x, varname=v, v0='min').shape == (9, )\n"
			"dc = norm.normcov(rng.normal(size=(3, 40)))\n"
			"assert dc.shape == (4, 40) and (dc[3] == 1).all()\n"
			"assert qc.qc_outlier(np.exp(0.1 * rng.normal(size=500))).shape == (500, )\n"
			"rows, cols = np.array([5, 1, 1]), np.arange(40) % 3 == 0\n"
			"assert np.array_equal(qc.subset(x, rows, cols), x[rows][:, cols])\n"
			"s = qc.subset(scipy.sparse.coo_matrix(x), [1, 5], cols)\n"
			"assert scipy.sparse.issparse(s) and s.format == 'csr' and np.array_equal(s.toarray(), x[[1, 5]][:, cols]) and s.dtype == x.dtype\n"
			"for bad, err in (((x, [9], None), IndexError), ((scipy.sparse.csr_matrix(x), [5, 1], None), ValueError), ((x[0], None, None), ValueError),\n"
			"				 ((x, np.ones(8, dtype=bool), None), IndexError), ((x.astype(complex), None, None), TypeError)):\n"
			"	try:\n"
			"		qc.subset(*bad)\n"
			"		raise SystemExit('no error for a bad subset')\n"
			"	except err:\n"
			"		pass\n"
			"assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]\n"
			"print('front half without torch ok')\n").format(ROOT)
	r = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
	assert r.returncode == 0 and 'front half without torch ok' in r.stdout, r.stdout[-3000:]


def test_wide_compute_var_restatement_is_stable():
	"""The bound of the GPU test for 63 covariates of rank 62, close(1e-9, floor=1), means something only if the numpy restatement it compares with does not
	itself move by that much: two orders of the covariate rows (the fit does not depend on the order) agree within the bound, for the seed the GPU test uses."""
	y, dc = child.fitvar_wide()
	assert y.shape == (child.FITVAR_TILE + 1, 1030) and y.dtype == np.float32 and dc.shape == (63, 1030) and np.linalg.matrix_rank(dc) == 62
	a = front_numpy.compute_var(y, dc, stepmax=2)
	b = front_numpy.compute_var(y, dc[np.random.default_rng(1).permutation(63)], stepmax=2)
	print('two row orders differ by', np.abs(a - b).max())
	assert close(a, b, 1e-9, floor=1.0) and a.min() == 1
