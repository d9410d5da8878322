"""CPU-only checks of the pipeline's front half (lcpm, scaling_factor, normcov, compute_var): the library's digamma table against scipy's values, normcov
against what the reference returned, argument validation before any device call, the command line's parser, and the numpy restatements of
tests/front_numpy.py -- the independent check of the GPU tests' random shapes -- against the reference's results in golden G18 (tests/golden/make_g18.py).
Tolerances: 1e-9 with an absolute floor of 1 for fp64 quantities that are O(1) and pass through zero (the project's bound for fp64 quantities that are not
P-values), 1e-12 absolute for scaling factors (exact integers through three fp64 operations), 1e-14 relative + 1e-15 absolute for psi(1 + x)."""
import warnings

import numpy as np
import pytest

import front_numpy
from test_gpu_parity import close


def test_digamma_table_against_scipy_values(golden):
	from normalisr_amd.lcpm import digamma_table
	g = golden('G18_front')
	xs, ref = g['psi_x'], g['psi_digamma']
	psi, _ = digamma_table(int(xs.max()), 3.0)
	err = np.abs(psi[xs] - ref) / (1e-14 * np.abs(ref) + 1e-15)
	print('psi(1 + x): worst error / bound = %.3g at x = %d' % (err.max(), xs[err.argmax()]))
	assert err.max() <= 1.0
	for t0, r in zip(g['psi_t0'], g['psi_t0_digamma']):
		_, v = digamma_table(0, float(t0))
		assert abs(v - r) <= 1e-14 * abs(r) + 1e-15, (t0, v, r)
	with pytest.raises(NotImplementedError):
		digamma_table(1 << 24, 3.0)  # beyond the table's cap


def test_normcov_against_reference(golden):
	from normalisr_amd.normalisr import normcov
	g = golden('G18_front_chain')
	raw = g['cov_raw']
	out = normcov(raw)
	assert out.shape == g['normcov_c'].shape and close(out, g['normcov_c'], 1e-9, floor=1.0)
	assert (out[:4] == raw[:4]).all() and (out[-1] == 1).all()  # one-hot rows untouched, the intercept appended
	out = normcov(raw, c=False)
	assert out.shape == g['normcov_noc'].shape and close(out, g['normcov_noc'], 1e-9, floor=1.0)
	assert (normcov(np.zeros((0, 7))) == np.ones((1, 7))).all() and normcov(np.zeros((0, 7)), c=False).shape == (0, 7)
	with pytest.raises(ValueError):
		normcov(raw[0])
	with pytest.raises(ValueError):
		normcov(np.vstack([raw, 3 * np.ones((1, raw.shape[1]))]))  # a constant covariate
	near = raw.copy()
	near[4] = 1E8 + 1E-3 * np.sin(np.arange(raw.shape[1]))
	with pytest.warns(RuntimeWarning):
		normcov(near)


def test_argument_validation_before_any_device_call():
	import normalisr_amd.normalisr as norm
	x = np.ones((3, 5), dtype=np.int64)
	with pytest.raises(ValueError):
		norm.lcpm(x[0])
	with pytest.raises(ValueError):
		norm.lcpm(x - 2)
	with pytest.raises(ValueError):
		norm.lcpm(x.astype(np.float64) - 1.5)
	with pytest.raises(ValueError):
		norm.lcpm(x, varscale=-1)
	with pytest.raises(NotImplementedError):
		norm.lcpm(x, varscale=1)
	with pytest.raises(AssertionError):
		norm.lcpm(np.zeros((0, 5), dtype=np.int64))
	with pytest.raises(ValueError):
		norm.lcpm(x, out_dtype=np.float16)
	with pytest.raises(ValueError):
		norm.scaling_factor(x[0])
	with pytest.raises(ValueError):
		norm.scaling_factor(x, varname='median')
	y, c = np.zeros((3, 5)), np.ones((2, 5))
	with pytest.raises(ValueError):
		norm.compute_var(y, c, eps=0)
	with pytest.raises(ValueError):
		norm.compute_var(y, c, stepmax=0)
	with pytest.raises(ValueError):
		norm.compute_var(y[0], c)
	with pytest.raises(ValueError):
		norm.compute_var(y, c[:, :4])
	with pytest.raises(NotImplementedError):
		norm.compute_var(y, np.ones((64, 5)))
	for name in ('qc_reads', 'qc_outlier', 'gotop', 'pccovt'):
		with pytest.raises(NotImplementedError):
			getattr(norm, name)


def test_parser_accepts_the_front_sub_commands():
	from normalisr_amd.__main__ import build_parser
	p = build_parser()
	a = vars(p.parse_args(['lcpm', 'r.tsv', 'l.tsv', 's.tsv', 'c.tsv']))
	assert (a['cmd'], a['reads_in'], a['lcpm_out'], a['scale_out'], a['cov_out']) == ('lcpm', 'r.tsv', 'l.tsv', 's.tsv', 'c.tsv')
	assert a['sparse'] is False and a['rseed'] is None and a['nth'] == 0 and a['cov_in'] is None and a['var_out'] is None
	a = vars(p.parse_args(['lcpm', '-s', '-r', '3', '-n', '2', '-c', 'b.tsv', '--var_out', 'v.tsv', 'r.mtx', 'l.tsv', 's.tsv', 'c.tsv']))
	assert a['sparse'] is True and a['rseed'] == 3 and a['nth'] == 2 and a['cov_in'] == 'b.tsv' and a['var_out'] == 'v.tsv'
	a = vars(p.parse_args(['normcov', 'a.tsv', 'b.tsv']))
	assert (a['cmd'], a['cov_in'], a['cov_out'], a['no1']) == ('normcov', 'a.tsv', 'b.tsv', False)
	assert vars(p.parse_args(['normcov', '--no1', 'a.tsv', 'b.tsv']))['no1'] is True
	a = vars(p.parse_args(['fitvar', 'l.tsv', 'c.tsv', 'w.tsv']))
	assert (a['cmd'], a['lcpm_in'], a['cov_in'], a['weights_out']) == ('fitvar', 'l.tsv', 'c.tsv', 'w.tsv')
	from normalisr_amd import run
	assert all(callable(getattr(run, c)) for c in ('lcpm', 'normcov', 'fitvar'))


def test_numpy_restatements_match_the_reference(golden):
	g, h = golden('G18_front'), golden('G18_front_chain')
	reads = g['reads']
	assert reads.max() > 255 and 0.5 < (reads == 0).mean() < 0.7
	lc, cov = front_numpy.lcpm(reads)
	assert close(lc, g['lcpm'], 1e-9, floor=1.0) and close(cov[[0, 2]], g['cov'][[0, 2]], 1e-9, floor=1.0) and (cov[1] == g['cov'][1]).all()
	assert close(front_numpy.lcpm(reads, normalize=False)[0], g['nonorm_lcpm'], 1e-9, floor=1.0)
	assert close(front_numpy.lcpm(reads, ntot=1E9)[0], g['ntot_lcpm'], 1e-9, floor=1.0)
	lc5, cov5 = front_numpy.lcpm(reads, nocov=True)
	assert cov5 is None and close(lc5, h['nocov_lcpm'], 1e-9, floor=1.0)
	assert bool(h['lowmem_lcpm_equal']) and close(lc, h['lowmem_mean'], 1e-9, floor=1.0) and (h['lowmem_var'] == 0).all()
	assert np.abs(front_numpy.scaling_factor(reads) - g['sf']).max() <= 1e-12
	dc = h['normcov_c']
	assert np.linalg.matrix_rank(dc) == dc.shape[0] - 1  # one-hot batches + the intercept: rank-deficient by one
	for steps, key in ((1, 'w1'), (3, 'w3')):
		w = front_numpy.compute_var(g['lcpm'], dc, stepmax=steps)
		print('compute_var stepmax=%d: max relative error %.3g' % (steps, np.abs(w / h[key] - 1).max()))
		assert close(w, h[key], 1e-9, floor=1.0)
