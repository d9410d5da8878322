"""CPU: the extended-precision stage references of tests/front_longdouble.py against what the reference returned (golden G18), to 1e-12 -- a thousand times
tighter than tests/front_numpy.py is held --, the stage functions chained against the end-to-end function, and the library's host digamma against mpmath over
the whole range of its table (bound as in tests/test_front_cpu.py: 1e-14 |psi| + 1e-15)."""
import numpy as np
import pytest

import front_longdouble as fl
from normalisr_amd.association import inv_rank

pytest.importorskip('mpmath')


def rel(a, b, floor=0.0):
	a, b = fl.ld(a), fl.ld(b)
	return float(np.max(np.abs(a - b) / (np.abs(b) + floor)))


def test_longdouble_is_wider_than_fp64():
	assert np.finfo(np.longdouble).eps < 2.0**-60  # the references below are worth nothing where longdouble is fp64


def test_lcpm_reference_against_g18(golden):
	g = golden('G18_front')
	reads = g['reads']
	lc, t1, _ = fl.lcpm(reads)
	e = rel(lc, g['lcpm'], 1.0)
	print('lcpm: max error relative to |lcpm| + 1: %.3g' % e)
	assert e <= 1e-12
	assert rel(fl.lcpm(reads, normalize=False)[0], g['nonorm_lcpm'], 1.0) <= 1e-12
	assert rel(fl.lcpm(reads, ntot=1E9)[0], g['ntot_lcpm'], 1.0) <= 1e-12
	c = fl.counts(reads)
	assert (c['cell_nnz'] == reads.shape[0] - g['cov'][1]).all() and rel(np.log(fl.ld(c['cell_total'])), g['cov'][0]) <= 1e-12
	assert c['total'] == int(reads.sum()) and c['max'] == int(reads.max())
	sf = c['gene_zero'] / reads.shape[1]
	assert np.abs(sf / sf.max() - g['sf']).max() <= 1e-12
	# the stage functions on the fp64 tables reproduce the end-to-end function to the tables' rounding
	vals = np.arange(int(reads.max()) + 1)
	p, p0 = fl.psi_values(vals, c['total'] + 2)
	tab = (p - p0).astype(np.float64)
	s, t1s = fl.colsum(reads, np.exp(tab))
	assert np.abs(t1s - t1).max() <= 8 * fl.U
	assert np.abs(fl.write(reads, tab, t1s.astype(np.float64)) - lc).max() <= 8 * fl.U * (1 + np.abs(lc).max())


@pytest.mark.parametrize('steps,key', [(1, 'w1'), (3, 'w3')])
def test_compute_var_reference_against_g18(golden, steps, key):
	g, h = golden('G18_front'), golden('G18_front_chain')
	lc, dc = g['lcpm'], h['normcov_c']
	assert np.linalg.matrix_rank(dc) == dc.shape[0] - 1 and np.linalg.matrix_rank(dc[1:]) == dc.shape[0] - 1  # one-hot batches + the intercept: drop one batch
	w, t1s = fl.compute_var(lc, dc[1:], dc[1:], stepmax=steps)
	e = rel(w, h[key])
	print('compute_var stepmax=%d: max relative error %.3g, t1 per iteration %s' % (steps, e, [float(t) for t in t1s]))
	assert len(t1s) == steps and e <= 1e-12
	e2 = rel(fl.compute_var_fp64(lc, dc, stepmax=steps), w)
	print('the fp64 inv_rank restatement against longdouble: %.3g' % e2)
	assert e2 <= 1e-12


def test_stage_functions_chain_to_the_end_to_end_function():
	rng = np.random.default_rng(5)
	ng, n, nc = 37, 131, 4
	dc = rng.normal(size=(nc, n)) * np.array([30.0, 1 / 30.0, 1.0, 1.0])[:, None]
	dc[2] += 3.0
	dt = rng.uniform(0, 14, ng)[:, None] + np.exp(rng.normal(size=ng))[:, None] * rng.normal(size=(ng, n)) * np.exp(0.9 * dc[-1])
	c1 = np.vstack([dc, np.ones((1, n))])
	w, t1s = fl.compute_var(dt, dc, c1, stepmax=2, eps=1e-300)
	s, best, state = np.ones(n), np.full(n, np.nan), np.array([1e300, 0.0, np.nan, 0.0])
	m2i = inv_rank(c1 @ c1.T)[0]
	for it in range(2):
		u, cw, m, _ = fl.design(dc, s)
		mi = inv_rank(m.astype(np.float64))[0]
		a, _ = fl.moments(dt, cw)
		b, _ = fl.coef(a, mi)
		r, _ = fl.resid(dt, u, dc, b)
		mean, sc = fl.gene_stats(r)
		v = fl.cell_var(r, mean, sc)
		_, gl, _ = fl.logsum(v, dc)
		new = fl.new_scale(gl, m2i, dc, s)[2]
		new = (new / new.min()).astype(np.float64)
		s, best, state = fl.transition(new, s, best, state, 1e-300)
		assert state[1] == it + 1 and abs(state[2] / float(t1s[it]) - 1) <= 1e-9
	assert state[0] == min(float(t) for t in t1s) or abs(state[0] / float(min(t1s)) - 1) <= 1e-9
	assert rel(fl.weights(best), w) <= 1e-9  # (inv_rank in fp64 between the longdouble stages)


def test_transition_rules():
	s, best = np.array([1.0, 2.0, 4.0]), np.array([1.0, 1.0, 1.0])
	new = np.array([1.0, 3.0, 4.0])  # t1 = 0.5
	for bestv, better in ((0.6, True), (0.5, False), (0.4, False)):  # t1 below, equal to and above bestv
		s2, b2, st = fl.transition(new, s, best, np.array([bestv, 2.0, 9.0, 0.0]), 1e-6)
		assert np.array_equal(s2, new) and np.array_equal(b2, new if better else best) and np.array_equal(st, [0.5 if better else bestv, 3.0, 0.5, 0.0])
	s2, b2, st = fl.transition(new, s, best, np.array([1e-7, 2.0, 9.0, 0.0]), 1e-6)  # stopped: everything stays
	assert np.array_equal(s2, s) and np.array_equal(b2, best) and np.array_equal(st, [1e-7, 2.0, 9.0, 0.0])
	nan = np.array([1.0, np.nan, 4.0])
	s2, b2, st = fl.transition(nan, s, best, np.array([0.6, 0.0, 9.0, 0.0]), 1e-6)  # a NaN t1 is never the best step
	assert np.array_equal(b2, best) and st[0] == 0.6 and st[1] == 1.0 and np.isnan(st[2]) and np.isnan(s2[1])


def test_orthonormal_basis():
	rng = np.random.default_rng(2)
	x = rng.normal(size=(9, 200)) * 10.0**rng.uniform(-3, 3, 9)[:, None]
	q = fl.orthonormal(x)
	assert np.abs(q @ q.T - np.eye(9)).max() <= 1e-17
	assert np.abs((x @ q.T) @ q - x).max() <= 1e-15 * np.abs(x).max()


# ---- the library's digamma against mpmath ----------------------------------------------------------------------------------------------------------------
def _bound(ref):
	return 1e-14 * np.abs(ref.astype(np.float64)) + 1e-15


def test_digamma_table_against_mpmath_small_and_sampled():
	from normalisr_amd.lcpm import digamma_table
	top = (1 << 24) - 1
	psi, _ = digamma_table(top, 3.0)
	assert psi.shape == (top + 1, )
	xs = np.unique(np.concatenate([np.arange(4097), np.round(np.exp(np.linspace(np.log(4097.0), np.log(top), 600))).astype(np.int64), [top - 1, top]]))
	ref = fl.psi_values(xs, 3.0)[0]
	err = np.abs(fl.ld(psi[xs]) - ref).astype(np.float64) / _bound(ref)
	print('psi(1 + x), %d values up to 2^24 - 1: worst error / bound = %.3g at x = %d' % (xs.size, err.max(), xs[err.argmax()]))
	assert err.max() <= 1.0
	assert np.all(np.diff(psi[:100000]) > 0)  # increasing: what the CSR route's E[x] - E[0] >= 0 rests on


def test_digamma_t0_against_mpmath():
	from normalisr_amd.lcpm import digamma_table
	t0s = np.concatenate([2 + 2.0**-np.arange(1, 53, 3), [2.5, np.pi, 3.0, 7.25, 11.0, 11.5, np.nextafter(12.0, 0), 12.0, np.nextafter(12.0, 13), 12.5, 13.0, 100.75, 1e9 + 2, 2.0**40 + 0.5]])
	worst = 0.0
	for t0 in t0s:
		ref = fl.psi_values([], float(t0))[1]
		got = digamma_table(0, float(t0))[1]
		e = float(abs(fl.LD(got) - ref)) / float(1e-14 * abs(ref) + 1e-15)
		worst = max(worst, e)
		assert e <= 1.0, (t0, got, float(ref))
	print('psi(t0), %d arguments from just above 2 through the switch at 12: worst error / bound = %.3g' % (t0s.size, worst))
