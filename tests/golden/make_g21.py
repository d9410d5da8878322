#!/usr/bin/env python3
"""Generate tests/golden/G21_pccovt.npz by IMPORTING the reference (dev container only, like make_g20.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g21.py

Principal genes: a seeded symmetric 97-gene network whose degrees tie at the thresholds, through the reference's own gotop for n = 5, 20 and 60 with its GO
enrichment (goatools and a web service) replaced by a stub, so that the reference's selection code runs and its enrichment does not.
pccovt: five cases with covariates as normcov builds them (4 one-hot batches, 3 continuous ones in units of 1, 30 and 0.01, the intercept).  The reference
takes the component from a randomized SVD with an unseeded generator, so a case is a fixture only where the reference reproduces itself: the script asserts
that 10 calls stay within 1e-11 of the exact restatement (tests/pc_numpy.py in float64), relative to max |score| -- 5e-7 for the fp32 case, which the reference
computes in fp32 -- and stores the first call.  Arrays and name lists only; every input is exactly representable in fp32 and stored as fp32, case 3 (300 x 2000)
as int8 codes with x = 200 + code / 8.  One file, below 1 MB.
"""
import os
import sys
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')
sys.path.insert(0, os.path.dirname(HERE))

import normalisr.gocovt as refgo  # noqa: E402
import normalisr.norm as refnorm  # noqa: E402
import pc_numpy  # noqa: E402


def covariates(rng, n):
	batch = rng.integers(0, 4, n)
	batch[:4] = np.arange(4)
	raw = np.concatenate([(batch[None, :] == np.arange(4)[:, None]).astype(float), rng.normal(0, 1, (1, n)), rng.normal(100, 30, (1, n)), rng.normal(0.05, 0.01, (1, n))])
	dc = refnorm.normcov(raw)
	assert dc.shape == (8, n) and (dc[-1] == 1).all()
	return dc


def expression(rng, ng, n, dc, strength, shift=0.0, second=0.0):
	"""noise + a common factor of mixed sign (+ a weaker second one) + covariate effects + shift, rounded to fp32."""
	load = rng.choice([-1.0, 1.0], ng) * rng.uniform(0.6, 1.4, ng)
	x = rng.normal(0, 1, (ng, n)) + strength * load[:, None] * rng.normal(0, 1, n)[None, :]
	if second:
		x += second * rng.normal(0, 1, ng)[:, None] * rng.normal(0, 1, n)[None, :]
	if dc is not None:
		x += rng.normal(0, 0.5, (ng, dc.shape[0])) @ dc
	return (x + shift).astype(np.float32)


def settle(name, dt, dc, namet, genes, condcov, bound, out):
	"""10 calls of the reference against the exact restatement; stores the first call under name + '_out'."""
	where = dict(zip(namet, range(len(namet))))
	idx = np.array([where[g] for g in genes], dtype=np.int64)
	score, v, lam, z = pc_numpy.pccovt(dt, dc, idx, condcov=condcov, return_all=True)
	ratio = pc_numpy.singular_ratio(z)
	worst, first = 0.0, None
	for _ in range(10):
		got = refgo.pccovt(dt, dc, namet, genes, condcov=condcov)
		assert got.shape == (dc.shape[0] + 1, dt.shape[1]) and np.array_equal(got[:-1], dc)
		first = got if first is None else first
		worst = max(worst, float(np.abs(got[-1].astype(np.float64) - score).max() / np.abs(score).max()))
	print('{}: genes {} m {} cells {} sigma2/sigma1 {:.3f} dtype {} -> {}: worst deviation of 10 reference calls {:.3g} (bound {:g})'.format(
		name, dt.shape[0], len(idx), dt.shape[1], ratio, dt.dtype, first.dtype, worst, bound))
	assert worst <= bound, (name, worst)
	out[name + '_idx'] = idx
	out[name + '_genes'] = np.array(genes)
	out[name + '_namet'] = np.array(namet)
	out[name + '_out'] = first
	out[name + '_ratio'] = ratio


def main():
	import logging
	logging.disable(logging.WARNING)
	out = {}
	# ---- principal genes ----
	rng = np.random.default_rng(2101)
	ng = 97
	p = np.minimum(1.0, np.outer(rng.uniform(0.02, 0.9, ng), rng.uniform(0.02, 0.9, ng)) * 0.5)
	net = np.triu(rng.random((ng, ng)) < p, 1)
	net = net | net.T
	names = np.array(['G%04d' % i for i in range(ng)])
	refgo.goe = lambda genelist, go_file, goa_file, bg=None, **ka: (None, 'GO:0000000', list(genelist))  # the enrichment does not run; the selection does
	out['net'] = net
	out['net_names'] = names
	for n in (5, 20, 60):
		got = refgo.gotop(net, names, None, None, n=n)[0]
		mine = pc_numpy.principal(net, n)
		assert got == [str(v) for v in names[mine]], n
		deg = net.sum(axis=1)
		thr = np.sort(deg)[::-1][n]
		print('principal n = {}: {} genes, threshold degree {}, {} genes at the threshold'.format(n, len(mine), thr, int((deg == thr).sum())))
		out['principal_%d' % n] = mine
		out['principal_names_%d' % n] = np.array(got)
	assert len(out['principal_5']) > 6  # (ties at the threshold)
	# ---- pccovt ----
	rng = np.random.default_rng(2102)
	# case 1: 40 genes, 7 chosen by name; one name stands twice in namet (the last one is taken) and one gene twice in genes
	dc1 = covariates(rng, 257)
	dt1 = expression(rng, 40, 257, dc1, 0.9, shift=3.0)
	namet1 = ['G%04d' % i for i in range(40)]
	namet1[20] = namet1[3]
	genes1 = [namet1[i] for i in (31, 3, 8, 17, 8, 25, 38)]
	settle('c1', dt1.astype(np.float64), dc1, namet1, genes1, True, 1e-11, out)
	out['c1_dt'], out['c1_dc'] = dt1, dc1
	# case 2: no covariates
	dt2 = expression(rng, 64, 333, None, 0.6, shift=1.0)
	namet2 = ['G%04d' % i for i in range(64)]
	genes2 = [namet2[i] for i in (5, 60, 11, 12, 33, 40, 2, 63, 21)]
	dc2 = np.zeros((0, 333))
	settle('c2', dt2.astype(np.float64), dc2, namet2, genes2, True, 1e-11, out)
	out['c2_dt'], out['c2_dc'] = dt2, dc2
	# case 3: 300 genes, 200 chosen, a planted common factor of mixed sign, every row shifted by 200; int8 codes
	dc3 = covariates(rng, 2000)
	raw = expression(rng, 300, 2000, dc3, 1.1).astype(np.float64)
	code = np.clip(np.rint(raw * 8), -127, 127).astype(np.int8)
	dt3 = 200.0 + code.astype(np.float64) / 8
	assert np.array_equal(dt3.astype(np.float32).astype(np.float64), dt3)
	namet3 = ['G%04d' % i for i in range(300)]
	genes3 = [namet3[i] for i in rng.permutation(300)[:200]]
	settle('c3', dt3, dc3, namet3, genes3, True, 1e-11, out)
	out['c3_code'], out['c3_dc'] = code, dc3
	# cases 4 and 5: condcov=False on case 1's matrix, 9 genes, fp64 and fp32
	genes4 = [namet1[i] for i in (0, 39, 7, 22, 13, 14, 29, 35, 1)]
	settle('c4', dt1.astype(np.float64), dc1, namet1, genes4, False, 1e-11, out)
	settle('c5', dt1, dc1.astype(np.float32), namet1, genes4, False, 5e-7, out)
	assert out['c5_out'].dtype == np.float32 and out['c4_out'].dtype == np.float64
	assert all(v.dtype != object for v in map(np.asarray, out.values()))
	path = os.path.join(HERE, 'G21_pccovt.npz')
	np.savez_compressed(path, **out)
	print(os.path.basename(path), os.path.getsize(path), 'bytes')
	assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
	main()
