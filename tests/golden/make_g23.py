#!/usr/bin/env python3
"""Generate tests/golden/G23_coex_levels.npz by IMPORTING the reference (dev container only, like make_g22.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g23.py

The two problems of tests/golden/g23_inputs.py (A 48 genes x 700 cells, B 24 genes x 30 000 cells): per cumulative covariate set -- the 8 normcov rows, then one
appended row after the other -- the reference's coex (p, dot, var) on the fp32 expression upcast to fp64.  The script asserts that the reference's normcov
returns the covariates of g23_inputs, that the ranks by the reference's inv_rank are 7, 8, 9, 9, 10, and that the restatement of tests/levels_numpy.py, updating
level by level, agrees with the reference to 1e-9 on P; it prints the worst values.  Problem A's inputs are stored; B's (2.9 MB of expression alone) are rebuilt from
their seed by the tests and held to the check sums stored here.  Arrays only; one file, below 1 MB.
"""
import os
import sys
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import normalisr.norm as refnorm  # noqa: E402
from normalisr.association import inv_rank as ref_inv_rank  # noqa: E402
from normalisr.coex import coex as ref_coex  # noqa: E402
import levels_numpy as ln  # noqa: E402
from g23_inputs import RANKS, checksum, g23_inputs  # noqa: E402


def rel_p(p, want):
	"""(largest relative error where the reference's P >= 1e-290 off the diagonal, largest P elsewhere off the diagonal)."""
	off = ~np.eye(len(p), dtype=bool)
	big = off & (want >= 1e-290)
	small = off & ~big
	return float((np.abs(p[big] - want[big]) / want[big]).max()) if big.any() else 0.0, float(p[small].max()) if small.any() else 0.0


def case(name, out):
	dt32, dc, rows, raw = g23_inputs(name)
	assert np.array_equal(refnorm.normcov(raw), dc), name
	dt = dt32.astype(np.float64)
	lv = ln.Levels(dt, dc)
	worst = dict(p=0.0, small=0.0, dot=0.0, var=0.0)
	for k in range(5):
		cov = np.concatenate([dc, rows[:k]])
		rank = ref_inv_rank(np.matmul(cov, cov.T))[1]
		assert rank == RANKS[k], (name, k, rank)
		p, dot, var = ref_coex(dt, cov)
		if k:
			lv.append(rows[k - 1])
			assert not lv.rebuilt[-1], (name, k, lv.info)
		assert lv.rank == rank
		mp, mdot, mvar = lv.results()
		ep, small = rel_p(mp, p)
		worst['p'], worst['small'] = max(worst['p'], ep), max(worst['small'], small)
		worst['dot'] = max(worst['dot'], float(np.abs(mdot - dot).max() / np.abs(dot).max()))
		worst['var'] = max(worst['var'], float(np.abs(mvar - var).max() / np.abs(var).max()))
		for key, v in (('p', p), ('dot', dot), ('var', var)):
			out['{}_{}{}'.format(name, key, k)] = v
	print('{}: {} genes x {} cells; restatement (updates, fp64) against the reference: P {:.3g} relative, P below 1e-290 at most {:.3g}, dot {:.3g}, var {:.3g} of the '
		  'largest entry; gene 1 keeps {:.4f} of its variance, gene 2 mean / spread {:.0f}'.format(
			  name, dt.shape[0], dt.shape[1], worst['p'], worst['small'], worst['dot'], worst['var'], out[name + '_var2'][1] / out[name + '_var1'][1],
			  dt[2].mean() / dt[2].std()))
	assert worst['p'] < 1e-9 and worst['small'] < 1e-289 and worst['dot'] < 1e-10 and worst['var'] < 1e-10
	assert 0.005 < out[name + '_var2'][1] / out[name + '_var1'][1] < 0.02
	for key, v in (('dt', dt32), ('dc', dc), ('rows', rows)):
		out['{}_sum_{}'.format(name, key)] = checksum(v)
		if name == 'A':
			out['{}_{}'.format(name, key)] = v


def main():
	import logging
	logging.disable(logging.WARNING)
	out = {}
	for name in ('A', 'B'):
		case(name, out)
	path = os.path.join(HERE, 'G23_coex_levels.npz')
	np.savez_compressed(path, **out)
	print(os.path.basename(path), os.path.getsize(path), 'bytes')
	assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
	main()
