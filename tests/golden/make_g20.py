#!/usr/bin/env python3
"""Generate tests/golden/G20_qc.npz by IMPORTING the reference (dev container only, like make_g19.py):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_g20.py

Quality control: qc_reads on three seeded count matrices (Poisson of gene mean x cell depth, gene means exp(N(mean, sd)), depths exp(N(0, 0.9))) that take
4, 3 and 2 iterations -- a fixture that converges in one pass would not test the masks --, qc_outlier on 4000 log-normal weights with 25 planted outliers at
two cutoffs, and the files the reference's command line writes for qc_reads, subset and qc_outlier on case b.  Arrays and name lists only: the counts, the
parameters and what the reference returned for them.  One file, below 1 MB.
"""
import os
import sys
import tempfile
import warnings

import numpy as np

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference/src')
sys.path.insert(0, os.path.dirname(HERE))

import normalisr.qc as refqc  # noqa: E402
import normalisr.run as refrun  # noqa: E402
import qc_numpy  # noqa: E402

CASES = dict(  # genes, cells, mean and sd of the log gene means, the six thresholds, what the reference gives: iterations, genes kept, cells kept
	a=(300, 517, -2.0, 1.6, (50, 12, 0.02, 60, 25, 0.08), (4, 185, 374)),
	b=(97, 1030, -1.5, 1.4, (40, 20, 0.05, 30, 10, 0.15), (3, 86, 682)),
	c=(300, 517, -2.0, 1.6, (0, 0, 0.03, 0, 0, 0.1), (2, 256, 463)),
)


def counts(rng, ng, n, mean, sd):
	mu = np.exp(rng.normal(mean, sd, ng))
	depth = np.exp(rng.normal(0.0, 0.9, n))
	return rng.poisson(mu[:, None] * depth[None, :]).astype(np.int64)


def main():
	import logging
	logging.disable(logging.WARNING)
	rng = np.random.default_rng(20)
	out = {}
	for name, (ng, n, mean, sd, params, want) in CASES.items():
		x = counts(rng, ng, n, mean, sd)
		genes, cells = refqc.qc_reads(x, *params)
		g2, c2, it = qc_numpy.qc_reads(x, params)
		assert np.array_equal(genes, g2) and np.array_equal(cells, c2)
		assert (it, len(genes), len(cells)) == want, (name, it, len(genes), len(cells))
		assert x.max() < 2**31
		out.update({name + '_reads': x.astype(np.int32), name + '_params': np.array(params, dtype=np.float64), name + '_genes': genes.astype(np.int64),
					name + '_cells': cells.astype(np.int64), name + '_iterations': it})
		print(name, x.shape, 'zeros %.2f' % (x == 0).mean(), 'max', x.max(), 'iterations', it, 'genes', len(genes), 'cells', len(cells))
	# qc_outlier
	rng = np.random.default_rng(21)
	n = 4000
	w = np.exp(rng.normal(0, 0.12, n))
	w[rng.choice(n, 25, replace=False)] *= rng.choice([0.2, 3.5], 25)
	out['w'] = w
	for key, pcut in (('w_pass_1e10', 1e-10), ('w_pass_1e3', 1e-3)):
		ref = refqc.qc_outlier(w, pcut=pcut)
		mine, steps, margin = qc_numpy.qc_outlier(w, pcut)
		assert np.array_equal(ref, mine) and margin > 1e-6, (pcut, margin)
		out[key] = ref
		print('qc_outlier pcut', pcut, 'removed', (~ref).sum(), 'steps', steps, 'closest |t| / z - 1: %.3g' % margin)
	# the command line on case b
	x = out['b_reads']
	gn = np.array(['G%04d' % i for i in range(x.shape[0])])
	cn = np.array(['C%05d' % i for i in range(x.shape[1])])
	wn = np.array(['W%04d' % i for i in range(n)])
	p = [float(v) for v in out['b_params']]
	with tempfile.TemporaryDirectory() as tmp:
		f = lambda name: os.path.join(tmp, name)
		np.savetxt(f('reads.tsv'), x, delimiter='\t', fmt='%i')
		np.savetxt(f('w.tsv'), w, delimiter='\t', fmt='%.8G')
		for name, names in (('genes.txt', gn), ('cells.txt', cn), ('wcells.txt', wn)):
			with open(f(name), 'w') as fh:
				fh.write('\n'.join(names))
		refrun.qc_reads(dict(reads_in=f('reads.tsv'), genes_in=f('genes.txt'), cells_in=f('cells.txt'), genes_out=f('genes_out.txt'), cells_out=f('cells_out.txt'),
							 n_gene=int(p[0]), nc_gene=int(p[1]), ncp_gene=p[2], n_cell=int(p[3]), nt_cell=int(p[4]), ntp_cell=p[5], sparse=False))
		refrun.subset(dict(matrix_in=f('reads.tsv'), matrix_out=f('sub.tsv'), r=[f('genes.txt'), f('genes_out.txt')], c=[f('cells.txt'), f('cells_out.txt')],
						   nodummy=False, sparse=False))
		refrun.qc_outlier(dict(weights_in=f('w.tsv'), cells_in=f('wcells.txt'), cells_out=f('wcells_out.txt'), pcut=1e-10, outrate=0.02))
		read = lambda name: np.array([v.strip() for v in open(f(name)) if v.strip()])
		out.update(cli_genes_in=gn, cli_cells_in=cn, cli_wcells_in=wn, cli_genes_out=read('genes_out.txt'), cli_cells_out=read('cells_out.txt'),
				   cli_subset=np.loadtxt(f('sub.tsv'), delimiter='\t', ndmin=2).astype(np.int32), cli_wcells_out=read('wcells_out.txt'))
	assert np.array_equal(out['cli_genes_out'], gn[out['b_genes']]) and np.array_equal(out['cli_cells_out'], cn[out['b_cells']])
	assert np.array_equal(out['cli_subset'], x[out['b_genes']][:, out['b_cells']])
	# (the weights went through '%.8G' text: the outliers are the same cells)
	assert np.array_equal(out['cli_wcells_out'], wn[out['w_pass_1e10']])
	assert all(v.dtype != object for v in map(np.asarray, out.values()))
	path = os.path.join(HERE, 'G20_qc.npz')
	np.savez_compressed(path, **out)
	print(os.path.basename(path), os.path.getsize(path), 'bytes')
	assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
	main()
