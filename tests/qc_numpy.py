"""Plain-numpy restatements of quality control, the independent check of the device route: qc_reads as masks over a matrix that is never rewritten (what the
kernels of csrc/nrm_qc.hip compute), its statistics alone, and qc_outlier's fitting loop with the distance of the closest cell from the cut."""
import math

import numpy as np


def stats(x, gene_alive, cell_alive):
	"""(gene_total, gene_nnz, cell_total, cell_nnz) over the entries whose gene and cell are alive, int64; 0 at dead indices."""
	x = np.asarray(x).astype(np.int64)
	g, c = np.asarray(gene_alive, dtype=bool), np.asarray(cell_alive, dtype=bool)
	m = x * (g[:, None] & c[None, :])
	return m.sum(axis=1), (m > 0).sum(axis=1), m.sum(axis=0), (m > 0).sum(axis=0)


def thresholds(params, nt, ns):
	n_gene, nc_gene, ncp_gene, n_cell, nt_cell, ntp_cell = params
	return (math.ceil(n_gene), math.ceil(nc_gene), math.ceil(ncp_gene * ns), math.ceil(n_cell), math.ceil(nt_cell), math.ceil(ntp_cell * nt))


def decide(st, thr, gene_alive, cell_alive):
	"""The masks after one decision on the statistics st with the integer thresholds thr."""
	gt, gn, ct, cn = st
	g = gene_alive & (gt >= thr[0]) & (gn >= thr[1]) & (gn >= thr[2])
	c = cell_alive & (ct >= thr[3]) & (cn >= thr[4]) & (cn >= thr[5])
	return g, c


def qc_reads(x, params):
	"""(genes, cells, iterations): the masked loop.  RuntimeError as the reference's when nothing is left, genes first."""
	nt, ns = x.shape
	g, c = np.ones(nt, dtype=bool), np.ones(ns, dtype=bool)
	nt0 = ns0 = it = 0
	while nt0 != nt or ns0 != ns:
		nt0, ns0, it = nt, ns, it + 1
		g, c = decide(stats(x, g, c), thresholds(params, nt, ns), g, c)
		nt, ns = int(g.sum()), int(c.sum())
		if nt == 0:
			raise RuntimeError('All genes removed in QC.')
		if ns == 0:
			raise RuntimeError('All cells removed in QC.')
	return np.flatnonzero(g), np.flatnonzero(c), it


def two_sided_z(q):
	lo, hi = 0.0, 40.0
	for _ in range(200):
		mid = 0.5 * (lo + hi)
		if math.erfc(mid / math.sqrt(2.0)) > q:
			lo = mid
		else:
			hi = mid
	return lo


def qc_outlier(dw, pcut=1E-10, outrate=0.02):
	"""(passing cells, fitting steps, the smallest | |t| / z - 1 | over every cell and step): the loop in z instead of P-values."""
	ns = len(dw)
	z = two_sided_z(pcut / ns)
	lo, hi = int(np.ceil(outrate * ns)), int(np.floor((1 - outrate) * ns))
	part = np.partition(dw, [lo, hi])
	fit = (dw >= part[lo]) & (dw <= part[hi])
	samples, seen, margin = np.ones(ns, dtype=bool), [], np.inf
	while True:
		seen.append(samples)
		mean = dw[fit].mean()
		t = np.abs((dw - mean) / np.sqrt(((dw[fit] - mean)**2).mean()))
		margin = min(margin, float(np.abs(t / z - 1).min()))
		samples = fit = t <= z
		same = sum(np.array_equal(samples, s) for s in seen)
		if same >= 0.1 * len(seen) and same >= 3:
			return samples, len(seen), margin
