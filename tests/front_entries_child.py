"""The child side of tests/test_gpu_front_entries.py: a process in which torch cannot be imported runs lcpm, scaling_factor, compute_var, qc_reads, subset and
the command line on host arrays -- through the library's whole-problem entries (nrm_lcpm_host, nrm_lcpm_csr_host, nrm_compute_var_host, nrm_qc_reads_host,
nrm_qc_reads_csr_host) -- and writes what it got to an .npz and, for the command line, to files in a directory; the parent compares with the golden fixtures.
`python tests/front_entries_child.py OUT.npz WORKDIR`.  The input generators at the top are shared with the parent and with tests/test_front_entries_cpu.py (which
import this module; nothing here touches torch); the frame of the child is cabi_harness.without_torch."""
import os
import sys

import numpy as np

import cabi_harness as h

ROOT = h.ROOT
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NTOT = 1E9  # (what tests/golden/make_g18.py and make_g19.py passed for the ntot_* arrays)
LCPM_TILE, FITVAR_TILE = 32, 32  # nrm_lcpm_row_tile(), nrm_fitvar_row_tile(): the parent asserts both


def small_counts(rows, n, seed, zero_cell=None):
	"""rows x n Poisson counts, gene row 3 (when there is one) all zero, every cell with a read but `zero_cell`."""
	rng = np.random.default_rng(seed)
	mu = np.exp(rng.normal(-0.8, 1.2, rows))
	x = rng.poisson(mu[:, None] * np.exp(rng.normal(0, 0.4, n))[None, :]).astype(np.int32)
	if rows > 3:
		x[3] = 0
	empty = x.sum(axis=0) == 0
	x[0, empty] = 1
	if zero_cell is not None:
		x[:, zero_cell] = 0
	return x


def with_stored_zeros(x, seed):
	"""x as a scipy COO matrix with a stored zero added at thirty places where x is zero (the matrix it stands for is still x)."""
	import scipy.sparse
	rng = np.random.default_rng(seed)
	c = scipy.sparse.coo_matrix(x)
	zr, zc = np.nonzero(x == 0)
	pick = rng.choice(zr.size, 30, replace=False)
	return scipy.sparse.coo_matrix((np.concatenate([c.data, np.zeros(30, dtype=c.data.dtype)]), (np.concatenate([c.row, zr[pick]]), np.concatenate([c.col, zc[pick]]))),
								   shape=x.shape)


def fitvar_small():
	"""2 genes x 5 cells, one covariate."""
	rng = np.random.default_rng(41)
	return rng.normal(size=(2, 5)), rng.normal(size=(1, 5))


WIDE_SEED = 5


def fitvar_wide(seed=WIDE_SEED):
	"""(nrm_fitvar_row_tile() + 1) genes x 1030 cells in fp32, 63 covariates: 61 random rows, a copy of row 7 at row 40 and the ones row (rank 62 of 63)."""
	rng = np.random.default_rng(seed)
	n = 1030
	dc = np.vstack([rng.normal(size=(62, n)), np.ones((1, n))])
	dc[40] = dc[7]
	y = (rng.normal(size=(FITVAR_TILE + 1, n)) * np.exp(0.3 * rng.normal(size=n))[None, :] + 0.5 * dc[0]).astype(np.float32)
	return y, dc


def golden(name):
	return np.load(os.path.join(GOLDEN, name + '.npz'))


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------------------
_raised = lambda f, *a, **ka: h.raised(lambda: f(*a, **ka), 'no error', Exception)


def _debug(value):
	"""NRM_DEBUG for the calls that follow (None: unset)."""
	if value is None:
		os.environ.pop('NRM_DEBUG', None)
	else:
		os.environ['NRM_DEBUG'] = value


def dense_lcpm(out, notes, lcpm, norm):
	g = golden('G18_front')
	reads = g['reads']
	for dt in ('int32', 'int64'):
		x = reads.astype(dt)
		out['d.{}.lcpm'.format(dt)], _, _, out['d.{}.cov'.format(dt)] = lcpm.lcpm(x)
		out['d.{}.nonorm'.format(dt)], _, _, out['d.{}.nonorm_cov'.format(dt)] = lcpm.lcpm(x, normalize=False)
		out['d.{}.ntot'.format(dt)], _, _, out['d.{}.ntot_cov'.format(dt)] = lcpm.lcpm(x, ntot=NTOT)
		r = lcpm.lcpm(x, nocov=True, nth=3, seed=5)
		out['d.{}.nocov'.format(dt)] = r[0]
		notes['d.{}.nocov_cov'.format(dt)] = repr(r[3])
		r = lcpm.lcpm(x, lowmem=False)
		out['d.{}.mean'.format(dt)], out['d.{}.var'.format(dt)] = r[1], r[2]
		out['d.{}.f32'.format(dt)] = lcpm.lcpm(x, out_dtype=np.float32)[0]
		out['d.{}.sf'.format(dt)] = lcpm.scaling_factor(x)
	clipped = np.minimum(reads, 255).astype(np.uint8)
	out['d.uint8.lcpm'], _, _, out['d.uint8.cov'] = lcpm.lcpm(clipped)
	out['d.uint8.sf'] = lcpm.scaling_factor(clipped)
	out['d.sf_other'] = lcpm.scaling_factor(reads, varname='logtpropmean', v0='min')
	notes['device_out'] = _raised(lcpm.lcpm, reads, device_out=True)
	notes['varscale'] = _raised(lcpm.lcpm, reads, varscale=1)
	huge = reads.astype(np.int64)
	huge[0, 0] = 1 << 24
	notes['huge'] = _raised(lcpm.lcpm, huge)
	neg = reads.astype(np.int16)
	neg[5, 7] = -1
	notes['negative'] = _raised(lcpm.lcpm, neg)
	out['d.sf_negative'] = lcpm.scaling_factor(neg)  # (the share of zero entries does not depend on it: lcpm.py:258 does not look either)


def sparse_lcpm(out, notes, lcpm, norm):
	import scipy.sparse
	g = golden('G19_lcpm_sparse')
	for case in ('lo', 'hi'):
		reads = g[case + '_reads']
		_debug('lcpm_sparse=force' if case == 'hi' else None)
		coo = with_stored_zeros(reads, 19)
		notes[case + '.stored_zeros'] = int((coo.data == 0).sum())
		for form, m in (('csr', scipy.sparse.csr_matrix(reads)), ('coo', coo), ('csc', scipy.sparse.csc_matrix(reads))):
			k = 's.{}.{}.'.format(case, form)
			out[k + 'lcpm'], _, _, out[k + 'cov'] = lcpm.lcpm(m)
			out[k + 'nonorm'] = lcpm.lcpm(m, normalize=False)[0]
			out[k + 'ntot'] = lcpm.lcpm(m, ntot=NTOT)[0]
			out[k + 'nocov'] = lcpm.lcpm(m, nocov=True)[0]
			out[k + 'f32'] = lcpm.lcpm(m, out_dtype=np.float32)[0]
			out[k + 'sf'] = lcpm.scaling_factor(m)
		_debug(None)
		out['s.{}.dense.lcpm'.format(case)] = lcpm.lcpm(coo.toarray())[0]
		_debug('lcpm_sparse=0')  # (the scipy matrix densified on the host: the dense entry)
		out['s.{}.densified.lcpm'.format(case)] = lcpm.lcpm(coo)[0]
		_debug(None)
	# a matrix whose columns are out of order inside a row, given to the entry as it is
	indptr, indices, data = lcpm.canonical_csr(scipy.sparse.csr_matrix(g['hi_reads']))
	row = int(np.flatnonzero(np.diff(indptr) >= 2)[0])
	bad = indices.copy()
	bad[indptr[row]], bad[indptr[row] + 1] = indices[indptr[row] + 1], indices[indptr[row]]
	notes['malformed'] = _raised(lcpm._lcpm_host_entry, (indptr, bad, data), g['hi_reads'].shape, otype=np.float64)
	notes['malformed_text'] = lcpm.MALFORMED_CSR


def small_shapes(out, notes, lcpm, norm):
	import scipy.sparse
	one = np.array([[1]], dtype=np.int64)
	out['m.one.lcpm'], _, _, out['m.one.cov'] = lcpm.lcpm(one)
	notes['m.one.sf'] = _raised(lcpm.scaling_factor, one)  # (no zero entry: v1 == v0 = 0, the reference's assertion)
	x = small_counts(LCPM_TILE + 1, 1025, 23)
	out['m.tile.lcpm'], _, _, out['m.tile.cov'] = lcpm.lcpm(x)
	out['m.tile.sf'] = lcpm.scaling_factor(x)
	_debug('lcpm_sparse=force')
	out['m.tile.csr.lcpm'], _, _, out['m.tile.csr.cov'] = lcpm.lcpm(scipy.sparse.csr_matrix(x))
	out['m.tile.csr.sf'] = lcpm.scaling_factor(scipy.sparse.csr_matrix(x))
	z = small_counts(LCPM_TILE + 1, 1025, 23, zero_cell=1024)
	for form, m in (('dense', z), ('csr', scipy.sparse.csr_matrix(z))):
		notes['m.zero.{}.cov'.format(form)] = _raised(lcpm.lcpm, m)
		out['m.zero.{}.nocov'.format(form)] = lcpm.lcpm(m, nocov=True)[0]
	_debug(None)


def fitvar(out, notes, lcpm, norm):
	g, h = golden('G18_front'), golden('G18_front_chain')
	lc, dc = g['lcpm'], h['normcov_c']
	for steps in (1, 3):
		out['f.w{}'.format(steps)] = norm.compute_var(lc, dc, stepmax=steps)
		w, change, taken = norm._compute_var_host_entry(lc, np.ascontiguousarray(dc), steps, 1E-6)
		out['f.w{}.again'.format(steps)] = w
		notes['f.w{}.state'.format(steps)] = [change, taken]
	out['f.w1.f32'] = norm.compute_var(lc.astype(np.float32), dc)
	w, change, taken = norm._compute_var_host_entry(lc, np.ascontiguousarray(dc), 50, 0.5)  # (stops as soon as a step changes the scale by less than a half)
	notes['f.eps.state'] = [change, taken]
	y, c = fitvar_small()
	out['f.small'] = norm.compute_var(y, c, stepmax=2)
	y, c = fitvar_wide()
	out['f.wide'] = norm.compute_var(y, c, stepmax=2)
	flat = lc.copy()
	flat[9] = 0.0  # the covariates (with their ones row) explain a constant row exactly: its residual is constant, its spread zero
	notes['f.constant'] = _raised(norm.compute_var, flat, dc)
	notes['f.64'] = _raised(norm.compute_var, y, np.vstack([c, np.random.default_rng(2).normal(size=(1, c.shape[1]))]))
	notes['f.0'] = _raised(norm.compute_var, y, c[:0])


def qc_reads(out, notes, lcpm, norm):
	import scipy.sparse
	from normalisr_amd import qc
	g = golden('G20_qc')
	for case in 'abc':
		x, p = g[case + '_reads'], g[case + '_params']
		for form, m in (('dense', x), ('csr', scipy.sparse.csr_matrix(x))):
			genes, cells, info = qc.qc_reads(m, *p, return_info=True)
			k = 'q.{}.{}.'.format(case, form)
			out[k + 'genes'], out[k + 'cells'], out[k + 'gene_mask'], out[k + 'cell_mask'] = genes, cells, info['gene_mask'], info['cell_mask']
			notes[k + 'iterations'] = info['iterations']
	x = g['a_reads'].copy()
	notes['q.all_genes'] = _raised(qc.qc_reads, x, 1E9, 0, 0, 1E9, 0, 0)
	notes['q.all_cells'] = _raised(qc.qc_reads, x, 0, 0, 0, 1E9, 0, 0)
	notes['q.bad_param'] = _raised(qc.qc_reads, x, -1, 0, 0, 0, 0, 0)
	x[4, 4] = -3
	notes['q.negative'] = _raised(qc.qc_reads, x, *g['a_params'])
	notes['q.device_out'] = _raised(qc.qc_reads, g['a_reads'], *g['a_params'], device_out=True)
	# subset on the host: the survivors of case b, dense and sparse
	x = g['b_reads']
	out['q.subset'] = qc.subset(x, g['b_genes'], g['b_cells'])
	out['q.subset_csr'] = qc.subset(scipy.sparse.csr_matrix(x), g['b_genes'], g['b_cells']).toarray()
	out['q.subset_f32'] = qc.subset(x.astype(np.float32), g['b_genes'][::-1], None)
	notes['q.subset_order'] = _raised(qc.subset, scipy.sparse.csr_matrix(x), g['b_genes'][::-1], None)
	notes['q.subset_range'] = _raised(qc.subset, x, [x.shape[0]], None)
	out['q.outlier'] = qc.qc_outlier(g['w'])


def command_line(out, notes, work):
	"""qc_reads, subset, lcpm (dense text and -s from a Matrix Market file), normcov, fitvar, qc_outlier through main([...]) in this process; the parent reads the files."""
	import scipy.io
	import scipy.sparse
	from normalisr_amd.__main__ import main
	g, h, q = golden('G18_front'), golden('G18_front_chain'), golden('G20_qc')
	f = lambda name: os.path.join(work, name)
	x, p = q['b_reads'], q['b_params']
	np.savetxt(f('reads.tsv'), x, delimiter='\t', fmt='%i')
	scipy.io.mmwrite(f('reads.mtx'), scipy.sparse.coo_matrix(x))
	np.savetxt(f('w.tsv'), q['w'], delimiter='\t', fmt='%.8G')
	for name, key in (('genes.txt', 'cli_genes_in'), ('cells.txt', 'cli_cells_in'), ('wcells.txt', 'cli_wcells_in')):
		with open(f(name), 'w') as fh:
			fh.write('\n'.join(q[key]))
	flags = ['--gene_read_count', str(int(p[0])), '--gene_cell_count', str(int(p[1])), '--gene_cell_prop', repr(float(p[2])), '--cell_read_count', str(int(p[3])),
			 '--cell_gene_count', str(int(p[4])), '--cell_gene_prop', repr(float(p[5]))]
	main(['qc_reads', f('reads.tsv'), f('genes.txt'), f('cells.txt'), f('genes_out.txt'), f('cells_out.txt')] + flags)
	main(['qc_reads', '-s', f('reads.mtx'), f('genes.txt'), f('cells.txt'), f('genes_s.txt'), f('cells_s.txt')] + flags)
	main(['subset', f('reads.tsv'), f('sub.tsv'), '-r', f('genes.txt'), f('genes_out.txt'), '-c', f('cells.txt'), f('cells_out.txt')])
	main(['subset', '-s', f('reads.mtx'), f('sub_s.tsv'), '-r', f('genes.txt'), f('genes_out.txt'), '-c', f('cells.txt'), f('cells_out.txt')])
	main(['qc_outlier', f('w.tsv'), f('wcells.txt'), f('wcells_out.txt')])
	np.savetxt(f('g18.tsv'), g['reads'], fmt='%i', delimiter='\t')
	scipy.io.mmwrite(f('g18.mtx'), scipy.sparse.coo_matrix(g['reads']))
	np.savetxt(f('batch.tsv'), h['cov_raw'][:4], fmt='%.8G', delimiter='\t')
	main(['lcpm', '-c', f('batch.tsv'), '--var_out', f('var.tsv'), f('g18.tsv'), f('lcpm.tsv'), f('scale.tsv'), f('cov.tsv')])
	_debug('lcpm_sparse=force')
	main(['lcpm', '-s', f('g18.mtx'), f('lcpm_s.tsv'), f('scale_s.tsv'), f('cov_s.tsv')])
	_debug(None)
	main(['normcov', f('cov.tsv'), f('ncov.tsv')])
	main(['fitvar', f('lcpm.tsv'), f('ncov.tsv'), f('w1.tsv')])


def main(argv):
	dst, work = argv[1:3]

	def run(out):
		os.environ.pop('NRM_HOST_ENTRY', None)
		import normalisr_amd.lcpm as lcpm
		import normalisr_amd.norm as norm
		import normalisr_amd.qc  # noqa: F401
		import normalisr_amd.run  # noqa: F401
		notes = {}
		for part in (dense_lcpm, sparse_lcpm, small_shapes, fitvar, qc_reads):
			part(out, notes, lcpm, norm)
		command_line(out, notes, work)
		return notes
	h.without_torch(dst, run)


if __name__ == '__main__':
	main(sys.argv)
