"""Command runners and matrix IO behind `normalisr qc_reads | subset | lcpm | normcov | fitvar | qc_outlier | normvar | de | coex | binnet | bh | principal | enrich | pccovt | coex_levels`.

Every sub-command is one row of COMMANDS: which files are read (and how they are shaped), which command-line
options become which keyword arguments, which function runs, and which of its results go to which file.
The file contract is the reference's (run.py:20-35,258-321): tab-delimited text without headers, one row
per line, '%.8G' for floats, '.gz' by suffix (numpy handles it), a single row read back as shape (1, n).
Extension of this build: names ending in '.npy' are read / written as binary numpy arrays; and the text files themselves go
through the library's threaded parser / printer (csrc/nrm_tsv.hip: the same numbers in, byte for byte the same text out) instead of
numpy.loadtxt / numpy.savetxt, which take minutes for a 20k x 100k matrix where the association takes milliseconds (NRM_TSV=numpy: back).
"""
import logging

import numpy as np

from . import _opts

fmt_float = '%.8G'
fmt_int = '%i'


def _is_binary(name):
	return name.endswith('.npy')


def _native_text():
	"""The library's text reader / writer unless NRM_TSV=numpy asks for numpy.loadtxt / numpy.savetxt (the reference's own calls)."""
	import os
	return _opts.debug('tsv', 'native') != 'numpy'


def _open_bytes(f):
	if f.endswith('.gz'):  # '.gz' by suffix, as numpy does for the reference
		import gzip
		with gzip.open(f, 'rb') as fh:
			return np.frombuffer(fh.read(), dtype=np.uint8)
	if f.endswith('.bz2') or f.endswith('.xz'):
		return None
	return np.fromfile(f, dtype=np.uint8)


def parse_text(buf, delimiter='\t', dtype=np.float64):
	"""The matrix in a buffer of text (uint8 array), 2-D, through the library's threaded parser (csrc/nrm_tsv.hip): the numbers
	numpy.loadtxt reads (correctly rounded, as float()), '#' comments and blank lines skipped, ValueError for a field that is not a number
	or a row of another length.  None for a buffer without data (numpy warns and returns an empty array: left to numpy)."""
	import ctypes
	from . import _lib
	lib = _lib.load()
	buf = np.ascontiguousarray(buf, dtype=np.uint8)
	rows, cols = ctypes.c_int64(), ctypes.c_int64()
	_lib.check(lib.nrm_tsv_shape(buf.ctypes.data, buf.size, ord(delimiter), 0, ctypes.addressof(rows), ctypes.addressof(cols)))
	if rows.value == 0:
		return None
	out = np.empty((rows.value, cols.value), dtype=dtype)
	_lib.check(lib.nrm_tsv_parse(buf.ctypes.data, buf.size, ord(delimiter), 0, out.ctypes.data, _lib.NRM_F64 if out.dtype == np.float64 else _lib.NRM_F32,
								 rows.value, cols.value, cols.value))
	return out


def _read_text(f, delimiter, dtype):
	"""numpy.loadtxt(f, delimiter=delimiter) through parse_text."""
	buf = _open_bytes(f)
	if buf is None:
		return None
	try:
		out = parse_text(buf, delimiter, dtype)
	except ValueError:
		return None  # text the library's parser does not take: numpy.loadtxt answers -- its matrix or its exception are the reference's (run.py:20-27)
	return None if out is None else out.squeeze()  # loadtxt's own squeeze (a single row or column comes back 1-D)


def file_read_tsv(f, delimiter='\t', **ka):
	"""Matrix from a TSV (or .npy) file, always 2-D."""
	logging.debug('Start reading file ' + f)
	ans = None
	if _is_binary(f):
		ans = np.load(f, allow_pickle=False)
		if 'dtype' in ka:
			ans = ans.astype(ka['dtype'], copy=False)
	elif _native_text() and len(delimiter) == 1 and set(ka) <= {'dtype'} and np.dtype(ka.get('dtype', np.float64)) in (np.dtype(np.float32), np.dtype(np.float64)):
		ans = _read_text(f, delimiter, np.dtype(ka.get('dtype', np.float64)))
	if ans is None:
		ans = np.loadtxt(f, delimiter=delimiter, **ka)
	logging.debug('Finish reading file ' + f)
	return ans.reshape(1, -1) if ans.ndim < 2 else ans


def _write_text(f, d, delimiter, fmt):
	"""numpy.savetxt(f, d, delimiter=delimiter, fmt=fmt) for the two formats the command line writes ('%.8G' of floats, '%i' of integers),
	printed by the library's threads in blocks of rows; byte for byte the text numpy writes.  False: not a case of ours."""
	import os
	from . import _lib
	d = np.asarray(d)
	if d.ndim == 1:
		d = d.reshape(-1, 1)  # savetxt writes a vector as a column
	if d.ndim != 2 or len(delimiter) != 1 or f.endswith('.bz2') or f.endswith('.xz'):
		return False
	if fmt == fmt_float and d.dtype in (np.float32, np.float64):
		kind, code = 0, _lib.NRM_F64 if d.dtype == np.float64 else _lib.NRM_F32
	elif fmt == fmt_int and d.dtype.kind in 'biu' and d.dtype != np.uint64:
		kind = 1
		if d.dtype.itemsize == 1 and d.dtype.kind in 'bu':
			d, code = d.view(np.uint8), _lib.NRM_TSV_U8
		elif d.dtype == np.int32:
			code = _lib.NRM_TSV_I32
		else:
			d, code = d.astype(np.int64), _lib.NRM_TSV_I64
	else:
		return False
	lib = _lib.load()
	d = np.ascontiguousarray(d)
	rows, cols = d.shape
	width = int(lib.nrm_tsv_width(kind)) * max(cols, 1)
	block = max(1, min(rows, (256 << 20) // width))  # rows per call: at most 256 MB of text at a time
	parts = max(1, min(os.cpu_count() or 1, 64, block))
	cap = -(-block // parts) * width
	text = np.empty(parts * cap, dtype=np.uint8)
	lens = np.zeros(parts, dtype=np.int64)
	if f.endswith('.gz'):
		import gzip
		fh = gzip.open(f, 'wb')
	else:
		fh = open(f, 'wb')
	with fh:
		for r0 in range(0, rows, block):
			r1 = min(rows, r0 + block)
			_lib.check(lib.nrm_tsv_format(d[r0:r1].ctypes.data, code, r1 - r0, cols, cols, ord(delimiter), kind, text.ctypes.data, cap, lens.ctypes.data, parts))
			for t in range(parts):
				if lens[t]:
					fh.write(memoryview(text[t * cap:t * cap + int(lens[t])]))
	return True


def file_write_tsv(f, d, delimiter='\t', fmt=fmt_float, **ka):
	"""Matrix or vector to a TSV (or .npy) file."""
	logging.debug('Start writing file ' + f)
	if _is_binary(f):
		np.save(f, np.asarray(d), allow_pickle=False)
	elif not (_native_text() and not ka and _write_text(f, d, delimiter, fmt)):
		np.savetxt(f, d, delimiter=delimiter, fmt=fmt, **ka)
	logging.debug('Finish writing file ' + f)


_DE_METHODS = {'ignore': 0, 'single': 1, 'covariate': 4}


def _de_method(name):
	if name not in _DE_METHODS:
		raise ValueError('Unknown method {}'.format(name))
	return _DE_METHODS[name]


def _flat_alpha(a):
	return a.reshape(a.shape[0], -1)  # (predictor, gene * covariate), row-major


def _nth(v):
	if int(v) < 0:
		raise ValueError('Parameter nth must be non-negative.')
	return int(v)


def _call_de(m, ka):
	from .de import de
	return de(m['design_in'], m['exp_in'], m['cov_in'], **ka)


def _call_coex(m, ka):
	from .coex import coex
	return coex(m['exp_in'], m['cov_in'], **ka)


def _call_normvar(m, ka):
	from .norm import normvar
	return normvar(m['lcpm_in'], m['cov_in'], m['weights_in'].ravel(), m['scale_in'].ravel(), **ka)


def _call_normcov(m, ka):
	from .norm import normcov
	return (normcov(m['cov_in'], **ka), )


def _call_fitvar(m, ka):
	from .norm import compute_var
	return (compute_var(m['lcpm_in'], m['cov_in']), )


def file_read_coo(f):
	"""Sparse count matrix from a Matrix Market file (.mtx, .mtx.gz), as the reference reads it for `lcpm -s` (run.py:37-43)."""
	try:
		from scipy.io import mmread
	except ImportError:
		raise RuntimeError('normalisr lcpm -s reads Matrix Market files through scipy.io.mmread, and scipy is not installed; convert the matrix to a dense TSV '
						   '(or .npy) file, or install scipy.')
	logging.debug('Start reading file ' + f)
	ans = mmread(f)
	logging.debug('Finish reading file ' + f)
	return ans


def _call_lcpm(m, ka):
	"""lcpm and scaling_factor on one upload of the counts; the covariates of -c come first in cov_out (run.py:153-189)."""
	from .lcpm import lcpm, scaling_factor, _takes_csr
	from .association import _use_host_entry
	d = m['reads_in']
	if _use_host_entry():
		# one call of the library's whole-problem entry per input: lcpm and the zero counts scaling_factor needs, torch not imported
		if not hasattr(d, 'toarray'):
			d = np.asarray(d)
			if d.dtype.kind == 'f':
				d = d.astype(np.int64)  # the reference reads the file with dtype=int (run.py:157-159)
		ans = lcpm(d, _scale=True, **ka)
		sf = ans[4]
	else:
		from .lcpm import DeviceCSR
		from . import engine as _engine
		if hasattr(d, 'toarray') and _takes_csr(d):
			x = DeviceCSR.from_scipy(d)  # (`lcpm -s`: the stored entries only, uploaded once for both calls)
		else:
			if hasattr(d, 'toarray'):
				d = d.toarray()
			d = np.asarray(d)
			if d.dtype.kind == 'f':
				d = d.astype(np.int64)  # the reference reads the file with dtype=int (run.py:157-159)
			eng = _engine.get_engine()
			x = eng.upload(d if d.dtype in (np.int32, np.int64) else d.astype(np.int64))
		ans = lcpm(x, **ka)
		sf = scaling_factor(x)
	cov = ans[3] if m.get('cov_in') is None else np.concatenate([m['cov_in'], ans[3]], axis=0)
	return (ans[0], sf, cov, ans[2])


def _call_binnet(m, ka):
	from .binnet import binnet
	return (binnet(m['pv_in'], ka['qcut'], logp=bool(ka.get('logp'))).astype('u1', copy=False), )


def _call_bh(m, ka):
	"""Benjamini-Hochberg q-values over ALL entries of the matrix (what de's pv_out holds), in its shape; on the device (nrm_bh_host_pk).  --logp: ln P in, ln q out."""
	from .binnet import bh
	return (bh(m['pv_in'], on_device=True, logp=bool(ka.get('logp'))), )


# name -> inputs (matrix arguments), options (argument key -> (keyword, converter)), call, outputs (argument key ->
# (index into the result tuple, transform, format); written when the argument was given)
COMMANDS = {
	'de': dict(inputs=('design_in', 'exp_in', 'cov_in'),
			   options=dict(nth=('nth', int), bs=('bs', int), dimr=('dimreduce', int), method=('single', _de_method), logp=('logp', bool),
							# the reference leaves lowmem=True and then fails writing None: asking for the file asks for alpha
							clfc_out=('lowmem', lambda name: False)),
			   call=_call_de,
			   outputs=dict(pv_out=(0, None, fmt_float), lfc_out=(1, None, fmt_float), clfc_out=(2, _flat_alpha, fmt_float),
							vard_out=(3, None, fmt_float), vart_out=(4, None, fmt_float))),
	'coex': dict(inputs=('exp_in', 'cov_in'), options=dict(nth=('nth', int), bs=('bs', int), dimr=('dimreduce', int), logp=('logp', bool)), call=_call_coex,
				 outputs=dict(pv_out=(0, None, fmt_float), dot_out=(1, None, fmt_float), var_out=(2, None, fmt_float))),
	'normvar': dict(inputs=('lcpm_in', 'cov_in', 'weights_in', 'scale_in'), options=dict(nth=('nth', int), bs=('bs', int)), call=_call_normvar,
					outputs=dict(exp_out=(0, None, fmt_float), cov_out=(1, None, fmt_float))),
	'binnet': dict(inputs=('pv_in', ), options=dict(qcut=('qcut', float), logp=('logp', bool)), call=_call_binnet, outputs=dict(net_out=(0, None, fmt_int))),
	'bh': dict(inputs=('pv_in', ), options=dict(logp=('logp', bool)), call=_call_bh, outputs=dict(q_out=(0, None, fmt_float))),
	# the reference passes var=None to its writer when --var_out is given (lowmem stays True, run.py:175,188-189) and fails: asking for the file asks for lowmem=False
	'lcpm': dict(inputs=('reads_in', 'cov_in'), options=dict(nth=('nth', _nth), rseed=('seed', int), var_out=('lowmem', lambda name: False)), call=_call_lcpm,
				 outputs=dict(lcpm_out=(0, None, fmt_float), cov_out=(2, None, fmt_float), scale_out=(1, None, fmt_float), var_out=(3, None, fmt_float))),
	'normcov': dict(inputs=('cov_in', ), options=dict(no1=('c', lambda no1: not no1)), call=_call_normcov, outputs=dict(cov_out=(0, None, fmt_float))),
	'fitvar': dict(inputs=('lcpm_in', 'cov_in'), options={}, call=_call_fitvar, outputs=dict(weights_out=(0, None, fmt_float))),
}


def run(cmd, args):
	"""Run sub-command `cmd` with the parsed command line `args` (a dict of argparse destinations)."""
	spec = COMMANDS[cmd]
	if cmd in ('de', 'coex', 'binnet', 'bh', 'normvar', 'lcpm', 'normcov', 'fitvar'):
		# files in, files out, one GPU: the library's whole-problem entries (include/normalisr_hip.h) do everything these commands need -- same kernels,
		# same results -- and torch's import (1.0 of a 1.3 s call) is not paid; NRM_HOST_ENTRY=0 keeps the torch engine.  Calls the entries do not
		# cover fall back to it by themselves.
		from . import _lib
		prev = _lib.prefer_host_entry(True)
		try:
			return _run(cmd, spec, args)
		finally:
			_lib.prefer_host_entry(prev)  # (a preference of this call, not of the process: tests and notebooks call run() beside the torch engine)
	return _run(cmd, spec, args)


def _run(cmd, spec, args):
	mats = {}
	for k in spec['inputs']:
		if args.get(k) is None:
			mats[k] = None  # (an optional input: lcpm's -c)
		elif cmd == 'lcpm' and k == 'reads_in' and args.get('sparse'):
			mats[k] = file_read_coo(args[k])
		else:
			mats[k] = file_read_tsv(args[k])
	ka = {}
	for key, (kw, conv) in spec['options'].items():
		if args.get(key) is not None:
			ka[kw] = conv(args[key])
	logging.debug('Start calculation.')
	res = spec['call'](mats, ka)
	logging.debug('Finish calculation.')
	for key, (idx, transform, fmt) in spec['outputs'].items():
		if args.get(key) is not None:
			file_write_tsv(args[key], res[idx] if transform is None else transform(res[idx]), fmt=fmt)


def _runner(cmd):
	def f(args):
		return run(cmd, args)
	f.__name__ = cmd
	f.__doc__ = 'normalisr {} (see COMMANDS)'.format(cmd)
	return f


de, coex, normvar, binnet, bh, lcpm, normcov, fitvar = (_runner(c) for c in ('de', 'coex', 'normvar', 'binnet', 'bh', 'lcpm', 'normcov', 'fitvar'))  # module-level entry points, as in the reference's run module


# ---- quality control: qc_reads, subset, qc_outlier (reference run.py:48-150,220-234) -----------------------------------------------------------------------
# These three read and write name lists beside the matrices, so they are functions of their own, not rows of COMMANDS.  Like run() they prefer the library's
# whole-problem entries (nrm_qc_reads_host, nrm_qc_reads_csr_host; subset and qc_outlier are numpy on the host): torch is not imported unless NRM_HOST_ENTRY=0.

def _prefers_host_entry(f):
	import functools

	@functools.wraps(f)
	def g(args):
		from . import _lib
		prev = _lib.prefer_host_entry(True)
		try:
			return f(args)
		finally:
			_lib.prefer_host_entry(prev)
	return g


def file_read_txtlist(f, **ka):
	"""The names in a text file, one per line, as a numpy array of strings: surrounding blanks stripped, empty lines dropped."""
	logging.debug('Start reading file ' + f)
	with open(f, 'r', **ka) as fh:
		names = [line.strip() for line in fh]
	logging.debug('Finish reading file ' + f)
	return np.array([v for v in names if v])


def file_write_txtlist(f, d, **ka):
	"""Names to a text file, one per line (no line end after the last, as the reference writes it); returns the text."""
	import os
	text = os.linesep.join(d)
	logging.debug('Start writing file ' + f)
	with open(f, 'w', **ka) as fh:
		fh.write(text)
	logging.debug('Finish writing file ' + f)
	return text


def _read_counts(f):
	"""A dense count matrix from a text (or .npy) file as int64: the library's parser where every field holds an integer, numpy.loadtxt(dtype=int) -- the
	reference's call, and its exception -- for anything else."""
	d = file_read_tsv(f)
	if d.dtype.kind in 'iu':
		return d.astype(np.int64, copy=False)
	if np.isfinite(d).all() and (d == np.rint(d)).all() and (np.abs(d) < 2.0**53).all():
		return d.astype(np.int64)
	return file_read_tsv(f, dtype=int)


def _read_sparse_counts(f):
	return file_read_coo(f).astype(int, copy=False)


@_prefers_host_entry
def qc_reads(args):
	"""normalisr qc_reads: the names of the genes and cells that pass (reference run.py:70-97).  With -s the Matrix Market counts are uploaded as CSR and stay
	sparse on the device."""
	from . import qc
	d = _read_sparse_counts(args['reads_in']) if args['sparse'] else _read_counts(args['reads_in'])
	nt, ns = d.shape
	genes = file_read_txtlist(args['genes_in'])
	if len(genes) != nt:
		raise ValueError("Gene count in genes_in doesn't match row count in reads_in.")
	cells = file_read_txtlist(args['cells_in'])
	if len(cells) != ns:
		raise ValueError("Cell count in cells_in doesn't match column count in reads_in.")
	logging.debug('Start calculation.')
	keep = qc.qc_reads(d, args['n_gene'], args['nc_gene'], args['ncp_gene'], args['n_cell'], args['nt_cell'], args['ntp_cell'])
	logging.debug('Finish calculation.')
	file_write_txtlist(args['genes_out'], genes[keep[0]])
	file_write_txtlist(args['cells_out'], cells[keep[1]])


def _name_positions(files, size, what):
	"""The positions, in the list of names before subsetting, of the names after it (reference run.py:114-123: same checks, same message)."""
	before, after = (file_read_txtlist(f) for f in files)
	assert len(before) == size
	assert len(set(before)) == len(before) and len(set(after)) == len(after)
	where = {name: i for i, name in enumerate(before)}
	missing = [name for name in after if name not in where]
	if missing:
		raise ValueError('Subset {} names not found: {}...'.format(what, ','.join(missing[:3])))
	return np.array([where[name] for name in after], dtype=np.int64)


@_prefers_host_entry
def subset(args):
	"""normalisr subset: matrix_in cut down to the named rows and columns (reference run.py:100-150).  A dense matrix goes through the gather kernel, names in any
	order; -s with names in their original order goes through the CSR subset and is densified for the text output, -s with any other order is indexed on the
	host.  --nodummy is applied on the host to the matrix about to be written."""
	from . import qc
	if args['r'] is None and args['c'] is None:
		raise ValueError('Please indicate row (-r) or column (-c) for subsetting.')
	if args['nodummy'] and args['r'] is not None and args['c'] is not None:
		raise ValueError('Only supports nodumy when one of row or column needs subsetting.')
	d = _read_sparse_counts(args['matrix_in']) if args['sparse'] else file_read_tsv(args['matrix_in'])
	rows = None if args['r'] is None else _name_positions(args['r'], d.shape[0], 'row')
	cols = None if args['c'] is None else _name_positions(args['c'], d.shape[1], 'column')
	logging.debug('Start calculation.')
	if not args['sparse']:
		out = qc.subset(d, rows, cols)
	elif all(v is None or (np.diff(v) > 0).all() for v in (rows, cols)):
		out = qc.subset(d, rows, cols).toarray()
	else:
		out = d.tocsr()[slice(None) if rows is None else rows][:, slice(None) if cols is None else cols].toarray()
	if args['nodummy']:
		if rows is not None:
			out = out[:, [len(np.unique(v)) > 1 for v in out.T]]
		else:
			out = out[[len(np.unique(v)) > 1 for v in out]]
	logging.debug('Finish calculation.')
	if 0 in out.shape:
		raise RuntimeError('Empty matrix after subsetting, maybe because nodummy option.')
	file_write_tsv(args['matrix_out'], out, fmt=fmt_int if np.issubdtype(out.dtype, np.integer) else fmt_float)


@_prefers_host_entry
def qc_outlier(args):
	"""normalisr qc_outlier: the names of the cells whose fitted weight is no outlier (reference run.py:220-234)."""
	from . import qc
	w = file_read_tsv(args['weights_in']).ravel()
	cells = file_read_txtlist(args['cells_in'])
	if len(cells) != len(w):
		raise ValueError("Cell count in cells_in doesn't match entry count in weights_in.")
	logging.debug('Start calculation.')
	keep = qc.qc_outlier(w, outrate=args['outrate'], pcut=args['pcut'])
	logging.debug('Finish calculation.')
	file_write_txtlist(args['cells_out'], cells[keep])


# ---- the covariate of a pathway's top principal component: principal, pccovt (the numerical parts of reference run.py:324-354) ---------------------------------
# The reference's gocovt runs gotop (selection + GO enrichment) and pccovt in one command; its enrichment (goatools and a web service) is not part of this build, so
# the two parts are commands of their own and the list of genes between them is a file.  `enrich` (below) writes that file from local gene-set files.

def principal(args):
	"""normalisr principal: the names of the principal genes of a binary network (what the reference's gocovt writes to --master_out)."""
	from . import gocovt
	net = file_read_tsv(args['net_in'], dtype='u1')
	genes = file_read_txtlist(args['genes_in'])
	if net.shape != (len(genes), len(genes)):
		raise ValueError('Wrong shape for net or namet.')
	logging.debug('Start calculation.')
	keep = gocovt.principal_genes(net, n=args['n'])
	logging.debug('Finish calculation.')
	file_write_txtlist(args['master_out'], genes[keep])


def pccovt(args):
	"""normalisr pccovt: cov_in with the top principal component of the genes named in pathway_in as its last row."""
	from . import gocovt
	dt = file_read_tsv(args['exp_in'])
	dc = file_read_tsv(args['cov_in'])
	namet = file_read_txtlist(args['genes_in'])
	pathway = file_read_txtlist(args['pathway_in'])
	logging.debug('Start calculation.')
	out = gocovt.pccovt(dt, dc, namet, pathway, condcov=not args['nocond'])
	logging.debug('Finish calculation.')
	file_write_tsv(args['cov_out'], out)


def enrich(args):
	"""normalisr enrich: the principal genes of a binary network, their enrichment in gene sets read from local files with every gene of genes_in as the
	background, and the genes of the top set written for `normalisr pccovt`.  Files in, files out: through the library's whole-problem entry (nrm_enrich_host),
	torch not imported; the degrees of the network, already on the host, are summed there."""
	from . import _lib, gocovt
	from . import enrich as _enrich
	net = file_read_tsv(args['net_in'], dtype='u1')
	genes = file_read_txtlist(args['genes_in'])
	if net.shape != (len(genes), len(genes)):
		raise ValueError('Wrong shape for net or namet.')
	gocovt._check_principal_args(net.shape, args['n'])
	if args.get('gmt') is not None:
		sets = _enrich.read_gmt(args['gmt'])
	else:
		sets = _enrich.read_go(args['go'][0], args['go'][1], key=args.get('key') or 'id')
	logging.debug('Start calculation.')
	sel = gocovt._select_principal((net != 0).sum(axis=1), args['n'])
	prev = _lib.prefer_host_entry(True)
	try:
		res = _enrich.enrich(sel, sets, namet=genes, nmin=args['nmin'])
	finally:
		_lib.prefer_host_entry(prev)
	logging.debug('Finish calculation.')
	if args.get('master_out') is not None:
		file_write_txtlist(args['master_out'], genes[sel])
	if args.get('goe_out') is not None:
		with open(args['goe_out'], 'w') as fh:
			fh.write('\t'.join(_enrich.COLUMNS) + '\n')
			for row in res.table(0):
				fh.write('\t'.join(fmt_float % v if isinstance(v, float) else str(v) for v in row) + '\n')
	top = res.top_sets(0)  # (ValueError when no set qualifies: the table above is written first, to see why)
	if args.get('go_out') is not None:
		file_write_txtlist(args['go_out'], [top])
	file_write_txtlist(args['pathway_out'], [str(x) for x in res.genes(int(res.top[0]))])



def _write_goe(f, res):
	with open(f, 'w') as fh:
		from . import enrich as _enrich
		fh.write('\t'.join(_enrich.COLUMNS) + '\n')
		for row in res.table(0):
			fh.write('\t'.join(fmt_float % v if isinstance(v, float) else str(v) for v in row) + '\n')


def coex_levels(args):
	"""normalisr coex_levels: the loop of the reference's co-expression example (cmd_coex.sh:37-46) in one process, the problem resident on the device
	(normalisr_amd.levels).  Per level k it writes, under out_dir and with the example's names, lv{k}_net, lv{k}_master.txt, lv{k}_go.txt, lv{k}_pathway.txt, lv{k}_goe.tsv
	and lv{k+1}_cov, on request lv{k}_pv, lv{k}_dot and lv{k}_var; matrices carry --ext.  A level is written as soon as it completes; a level whose step fails
	leaves what it had produced and the command raises what the step raised."""
	import os
	from . import enrich as _enrich
	from . import levels as _levels
	dt = file_read_tsv(args['exp_in'])
	dc = file_read_tsv(args['cov_in'])
	genes = file_read_txtlist(args['genes_in'])
	if args.get('gmt') is not None:
		sets = _enrich.read_gmt(args['gmt'])
	else:
		sets = _enrich.read_go(args['go'][0], args['go'][1], key=args.get('key') or 'id')
	ext = args.get('ext') or '.tsv'
	keep = ('net', ) + tuple(k for k, flag in (('p', 'pv'), ('dot', 'dot'), ('var', 'var')) if args.get(flag))
	ka = {} if args.get('dimr') is None else dict(dimreduce=int(args['dimr']))
	out = lambda name: os.path.join(args['out_dir'], name)
	logging.debug('Start calculation.')
	it = _levels._iter_levels(dt, dc, genes, sets, float(args['qcut']), args['lvmax'], args['n'], args['nmin'], ka.get('dimreduce', 0), True, keep, False)
	for rec in it:  # (the arguments are checked before the first record: nothing is written for a call that fails them)
		os.makedirs(args['out_dir'], exist_ok=True)
		lv = 'lv{}_'.format(rec['level'])
		for key, name in (('p', 'pv'), ('dot', 'dot'), ('var', 'var')):
			if key in rec:
				file_write_tsv(out(lv + name + ext), rec[key])
		if 'net' in rec:
			file_write_tsv(out(lv + 'net' + ext), rec['net'].astype('u1', copy=False), fmt=fmt_int)
		if 'principals' in rec:
			file_write_txtlist(out(lv + 'master.txt'), rec['principals'])
			_write_goe(out(lv + 'goe.tsv'), rec['result'])
			file_write_txtlist(out(lv + 'go.txt'), [rec['top']])
			file_write_txtlist(out(lv + 'pathway.txt'), rec['genes'])
		if 'cov_next' in rec:
			file_write_tsv(out('lv{}_cov'.format(rec['level'] + 1) + ext), rec['cov_next'])
		if 'error' in rec:
			raise rec['error']
	logging.debug('Finish calculation.')


assert __name__ != "__main__"
