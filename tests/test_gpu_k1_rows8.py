"""GPU: k_residualize_v8 (csrc/nrm_residualize.hip) -- eight rows per workgroup, the covariate slices of every 1024-cell step staged in LDS -- writes
bit for bit what k_residualize_v4 writes.  Every case is run twice through the same direct call (tests/test_gpu_k1_stages.py run_k1: pattern-filled
outputs with guards, so padding and pitch gaps are compared too): as routed, with NRM_DEBUG="k1_rows8=1" -- the launcher reads it at every launch and then
runs the new kernel wherever it can, also on rows shorter than the 16 384 cells from which it is the default -- and with "k1_rows8=0", which keeps the old
kernel; every output buffer is compared as bytes.  CASES is shared with tests/test_k1_rows8_route_cpu.py, which asserts from the launcher's own conditions
which of them reach the new kernel, forced and by default."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import k1_longdouble as k1

ROWS = (5, 8, 9, 12, 129)
CELLS = (16, 1020, 1024, 1028, 2050, 4100)  # one short slice; ragged last slices; n % 4 != 0 (2050: a scalar tail); a tail that opens a slice of its own (1028, 4100)
NCS = (1, 3, 4, 5, 8)
NSS = (0, 5, 6)


def _grid():
	"""Every cell count with every covariate count; rows, row type, slices and the caller's maxima cycle so that each value meets each cell count and each
	covariate count at least once.  rows_pad: a multiple of 128 with digit planes; without, the rows rounded up to 4 (the old kernel's unit: 12 and 132 rows
	keep the old kernel) or to 8."""
	out, i = [], 0
	for n in CELLS:
		for nc in NCS:
			rows, ns = ROWS[i % 5], NSS[(i // 5 + i) % 3]
			out.append(dict(rows=rows, n=n, nc=nc, dtype='float32' if (i + i // 5) % 2 == 0 else 'float64', ns=ns, cmax=i % 3 != 1,
							rows_pad=None if ns else k1.round_up(rows, 8 if i % 4 else 4), chunks=0, block=None, special=None))
			i += 1
	return out


def _special():
	base = dict(rows=8, n=2050, nc=3, dtype='float32', ns=6, cmax=True, rows_pad=None, chunks=0, block=None, special=None)
	return [
		dict(base, special=('copy', 1)),  # a row of group 0 is a copy of a covariate: group 0 sweeps for its maxima, group 1 accepts its bound
		dict(base, special=('copy', 6), dtype='float64', ns=5),  # the other way round
		dict(base, rows=129, block=(128, 512)),  # the rows are a block of a larger quantised matrix: plane pitch above the block
		dict(base, rows=12, nc=5, ns=5, block=(256, 384), dtype='float64'),
		dict(base, chunks=2),  # two cell chunks, the last one ragged (65 k-steps as 33 + 32)
		dict(base, rows=9, nc=8, chunks=2, cmax=False, dtype='float64'),
		dict(base, rows=129, n=4100, nc=4, ns=0, rows_pad=136),  # NS = 0 on 17 workgroups, the last with seven padding rows
		dict(base, rows=5, n=1028, nc=1, ns=0, rows_pad=16, dtype='float64'),  # a workgroup of padding rows only
		dict(base, rows=9, n=16390, nc=3),  # rows long enough for the new kernel to be the launcher's own choice
	]


CASES = _grid() + _special()


def case_id(c):
	return '%dx%d-nc%d-%s-ns%d%s%s%s%s' % (c['rows'], c['n'], c['nc'], c['dtype'][-2:], c['ns'], '' if c['cmax'] else '-nocmax',
										   '-pad%d' % c['rows_pad'] if c['rows_pad'] else '', '-chunks' if c['chunks'] else '', '-block' if c['block'] else '') + \
		('-copy%d' % c['special'][1] if c['special'] else '')


def rows_pad_of(c):
	"""The rows_pad the call is made with (run_k1's default when the case names none)."""
	return c['rows_pad'] if c['rows_pad'] is not None else k1.round_up(max(c['rows'], 1), 128 if c['ns'] else 4)


def inputs(c):
	rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(c))))  # (a seed of the case's name, the same in every process)
	rows, n, nc = c['rows'], c['n'], c['nc']
	C = rng.normal(size=(nc, n)) * rng.uniform(0.5, 4, (nc, 1))
	C[-1] = 1.0 if nc > 1 else C[-1]
	x = rng.normal(size=(rows, n)) * np.exp(rng.normal(size=(rows, 1))) + 3.0 + 0.5 * C[0]
	if c['special']:
		x[c['special'][1]] = 2.5 * C[0]
	x = x.astype(c['dtype'])
	C64, dci, rank = k1.prepare(C)
	return x, C64, dci, rank


@contextmanager
def rows8_switch(mode):
	"""NRM_DEBUG k1_rows8=0 for the old kernel, =1 for the new one wherever it can run, None for the launcher's choice; other keys are kept."""
	old = os.environ.get('NRM_DEBUG')
	keep = [p for p in (old or '').split(',') if p.strip() and not p.strip().lower().startswith('k1_rows8=')]
	os.environ['NRM_DEBUG'] = ','.join(keep + ([] if mode is None else ['k1_rows8=%d' % mode]))
	try:
		yield
	finally:
		if old is None:
			del os.environ['NRM_DEBUG']
		else:
			os.environ['NRM_DEBUG'] = old


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_k1_rows8_writes_the_bytes_of_the_four_row_kernel(c):
	from test_gpu_k1_stages import run_k1
	x, C64, dci, rank = inputs(c)
	assert rank > 0
	got = {}
	for mode in (None, 1, 0):
		with rows8_switch(mode):
			got[mode] = run_k1(x, C64, dci, rank, c['ns'], rows_pad=c['rows_pad'], keep=not c['chunks'], cmax=c['cmax'], chunks=c['chunks'], block=c['block'])
	names = [k for k, v in got[0].items() if isinstance(v, np.ndarray)]
	assert {'ss'} <= set(names) and (not c['ns'] or {'planes', 'exps', 'fix'} <= set(names)) and (c['chunks'] or {'out', 'coef'} <= set(names))
	for mode in (None, 1):
		for k in names:
			a, b = got[mode][k], got[0][k]
			assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (k, mode, case_id(c))
	# the run did something: sums of squares of the valid rows are finite, the digit planes are not the fill pattern
	assert np.isfinite(got[1]['ss'][:c['rows']]).all()
	if c['ns']:
		assert (got[1]['exps'][:c['rows']] != 0x7f7f7f7f).all()
