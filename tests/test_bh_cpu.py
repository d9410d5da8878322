"""bh without a device: the numpy restatement of the device algorithm (tests/bh_numpy.py) equals the reference's steps (oracle.bh, binnet.py:77-131) and the
package's host bh in bytes, for every case of the generator the GPU tests use and for the reference-held golden vectors; the new Python branch checks its
arguments before it reaches a device; the library exports the entries and the command line knows the sub-command."""
import ctypes

import numpy as np
import pytest

import bh_numpy
import oracle
from normalisr_amd import _lib
from normalisr_amd import binnet as nb

TILE = 4096  # nrm_bh_tile() of this build (asserted below): the generator's sizes are laid around it


def same_bytes(a, b):
	a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
	return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_tile_is_the_one_the_cases_are_laid_around():
	assert int(_lib.load().nrm_bh_tile()) == TILE


@pytest.mark.parametrize('dtype', bh_numpy.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', bh_numpy.sizes(TILE))
def test_restatement_equals_reference_and_host_bh(n, dtype):
	for name, pv in bh_numpy.cases(n, dtype, TILE).items():
		assert pv.dtype == dtype and pv.shape == (n, ) and np.isfinite(pv).all() and pv.min() >= 0 and pv.max() <= 1, name
		st = bh_numpy.stages(pv)
		ref = oracle.bh(pv)
		assert same_bytes(st['out'], ref), (name, n)
		assert same_bytes(nb.bh(pv), ref), (name, n)
		assert same_bytes(nb.bh(pv, on_device=False), ref), (name, n)
		# the stages are what they are called: c counts entries <= u, q is monotone over the sorted keys
		assert np.array_equal(st['sorted'], np.sort(bh_numpy.keys(pv))) and st['c'][-1] == n
		assert (np.diff(st['q'].astype(np.float64)) >= 0).all()


def test_restatement_on_golden_vectors(golden):
	g = golden('G8_binnet')
	assert same_bytes(bh_numpy.bh(g['bh_in']), g['bh_out'])
	assert same_bytes(nb.bh(g['bh_in']), g['bh_out'])
	p32 = g['bh_in'].astype(np.float32)
	assert same_bytes(bh_numpy.bh(p32), oracle.bh(p32))


def test_tie_families_lie_where_they_claim():
	for dtype in bh_numpy.DTYPES:
		c = bh_numpy.cases(3 * TILE + 17, dtype, TILE)
		for name, (lo, hi) in (('tie_across_tiles', (TILE - 1, TILE + 2)), ('tie_whole_tiles', (TILE - 5, 3 * TILE + 3))):
			s = np.sort(c[name])
			assert (s[lo:hi] == s[lo]).all() and s[lo - 1] < s[lo] < s[hi] and np.unique(s).size == s.size - (hi - lo) + 1
		for b in range(np.dtype(dtype).itemsize):
			k = bh_numpy.keys(c['byte{}'.format(b)])
			mask = ~(bh_numpy.KEY[np.dtype(dtype)](0xff) << bh_numpy.KEY[np.dtype(dtype)](8 * b))
			assert np.unique(k & mask).size == 1 and np.unique(k).size > 32


def test_bh_python_branch_checks_arguments_without_a_device():
	p = np.array([0.1, 0.2, 0.2, 0.9])
	w = np.array([1., 2., 1., 1.])
	# weights always run the host code, whatever on_device says
	assert same_bytes(nb.bh(p, weight=w, on_device=True), oracle.bh(p, weight=w))
	# dtypes the device does not take run the host code and raise what it raises
	assert same_bytes(nb.bh(p.astype(np.float16), on_device=True), nb.bh(p.astype(np.float16)))
	with pytest.raises(TypeError):
		nb.bh(np.array([0, 1, 1]), on_device=True)
	with pytest.raises(AssertionError):
		nb.bh(np.zeros((2, 2)))  # the host path keeps the reference's 1-D assertion
	with pytest.raises(AssertionError):
		nb.bh(np.array([0.5, np.nan]))
	with pytest.raises(AssertionError):
		nb.bh(np.zeros(0), on_device=True)
	with pytest.raises(AssertionError):
		nb.bh(np.zeros((2, 2, 2)), on_device=True)


def test_bh_entries_check_arguments_before_the_device():
	lib = _lib.load()
	assert lib.nrm_bh_workspace_bytes(0, _lib.NRM_F64) == _lib.NRM_E_ARG
	assert lib.nrm_bh_workspace_bytes(1 << 31, _lib.NRM_F64) == _lib.NRM_E_UNSUPPORTED
	assert lib.nrm_bh_workspace_bytes(10, 7) == _lib.NRM_E_ARG
	small, large = lib.nrm_bh_workspace_bytes(1, _lib.NRM_F32), lib.nrm_bh_workspace_bytes((1 << 31) - 1, _lib.NRM_F64)
	assert 0 < small < (1 << 16) and 3 * 8 * ((1 << 31) - 1) < large < 4 * 8 * (1 << 31)
	off = (ctypes.c_int64 * 4)()
	for code, ksz in ((_lib.NRM_F32, 4), (_lib.NRM_F64, 8)):
		n = 3 * TILE + 17
		assert lib.nrm_bh_layout(n, code, off) == 0
		o = list(off)
		assert o[0] == 0 and o[3] == 0 and o[1] >= n * ksz and o[2] >= o[1] + n * ksz and o[2] + n * ksz <= lib.nrm_bh_workspace_bytes(n, code)
		assert all(v % 256 == 0 for v in o)
	assert lib.nrm_bh_layout(0, _lib.NRM_F64, off) == _lib.NRM_E_ARG
	fl = (ctypes.c_int32 * 2)()
	buf = ctypes.create_string_buffer(64)
	for args, rc in (((None, _lib.NRM_F64, 1, 8, 8, None, 8, None, 0, None, None), _lib.NRM_E_ARG),  # null pointers
					 ((1, _lib.NRM_F64, 0, 8, 8, 1, 8, 1, 0, 1, None), _lib.NRM_E_ARG),  # no entries
					 ((1, _lib.NRM_F64, 1 << 16, 1 << 16, 1 << 16, 1, 1 << 16, 1, 0, 1, None), _lib.NRM_E_UNSUPPORTED),  # 2^32 entries
					 ((1, _lib.NRM_F64, 2, 8, 4, 1, 8, 1, 0, 1, None), _lib.NRM_E_ARG)):  # a pitch below the row length
		assert lib.nrm_bh(*args) == rc, args
	with pytest.raises(ValueError):
		_lib.check(lib.nrm_bh(ctypes.addressof(buf), _lib.NRM_F64, 1, 4, 4, ctypes.addressof(buf), 4, ctypes.addressof(buf), 0, ctypes.addressof(fl), None))  # alignment / workspace size


def test_cli_knows_bh():
	from normalisr_amd.__main__ import build_parser
	from normalisr_amd import run
	a = vars(build_parser().parse_args(['bh', 'p.tsv', 'q.tsv']))
	assert a['cmd'] == 'bh' and a['pv_in'] == 'p.tsv' and a['q_out'] == 'q.tsv'
	assert callable(run.bh) and run.COMMANDS['bh']['inputs'] == ('pv_in', )
