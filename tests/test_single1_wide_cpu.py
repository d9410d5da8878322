"""CPU: nrm_single1_group_info_wide_host -- the routine k_s1_group_info_wide runs with a wave per grouping (csrc/nrm_single1.hip: s1_group_info_wide_one), here
with one lane on host arrays -- against the longdouble reference s1_reference.group_info on the shared cells' matrix as gram_from_parts adds it up, for 9 .. 32
covariates: ns, the rank (through dof) and the counters exactly, vx, ccx and M+ within judge_group_info's bounds, the plan columns bit for bit
nrm_pvalue_plan_fill_many at the same dof.  The Gram blocks of the problems only add up to the matrix, over every block pair and every partial sum."""
import ctypes

import numpy as np
import pytest

import s1_reference as s1
import s1_wide as sw
from normalisr_amd import _lib

F64 = np.float64


def plans(dof):
	d = np.ascontiguousarray(dof, dtype=F64)
	out = np.zeros((len(d), s1.HEAD - 2))
	_lib.check(_lib.load().nrm_pvalue_plan_fill_many(d.ctypes.data_as(ctypes.c_void_p), len(d), out.ctypes.data_as(ctypes.c_void_p), s1.HEAD - 2))
	return out


def judge(ws, case):
	for name, w in ws.items():
		print('%-14s worst error / bound %.3g at %s  (%s; %s)' % (name, w.ratio, w.where, w.what, case))
	bad = {k: w for k, w in ws.items() if not w.ratio <= 1}
	assert not bad, (case, bad)


@pytest.mark.parametrize('variant', sw.GI_VARIANTS)
@pytest.mark.parametrize('nc', sw.GI_NC)
@pytest.mark.parametrize('nx', sw.GI_NX)
def test_group_info_wide_host(nx, nc, variant):
	pb = sw.gi_problem(nx, nc, variant)
	ref = sw.gi_reference(pb)
	info, varx, flags = sw.gi_host(_lib.load(), _lib.check, pb)
	assert (flags[[0, 1]] == 0).all() and (flags[5:] == -7).all(), flags
	judge(sw.gi_judge(info, varx, flags, pb, ref, plans), 'nx%d nc%d %s' % (nx, nc, variant))
	# the ranks the variants are built for, through dof = ns - 1 - rank - dimreduce of the groupings that keep a positive dof
	if variant != 'no shared cells':
		want = {'duplicate': nc - 1, 'zero covariate': nc - 1, 'one-hot': nc - 1}.get(variant, nc)
		ok = ~ref['fallback']
		assert (ref['rank'][ok] == want).all(), (variant, ref['rank'])
		assert (info[ok, 0] - 1 - ref['dof'][ok] - pb['dimreduce'] == want).all()
	else:
		assert flags[3] > 0 and (ref['rank'] < nc).all()


def test_group_info_wide_host_counts_on_top_of_the_flags_it_finds():
	"""The counters are added to (a plan's steps accumulate them until it looks), and two runs give the same bits."""
	pb = sw.gi_problem(65, 12, 'plain')
	one = sw.gi_host(_lib.load(), _lib.check, pb, extra_pitch=0, prefill=(0, 0, 0, 0, 0, 0, 0, 0))
	two = sw.gi_host(_lib.load(), _lib.check, pb, extra_pitch=0, prefill=(5, 6, 1, 2, 3, 9, 9, 9))
	assert (two[2] - one[2] == [5, 6, 1, 2, 3, 9, 9, 9]).all() and one[2][2] == 1 and one[2][4] == 1
	assert s1.same_bits(one[0], two[0]).all() and s1.same_bits(one[1], two[1]).all()


def test_a_dropped_block_or_partial_is_caught():
	"""The problems are built so that the comparison depends on every block pair and every partial sum of gpart: zeroing one moves M+ out of its bound."""
	pb = sw.gi_problem(1, 17, 'plain')
	ref = sw.gi_reference(pb)
	for q, g in ((0, 63), (2, 0), (5, 31)):
		cut = dict(pb, gpart=pb['gpart'].copy())
		cut['gpart'][q, g] = 0.0
		info, varx, flags = sw.gi_host(_lib.load(), _lib.check, cut)
		assert s1.judge_group_info(info, varx, flags, ref, 17)['M+'].ratio > 1, (q, g)


def test_group_info_wide_host_refuses():
	lib = _lib.load()
	pb = sw.gi_problem(1, 9, 'plain')
	for bad in (dict(nc=0), dict(nc=33), dict(nx=0)):
		with pytest.raises(Exception):
			sw.gi_host(lib, _lib.check, dict(pb, **bad))
	a = np.zeros(2000)
	vp = a.ctypes.data_as(ctypes.c_void_p)
	assert lib.nrm_single1_group_info_wide_host(vp, vp, vp, vp, 9, 1, 0, vp, s1.HEAD + 9 + 81 - 1, vp, vp) != 0  # a pitch one too small
	for k in (0, 1, 2, 3, 7, 9, 10):
		args = [vp, vp, vp, vp, 9, 1, 0, vp, s1.HEAD + 9 + 81, vp, vp]
		args[k] = None
		assert lib.nrm_single1_group_info_wide_host(*args) != 0, k
	assert not a.any()
