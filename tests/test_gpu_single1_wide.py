"""GPU: single=1 with 9 .. 32 covariates wholly on the device.

Kernel level (through the C ABI, buffers pre-filled with NaN at a pitch above the minimum and followed by a tail that must stay untouched, every call made twice
with identical bits): nrm_single1_group_stats_wide against the longdouble sums -- bit for bit on small integers, within (len + 1) u sum |terms| on real data,
len being the one fma chain over the segment's cells that the kernel's comment states --; nrm_single1_group_info_wide on the problems of
tests/test_single1_wide_cpu.py against the same reference and bounds, its ranks and counters equal to the host twin's; the refusals of both.

End to end (65 groupings x 69 genes x 2051 cells, the chain test's shape): Single1Plan at 9, 12 and 32 covariates against the oracle's per-grouping loop with the
tolerances tests/test_gpu_round6.py::test_single1_plan_keeps_the_host_out_of_a_step uses up to 8, five steps of which the later ones are graph replays with the
first step's bits, the public call, the host route of NRM_DEBUG=single1_stats=host, what the reference raises; golden G24 (the reference's own arrays) through
the public call and through nrm_association_tests_single1_host in a process without torch, which reports where it finished the groupings' statistics."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import s1_reference as s1
import s1_wide as sw
from cabi_harness import held
from test_gpu_parity import close, p_close
from test_gpu_s1_stages import F32, F64, I32, I64, Buf, _env, _sync, note, plans, same, twice

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- nrm_single1_group_stats_wide ---------------------------------------------------------------------------------------------------------------------------
def run_group_stats_wide(pb):
	_, _lib, eng = _env()
	nc, seg = pb['nc'], pb['seg']
	nx = len(seg) - 1
	npk = nc * (nc + 1) // 2 + nc + 1

	def run():
		d_seg, d_xe, d_ce = Buf(nx + 1, I64, data=seg), Buf(len(pb['xe']), F64, data=pb['xe']), Buf(pb['ce'].shape, F64, data=pb['ce'])
		out = Buf((nx, npk), F64)
		_lib.check(eng.lib.nrm_single1_group_stats_wide(d_seg.ptr, d_xe.ptr, d_ce.ptr, nc, nx, out.ptr, eng._stream()))
		_sync()
		return dict(gs=out.get())
	return twice(run)['gs']


@pytest.mark.parametrize('nc', sw.GS_NC)
def test_group_stats_wide(nc):
	"""k_s1_group_stats_wide: segments of 0 (zeros), 1, 63, 64, 65 and 130 cells (no, one, two and three chunks of 64, full and ragged); 66 .. 561 outputs, so
	that lanes own two to nine of them and the last slot is ragged."""
	for exact in (True, False):
		pb = sw.gs_problem(nc, exact)
		ref, bound = sw.gs_reference(pb)
		got = run_group_stats_wide(pb)
		assert not got[0].any(), 'the empty segment'
		w = s1.bits(got, np.asarray(ref, F64), 'gs (exact)') if exact else s1.worst(np.abs(s1.ld(got) - ref), bound, 'gs')
		note('nrm_single1_group_stats_wide', dict(gs=w), 'nc%d %s' % (nc, 'exact' if exact else 'real'))


# ---- nrm_single1_group_info_wide ----------------------------------------------------------------------------------------------------------------------------
def run_group_info_wide(pb, extra_pitch=5, prefill=(0, 0, 0, 0, 0, -7, -7, -7)):
	_, _lib, eng = _env()
	nx, nc = pb['nx'], pb['nc']
	width = s1.HEAD + nc + nc * nc
	pitch = width + extra_pitch

	def run():
		d_gs, d_rows = Buf(pb['gs'].shape, F64, data=pb['gs']), Buf((nx, 3), F64, data=pb['rowinfo'])
		d_gp = Buf(pb['gpart'].shape, F64, data=pb['gpart'])
		sel = np.full(8, -7, I64)
		sel[3] = pb['n_common']
		d_sel = Buf(8, I64, data=sel)
		info, varx, flags = Buf((nx, width), F64, pitch=pitch), Buf(nx, F64), Buf(8, I32, data=prefill)
		_lib.check(eng.lib.nrm_single1_group_info_wide(d_gs.ptr, d_gp.ptr, d_rows.ptr, d_sel.ptr, nc, nx, pb['dimreduce'], info.ptr, pitch, varx.ptr, flags.ptr, eng._stream()))
		_sync()
		return dict(info=info.get(), varx=varx.get(), flags=flags.get())
	return twice(run)


@pytest.mark.parametrize('nc', sw.GI_NC)
@pytest.mark.parametrize('nx', sw.GI_NX)
def test_group_info_wide(nx, nc):
	"""k_s1_group_info_wide on the problems of the CPU file: one, two, three and four blocks of covariates (1, 3, 6 and 10 block pairs), a ragged last block."""
	_, _lib, eng = _env()
	for variant in sw.GI_VARIANTS:
		pb = sw.gi_problem(nx, nc, variant)
		ref = sw.gi_reference(pb)
		got = run_group_info_wide(pb)
		assert (got['flags'][[0, 1]] == 0).all() and (got['flags'][5:] == -7).all(), got['flags']
		note('k_s1_group_info_wide', sw.gi_judge(got['info'], got['varx'], got['flags'], pb, ref, plans), 'nx%d nc%d %s' % (nx, nc, variant))
		# the host twin: the same integers -- ns, the rank through the plan of dof, the counters
		h_info, h_varx, h_flags = sw.gi_host(eng.lib, _lib.check, pb)
		assert same(got['info'][:, 0].copy(), h_info[:, 0].copy()) and same(got['info'][:, 2:s1.HEAD].copy(), h_info[:, 2:s1.HEAD].copy()), 'ns / dof differ from the host twin'
		assert (got['flags'] == h_flags).all(), (got['flags'], h_flags)
	# counters are added to
	pb = sw.gi_problem(nx, nc, 'plain')
	a = run_group_info_wide(pb, extra_pitch=0, prefill=(0, 0, 0, 0, 0, 0, 0, 0))['flags']
	b = run_group_info_wide(pb, extra_pitch=0, prefill=(5, 6, 1, 2, 3, 9, 9, 9))['flags']
	assert (b - a == [5, 6, 1, 2, 3, 9, 9, 9]).all()


def test_wide_refusals_write_nothing():
	"""Both wide entries: nc = 0, nc = 33, a pitch one too small, null pointers -- an error code, and nothing written."""
	_, _lib, eng = _env()
	lib, st = eng.lib, eng._stream()
	nx, nc = 3, 9
	width = s1.HEAD + nc + nc * nc
	seg = Buf(nx + 1, I64, data=np.zeros(nx + 1, I64))
	ins = Buf(64 * 64, F64, data=np.ones(64 * 64))
	outs = dict(gs=Buf(nx * 600, F64), rec=Buf(nx * 1200, F64), varx=Buf(nx, F64), flags=Buf(8, I32))
	o = {k: b.ptr for k, b in outs.items()}

	def gstats(nc_=nc, seg_=seg.ptr, xe=ins.ptr, ce=ins.ptr, out=o['gs']):
		return lib.nrm_single1_group_stats_wide(seg_, xe, ce, nc_, nx, out, st)

	def ginfo(nc_=nc, pitch=1100, gs=ins.ptr, gp=ins.ptr, rows=ins.ptr, sel=seg.ptr, rec=o['rec'], varx=o['varx'], flags=o['flags']):
		return lib.nrm_single1_group_info_wide(gs, gp, rows, sel, nc_, nx, 0, rec, pitch, varx, flags, st)

	for what, call in (('group_stats_wide: nc = 0', lambda: gstats(nc_=0)), ('group_stats_wide: nc = 33', lambda: gstats(nc_=33)), ('group_stats_wide: null seg', lambda: gstats(seg_=0)),
					   ('group_stats_wide: null xe', lambda: gstats(xe=0)), ('group_stats_wide: null ce', lambda: gstats(ce=0)), ('group_stats_wide: null out', lambda: gstats(out=0)),
					   ('group_info_wide: nc = 0', lambda: ginfo(nc_=0)), ('group_info_wide: nc = 33', lambda: ginfo(nc_=33, pitch=1200)),
					   ('group_info_wide: pitch too small', lambda: ginfo(pitch=width - 1)), ('group_info_wide: null gs', lambda: ginfo(gs=0)),
					   ('group_info_wide: null gram_part', lambda: ginfo(gp=0)), ('group_info_wide: null rowinfo', lambda: ginfo(rows=0)),
					   ('group_info_wide: null sel_info', lambda: ginfo(sel=0)), ('group_info_wide: null info', lambda: ginfo(rec=0)),
					   ('group_info_wide: null varx', lambda: ginfo(varx=0)), ('group_info_wide: null flags', lambda: ginfo(flags=0))):
		rc = call()
		_sync()
		print('%-36s -> %d  %s' % (what, rc, lib.nrm_last_error().decode()))
		assert rc != 0, what
		dirty = [k for k, b in outs.items() if not b.clean()]
		assert not dirty, (what, dirty)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------------
NX, NY, N = (s1.CHAIN[k] for k in ('nx', 'ny', 'n'))


def screen(nc, kind, seed=0):
	"""65 groupings x 69 genes x 2051 cells at one grouping per cell on average; covariates: the intercept last, 'dup': covariate 1 repeats covariate 0 (rank
	nc - 1), 'onehot': six one-hot batches in front, whose sum is the intercept (rank nc - 1)."""
	rng = np.random.default_rng([seed, nc, 61])
	dx = (rng.random((NX, N)) < 1.0 / NX).astype(F64)
	dy = rng.normal(size=(NY, N))
	dy[:5] += 0.5 * dx[0]
	dc = np.vstack([rng.normal(size=(nc - 1, N)), np.ones((1, N))])
	if kind == 'dup':
		dc[1] = dc[0]
	if kind == 'onehot':
		dc[:6] = rng.integers(6, size=N)[None] == np.arange(6)[:, None]
	return dx, dy, dc


@pytest.mark.parametrize('nc,kind,dtype', [(9, 'plain', F32), (9, 'dup', F64), (12, 'onehot', F32), (12, 'plain', F64), (32, 'dup', F32), (32, 'onehot', F64)])
def test_single1_plan_wide(nc, kind, dtype):
	import torch
	from normalisr_amd.single1 import Single1Plan, association_tests_single1
	dx, dy, dc = screen(nc, kind)
	dy = dy.astype(dtype)
	want = oracle.association_tests(dx, dy.astype(F64), dc, single=1, return_dot=False, lowmem=False)
	plan = Single1Plan(torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda(), dc, return_dot=False, lowmem=False)
	nb = (nc + 7) // 8
	assert plan.gpart.shape[0] == nb * (nb + 1) // 2
	plan.step()
	first = plan.results()
	held(first, want, dtype, nc)
	for _ in range(4):
		plan.step()
	assert plan._graph.graph is not None  # captured: no synchronisation, read-back or upload inside a step
	again = plan.results()
	assert all(np.array_equal(a, b) for a, b in zip(first, again))
	got = association_tests_single1(dx, dy, dc, return_dot=False, lowmem=False)
	assert all(np.array_equal(a, b) for a, b in zip(first, got)), 'the public call and the plan differ'
	os.environ['NRM_DEBUG'] = 'single1_stats=host'
	try:
		host = association_tests_single1(dx, dy, dc, return_dot=False, lowmem=False)
	finally:
		del os.environ['NRM_DEBUG']
	assert p_close(host[0], first[0], 1e-9) and close(host[1], first[1], 1e-9, 1e-12) and close(host[3], first[3], 1e-9)


def test_single1_wide_raises_what_the_reference_raises():
	from normalisr_amd.single1 import association_tests_single1
	nc = 12
	dx, dy, dc = screen(nc, 'plain', seed=1)
	with pytest.raises(RuntimeError):
		association_tests_single1(dx, dy, dc, dimreduce=N)
	bad = dc.copy()
	bad[0, np.nonzero(dx.sum(axis=0) == 0)[0][0]] = np.nan  # (at a cell every grouping shares)
	with pytest.raises(ValueError):
		association_tests_single1(dx, dy, bad)
	one = np.zeros_like(dx)
	for i in range(NX):
		one[i, i::NX] = 1  # every cell carries exactly one grouping: no shared cells, grouping i is constant 1 on its own cells
	with pytest.raises(AssertionError):
		association_tests_single1(one, dy, dc)


# ---- golden G24: the reference's own arrays ------------------------------------------------------------------------------------------------------------------
def g24():
	return np.load(os.path.join(HERE, 'golden', 'g24.npz'))


def run_child(tmp_path, name, dx, dy, dc, debug):
	src, dst = str(tmp_path / (name + '_in.npz')), str(tmp_path / (name + '_out.npz'))
	np.savez(src, dx=dx, dy=dy, dc=dc)
	env = dict(os.environ, NRM_DEBUG=debug)
	r = subprocess.run([sys.executable, os.path.join(HERE, 'single1_wide_child.py'), src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
	assert r.returncode == 0 and 'child ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
	out = np.load(dst)
	return tuple(out[k] for k in ('p', 'gamma', 'alpha', 'varx', 'vary')), r.stderr


@pytest.mark.parametrize('name', ['c12', 'c32'])
def test_g24_public_call_and_c_entry(name, tmp_path):
	from normalisr_amd.single1 import association_tests_single1
	g = g24()
	dx, dy, dc = g['dx'], g['dy'], g[name + '_dc']
	want = tuple(g['%s_%s' % (name, k)] for k in ('p', 'gamma', 'alpha', 'varx', 'vary'))
	assert (g[name + '_rank'] == (11 if name == 'c12' else 32)).all()
	held(association_tests_single1(dx, dy, dc, return_dot=False, lowmem=False), want, F64, dc.shape[0])
	got, err = run_child(tmp_path, name, dx, dy, dc, 's1_trace=1')
	held(got, want, F64, dc.shape[0])
	# where the entry finished the groupings' statistics: on the device -- no download of the sums, no host pseudo-inverse
	assert 'statistics on the device (wide)' in err and 'statistics on the host' not in err, err
	if name == 'c12':
		host, err = run_child(tmp_path, name + '_host', dx, dy, dc, 's1_trace=1,single1_stats=host')
		assert 'statistics on the host' in err and 'on the device' not in err, err
		assert p_close(host[0], got[0], 1e-9) and close(host[1], got[1], 1e-9, 1e-12)
