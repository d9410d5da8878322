"""Which cases of tests/test_gpu_k1_rows8.py reach k_residualize_v8: asked of the launcher's own conditions (csrc/nrm_host_logic.h nrm_k1_vec,
nrm_k1_stream_rows, nrm_k1_rows8 and nrm_k1_rows8_pays -- launch_residualize calls the same functions: the new kernel runs where nrm_k1_rows8 holds and either
nrm_k1_rows8_pays does or NRM_DEBUG="k1_rows8=1" is set, as the GPU test sets it), built by g++ into a stand-alone program (tests/host/k1_route.cpp)."""
import os
import shutil
import subprocess

import pytest

import k1_longdouble as k1
from conftest import ROOT
from test_gpu_k1_rows8 import CASES, case_id, rows_pad_of


def route(tmp_path, calls):
	gxx = shutil.which('g++')
	if gxx is None:
		pytest.skip('no g++')
	exe = str(tmp_path / 'k1_route')
	r = subprocess.run([gxx, '-std=c++17', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'host', 'k1_route.cpp')], stdout=subprocess.PIPE,
					   stderr=subprocess.STDOUT, text=True)
	assert r.returncode == 0, r.stdout[-3000:]
	r = subprocess.run([exe], input=''.join(' '.join(str(int(v)) for v in call) + '\n' for call in calls), stdout=subprocess.PIPE, text=True, timeout=60)
	assert r.returncode == 0
	out = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
	assert len(out) == len(calls)
	return out


def call_of(c):
	"""The call run_k1 makes for a case: rows and covariates at a pitch of the cells rounded up to 16, fp64 output at the same pitch unless chunked."""
	kp = k1.round_up(c['n'], 16)
	return (4 if c['dtype'] == 'float32' else 8, kp, 0 if c['chunks'] else 1, kp, 1, kp, c['nc'], c['n'], rows_pad_of(c))


def test_cases_reach_the_eight_row_kernel(tmp_path):
	got = route(tmp_path, [call_of(c) for c in CASES])
	expect = [rows_pad_of(c) % 8 == 0 for c in CASES]  # all cases are aligned, active, of at most 8 covariates and far below 8 MB of them
	assert [g[:3] == (1, 0, int(e)) for g, e in zip(got, expect)] == [True] * len(CASES), [case_id(c) for c, g, e in zip(CASES, got, expect) if g[:3] != (1, 0, int(e))]
	assert [g[3] for g in got] == [int(c['n'] >= 16384) for c in CASES]
	assert any(g[2] and g[3] for g in got)  # one case is the launcher's own choice
	routed = [c for c, g in zip(CASES, got) if g[2]]
	kept = [c for c, g in zip(CASES, got) if not g[2]]
	assert kept and all(c['ns'] == 0 for c in kept)
	# every branch of the new kernel is reached by a routed case
	has = lambda f: any(f(c) for c in routed)
	for n in (16, 1020, 1024, 1028, 2050, 4100):
		assert has(lambda c: c['n'] == n), n
	for nc in (1, 3, 4, 5, 8):
		assert has(lambda c: c['nc'] == nc), nc
	for rows in (5, 8, 9, 12, 129):
		assert has(lambda c: c['rows'] == rows), rows
	for ns in (0, 5, 6):
		for dtype in ('float32', 'float64'):
			assert has(lambda c: c['ns'] == ns and c['dtype'] == dtype), (ns, dtype)
		assert has(lambda c: c['ns'] == ns and c['nc'] <= 4) and has(lambda c: c['ns'] == ns and c['nc'] > 4), ns
	assert has(lambda c: c['ns'] and not c['cmax']) and has(lambda c: c['ns'] and c['cmax'])  # the extra sweep for everybody / the bound
	assert has(lambda c: c['special'] and c['special'][1] < 4) and has(lambda c: c['special'] and c['special'][1] >= 4)  # one group sweeps, its neighbour not
	assert has(lambda c: c['block']) and has(lambda c: c['chunks'])
	assert has(lambda c: c['n'] % 4 != 0) and has(lambda c: c['n'] % 1024 != 0 and c['n'] > 1024)
	assert has(lambda c: rows_pad_of(c) - c['rows'] >= 8)  # a workgroup of padding rows only


def test_what_keeps_the_four_row_kernel(tmp_path):
	"""The launcher's other conditions one at a time: an odd pitch (no vector loads at all), no covariates, more than 8 of them, rows_pad no multiple of 8,
	fp32 rows against 8 MB of covariates (streamed rows); fp64 rows against the same covariates do route."""
	base = dict(xb=4, ldx=1024, has_out=1, ldo=1024, active=1, ldc=1024, nc=3, n=1000, rows_pad=128)
	def call(**kw):
		d = dict(base, **kw)
		return tuple(d[k] for k in ('xb', 'ldx', 'has_out', 'ldo', 'active', 'ldc', 'nc', 'n', 'rows_pad'))
	got = route(tmp_path, [call(), call(ldx=1023), call(ldc=1023), call(active=0), call(nc=9), call(rows_pad=132),
						   call(nc=8, n=131072, ldx=131072, ldo=131072, ldc=131072), call(xb=8, nc=8, n=131072, ldx=131072, ldo=131072, ldc=131072),
						   call(nc=8, n=131071, ldx=131072, ldo=131072, ldc=131072)])
	assert [g[:3] for g in got] == [(1, 0, 1), (0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 1)]
	assert [g[3] for g in got] == [0, 0, 0, 0, 0, 0, 1, 1, 1]
	assert [g[3] for g in route(tmp_path, [call(n=16383, ldx=16384, ldo=16384, ldc=16384), call(n=16384, ldx=16384, ldo=16384, ldc=16384)])] == [0, 1]
