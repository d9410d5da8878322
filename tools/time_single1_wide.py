"""single=1 with 12 and 32 covariates at the configs[3] screen (1000 groupings x 15 000 genes x 50 000 cells, fp32, resident in HBM): the device route
(Single1Plan: the wide kernels beside k_s1_stream on the side stream) next to the route the parent commit took for more than 8 covariates
(association_tests_single1 under NRM_DEBUG=single1_stats=host: read-backs, host pseudo-inverses, an upload), three processes each, alternating.

    python tools/time_single1_wide.py [steps]            -> profiles/single1_wide.json, and the summary on stdout

Covariates as norm.normcov leaves them: one-hot batches untouched, continuous covariates standardised, the intercept last (12: 6 + 5 + 1; 32: 16 + 15 + 1).
Per process and covariate count -- device: HIP-event time per graph-replayed step, and on one stream by themselves the side stream's launches
(nrm_single1_common_gram + nrm_single1_group_stats_wide + nrm_single1_group_info_wide) and nrm_single1_stream, whose time they have to stay inside for the
step not to be lengthened by them; host: wall-clock per call, closed by a device synchronisation.  A child is `... --child device|host STEPS`."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, N = 1000, 15000, 50000
COVS = {12: 6, 32: 16}  # covariates: one-hot batches among them


def screen(torch, nc):
	from normalisr_amd.norm import normcov
	g = torch.Generator(device='cuda').manual_seed(4)
	dx = (torch.rand((NX, N), generator=g, device='cuda') < 0.001).to(torch.float32)
	dy = torch.randn((NY, N), generator=g, device='cuda')
	rng = np.random.default_rng(nc)
	nb = COVS[nc]
	raw = np.concatenate([(rng.integers(nb, size=N)[None] == np.arange(nb)[:, None]).astype(np.float64), rng.normal(2.0, 3.0, size=(nc - 1 - nb, N))])
	dc = normcov(raw)
	assert dc.shape == (nc, N)
	return dx, dy, dc


def events(torch, fn, reps):
	for _ in range(3):
		fn()
	torch.cuda.synchronize()
	a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	a.record()
	for _ in range(reps):
		fn()
	b.record()
	torch.cuda.synchronize()
	return a.elapsed_time(b) / reps


def child(route, steps):
	sys.path.insert(0, ROOT)
	if route == 'host':
		os.environ['NRM_DEBUG'] = 'single1_stats=host'
	import torch
	from normalisr_amd import _lib
	from normalisr_amd import engine as _engine
	from normalisr_amd.single1 import Single1Plan, association_tests_single1
	out = {}
	for nc in COVS:
		dx, dy, dc = screen(torch, nc)
		if route == 'host':
			call = lambda: association_tests_single1(dx, dy, dc, return_dot=False, device_out=True)
			for _ in range(2):
				call()
			torch.cuda.synchronize()
			ts = []
			for _ in range(max(steps // 4, 5)):
				t0 = time.perf_counter()
				call()
				torch.cuda.synchronize()
				ts.append(1e3 * (time.perf_counter() - t0))
			out[str(nc)] = dict(call_ms_min=min(ts), call_ms_median=float(np.median(ts)), call_ms_max=max(ts))
			continue
		plan = Single1Plan(dx, dy, dc, return_dot=False)
		step = events(torch, plan.step, steps)
		assert plan._graph.graph is not None
		plan.check()
		lib, eng = plan.eng.lib, plan.eng
		st = eng._stream()
		n = N

		def side():
			_lib.check(lib.nrm_single1_common_gram(plan.cnt.data_ptr(), n, plan.d_c.data_ptr(), n, nc, plan.gpart.data_ptr(), st))
			_lib.check(lib.nrm_single1_group_stats_wide(plan.seg.data_ptr(), plan.xe.data_ptr(), plan.ce.data_ptr(), nc, NX, plan.gs.data_ptr(), st))
			_lib.check(lib.nrm_single1_group_info_wide(plan.gs.data_ptr(), plan.gpart.data_ptr(), plan.rowinfo.data_ptr(), plan.sel_info.data_ptr(), nc, NX, 0, plan.info.data_ptr(),
													   plan.pitch, plan.varx.data_ptr(), plan.flags.data_ptr(), st))

		def group_info():
			_lib.check(lib.nrm_single1_group_info_wide(plan.gs.data_ptr(), plan.gpart.data_ptr(), plan.rowinfo.data_ptr(), plan.sel_info.data_ptr(), nc, NX, 0, plan.info.data_ptr(),
													   plan.pitch, plan.varx.data_ptr(), plan.flags.data_ptr(), st))

		def stream():
			_lib.check(lib.nrm_single1_stream(plan.d_y.data_ptr(), _engine.dtype_code(plan.d_y), plan.d_y.stride(0), plan.d_c.data_ptr(), n, nc, plan.code.data_ptr(), n, NY,
											  plan.common.data_ptr(), plan.ye.data_ptr(), plan.ldye, st))
		with eng.lock, torch.cuda.device(eng.device):
			out[str(nc)] = dict(step_ms=step, side_ms=events(torch, side, steps), group_info_ms=events(torch, group_info, steps), stream_ms=events(torch, stream, steps),
								cells_kept=plan.cells_kept())
		plan.check()
		del plan
	print('RESULT ' + json.dumps(dict(route=route, results=out)))


def main():
	steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
	runs = []
	for k in range(3):
		for route in ('device', 'host'):
			r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', route, str(steps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
			line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
			if r.returncode != 0 or not line:
				sys.exit('child %s failed (%d):\n%s' % (route, r.returncode, r.stdout[-3000:]))
			runs.append(dict(json.loads(line[0][7:]), process=k))
			print(route, k, json.dumps(runs[-1]['results']), flush=True)
	summary = {}
	for nc in COVS:
		dev = [r['results'][str(nc)] for r in runs if r['route'] == 'device']
		host = [r['results'][str(nc)] for r in runs if r['route'] == 'host']
		med = lambda rows, key: float(np.median([row[key] for row in rows]))
		summary[str(nc)] = dict(step_ms=med(dev, 'step_ms'), side_ms=med(dev, 'side_ms'), group_info_ms=med(dev, 'group_info_ms'), stream_ms=med(dev, 'stream_ms'),
								side_inside_stream=bool(all(row['side_ms'] < row['stream_ms'] for row in dev)), host_route_call_ms=med(host, 'call_ms_median'),
								host_route_call_ms_max=max(row['call_ms_max'] for row in host))
	os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
	doc = dict(shape=dict(nx=NX, ny=NY, n=N, dtype='float32'), steps=steps, protocol='three processes per route, alternating; medians over the processes', summary=summary, runs=runs)
	with open(os.path.join(ROOT, 'profiles', 'single1_wide.json'), 'w') as f:
		json.dump(doc, f, indent=1)
	print(json.dumps(summary, indent=1))


if __name__ == '__main__':
	if len(sys.argv) > 2 and sys.argv[1] == '--child':
		child(sys.argv[2], int(sys.argv[3]))
	else:
		main()
