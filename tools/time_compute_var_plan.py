"""compute_var at the front half's shape (5000 genes x 10 000 cells resident in HBM, 8 covariates of rank 7: 4 one-hot batches, lcpm's three and the intercept;
tools/time_front.py's problem) in ONE process, after warm-up: the public norm.compute_var (synchronised wall clock: the call ends in a read-back) and a
ComputeVarPlan.step() (HIP events around the graph replay), for fp32 and fp64 logCPM and stepmax 1 and 3 (eps so small that every iteration runs).  The public
call is untouched by the plan, so its figure is the figure of the commit before it.  Then the entries of csrc/nrm_fitvar_plan.hip one by one, eagerly, with
HIP events around each (an entry is one to four small kernels; the three streaming passes beside them for scale).  Writes one JSON record.

Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_compute_var_plan.py --reps 5 --out /dev/null
    python tools/time_compute_var_plan.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/compute_var_plan.json      (merges them into the record; no GPU needed)

Usage: time_compute_var_plan.py [--reps R] [--warmup W] [--out profiles/compute_var_plan.json] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NG, N, SEED = 5000, 10000, 18


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=50)
	ap.add_argument('--warmup', type=int, default=5)
	ap.add_argument('--out', default='profiles/compute_var_plan.json')
	ap.add_argument('--kernel-stats', default=None)
	args = ap.parse_args()
	if args.kernel_stats:
		rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
		rec['kernels'] = {}
		for r in csv.DictReader(open(args.kernel_stats)):
			name = r.get('Name') or ''
			if 'k_fvp_' in name or 'k_fv_' in name:
				rec['kernels'][name.replace('void ', '').split('(')[0]] = dict(calls=int(float(r.get('Calls') or 0)), avg_ms=round(float(r.get('AverageNs') or 0) / 1e6, 5))
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')
		print(json.dumps(rec['kernels']))
		return
	import torch
	import normalisr_amd.normalisr as norm
	from normalisr_amd import _lib
	from normalisr_amd.norm import ComputeVarPlan
	rng = np.random.default_rng(SEED)
	mu = np.exp(rng.normal(-1.0, 1.3, NG))
	depth = np.exp(rng.normal(0.0, 0.5, N))
	x = rng.poisson(mu[:, None] * depth[None, :]).astype(np.int32)
	x[0, x.sum(axis=0) == 0] = 1
	batch = rng.integers(0, 4, N)
	onehot = (batch[None, :] == np.arange(4)[:, None]).astype(np.float64)
	reads = torch.as_tensor(x).cuda()

	def stats(ms):
		return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))

	def events(fn, reps=None):
		for _ in range(args.warmup):
			fn()
		ms = []
		for _ in range(reps or args.reps):
			torch.cuda.synchronize()
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			fn()
			e1.record()
			torch.cuda.synchronize()
			ms.append(e0.elapsed_time(e1))
		return stats(ms)

	def wall(fn):
		for _ in range(args.warmup):
			fn()
		ms = []
		for _ in range(args.reps):
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			fn()
			torch.cuda.synchronize()
			ms.append((time.perf_counter() - t0) * 1e3)
		return stats(ms)

	rec = dict(tool='time_compute_var_plan', device=torch.cuda.get_device_name(0), warmup=args.warmup, cases={},
			   shape=dict(genes=NG, cells=N, covariates=8, covariate_rank=7),
			   note='public: norm.compute_var on the resident tensor, host clock between synchronisations; plan: ComputeVarPlan.step(), HIP events, graph replay')
	for name, odt in (('fp32', np.float32), ('fp64', np.float64)):
		lc, _, _, cov = norm.lcpm(reads, device_out=True, out_dtype=odt)
		dc = norm.normcov(np.vstack([onehot, cov]))
		for steps in (1, 3):
			plan = ComputeVarPlan(lc, dc, stepmax=steps, eps=1e-300)
			case = dict(public=wall(lambda: norm.compute_var(lc, dc, stepmax=steps, eps=1e-300)), plan_step=events(plan.step))
			w = plan.results()
			pub = norm.compute_var(lc, dc, stepmax=steps, eps=1e-300)
			case.update(graph=plan._graph.graph is not None, steps_taken=plan.steps_taken, best_change=plan.best_change, max_rel_diff_to_public=float(np.abs(w / pub - 1).max()),
						speedup=round(case['public']['median_ms'] / case['plan_step']['median_ms'], 3))
			rec['cases']['{}_stepmax{}'.format(name, steps)] = case
		if name == 'fp32':  # the entries of one iteration, eagerly, one by one (the state is that of a first iteration: nothing has stopped)
			p = ComputeVarPlan(lc, dc, stepmax=1, eps=1e-300)
			p.step()
			lib, ptr = p.eng.lib, lambda t: t.data_ptr()
			nt, ns, nc, st = NG, N, dc.shape[0], p.eng._stream()
			now, nxt = ptr(p._state[0]), ptr(p._state[1])
			ck = _lib.check
			ycode = _lib.NRM_F32
			ent = dict(
				plan_start=lambda: ck(lib.nrm_fitvar_plan_start(ns, ptr(p._s), ptr(p._best), now, st)),
				design=lambda: ck(lib.nrm_fitvar_design(ptr(p._c), nc, ns, ns, ptr(p._s), now, p.eps, ptr(p._u), ptr(p._cw), ptr(p._ws), st)),
				pinv=lambda: ck(lib.nrm_fitvar_pinv(ns, nc, 1E-8, now, p.eps, ptr(p._ws), ptr(p._mi), ptr(p._rank), st)),
				moments=lambda: ck(lib.nrm_fitvar_moments(ptr(lc), ycode, nt, ns, lc.stride(0), ptr(p._cw), nc, ns, ptr(p._a), st)),
				genes=lambda: ck(lib.nrm_fitvar_genes(ptr(lc), ycode, nt, ns, lc.stride(0), ptr(p._u), ptr(p._c), nc, ns, ptr(p._a), ptr(p._mi), ptr(p._b), ptr(p._mean), ptr(p._sc),
													  ptr(p._flags), st)),
				cells=lambda: ck(lib.nrm_fitvar_cells(ptr(lc), ycode, nt, ns, lc.stride(0), ptr(p._u), ptr(p._c), nc, ns, ptr(p._b), ptr(p._mean), ptr(p._sc), ptr(p._part),
													  ptr(p._v), st)),
				update=lambda: ck(lib.nrm_fitvar_update(ptr(p._v), ptr(p._c), nc, ns, ns, ptr(p._m2i), ptr(p._s), ptr(p._best), now, nxt, p.eps, ptr(p._ws), st)),
				weights=lambda: ck(lib.nrm_fitvar_weights(ptr(p._best), ns, ptr(p._ws), ptr(p.w), ptr(p._flags), st)),
			)
			rec['entries_fp32_eager'] = {}
			for k in ('plan_start', 'design', 'pinv', 'moments', 'genes', 'cells', 'update', 'weights'):  # (in the order of a step: each leaves what the next reads)
				ent['plan_start']()
				rec['entries_fp32_eager'][k] = events(ent[k], reps=20)
			rec['entries_fp32_eager']['note'] = ('HIP events around ONE eager call: the launch is inside the figure; design, pinv, update (4 kernels) and weights (2) are new, '
												 'plan_start the fill, moments / genes / cells the unchanged streaming passes')
	print(json.dumps(rec))
	if args.out != '/dev/null':
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
	main()
