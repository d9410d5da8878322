"""single=4 at BASELINE configs[3] shapes (1000 gRNAs x 15000 genes x 50000 cells, fp32, resident in HBM) on two covariate sets in ONE process:
SURVEY's C4 set -- one-hot batches, 3 continuous covariates and the intercept, rank deficient by one (the batch rows sum to the intercept) -- and
bench.py's full-rank set (4 Gaussian rows and the intercept).  For each set: the Single4Plan step (one captured HIP graph) and the public call
association_tests_single4(device_out=True), timed with device events; the sets alternate after warm-up.  Writes one JSON record.

Usage: time_single4_rank_deficient.py [--rounds R] [--steps K] [--calls C] [--out profiles/single4_rank_deficient.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--rounds', type=int, default=3)
	ap.add_argument('--steps', type=int, default=10)
	ap.add_argument('--calls', type=int, default=3)
	ap.add_argument('--out', default='profiles/single4_rank_deficient.json')
	args = ap.parse_args()
	import torch
	from normalisr_amd.engine import get_engine
	from normalisr_amd.single4 import Single4Plan, association_tests_single4
	nx, ny, n, seed = 1000, 15000, 50000, 4
	dev = torch.device('cuda', torch.cuda.current_device())
	g = torch.Generator(device=dev)
	g.manual_seed(seed)
	dx = (torch.rand((nx, n), generator=g, device=dev) < 0.01).to(torch.float32)
	dy = torch.randn((ny, n), generator=g, device=dev, dtype=torch.float32)
	dy[:16] += 0.2 * dx[0]
	rng = np.random.default_rng(seed)
	batch = rng.integers(0, 4, n)
	sets = {
		'full_rank': np.vstack([rng.normal(size=(4, n)), np.ones((1, n))]),
		'c4_onehot': np.vstack([(batch[None, :] == np.arange(4)[:, None]).astype(np.float64), rng.normal(size=(3, n)), np.ones((1, n))]),
	}
	eng = get_engine()
	plans = {k: Single4Plan(dx, dy, dc, return_dot=False) for k, dc in sets.items()}
	t0 = time.perf_counter()
	for k, plan in plans.items():  # warm-up: the first step decides (public call), the second runs eagerly, the third captures
		for _ in range(3):
			plan.step()
		assert plan.check(), k
	warm_s = time.perf_counter() - t0
	ev = lambda: torch.cuda.Event(enable_timing=True)
	step_ms = {k: [] for k in sets}
	call_ms = {k: [] for k in sets}
	for _ in range(args.rounds):
		for k, plan in plans.items():
			torch.cuda.synchronize()
			e0, e1 = ev(), ev()
			e0.record()
			for _ in range(args.steps):
				plan.step()
			e1.record()
			torch.cuda.synchronize()
			step_ms[k].append(e0.elapsed_time(e1) / args.steps)
			assert plan.check() and plan.fallbacks == 0, k
		for k, dc in sets.items():
			for _ in range(args.calls):
				torch.cuda.synchronize()
				e0, e1 = ev(), ev()
				e0.record()
				out = association_tests_single4(dx, dy, dc, return_dot=False, device_out=True)
				e1.record()
				torch.cuda.synchronize()
				call_ms[k].append(e0.elapsed_time(e1))
				del out
	rec = dict(tool='time_single4_rank_deficient', shape=dict(nx=nx, ny=ny, n=n, dtype='float32'), device=torch.cuda.get_device_name(dev),
			   rounds=args.rounds, steps_per_round=args.steps, calls_per_round=args.calls, warmup_s=round(warm_s, 2))
	for k, plan in plans.items():
		rec[k] = dict(nc=int(sets[k].shape[0]), rank=int(getattr(plan, 'dcr', -1)), lean=bool(plan.lean), graph=plan._graph.graph is not None, fallbacks=plan.fallbacks,
					  step_ms_median=float(np.median(step_ms[k])), step_ms=[round(v, 4) for v in step_ms[k]],
					  call_ms_median=float(np.median(call_ms[k])), call_ms=[round(v, 3) for v in call_ms[k]])
	rec['step_ratio_c4_over_full'] = rec['c4_onehot']['step_ms_median'] / rec['full_rank']['step_ms_median']
	rec['call_ratio_c4_over_full'] = rec['c4_onehot']['call_ms_median'] / rec['full_rank']['call_ms_median']
	rec['guard'] = dict(eng.last_guard) if getattr(eng, 'last_guard', None) else None
	line = json.dumps(rec)
	print(line)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as f:
		f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
	main()
