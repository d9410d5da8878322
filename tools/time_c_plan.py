"""The resident coex step through the library's own plan handle (nrm_coex_plan_*, normalisr_amd/cplan.py) against the step the project is quoted on
(normalisr_amd.distributed.CoexPlan.step, what bench.py times), at BASELINE configs[1]: 5000 genes x 10 000 cells fp32 with the covariates of bench.py's headline
(bench.synth_c2, seed 2).  Two kinds of child process, one on the GPU at a time, alternating `--rounds` times:

  yardstick   imports torch; distributed.CoexPlan on the matrix in HBM; `--warmup` steps, then `--reps` times `--steps` steps between two device events;
  c_plan      cannot import torch; cplan.CoexPlan on a plan-owned copy of the same values; the same warm-up, then `--reps` times CoexPlan.time(`--steps`).

A child's figure is the median of its reps (ms per step); the record holds, per side, the rounds' figures, their median and min-max, the plan's info() and the
guard's worst bound, and the verdict: the C plan's median is at most the yardstick's median plus the yardstick's own min-max spread in this run.

Per-kernel times come from a kernel trace of each child by itself (profiles/c_plan_kernel_stats.csv, profiles/c_plan_yardstick_kernel_stats.csv):
    python tools/time_c_plan.py --child yardstick --data DIR/c2      (writes DIR/c2.dt.npy and DIR/c2.dc.npy, which the other child reads)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_c_plan.py --child c_plan --data DIR/c2

Usage: time_c_plan.py [--rounds 3] [--steps 20] [--reps 5] [--warmup 5] [--out profiles/c_plan.json]"""
import json
import os
import sys

import numpy as np

import plan_timing as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NG, N, SEED = 5000, 10000, 2


def child_yardstick(args):
	import torch
	import bench
	from normalisr_amd import distributed as nd
	dev = torch.device('cuda', 0)
	dt, dc = bench.synth_c2(NG, N, SEED, dev, torch)
	if not os.path.exists(args.data + '.dt.npy'):  # the values the other side reads
		np.save(args.data + '.dc.npy', dc.cpu().numpy())
		np.save(args.data + '.dt.npy', dt.cpu().numpy())
	plan = nd.CoexPlan(dt, dc)
	for _ in range(args.warmup):
		plan.step()
	torch.cuda.synchronize()
	ms = []
	for _ in range(args.reps):
		t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		t0.record()
		for _ in range(args.steps):
			plan.step()
		t1.record()
		t1.synchronize()
		ms.append(t0.elapsed_time(t1) / args.steps)
	flags = np.zeros(4, dtype=np.int32) if plan.flags is None else np.ascontiguousarray(plan.flags.cpu().numpy()[:4], dtype=np.int32)  # (the counters of all steps so far)
	return dict(ms_per_step=ms, guard_hits=int(flags[2]), guard_worst=float(flags[3:4].view(np.float32)[0]))


def child_c_plan(args):
	sys.modules['torch'] = None  # `import torch` raises ImportError here
	from normalisr_amd import cplan
	dt, dc = np.load(args.data + '.dt.npy'), np.load(args.data + '.dc.npy')
	with cplan.CoexPlan(dt, dc) as plan:
		for _ in range(args.warmup):
			plan.step()
		plan.check()
		ms = [plan.time(args.steps) for _ in range(args.reps)]
		hits, worst = plan.check()
		info = plan.info()
	assert sys.modules['torch'] is None
	return dict(ms_per_step=ms, guard_hits=hits, guard_worst=worst, info=info)


def with_guard(runs):
	return dict(pt.side(runs, 'ms_per_step'), guard_hits=[r['guard_hits'] for r in runs], guard_worst=max(r['guard_worst'] for r in runs))


def main():
	args = pt.arg_parser('profiles/c_plan.json', 240).parse_args()
	if args.child:
		print(json.dumps(dict(yardstick=child_yardstick, c_plan=child_c_plan)[args.child](args)))
		return
	ys, cs = pt.alternate(__file__, args, ('yardstick', 'c_plan'), 'c2')
	y, c = with_guard(ys), with_guard(cs)
	c['info'] = cs[-1]['info']
	spread = y['max_ms'] - y['min_ms']
	rec = dict(shape=dict(genes=NG, cells=N, dtype='float32', covariates=3, seed=SEED), rounds=args.rounds, steps=args.steps, reps=args.reps, warmup=args.warmup,
			   yardstick=dict(what='normalisr_amd.distributed.CoexPlan.step (torch), device events around the steps', **y),
			   c_plan=dict(what='cplan.CoexPlan.time: nrm_coex_plan_time, one hipGraphLaunch per step, no torch in the process', **c),
			   margin_ms=round(spread, 4), within_margin=bool(c['median_ms'] <= y['median_ms'] + spread))
	pt.write(rec, args.out)


if __name__ == '__main__':
	main()
