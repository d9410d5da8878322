"""The resident single=1 step through the library's own plan handle (nrm_single1_plan_*, normalisr_amd/cplan.py: Single1Plan) against the step the project is quoted
on (normalisr_amd.single1.Single1Plan.step, what bench.py's de_c4_single1 times), at BASELINE configs[3] as bench.py builds it for single=1: 1000 gRNAs x 15 000 genes
x 50 000 cells fp32, five covariates, a low-MOI design (one entry in a thousand, seed 4).  Two kinds of child process, one on the GPU at a time, alternating
`--rounds` times:

  yardstick   imports torch; single1.Single1Plan on the matrices in HBM; `--warmup` steps, then `--reps` times `--steps` steps between two device events;
  c_plan      cannot import torch; cplan.Single1Plan on a plan-owned copy of the same values; the same warm-up, then `--reps` times Single1Plan.time(`--steps`)
              (nrm_single1_plan_time) -- without alpha or q --, and the same with q=True.

A child's figure is the median of its reps (ms per step).  The yardstick works at the level of association_tests: it runs neither de's re-inflation nor its
assertions, so the expectation is: the plan's median <= the yardstick's median + the yardstick's own min-max spread in this run + the time of the plan's own
kernel (k_s1_de_finish), which comes from a kernel trace of the c_plan child by itself (`--kernel-stats` names its CSV):
    python tools/time_single1_c_plan.py --child yardstick --data DIR/c4      (writes DIR/c4.*.npy, which the other child reads)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_single1_c_plan.py --child c_plan --data DIR/c4

Usage: time_single1_c_plan.py [--rounds 3] [--steps 20] [--reps 5] [--warmup 5] [--kernel-stats CSV] [--out profiles/single1_c_plan.json]"""
import json
import os
import sys

import numpy as np

import plan_timing as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX, NY, N, NC, SEED = 1000, 15000, 50000, 5, 4
OWN_KERNELS = ('k_s1_de_finish', )


def child_yardstick(args):
	import torch
	from normalisr_amd.single1 import Single1Plan
	dev = torch.device('cuda', 0)
	g = torch.Generator(device=dev)  # (bench.py: bench_de_method, single == 1, one rank)
	g.manual_seed(SEED)
	dc = torch.cat([torch.randn((NC - 1, N), generator=g, device=dev, dtype=torch.float32), torch.ones((1, N), device=dev, dtype=torch.float32)])
	dx = (torch.rand((NX, N), generator=g, device=dev) < 0.001).to(torch.float32)
	g2 = torch.Generator(device=dev)
	g2.manual_seed(SEED * 7919)
	dy = torch.randn((NY, N), generator=g2, device=dev, dtype=torch.float32)
	dy[:16] += 0.2 * dx[0]
	if not os.path.exists(args.data + '.dt.npy'):  # the values the other side reads
		np.save(args.data + '.dc.npy', dc.cpu().numpy())
		np.save(args.data + '.dg.npy', dx.cpu().numpy())
		np.save(args.data + '.dt.npy', dy.cpu().numpy())
	plan = Single1Plan(dx, dy, dc.cpu().numpy().astype(np.float64), return_dot=False)
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
	plan.check()
	return dict(ms_per_step=ms, cells_kept=plan.cells_kept())


def child_c_plan(args):
	sys.modules['torch'] = None  # `import torch` raises ImportError here
	from normalisr_amd import cplan
	dg, dt, dc = (np.load(args.data + '.{}.npy'.format(k)) for k in ('dg', 'dt', 'dc'))
	out = {}
	for key, q in (('step', False), ('step_q', True)):
		with cplan.Single1Plan(dg, dt, dc.astype(np.float64), q=q) as plan:
			for _ in range(args.warmup):
				plan.step()
			plan.check()
			out[key] = [plan.time(args.steps) for _ in range(args.reps)]
			plan.check()
			out[key + '_info'] = plan.info()
	assert sys.modules['torch'] is None
	return out


def main():
	args = pt.arg_parser('profiles/single1_c_plan.json', 420, warmup=5, kernel_stats=True).parse_args()
	if args.child:
		print(json.dumps(dict(yardstick=child_yardstick, c_plan=child_c_plan)[args.child](args)))
		return
	ys, cs = pt.alternate(__file__, args, ('yardstick', 'c_plan'), 'c4')
	y, c, cq = pt.side(ys, 'ms_per_step'), pt.side(cs, 'step'), pt.side(cs, 'step_q')
	c['info'], cq['info'] = cs[-1]['step_info'], cs[-1]['step_q_info']
	rec = dict(shape=dict(groupings=NX, genes=NY, cells=N, dtype='float32', covariates=NC, seed=SEED, cells_kept=ys[-1]['cells_kept']), rounds=args.rounds, steps=args.steps,
			   reps=args.reps, warmup=args.warmup,
			   yardstick=dict(what='normalisr_amd.single1.Single1Plan.step (torch), device events around the steps', **y),
			   c_plan=dict(what='cplan.Single1Plan.time without alpha or q: nrm_single1_plan_time, one hipGraphLaunch per step, no torch in the process', **c),
			   c_plan_q=dict(what='the same with q=True: nrm_bh over all P-values inside the step', **cq),
			   **pt.margin(y, c, OWN_KERNELS, args.kernel_stats))
	pt.write(rec, args.out)


if __name__ == '__main__':
	main()
