"""The resident de step through the library's own plan handle (nrm_de_plan_*, normalisr_amd/cplan.py: DePlan) against the step the project is quoted on
(normalisr_amd.distributed.DePlan.step, what bench.py's de_c4 times), at BASELINE configs[3]: 1000 gRNAs x 15 000 genes x 50 000 cells fp32, five covariates, the
design bench.py's de_c4 builds (seed 4).  Two kinds of child process, one on the GPU at a time, alternating `--rounds` times:

  yardstick   imports torch; distributed.DePlan on the matrices in HBM; `--warmup` steps, then `--reps` times `--steps` steps between two device events;
  c_plan      cannot import torch; cplan.DePlan on a plan-owned copy of the same values; the same warm-up, then `--reps` times DePlan.time(`--steps`) -- without alpha
              or q --, the same with q=True, and the cold step: set_design + step + check by the host's clock, alternating two designs.

A child's figure is the median of its reps (ms per step).  The yardstick writes none of de's full-size arrays and asserts nothing on the device, so the expectation is:
the plan's median <= the yardstick's median + the yardstick's own min-max spread in this run + the time of the plan's finish and bounds kernels, which comes from a
kernel trace of the c_plan child by itself (`--kernel-stats` names its CSV; profiles/de_plan_kernel_stats.csv):
    python tools/time_de_plan.py --child yardstick --data DIR/c4      (writes DIR/c4.*.npy, which the other child reads)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_de_plan.py --child c_plan --data DIR/c4

Usage: time_de_plan.py [--rounds 3] [--steps 20] [--reps 5] [--warmup 5] [--kernel-stats CSV] [--out profiles/de_plan.json]"""
import json
import os
import sys
import time

import numpy as np

import plan_timing as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX, NY, N, NC, SEED = 1000, 15000, 50000, 5, 4
OWN_KERNELS = ('k_de_inflate', 'k_de_varg', 'k_plan_var', 'k_de_bounds')


def child_yardstick(args):
	import torch
	from normalisr_amd import distributed as nd
	dev = torch.device('cuda', 0)
	g = torch.Generator(device=dev)  # (bench.py: bench_de, which == 'de_c4', one rank)
	g.manual_seed(SEED)
	dc = torch.cat([torch.randn((NC - 1, N), generator=g, device=dev, dtype=torch.float32), torch.ones((1, N), device=dev, dtype=torch.float32)])
	dx = (torch.rand((NX, N), generator=g, device=dev) < 0.01).to(torch.float32)
	g2 = torch.Generator(device=dev)
	g2.manual_seed(SEED * 7919)
	dy = torch.randn((NY, N), generator=g2, device=dev, dtype=torch.float32)
	dy[:16] += 0.2 * dx[0]
	if not os.path.exists(args.data + '.dt.npy'):  # the values the other side reads
		np.save(args.data + '.dc.npy', dc.cpu().numpy())
		np.save(args.data + '.dg.npy', dx.cpu().numpy())
		np.save(args.data + '.dt.npy', dy.cpu().numpy())
	plan = nd.DePlan(dx, dy, dc)
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
	return dict(ms_per_step=ms)


def child_c_plan(args):
	sys.modules['torch'] = None  # `import torch` raises ImportError here
	from normalisr_amd import cplan
	dg, dt, dc = (np.load(args.data + '.{}.npy'.format(k)) for k in ('dg', 'dt', 'dc'))
	out = {}
	for key, q in (('step', False), ('step_q', True)):
		with cplan.DePlan(dg, dt, dc, q=q) as plan:
			for _ in range(args.warmup):
				plan.step()
			back = plan.check()
			out[key] = [plan.time(args.steps) for _ in range(args.reps)]
			back += plan.check()
			out[key + '_info'] = dict(plan.info(), handed_back=back)
			if not q:  # the cold step: a new design every step
				dg2 = np.ascontiguousarray(dg[::-1])
				cold = []
				for i in range(max(args.reps, 2)):
					t0 = time.perf_counter()
					plan.set_design(dg2 if i % 2 == 0 else dg).step()
					plan.check()
					cold.append(1e3 * (time.perf_counter() - t0))
				out['cold'] = cold
	assert sys.modules['torch'] is None
	return out


def main():
	args = pt.arg_parser('profiles/de_plan.json', 420, warmup=5, kernel_stats=True).parse_args()
	if args.child:
		print(json.dumps(dict(yardstick=child_yardstick, c_plan=child_c_plan)[args.child](args)))
		return
	ys, cs = pt.alternate(__file__, args, ('yardstick', 'c_plan'), 'c4')
	y, c, cq, cold = pt.side(ys, 'ms_per_step'), pt.side(cs, 'step'), pt.side(cs, 'step_q'), pt.side(cs, 'cold')
	c['info'], cq['info'] = cs[-1]['step_info'], cs[-1]['step_q_info']
	rec = dict(shape=dict(groupings=NX, genes=NY, cells=N, dtype='float32', covariates=NC, seed=SEED), rounds=args.rounds, steps=args.steps, reps=args.reps, warmup=args.warmup,
			   yardstick=dict(what='normalisr_amd.distributed.DePlan.step (torch), device events around the steps', **y),
			   c_plan=dict(what='cplan.DePlan.time without alpha or q: nrm_de_plan_time, one hipGraphLaunch per step, no torch in the process', **c),
			   c_plan_q=dict(what='the same with q=True: nrm_bh over all P-values inside the step', **cq),
			   c_plan_cold=dict(what='set_design + step + check by the host clock, a new design every step', **cold),
			   **pt.margin(y, c, OWN_KERNELS, args.kernel_stats))
	pt.write(rec, args.out)


if __name__ == '__main__':
	main()
