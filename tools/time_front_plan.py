"""A step of the resident front-half plan (nrm_front_plan_*, normalisr_amd.cplan.FrontPlan: counts -> lcpm -> normcov -> compute_var -> scaling_factor -> normvar as
one HIP graph, no torch in the process) against the device-resident torch chain lcpm(device_out=True) -> normcov -> compute_var -> normvar(device_out=True), which
runs numpy and small copies between its launches, at 5000 genes x 10 000 cells int32 counts as tools/time_front.py builds them (seed 18), with 4 one-hot batches:
8 covariates in all.  Two kinds of child process, one on the GPU at a time, alternating `--rounds` times:

  yardstick   imports torch; the chain of tools/time_front.py (fp32 lcpm) on counts in HBM; `--warmup` calls, then `--reps` times `--steps` calls between two
              device events;
  c_plan      cannot import torch; cplan.FrontPlan(out_dtype=float32) on a plan-owned copy of the same counts; the same warm-up, then `--reps` times
              FrontPlan.time(`--steps`) (nrm_front_plan_time); and the same with fp64 output, the reference's, as a figure of its own.

A child's figure is the median of its reps (ms per step); the record holds, per side, the rounds' figures, their median and min-max spread.  There is no verdict
and no bar: the two numbers are compared within one run only.

--csr: the plan on sparse counts (cplan.FrontPlanCSR, nrm_front_plan_create_csr) against the dense plan instead, neither child able to import torch, on the same
counts (61 % zeros) and on a thinned matrix of the same shape with about 90 % zeros:

  dense_plan  cplan.FrontPlan(out_dtype=float32) on each matrix, timed as c_plan is;
  csr_plan    cplan.FrontPlanCSR(out_dtype=float32) on scipy.sparse.csr_matrix of each.

The record (profiles/front_plan_csr.json) holds both sides per matrix, their spreads and info()['bytes'] of every plan.  No bar here either.

Usage: time_front_plan.py [--csr] [--rounds 3] [--steps 20] [--reps 5] [--warmup 5] [--out profiles/front_plan.json | profiles/front_plan_csr.json]"""
import json
import os
import sys

import numpy as np

import plan_timing as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NG, N, SEED = 5000, 10000, 18


def problem():
	"""(counts int32, one-hot batches fp64): the matrix of tools/time_front.py."""
	rng = np.random.default_rng(SEED)
	mu = np.exp(rng.normal(-1.0, 1.3, NG))
	depth = np.exp(rng.normal(0.0, 0.5, N))
	x = rng.poisson(mu[:, None] * depth[None, :]).astype(np.int32)
	x[0, x.sum(axis=0) == 0] = 1
	batch = rng.integers(0, 4, N)
	return x, (batch[None, :] == np.arange(4)[:, None]).astype(np.float64)


def thinned(x, zeros=0.9):
	"""x with stored entries dropped at random until about `zeros` of the matrix is zero; every cell keeps a read."""
	rng = np.random.default_rng(SEED + 1)
	keep = (1.0 - zeros) / (x != 0).mean()
	y = np.where(rng.random(x.shape) < keep, x, 0).astype(x.dtype)
	y[0, y.sum(axis=0) == 0] = 1
	return y


MATRICES = ('counts', 'thinned')


def child_front(args, sparse):
	"""FrontPlan (sparse=False) or FrontPlanCSR on both matrices: ms per step of every rep, info() and the share of stored entries, per matrix."""
	sys.modules['torch'] = None  # `import torch` raises ImportError here
	import scipy.sparse
	from normalisr_amd import cplan
	x, onehot = problem()
	out = {}
	for name, m in zip(MATRICES, (x, thinned(x))):
		make = (lambda: cplan.FrontPlanCSR(scipy.sparse.csr_matrix(m), onehot, out_dtype=np.float32)) if sparse else (lambda: cplan.FrontPlan(m, onehot, out_dtype=np.float32))
		with make() as plan:
			for _ in range(args.warmup):
				plan.step()
			plan.check()
			out[name] = [plan.time(args.steps) for _ in range(args.reps)]
			plan.check()
			out[name + '_info'] = plan.info()
			out[name + '_stored'] = float((m != 0).mean())
	assert sys.modules['torch'] is None
	return out


def main_csr(args):
	ds, cs = pt.alternate(__file__, args, ('dense_plan', 'csr_plan'))
	rec = dict(tool='time_front_plan --csr', shape=dict(genes=NG, cells=N, counts='int32', user_covariates=4, covariates=8, seed=SEED, out_dtype='float32'), rounds=args.rounds,
			   steps=args.steps, reps=args.reps, warmup=args.warmup,
			   what=dict(dense_plan='cplan.FrontPlan(out_dtype=float32).time: nrm_front_plan_time, one hipGraphLaunch per step, no torch in the process',
						 csr_plan='cplan.FrontPlanCSR(out_dtype=float32).time on scipy.sparse.csr_matrix of the same counts: the same step with the CSR form of lcpm\'s three passes'),
			   matrices={}, note='no bar: the two sides are compared within this run only')
	for name in MATRICES:
		d, c = pt.side(ds, name), pt.side(cs, name)
		d['info'], c['info'] = ds[-1][name + '_info'], cs[-1][name + '_info']
		rec['matrices'][name] = dict(stored_share=round(ds[-1][name + '_stored'], 4), dense_plan=d, csr_plan=c,
									 spreads_ms=dict(dense_plan=round(d['max_ms'] - d['min_ms'], 4), csr_plan=round(c['max_ms'] - c['min_ms'], 4)),
									 bytes=dict(dense_plan=d['info']['bytes'], csr_plan=c['info']['bytes']))
	pt.write(rec, args.out)


def child_yardstick(args):
	import torch
	import normalisr_amd.normalisr as norm
	x, onehot = problem()
	reads = torch.as_tensor(x).cuda()

	def chain():
		lc, _, _, cv = norm.lcpm(reads, device_out=True, out_dtype=np.float32)
		c = norm.normcov(np.vstack([onehot, cv]))
		return norm.normvar(lc, c, norm.compute_var(lc, c), norm.scaling_factor(reads), device_out=True)
	for _ in range(args.warmup):
		chain()
	torch.cuda.synchronize()
	ms = []
	for _ in range(args.reps):
		t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		t0.record()
		for _ in range(args.steps):
			chain()
		t1.record()
		t1.synchronize()
		ms.append(t0.elapsed_time(t1) / args.steps)
	return dict(ms_per_step=ms)


def child_c_plan(args):
	sys.modules['torch'] = None  # `import torch` raises ImportError here
	from normalisr_amd import cplan
	x, onehot = problem()
	out = {}
	for key, dtype in (('ms_per_step', np.float32), ('ms_per_step_f64', np.float64)):
		with cplan.FrontPlan(x, onehot, out_dtype=dtype) as plan:
			for _ in range(args.warmup):
				plan.step()
			plan.check()
			out[key] = [plan.time(args.steps) for _ in range(args.reps)]
			plan.check()
			out['info' if dtype == np.float32 else 'info_f64'] = plan.info()
	assert sys.modules['torch'] is None
	return out


def main():
	ap = pt.arg_parser('profiles/front_plan.json', 300)
	ap.add_argument('--csr', action='store_true', help='FrontPlanCSR against FrontPlan on two matrices -> profiles/front_plan_csr.json')
	args = ap.parse_args()
	if args.child:
		kinds = dict(yardstick=child_yardstick, c_plan=child_c_plan, dense_plan=lambda a: child_front(a, False), csr_plan=lambda a: child_front(a, True))
		print(json.dumps(kinds[args.child](args)))
		return
	if args.csr:
		if args.out == 'profiles/front_plan.json':
			args.out = 'profiles/front_plan_csr.json'
		return main_csr(args)
	ys, cs = pt.alternate(__file__, args, ('yardstick', 'c_plan'))
	y, c, c64 = pt.side(ys, 'ms_per_step'), pt.side(cs, 'ms_per_step'), pt.side(cs, 'ms_per_step_f64')
	c['info'], c64['info'] = cs[-1]['info'], cs[-1]['info_f64']
	rec = dict(tool='time_front_plan', shape=dict(genes=NG, cells=N, counts='int32', user_covariates=4, covariates=8, seed=SEED), rounds=args.rounds, steps=args.steps, reps=args.reps,
			   warmup=args.warmup,
			   yardstick=dict(what='lcpm(device_out=True, fp32) -> normcov -> compute_var -> scaling_factor -> normvar(device_out=True) with torch, device events around the calls', **y),
			   c_plan=dict(what='cplan.FrontPlan(out_dtype=float32).time: nrm_front_plan_time, one hipGraphLaunch per step, no torch in the process', **c),
			   c_plan_f64=dict(what='the same with fp64 lcpm and dtn, the reference\'s output type', **c64),
			   spreads_ms=dict(yardstick=round(y['max_ms'] - y['min_ms'], 4), c_plan=round(c['max_ms'] - c['min_ms'], 4), c_plan_f64=round(c64['max_ms'] - c64['min_ms'], 4)),
			   note='no bar: the two sides are compared within this run only')
	pt.write(rec, args.out)


if __name__ == '__main__':
	main()
