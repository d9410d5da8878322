"""A step of norm.ComputeVarPlan with hundreds of covariates (orthonormal bases from the host once; per iteration (B u)(B u)^T on the fp64 matrix cores, its inverse by
csrc/nrm_chol_inverse.hip, the streaming passes, the second regression -- all stepmax iterations and the weights one HIP graph) against the public call
norm.compute_var(device tensor), which runs a 384 x 384 SVD, three uploads and a read-back on the host in every iteration.  5000 genes x 10 000 cells fp32 resident
in HBM, the 384 covariates (rank 377) of tools/time_wide_covariates.py, stepmax 1 and 3.  Three kinds of child process, one on the GPU at a time, the first two
alternating `--rounds` times:

  public   `--warmup` calls of compute_var(x, dc, stepmax), then `--reps` times `--steps` calls between two device events (every call ends in a read-back, so the
           host's part is inside);
  plan     ComputeVarPlan(x, dc, stepmax): the same warm-up (the second step captures the graph), then `--reps` times `--steps` steps between two device events,
           check() after them;
  chol     nrm_chol_inverse alone at r = 377 and 1024 on a seeded positive definite matrix: `--reps` times `--steps` calls (4 ceil(r / 64) - 1 launches each) back to
           back between two device events -- the launch sequence's time on the device, the gaps between its launches included.

A child's figure is the median of its reps (ms per step or per call); the record holds, per side, the rounds' figures, their median and min-max spread.  No verdict
and no bar: the sides are compared within one run only.

Usage: time_compute_var_plan_wide.py [--rounds 3] [--steps 10] [--reps 5] [--warmup 3] [--out profiles/compute_var_plan_wide.json]"""
import json
import os
import sys

import numpy as np

import plan_timing as pt
from time_wide_covariates import covariates, expression_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NG, N, SEED = 5000, 10000, 22
STEPMAX = (1, 3)
CHOL_R = (377, 1024)


def problem(torch, norm):
	dc = covariates(N, SEED, norm.normcov)
	return torch.as_tensor(expression_host(NG, N, dc, SEED)).cuda(), dc


def per_step_ms(torch, fn, args):
	for _ in range(args.warmup):
		fn()
	torch.cuda.synchronize()
	ms = []
	for _ in range(args.reps):
		t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		t0.record()
		for _ in range(args.steps):
			fn()
		t1.record()
		t1.synchronize()
		ms.append(t0.elapsed_time(t1) / args.steps)
	return ms


def child_public(args):
	import torch
	from normalisr_amd import norm
	x, dc = problem(torch, norm)
	return {'stepmax%d' % s: per_step_ms(torch, lambda: norm.compute_var(x, dc, stepmax=s), args) for s in STEPMAX}


def child_plan(args):
	import torch
	from normalisr_amd import norm
	x, dc = problem(torch, norm)
	out = {}
	for s in STEPMAX:
		plan = norm.ComputeVarPlan(x, dc, stepmax=s)
		out['stepmax%d' % s] = per_step_ms(torch, plan.step, args)
		w = plan.results()  # (check(): the counters of every step above)
		out['stepmax%d_info' % s] = dict(rank=int(plan.rank), steps_taken=int(plan.steps_taken), graph=bool(plan._graph.graph is not None),
										 max_rel_diff_to_public=float(np.abs(w / norm.compute_var(x, dc, stepmax=s) - 1).max()))
	return out


def child_chol(args):
	import torch
	from normalisr_amd import _lib
	lib = _lib.load()
	out = {}
	for r in CHOL_R:
		rng = np.random.default_rng(SEED + r)
		q = np.linalg.qr(rng.normal(size=(r, r)))[0]
		m = (q * np.exp(-np.log(1e4) * rng.permutation(r) / (r - 1))) @ q.T
		d_m = torch.as_tensor((m + m.T) / 2).cuda()
		d_inv = torch.empty((r, r), dtype=torch.float64, device='cuda')
		ws = torch.empty((int(lib.nrm_chol_inverse_workspace(r)), ), dtype=torch.float64, device='cuda')
		status = torch.zeros((2, ), dtype=torch.int32, device='cuda')
		st = torch.cuda.current_stream().cuda_stream
		out['r%d' % r] = per_step_ms(torch, lambda: _lib.check(lib.nrm_chol_inverse(d_m.data_ptr(), r, r, d_inv.data_ptr(), r, ws.data_ptr(), status.data_ptr(), st)), args)
		assert not status.cpu().numpy().any()
		out['r%d_launches' % r] = 4 * (-(-r // 64)) - 1
	return out


def main():
	ap = pt.arg_parser('profiles/compute_var_plan_wide.json', 600, warmup=3, steps=10)
	args = ap.parse_args()
	if args.child:
		print(json.dumps(dict(public=child_public, plan=child_plan, chol=child_chol)[args.child](args)))
		return
	pub, plan = pt.alternate(__file__, args, ('public', 'plan'))
	chol = [pt.run_child(__file__, 'chol', args)]
	rec = dict(tool='time_compute_var_plan_wide', shape=dict(genes=NG, cells=N, dtype='float32', covariates=384, seed=SEED), rounds=args.rounds, steps=args.steps, reps=args.reps,
			   warmup=args.warmup,
			   what=dict(public='norm.compute_var(device tensor, dc, stepmax): device events around the calls, the host\'s SVD, uploads and read-back inside',
						 plan='norm.ComputeVarPlan(device tensor, dc, stepmax).step(): one graph launch per step, device events around the steps',
						 chol_inverse='nrm_chol_inverse alone, calls back to back on one stream, device events around them: ms per call, launch gaps included'),
			   note='no bar: the sides are compared within this run only')
	for s in STEPMAX:
		k = 'stepmax%d' % s
		y, c = pt.side(pub, k), pt.side(plan, k)
		c['info'] = plan[-1][k + '_info']
		rec[k] = dict(public=y, plan=c, spreads_ms=dict(public=round(y['max_ms'] - y['min_ms'], 4), plan=round(c['max_ms'] - c['min_ms'], 4)))
	rec['chol_inverse'] = {('r%d' % r): dict(launches=chol[0]['r%d_launches' % r], **pt.side(chol, 'r%d' % r)) for r in CHOL_R}
	pt.write(rec, args.out)


if __name__ == '__main__':
	main()
