"""compute_var and normvar with hundreds of covariates on the device, in ONE process after warm-up, timed with device events.  Writes one JSON record
(profiles/wide_covariates.json).
  covariates   built like the reference's co-expression example (examples/GSE123139/code/prepare_raw.py:78-93): every level of the categorical columns a one-hot
               row -- the level counts of its `dysfunctional` subset, 164 + 164 + 19 + 25 + 4 + 2 + 2 = 380 --, three continuous rows, through normcov: 384 rows of
               rank 377
  size         5000 genes x 10 000 cells, fp32, resident in HBM
  compute_var  the whole call (stepmax 1 and 3: host numpy between the passes included) and the three streaming passes alone from the engine's trace
  normvar      normvar(device_out=True), the whole call, and the device part alone (weights, pair panels, Gram launches, Cholesky solves, the result pass)
  derived      the contraction's operations from the shapes (2 x genes x cells x r (r + 1) / 2) over the device part's time
  yardstick    the reference's normvar and compute_var on THIS machine's CPUs at --reference-genes x --reference-cells (a size it finishes), only with
               --reference DIR (its source directory); --reference-only times it alone and merges the figure into an existing record.  Another machine and another
               size: not a speed-up.
Usage: time_wide_covariates.py [--genes G] [--cells N] [--reps R] [--warmup W] [--out profiles/wide_covariates.json] [--reference DIR] [--reference-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = (164, 164, 19, 25, 4, 2, 2)


def covariates(n, seed, normcov):
	rng = np.random.default_rng(seed)
	rows = []
	for lv in LEVELS:
		f = rng.integers(0, lv, n)
		f[:lv] = np.arange(lv)
		rows.append((f[rng.permutation(n)][None, :] == np.arange(lv)[:, None]).astype(float))
	raw = np.concatenate(rows + [np.array([rng.normal(0, 1, n), rng.normal(100, 30, n), rng.normal(0.05, 0.01, n)])])
	return normcov(raw)


def expression_host(ng, n, dc, seed):
	rng = np.random.default_rng(seed)
	cell = np.exp(0.25 * (0.6 * dc[-2] + 0.4 * rng.normal(0, 1, n)))
	return (rng.normal(0, 1, (ng, n)) * cell + (rng.normal(0, 0.2, (ng, dc.shape[0])) @ dc) + 3.0).astype(np.float32)


def stats(ms):
	return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), max_ms=round(float(np.max(ms)), 3), reps=len(ms))


def reference_seconds(path, ng, n):
	"""The reference's compute_var(stepmax=3) and normvar from the source directory path at ng x n, timed once each; None without --reference or when the directory
	does not yield the reference (this build's own shim answers to the same module name: it is never timed as the yardstick)."""
	if not path:
		return None
	import importlib
	path = os.path.realpath(path)
	kept = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'normalisr' or k.startswith('normalisr.')}
	sys.path.insert(0, path)
	try:
		mod = importlib.import_module('normalisr.norm')
		where = os.path.realpath(getattr(mod, '__file__', None) or '')
		if not where.startswith(path + os.sep):
			return None
		dc = covariates(n, 22, mod.normcov)
		x = expression_host(ng, n, dc, 22).astype(np.float64)
		t0 = time.perf_counter()
		w = mod.compute_var(x, dc, stepmax=3)
		t1 = time.perf_counter()
		mod.normvar(x, dc, w, np.random.default_rng(22).uniform(0, 1, ng))
		t2 = time.perf_counter()
	except ImportError:
		return None
	finally:
		sys.path.remove(path)
		for k in [k for k in sys.modules if k == 'normalisr' or k.startswith('normalisr.')]:
			del sys.modules[k]
		sys.modules.update(kept)
	return dict(genes=ng, cells=n, covariates=int(dc.shape[0]), compute_var_stepmax3_seconds=round(t1 - t0, 3), normvar_seconds=round(t2 - t1, 3),
				normvar_seconds_per_gene=round((t2 - t1) / ng, 4), cpus=os.cpu_count(),
				note='the reference on the CPUs of the machine this record was merged on, at a size it finishes: another machine and size, not a speed-up')


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--genes', type=int, default=5000)
	ap.add_argument('--cells', type=int, default=10000)
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--warmup', type=int, default=1)
	ap.add_argument('--out', default='profiles/wide_covariates.json')
	ap.add_argument('--reference', default=None)
	ap.add_argument('--reference-only', action='store_true')
	ap.add_argument('--reference-genes', type=int, default=16)
	ap.add_argument('--reference-cells', type=int, default=1500)
	args = ap.parse_args()
	if args.reference_only:
		rec = json.load(open(args.out))
		rec['reference_cpu'] = reference_seconds(args.reference, args.reference_genes, args.reference_cells)
		json.dump(rec, open(args.out, 'w'), indent=1)
		print(json.dumps(rec['reference_cpu']))
		return
	import torch
	from normalisr_amd import engine, norm
	eng = engine.get_engine()
	ng, n = args.genes, args.cells
	dc = covariates(n, 22, norm.normcov)
	x = torch.as_tensor(expression_host(ng, n, dc, 22)).cuda()
	wt = np.random.default_rng(22).uniform(0, 1, ng)
	rec = dict(tool='time_wide_covariates', device=torch.cuda.get_device_name(0), genes=ng, cells=n, dtype='float32', covariates=int(dc.shape[0]), warmup=args.warmup)

	def timed(fn, span=None):
		"""Whole call between two device events (the call ends in a read-back, so the host's part is inside); span: the engine's trace entries of that name."""
		for _ in range(args.warmup):
			fn()
		ms, inner = [], []
		for _ in range(args.reps):
			eng.trace = []
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record()
			fn()
			b.record()
			b.synchronize()
			ms.append(a.elapsed_time(b))
			inner.append(sum(e0.elapsed_time(e1) for k, e0, e1 in eng.trace if k == span))
			eng.trace = None
		return stats(ms), stats(inner)

	for steps in (1, 3):
		call, passes = timed(lambda: norm.compute_var(x, dc, stepmax=steps), 'fitvar')
		rec['compute_var_stepmax%d' % steps] = dict(call=call, streaming_passes=passes)
	w = norm.compute_var(x, dc, stepmax=3)
	_, rank, certified, gaps = norm._wide_basis(dc, w, wt)
	call, device = timed(lambda: norm.normvar(x, dc, w, wt, device_out=True), 'normvar_wide')
	last = eng._normvar_wide_last
	flop = 2.0 * ng * n * (rank * (rank + 1) // 2 + rank)
	rec['normvar'] = dict(call=call, device_part=device, rank=int(rank), certified=bool(certified), lambda_r_over_lambda_1=gaps[0], lambda_r1_over_lambda_1=gaps[1], kappa=gaps[2],
						  gene_block=int(last['gene_block']), panel_rows=int(last['panel_rows']), contraction_flop=flop,
						  contraction_tflops_over_device_part=round(flop / (device['median_ms'] * 1e-3) / 1e12, 2),
						  note='device_part holds every kernel of the path, not the Gram launches alone: the rate is a lower bound of the contraction\'s')
	rec['reference_cpu'] = reference_seconds(args.reference, args.reference_genes, args.reference_cells)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	json.dump(rec, open(args.out, 'w'), indent=1)
	print(json.dumps(rec))


if __name__ == '__main__':
	main()
