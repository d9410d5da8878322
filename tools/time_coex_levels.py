"""One more covariate on a resident co-expression problem (normalisr_amd.levels.CoexLevels) against coex from scratch on the same covariates, at 5000 genes x
10 000 cells, fp32 resident in HBM, in ONE process after warm-up, timed with device events.  Writes one JSON record (profiles/coex_levels.json).
  covariates   `c8`: four one-hot batches, three continuous columns and the intercept (the shape of tools/time_front.py's set);
               `c384`: the 384 rows of tools/time_wide_covariates.py (the level counts of the reference's co-expression example)
  per set      construction (K1 + the fp64 Gram kernel + the basis on the host) against coex from scratch; then, per repetition and alternated, (a) the state is put
               back to the build, one row -- a latent factor of the expression -- is appended and the results are taken: the whole `append + results` between two
               events, and inside it the spans of nrm_coex_project, nrm_coex_downdate and the K3 sweep; (b) coex(dt, enlarged covariates, device_out=True), the
               from-scratch path.  Both include their host part (the rank of the enlarged covariates: an SVD of the covariates' Gram matrix).
  bytes        what each kernel moves, computed from the shapes.
Nothing here is a pass / fail bound.
Usage: time_coex_levels.py [--genes G] [--cells N] [--reps R] [--warmup W] [--out profiles/coex_levels.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
	ms = np.asarray(ms, dtype=np.float64)
	return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), max_ms=round(float(ms.max()), 4),
				p10_ms=round(float(np.percentile(ms, 10)), 4), p90_ms=round(float(np.percentile(ms, 90)), 4), reps=int(ms.size))


def covariates8(n, seed, normcov):
	rng = np.random.default_rng(seed)
	batch = rng.integers(0, 4, n)
	onehot = (batch[None, :] == np.arange(4)[:, None]).astype(np.float64)
	cont = np.array([rng.normal(0, 1, n), rng.normal(100, 30, n), rng.normal(0.05, 0.01, n)])
	return normcov(np.vstack([onehot, cont]))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--genes', type=int, default=5000)
	ap.add_argument('--cells', type=int, default=10000)
	ap.add_argument('--reps', type=int, default=20)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--out', default='profiles/coex_levels.json')
	args = ap.parse_args()
	import torch
	import normalisr_amd.normalisr as norm
	from normalisr_amd import engine, levels
	from time_wide_covariates import covariates as covariates384
	ng, n = args.genes, args.cells
	eng = engine.get_engine()
	rec = dict(tool='time_coex_levels', device=torch.cuda.get_device_name(0), genes=ng, cells=n, dtype='float32', warmup=args.warmup, sets={})
	osz = 4
	rec['bytes'] = dict(project=ng * n * 4 + n * 8 + ng * 8, downdate=int((ng * ng / 2 + 32 * ng) * 16 + 3 * ng * 8), sweep=int(ng * ng / 2 * 8 + 2 * ng * ng * osz),
						from_scratch_k1=ng * n * 4 + ng * n * 8, note='project: X once, one direction; downdate: the upper tiles of G read and written; sweep: the upper '
						'triangle of G read, p and dot written in fp32; K1 of a from-scratch level at least reads X and writes its operand')

	def event_ms(fn):
		torch.cuda.synchronize()
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		t0 = time.perf_counter()
		e0.record()
		out = fn()
		e1.record()
		torch.cuda.synchronize()
		return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), out

	for name, dc in (('c8', covariates8(n, 11, norm.normcov)), ('c384', covariates384(n, 22, norm.normcov))):
		rng = np.random.default_rng(5)
		fac = rng.standard_normal((2, n))
		x = rng.standard_normal((ng, n)).astype(np.float32) + (rng.standard_normal((ng, 2)) * (rng.random((ng, 2)) < 0.3)).astype(np.float32) @ fac.astype(np.float32) + 3
		x += (rng.normal(0, 0.2, (ng, dc.shape[0])) @ dc).astype(np.float32)
		dt = eng.upload(x.astype(np.float32))
		del x
		row = fac[0] + 0.1 * rng.standard_normal(n)
		dc1 = np.concatenate([dc, row[None, :]])
		one = dict(covariates=int(dc.shape[0]))
		build, scratch0 = [], []
		for i in range(args.warmup + max(5, args.reps // 4)):
			ms, _, lv = event_ms(lambda: levels.CoexLevels(dt, dc))
			ms0, _, _ = event_ms(lambda: norm.coex(dt, dc, device_out=True))
			if i >= args.warmup:
				build.append(ms)
				scratch0.append(ms0)
		one['construction'] = stats(build)
		one['coex_from_scratch_level0'] = stats(scratch0)
		one['rank'] = lv.rank
		g0, ss0, b0, rank0, dcs0 = lv._g.clone(), lv._ss.clone(), lv._b, lv.rank, lv.dc
		whole, wall, spans, scratch, scratch_wall = [], [], dict(coex_project=[], coex_downdate=[], sweep=[]), [], []

		def step():
			lv.append(row)
			return lv.results(device_out=True)

		for i in range(args.warmup + args.reps):
			lv._g.copy_(g0)
			lv._ss.copy_(ss0)
			lv._b, lv.rank, lv.dc, lv._cache, lv.level, lv.rebuilt = b0, rank0, dcs0, None, 0, []
			eng.trace = []
			ms, w, _ = event_ms(step)
			trace, eng.trace = eng.trace, None
			assert lv.rebuilt == [False], lv.info
			ms1, w1, _ = event_ms(lambda: norm.coex(dt, dc1, device_out=True))
			if i >= args.warmup:
				whole.append(ms)
				wall.append(w)
				scratch.append(ms1)
				scratch_wall.append(w1)
				for k in spans:
					spans[k].append(sum(a.elapsed_time(b) for nm, a, b in trace if nm == k))
		one['append_and_results'] = stats(whole)
		one['append_and_results_wall'] = stats(wall)
		one['kernels'] = {k: stats(v) for k, v in spans.items()}
		one['coex_from_scratch'] = stats(scratch)
		one['coex_from_scratch_wall'] = stats(scratch_wall)
		one['speedup_median'] = round(one['coex_from_scratch']['median_ms'] / one['append_and_results']['median_ms'], 2)
		rec['sets'][name] = one
		del lv, g0, ss0, dt
		torch.cuda.empty_cache()
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as f:
		f.write(json.dumps(rec, indent=1) + '\n')
	print(json.dumps(rec))


if __name__ == '__main__':
	main()
