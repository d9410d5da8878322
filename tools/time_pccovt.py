"""pccovt and principal_genes on the device, in ONE process after warm-up, timed with device events.  Writes one JSON record (profiles/pccovt.json).
  pccovt            the whole call on an expression matrix resident in HBM (namet=None, integer rows, the result left in HBM), and its stages from the engine's
                    trace: gather, K1 (residualize), K2 (gram), the correlation matrix, the power iterations with their count, the score pass
  sizes             5000 genes x 10 000 cells, fp32, m = 200 chosen genes, 8 covariates (4 one-hot batches, 3 continuous, the intercept);
                    15 000 x 50 000, m = 500
  principal_genes   on 5000^2 and 30 000^2 boolean networks in HBM, and the degree pass alone
  bandwidth         for the score pass (one read of the m x n fp64 residual rows) and the degree pass (one read of the network): bytes over time as a share of 8 TB/s
  yardstick         the reference's pccovt on the first size on THIS machine's CPUs, only with --reference DIR (its source directory; the module it yields must
                    lie under DIR -- this build's own normalisr shim is never timed in its place -- and the record holds null otherwise); --reference-only
                    times it alone and merges the figure into an existing record.  A different machine: not a speed-up.
The expression is seeded noise plus a common factor of mixed sign in the chosen genes plus covariate effects, made on the device.

Usage: time_pccovt.py [--reps R] [--warmup W] [--out profiles/pccovt.json] [--small-only] [--reference DIR] [--reference-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (('5000x10000', 5000, 10000, 200), ('15000x50000', 15000, 50000, 500))
NETS = (5000, 30000)
HBM_BYTES_PER_S = 8e12
STAGES = ('pc_gather', 'residualize', 'gram', 'pc_correlation', 'pc_power', 'pc_score')


def covariates(n, seed):
	rng = np.random.default_rng(seed)
	batch = rng.integers(0, 4, n)
	cont = rng.normal(size=(3, n))
	cont = (cont - cont.mean(axis=1, keepdims=True)) / cont.std(axis=1, keepdims=True)
	return np.concatenate([(batch[None, :] == np.arange(4)[:, None]).astype(float), cont, np.ones((1, n))])


def chosen(ng, m, seed):
	return np.sort(np.random.default_rng(seed).permutation(ng)[:m]).astype(np.int64)


def expression_host(ng, n, m, seed):
	"""The first size on the host, for the reference (the device copy is made by the same formula from torch's generator: not the same numbers)."""
	rng = np.random.default_rng(seed)
	dc = covariates(n, seed)
	idx = chosen(ng, m, seed)
	x = rng.normal(size=(ng, n)).astype(np.float32)
	x[idx] += (0.5 * rng.choice([-1.0, 1.0], m)[:, None] * rng.normal(size=n)[None, :]).astype(np.float32)
	x += (rng.normal(0, 0.3, (ng, 8)) @ dc).astype(np.float32) + 5
	return x, dc, idx


def stats(ms):
	return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))


def reference_seconds(path):
	"""The reference's pccovt from the source directory path, timed once; None without --reference, or when what that directory yields is not the reference
	(this build's own shim answers to the same module name: it is never timed as the yardstick)."""
	if not path:
		return None
	import importlib
	path = os.path.realpath(path)
	kept = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'normalisr' or k.startswith('normalisr.')}
	sys.path.insert(0, path)
	try:
		mod = importlib.import_module('normalisr.gocovt')
		where = os.path.realpath(getattr(mod, '__file__', None) or '')
		if not where.startswith(path + os.sep) or mod.pccovt.__module__.startswith('normalisr_amd'):
			return None
		pccovt = mod.pccovt
	except ImportError:
		return None
	finally:
		sys.path.remove(path)
		for k in [k for k in sys.modules if k == 'normalisr' or k.startswith('normalisr.')]:
			del sys.modules[k]
		sys.modules.update(kept)
	_, ng, n, m = SIZES[0]
	x, dc, idx = expression_host(ng, n, m, 21)
	names = np.array(['G%05d' % i for i in range(ng)])
	t0 = time.perf_counter()
	out = pccovt(x, dc, names, list(names[idx]))
	return dict(seconds=round(time.perf_counter() - t0, 3), size=SIZES[0][0], genes_chosen=m, shape=list(out.shape), cpus=os.cpu_count(),
				note='the reference on the CPUs of the machine this record was merged on: another machine, not a speed-up')


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=50)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--out', default='profiles/pccovt.json')
	ap.add_argument('--small-only', action='store_true')
	ap.add_argument('--reference', default=None)
	ap.add_argument('--reference-only', action='store_true')
	args = ap.parse_args()
	if args.reference_only:
		rec = json.load(open(args.out))
		rec['reference_pccovt_cpu'] = reference_seconds(args.reference)
		json.dump(rec, open(args.out, 'w'), indent=1)
		print(json.dumps(rec['reference_pccovt_cpu']))
		return
	import torch
	from normalisr_amd import _lib, engine, gocovt
	eng = engine.get_engine()
	rec = dict(tool='time_pccovt', device=torch.cuda.get_device_name(0), warmup=args.warmup, hbm_bytes_per_s_assumed=HBM_BYTES_PER_S)

	def timed(fn, reps=args.reps):
		for _ in range(args.warmup):
			fn()
		ms = []
		for _ in range(reps):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record()
			fn()
			b.record()
			b.synchronize()
			ms.append(a.elapsed_time(b))
		return stats(ms)

	for name, ng, n, m in SIZES[:1 if args.small_only else 2]:
		gen = torch.Generator(device='cuda').manual_seed(21)
		dc = covariates(n, 21)
		idx = chosen(ng, m, 21)
		x = torch.randn((ng, n), generator=gen, device='cuda', dtype=torch.float32)
		factor = torch.randn((n, ), generator=gen, device='cuda', dtype=torch.float32)
		sign = torch.from_numpy(np.random.default_rng(21).choice([-0.5, 0.5], m).astype(np.float32)).cuda()
		x[torch.from_numpy(idx).cuda()] += sign[:, None] * factor[None, :]
		x += (torch.randn((ng, 8), generator=gen, device='cuda', dtype=torch.float32) * 0.3) @ torch.from_numpy(dc.astype(np.float32)).cuda() + 5
		call = lambda: gocovt.pccovt(x, dc, None, idx, device_out=True, return_info=True)
		out, info = call()
		r = dict(genes=ng, cells=n, dtype='float32', genes_chosen=m, covariates=8, power_iterations=info['iterations'], converged=info['converged'],
				 eigenvalue=info['eigenvalue'], call=timed(call))
		per = {k: [] for k in STAGES}
		for _ in range(args.reps):
			eng.trace = []
			call()
			torch.cuda.synchronize()
			once = {}
			for k, e0, e1 in eng.trace:  # (K1 runs twice in a call: a stage is the sum of its spans)
				once[k] = once.get(k, 0.0) + e0.elapsed_time(e1)
			for k in per:
				if k in once:
					per[k].append(once[k])
			eng.trace = None
		r['stages'] = {k: stats(v) for k, v in per.items() if v}
		kp = -(-n // 16) * 16
		score_bytes = m * kp * 8
		r['score_pass_bytes'] = score_bytes
		r['score_pass_share_of_hbm'] = round(score_bytes / (r['stages']['pc_score']['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
		r['score_pass_note'] = 'the span holds the sign kernel, the score kernel and the fold: three launches'
		rec[name] = r
		del x
		torch.cuda.empty_cache()
	for ng in NETS[:1 if args.small_only else 2]:
		gen = torch.Generator(device='cuda').manual_seed(ng)
		net = torch.rand((ng, ng), generator=gen, device='cuda') < 0.02
		deg = torch.empty((ng, ), dtype=torch.int64, device='cuda')
		r = dict(genes=ng, principal_genes_call=timed(lambda: gocovt.principal_genes(net, n=100)),
				 degree_pass=timed(lambda: _lib.check(eng.lib.nrm_net_degree(net.data_ptr(), ng, net.stride(0), deg.data_ptr(), eng._stream()))))
		assert torch.equal(deg, net.sum(dim=1))
		r['degree_pass_bytes'] = ng * ng
		r['degree_pass_share_of_hbm'] = round(ng * ng / (r['degree_pass']['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
		rec['principal_%d' % ng] = r
		del net
		torch.cuda.empty_cache()
	rec['reference_pccovt_cpu'] = reference_seconds(args.reference)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	json.dump(rec, open(args.out, 'w'), indent=1)
	print(json.dumps(rec))


if __name__ == '__main__':
	main()
