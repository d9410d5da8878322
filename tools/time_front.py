"""The pipeline's front half at 5000 genes x 10 000 cells (int32 counts from a seed, resident in HBM; 8 covariates: 4 one-hot batches, lcpm's three and the
intercept) in ONE process, timed with device events after warm-up: lcpm (device in, device_out=True; fp32 and fp64 out), scaling_factor, compute_var
(stepmax=1), the resident chain reads -> lcpm -> normcov -> compute_var -> normvar, and -- the yardstick, on the same shape in the same run -- a NormvarPlan
step and a normvar(device_out=True) call: lcpm's lookup and write passes with fp32 output move the 12 bytes per element of an fp32 normvar (the count pass adds 4; normvar's output
is fp64, 16 bytes per element, when the covariates are).  Algorithmic bytes per stage come from
the shapes.  Writes one JSON record.

Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_front.py --reps 5 --out /dev/null
    python tools/time_front.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/front_half.json      (merges them into the record; no GPU needed)

Usage: time_front.py [--reps R] [--warmup W] [--out profiles/front_half.json] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NG, N, SEED = 5000, 10000, 18
HBM_BYTES_PER_S = 8e12
# the reference on the CPUs of the development container at this size (Poisson counts, 61 % zeros, 8 covariates): quoted, not measured by this tool
REFERENCE_CPU_S = dict(lcpm_nth8=1.24, compute_var=2.9)


def kernel_bytes(name):
	"""Algorithmic HBM bytes of one launch, from the kernel's name: every pass reads the matrix once (4-byte elements here) and the two writing passes store
	it once in their output type; what else a pass moves is O(cells) or O(genes) and left out.  None for the small kernels."""
	e = NG * N
	base = name.replace('void ', '').split('<')[0].split('(')[0].strip()
	targs = [a.strip() for a in name.split('<', 1)[1].split('>')[0].split(',')] if '<' in name else []
	if base in ('k_lc_count', 'k_lc_colsum', 'k_fv_moments', 'k_fv_genes', 'k_fv_cells', 'k_nv_moments'):
		return 4 * e
	if base in ('k_lc_write', 'k_nv_apply'):
		return 4 * e + (8 if targs[1] == 'double' else 4) * e
	return None


def merge_kernel_stats(rec, path):
	out = {}
	for r in csv.DictReader(open(path)):
		name = r.get('Name') or ''
		if not any(k in name for k in ('k_lc_', 'k_fv_', 'k_nv_')):
			continue
		avg_ms = float(r.get('AverageNs') or 0) / 1e6
		ent = dict(calls=int(float(r.get('Calls') or 0)), avg_ms=round(avg_ms, 4))
		nbytes = kernel_bytes(name)
		if nbytes is not None and avg_ms > 0:
			ent['algorithmic_bytes'] = nbytes
			ent['share_of_8TBps'] = round(nbytes / (avg_ms * 1e-3) / HBM_BYTES_PER_S, 3)
		out[name.replace('void ', '').split('(')[0]] = ent
	rec['kernels'] = out
	return rec


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=50)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--out', default='profiles/front_half.json')
	ap.add_argument('--kernel-stats', default=None)
	args = ap.parse_args()
	if args.kernel_stats:
		rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
		rec = merge_kernel_stats(rec, args.kernel_stats)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')
		print(json.dumps(rec['kernels']))
		return
	import torch
	import normalisr_amd.normalisr as norm
	from normalisr_amd.norm import NormvarPlan
	rng = np.random.default_rng(SEED)
	mu = np.exp(rng.normal(-1.0, 1.3, NG))
	depth = np.exp(rng.normal(0.0, 0.5, N))
	x = rng.poisson(mu[:, None] * depth[None, :]).astype(np.int32)
	empty = x.sum(axis=0) == 0
	x[0, empty] = 1
	batch = rng.integers(0, 4, N)
	onehot = (batch[None, :] == np.arange(4)[:, None]).astype(np.float64)
	reads = torch.as_tensor(x).cuda()

	def timed(fn):
		for _ in range(args.warmup):
			fn()
		ms = []
		for _ in range(args.reps):
			torch.cuda.synchronize()
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			fn()
			e1.record()
			torch.cuda.synchronize()
			ms.append(e0.elapsed_time(e1))
		return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))

	lc32, _, _, cov = norm.lcpm(reads, device_out=True, out_dtype=np.float32)
	dc = norm.normcov(np.vstack([onehot, cov]))
	sf = norm.scaling_factor(reads)
	w = norm.compute_var(lc32, dc)

	def chain():
		lc, _, _, cv = norm.lcpm(reads, device_out=True, out_dtype=np.float32)
		c = norm.normcov(np.vstack([onehot, cv]))
		return norm.normvar(lc, c, norm.compute_var(lc, c), norm.scaling_factor(reads), device_out=True)
	plan = NormvarPlan(lc32, dc, w, sf)
	e = NG * N
	rec = dict(tool='time_front', shape=dict(genes=NG, cells=N, counts='int32', covariates=int(dc.shape[0]), zero_fraction=round(float((x == 0).mean()), 3), max_count=int(x.max())),
			   device=torch.cuda.get_device_name(0), warmup=args.warmup,
			   lcpm_f32=timed(lambda: norm.lcpm(reads, device_out=True, out_dtype=np.float32)),
			   lcpm_f64=timed(lambda: norm.lcpm(reads, device_out=True)),
			   scaling_factor=timed(lambda: norm.scaling_factor(reads)),
			   compute_var=timed(lambda: norm.compute_var(lc32, dc)),
			   chain_to_normvar=timed(chain),
			   normvar_plan_step=timed(lambda: plan.step()),
			   normvar_call=timed(lambda: norm.normvar(lc32, dc, w, sf, device_out=True)),
			   algorithmic_bytes=dict(lcpm_f32=12 * e + 4 * e, lcpm_f64=12 * e + 8 * e, scaling_factor=4 * e, compute_var=12 * e, normvar=(8 + plan.out.element_size()) * e,
									  note='lcpm: three 4-byte reads (count, lookup, write passes) and one write per element; the count pass also serves scaling_factor'),
			   reference_cpu_s=dict(REFERENCE_CPU_S, note='quoted from the development container\'s CPUs, not measured in this run'))
	plan.check()
	for k in ('lcpm_f32', 'lcpm_f64', 'scaling_factor', 'compute_var'):
		rec[k]['share_of_8TBps'] = round(rec['algorithmic_bytes'][k] / (rec[k]['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
	rec['normvar_plan_step']['share_of_8TBps'] = round(rec['algorithmic_bytes']['normvar'] / (rec['normvar_plan_step']['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4)
	rec['lcpm_f32_over_normvar_call'] = round(rec['lcpm_f32']['median_ms'] / rec['normvar_call']['median_ms'], 3)
	print(json.dumps(rec))
	if args.out != '/dev/null':
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
	main()
