"""lcpm from SPARSE counts next to the dense route, in ONE process after warm-up (the companion of tools/time_front.py): 5000 genes x 10 000 cells at 1, 5,
10, 25 and 50 % stored entries from a seed, and 30 000 x 100 000 at 5 %.  Writes one JSON record.
  resident    lcpm(DeviceCSR, device_out=True, out_dtype=float32) and the dense route on the same counts resident as int32, alternating call by call,
              device events around each call (a call holds one small read-back and the host's table, so it is a call time, not the kernels' sum)
  from_host   lcpm(scipy csr, device_out=True, out_dtype=float32) through the CSR kernels (NRM_DEBUG lcpm_sparse=force) and densified on the host
              (lcpm_sparse=0: the code path every scipy.sparse input took before the CSR kernels existed), alternating, host clock around a call that ends in a
              synchronise.  The density at which the two cross is lcpm.SPARSE_MAX_DENSITY.
  peak memory torch.cuda.max_memory_allocated() of either resident route at the large shape, inputs included

Per-kernel times come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_front_sparse.py --profile-run
    python tools/time_front_sparse.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/front_half_sparse.json   (merges them; no GPU needed)

Usage: time_front_sparse.py [--reps R] [--host-reps H] [--warmup W] [--out profiles/front_half_sparse.json] [--no-large] [--profile-run] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NG, N, SEED = 5000, 10000, 19
DENSITIES = (0.01, 0.05, 0.10, 0.25, 0.50)
LARGE = (30000, 100000, 0.05)


def merge_kernel_stats(rec, path):
	out = {}
	for r in csv.DictReader(open(path)):
		name = r.get('Name') or ''
		if not any(k in name for k in ('k_lc_', 'k_lcs_')):
			continue
		out[name.replace('void ', '').split('(')[0]] = dict(calls=int(float(r.get('Calls') or 0)), avg_ms=round(float(r.get('AverageNs') or 0) / 1e6, 4))
	rec['kernels_at_5_percent'] = out
	return rec


def stats(ms):
	return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))


def set_route(mode):
	keep = [p for p in os.environ.get('NRM_DEBUG', '').split(',') if p.strip() and not p.strip().lower().startswith('lcpm_sparse=')]
	os.environ['NRM_DEBUG'] = ','.join(keep + ['lcpm_sparse=' + mode])


def device_counts(torch, nt, ns, density, seed, block=2500):
	"""(dense int32 tensor, DeviceCSR) of seeded counts made on the device block by block: a share `density` of the entries hold 1 .. 39."""
	from normalisr_amd.lcpm import DeviceCSR
	gen = torch.Generator(device='cuda')
	gen.manual_seed(seed)
	x = torch.empty((nt, ns), dtype=torch.int32, device='cuda')
	ptr, cols, vals = [torch.zeros(1, dtype=torch.int64, device='cuda')], [], []
	for r0 in range(0, nt, block):
		r1 = min(nt, r0 + block)
		keep = torch.rand((r1 - r0, ns), device='cuda', generator=gen) < density
		v = torch.randint(1, 40, (r1 - r0, ns), device='cuda', generator=gen, dtype=torch.int32) * keep
		x[r0:r1] = v
		ptr.append(keep.sum(dim=1))
		nz = keep.nonzero()
		cols.append(nz[:, 1].to(torch.int32))
		vals.append(v[keep])
		del keep, v, nz
	indptr = torch.cumsum(torch.cat(ptr), 0)
	return x, DeviceCSR(indptr, torch.cat(cols), torch.cat(vals), (nt, ns))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=30)
	ap.add_argument('--host-reps', type=int, default=5)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--out', default='profiles/front_half_sparse.json')
	ap.add_argument('--no-large', action='store_true')
	ap.add_argument('--profile-run', action='store_true', help='five calls of either resident route at 5 %% and nothing else: the run to put under the profiler')
	ap.add_argument('--kernel-stats', default=None)
	args = ap.parse_args()
	if args.kernel_stats:
		rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
		rec = merge_kernel_stats(rec, args.kernel_stats)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')
		print(json.dumps(rec['kernels_at_5_percent']))
		return
	import scipy.sparse
	import torch
	import normalisr_amd.normalisr as norm
	import normalisr_amd.lcpm as lcpm_mod

	def event_ms(fn):
		torch.cuda.synchronize()
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		e0.record()
		fn()
		e1.record()
		torch.cuda.synchronize()
		return e0.elapsed_time(e1)

	def host_ms(fn):
		torch.cuda.synchronize()
		t = time.perf_counter()
		fn()
		torch.cuda.synchronize()
		return 1e3 * (time.perf_counter() - t)

	def alternate(clock, fa, fb, reps):
		for _ in range(args.warmup):
			fa()
			fb()
		a, b = [], []
		for _ in range(reps):
			a.append(clock(fa))
			b.append(clock(fb))
		return stats(a), stats(b)

	ka = dict(device_out=True, out_dtype=np.float32)
	if args.profile_run:
		x, d = device_counts(torch, NG, N, 0.05, SEED)
		for _ in range(5):
			norm.lcpm(d, **ka)
			norm.lcpm(x, **ka)
		torch.cuda.synchronize()
		return
	rec = dict(tool='time_front_sparse', device=torch.cuda.get_device_name(0), warmup=args.warmup, shape=dict(genes=NG, cells=N), densities=[], threshold_before=lcpm_mod.SPARSE_MAX_DENSITY)
	for dens in DENSITIES:
		x, d = device_counts(torch, NG, N, dens, SEED + int(1000 * dens))
		a, b = norm.lcpm(d, **ka)[0], norm.lcpm(x, **ka)[0]
		same = bool(torch.allclose(a, b, rtol=0, atol=4e-6))  # (fp32 values up to 20: two units in the last place)
		sp, de = alternate(event_ms, lambda: norm.lcpm(d, **ka), lambda: norm.lcpm(x, **ka), args.reps)
		del a, b
		m = scipy.sparse.csr_matrix((d.data.cpu().numpy(), d.indices.cpu().numpy(), d.indptr.cpu().numpy()), shape=d.shape)

		def host_call(mode):
			def go():
				set_route(mode)
				norm.lcpm(m, **ka)
			return go
		hs, hd = alternate(host_ms, host_call('force'), host_call('0'), args.host_reps)
		ent = dict(density=dens, stored_entries=int(m.nnz), value_dtype_uploaded=str(lcpm_mod.canonical_csr(m)[2].dtype), results_agree=same,
				   resident=dict(csr=sp, dense=de, csr_over_dense=round(sp['median_ms'] / de['median_ms'], 3)),
				   from_host=dict(csr=hs, densified=hd, csr_over_densified=round(hs['median_ms'] / hd['median_ms'], 3)))
		print(json.dumps(ent), flush=True)
		rec['densities'].append(ent)
		del x, d, m
		torch.cuda.empty_cache()
	thr = 0.0
	for e in rec['densities']:  # (ascending)
		if e['from_host']['csr']['median_ms'] > e['from_host']['densified']['median_ms']:
			break
		thr = e['density']
	rec['from_host_threshold'] = dict(measured_threshold=thr, note='the highest measured density below the first at which the CSR route is slower than densifying on the '
									  'host; the highest measured if it never is')
	e5 = [e for e in rec['densities'] if e['density'] == 0.05][0]['resident']
	rec['resident_at_5_percent'] = dict(csr_minus_dense_ms=round(e5['csr']['median_ms'] - e5['dense']['median_ms'], 4), dense_spread_ms=round(e5['dense']['max_ms'] - e5['dense']['min_ms'], 4))
	if not args.no_large:
		nt, ns, dens = LARGE
		torch.cuda.empty_cache()
		x, d = device_counts(torch, nt, ns, dens, SEED + 7, block=1000)
		big = dict(genes=nt, cells=ns, density=dens, stored_entries=int(d.data.numel()))
		torch.cuda.synchronize()
		base = torch.cuda.memory_allocated()  # both inputs are resident: each route's peak is reported above the OTHER route's input
		dense_in, csr_in = x.numel() * 4, d.data.numel() * 8 + d.indptr.numel() * 8
		for name, src in (('csr', d), ('dense', x)):
			norm.lcpm(src, **ka)
			torch.cuda.synchronize()
			torch.cuda.empty_cache()
			torch.cuda.reset_peak_memory_stats()
			norm.lcpm(src, **ka)
			torch.cuda.synchronize()
			big[name + '_peak_bytes_with_its_input'] = int(torch.cuda.max_memory_allocated() - base + (csr_in if name == 'csr' else dense_in))
		sp, de = alternate(event_ms, lambda: norm.lcpm(d, **ka), lambda: norm.lcpm(x, **ka), max(3, args.reps // 6))
		big['resident'] = dict(csr=sp, dense=de, csr_over_dense=round(sp['median_ms'] / de['median_ms'], 3))
		big['input_bytes'] = dict(csr=int(csr_in), dense=int(dense_in), result_f32=int(nt * ns * 4))
		print(json.dumps(big), flush=True)
		rec['large'] = big
	print(json.dumps(rec))
	if args.out != '/dev/null':
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
	main()
