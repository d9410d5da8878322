"""bh over a resident 1000 x 15 000 result matrix (a CRISPR screen's de step: 1000 gRNAs x 15 000 genes, 1.5e7 P-values) in ONE process, after warm-up: nrm_bh on
the matrix in HBM (HIP events around the call; fp32 and fp64) and, beside it, the only route there was before -- the host binnet.bh on the same bytes (wall clock;
the download that precedes it timed separately).  The P-values are de's own: the seeded association_tests call de makes, of a 1000-row gRNA incidence design against 15 000 genes at a small
cell count (256 cells, 2 covariates, fp64), device_out=True -- the whole matrix, nothing tiled; the fp32 case is that matrix rounded to fp32.  --pvalues loguniform takes log-uniform P-values over 30 decades instead.
Writes one JSON record.  The kernels are launches of one entry, so the per-kernel rows come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_bh.py --reps 5 --host-reps 0 --out /dev/null
    python tools/time_bh.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/bh.json      (merges them into the record; no GPU needed)

Usage: time_bh.py [--reps R] [--warmup W] [--host-reps H] [--pvalues de|loguniform] [--out profiles/bh.json] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NX, NY, CELLS, SEED = 1000, 15000, 256, 23


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=20)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--host-reps', type=int, default=2)
	ap.add_argument('--pvalues', default='de', choices=('de', 'loguniform'))
	ap.add_argument('--out', default='profiles/bh.json')
	ap.add_argument('--kernel-stats', default=None)
	args = ap.parse_args()
	if args.kernel_stats:
		rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
		rec['kernels'] = {}
		for r in csv.DictReader(open(args.kernel_stats)):
			name = r.get('Name') or ''
			if 'k_bh_' in name:
				rec['kernels'][name.replace('void ', '').split('(')[0]] = dict(calls=int(float(r.get('Calls') or 0)), avg_ms=round(float(r.get('AverageNs') or 0) / 1e6, 5),
																				 total_ms=round(float(r.get('TotalDurationNs') or 0) / 1e6, 4))
		rec['kernels_note'] = 'rocprofv3 --kernel-trace --stats over a run of its own (both dtypes, warm-up included): calls, mean and total time per kernel'
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')
		print(json.dumps(rec['kernels']))
		return
	import torch
	from normalisr_amd import _lib, binnet, engine
	from normalisr_amd.association import association_tests
	eng = engine.get_engine()
	lib = eng.lib
	rng = np.random.default_rng(SEED)

	def stats(ms):
		return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))

	rec = dict(tool='time_bh', device=torch.cuda.get_device_name(0), warmup=args.warmup, shape=dict(rows=NX, cols=NY, entries=NX * NY), cases={},
			   tile=int(lib.nrm_bh_tile()),
			   note='device: nrm_bh on the resident matrix, HIP events around the call (launches included); host: binnet.bh (numpy) on the same bytes, wall clock on this '
					'machine\'s CPU; download: engine.download of the matrix, what the host route pays first')
	p64 = None
	for name, odt in (('fp32', np.float32), ('fp64', np.float64)):
		if args.pvalues == 'de':
			if p64 is None:  # one fp64 de call; the fp32 case takes its P-values rounded to fp32 on the device
				design = (rng.random((NX, CELLS)) < 0.05).astype(np.float64)
				design[:, 0], design[:, 1] = 1, 0  # (every gRNA varies)
				exp = rng.normal(size=(NY, CELLS))
				cov = np.vstack([np.ones(CELLS), rng.normal(size=CELLS)])
				p64 = association_tests(design, exp, cov, return_dot=False, device_out=True)[0]  # (de's own call, with the result left in HBM)
				assert p64.is_cuda and p64.dtype == torch.float64
			d_p = p64 if odt == np.float64 else p64.to(torch.float32)
			source = 'association_tests as de calls it (design {}x{} at 5% density, expression {}x{}, 2 covariates, fp64, seed {}), device_out=True{}'.format(
				NX, CELLS, NY, CELLS, SEED, '' if odt == np.float64 else ', rounded to fp32 on the device')
		else:
			d_p = eng.upload((10.0 ** (-30 * rng.random((NX, NY)))).astype(odt))
			source = 'log-uniform over 30 decades, seed {}'.format(SEED)
		assert tuple(d_p.shape) == (NX, NY) and d_p.is_contiguous()
		code = _lib.NRM_F64 if odt == np.float64 else _lib.NRM_F32
		nbytes = int(lib.nrm_bh_workspace_bytes(NX * NY, code))
		work = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
		out = torch.empty_like(d_p)
		flags = torch.zeros(2, dtype=torch.int32, device=eng.device)

		def step():
			_lib.check(lib.nrm_bh(d_p.data_ptr(), code, NX, NY, NY, out.data_ptr(), NY, work.data_ptr(), nbytes, flags.data_ptr(), eng._stream()))
		for _ in range(args.warmup):
			step()
		ms = []
		for _ in range(args.reps):
			torch.cuda.synchronize()
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record()
			step()
			e1.record()
			torch.cuda.synchronize()
			ms.append(e0.elapsed_time(e1))
		case = dict(pvalues=source, device=stats(ms), workspace_mb=round(nbytes / 2**20, 1), flags=flags.tolist())
		if args.host_reps:
			dl, host = [], []
			for _ in range(args.host_reps):
				torch.cuda.synchronize()
				t0 = time.perf_counter()
				h = eng.download(d_p)
				t1 = time.perf_counter()
				q = binnet.bh(h.ravel())
				t2 = time.perf_counter()
				dl.append((t1 - t0) * 1e3), host.append((t2 - t1) * 1e3)
			case.update(download=stats(dl), host=stats(host), identical_bytes=bool(np.array_equal(out.cpu().numpy().ravel().view(np.uint8), q.view(np.uint8))),
						distinct_values=int(np.unique(h).size))
		rec['cases'][name] = case
		del work, out
	print(json.dumps(rec))
	if args.out != '/dev/null':
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
	main()
