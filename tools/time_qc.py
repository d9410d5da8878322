"""Quality control on the device next to its yardsticks, in ONE process after warm-up: 5000 genes x 10 000 cells of seeded counts, resident as dense int32 and
as CSR.  Writes one JSON record (profiles/qc.json).
  stats pass   nrm_qc_stats / nrm_qc_csr_stats with every gene and cell alive, and again with the masks qc_reads ends with: device events around the launch
  qc_reads     the whole call (statistics, decision and one read-back of four integers per iteration; index arrays left in HBM), with its iteration count
  subset       the survivors cut out: the dense gather and the CSR count / scan / write, results left in HBM
  yardsticks   the lcpm count pass (nrm_lcpm_count / nrm_lcpm_csr_count) over the same bytes, timed here the same way -- profiles/front_half.json has 0.052 ms
               for its dense kernel alone --, and the reference's qc_reads on the same matrix on this machine's CPUs, when the reference can be imported
               (--reference DIR adds its source directory to the path; --reference-only times it alone and merges the figure into an existing record).
The thresholds are the reference's defaults for 10x data (--gene_cell_count 50, --gene_cell_prop 0.02, --cell_read_count 500, --cell_gene_count 100), the two
cell bounds scaled by 5000 / 20 000 genes: (0, 50, 0.02, 125, 25, 0).

Usage: time_qc.py [--reps R] [--warmup W] [--out profiles/qc.json] [--reference DIR] [--reference-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NG, N, SEED = 5000, 10000, 20
PARAMS = (0, 50, 0.02, 125, 25, 0)


def counts():
	rng = np.random.default_rng(SEED)
	mu = np.exp(rng.normal(-1.0, 1.6, NG))
	depth = np.exp(rng.normal(0.0, 0.9, N))
	return rng.poisson(mu[:, None] * depth[None, :]).astype(np.int32)


def stats(ms):
	return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))


def reference_seconds(x, path):
	if path:
		sys.path.insert(0, path)
	try:
		from normalisr.qc import qc_reads
	except ImportError:
		return None
	t0 = time.perf_counter()
	g, c = qc_reads(x.astype(np.int64), *PARAMS)
	return dict(seconds=round(time.perf_counter() - t0, 3), genes=int(len(g)), cells=int(len(c)), cpus=os.cpu_count())


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=30)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--out', default='profiles/qc.json')
	ap.add_argument('--reference', default=None)
	ap.add_argument('--reference-only', action='store_true')
	args = ap.parse_args()
	x = counts()
	if args.reference_only:
		rec = json.load(open(args.out))
		rec['reference_qc_reads_cpu'] = reference_seconds(x, args.reference)
		json.dump(rec, open(args.out, 'w'), indent=1)
		print(json.dumps(rec['reference_qc_reads_cpu']))
		return
	import scipy.sparse
	import torch
	from normalisr_amd import _lib, engine, lcpm, qc
	eng = engine.get_engine()
	m = scipy.sparse.csr_matrix(x)
	dense = eng.upload(x)
	csr = lcpm.DeviceCSR(eng.upload(m.indptr.astype(np.int64)), eng.upload(m.indices.astype(np.int32)), eng.upload(m.data.astype(np.int32)), m.shape)
	rec = dict(tool='time_qc', shape=dict(genes=NG, cells=N, counts='int32', zero_fraction=round(float((x == 0).mean()), 3), max_count=int(x.max()), stored_entries=int(m.nnz)),
			   thresholds=list(PARAMS), device=torch.cuda.get_device_name(0), warmup=args.warmup)

	def timed(fn):
		for _ in range(args.warmup):
			fn()
		ms = []
		for _ in range(args.reps):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record()
			fn()
			b.record()
			b.synchronize()
			ms.append(a.elapsed_time(b))
		return stats(ms)

	for name, src in (('dense', dense), ('csr', csr)):
		genes, cells, info = qc.qc_reads(src, *PARAMS, device_out=True, return_info=True)
		r = dict(iterations=info['iterations'], genes_kept=int(genes.numel()), cells_kept=int(cells.numel()))
		st = qc._Stats(eng, qc._counts_on_device(eng, src))
		r['stats_pass_all_alive'] = timed(st.stats)
		st.gene_alive.copy_(info['gene_mask'].to(torch.uint8))
		st.cell_alive.copy_(info['cell_mask'].to(torch.uint8))
		r['stats_pass_final_masks'] = timed(st.stats)
		r['qc_reads_call'] = timed(lambda: qc.qc_reads(src, *PARAMS, device_out=True))
		r['subset'] = timed(lambda: qc.subset(src, genes, cells))
		# the yardstick: lcpm's count pass over the same bytes
		cnt = torch.zeros((2 * N + NG + 4, ), dtype=torch.int64, device='cuda')
		out = (cnt[:N].data_ptr(), cnt[N:2 * N].data_ptr(), cnt[2 * N:2 * N + NG].data_ptr(), cnt[2 * N + NG:].data_ptr())
		if name == 'dense':
			part = torch.empty((int(eng.lib.nrm_lcpm_count_workspace(NG, N)), ), dtype=torch.int64, device='cuda')
			r['lcpm_count_pass'] = timed(lambda: _lib.check(eng.lib.nrm_lcpm_count(dense.data_ptr(), _lib.NRM_I32, NG, N, dense.stride(0), *out, part.data_ptr(), eng._stream())))
		else:
			k = lcpm._ready_csr(eng, csr)[0]
			part = torch.empty((int(eng.lib.nrm_lcpm_csr_workspace(NG, N)), ), dtype=torch.int64, device='cuda')
			r['lcpm_count_pass'] = timed(lambda: _lib.check(eng.lib.nrm_lcpm_csr_count(*k.args(), *out, part.data_ptr(), eng._stream())))
		r['stats_pass_over_lcpm_count_pass'] = round(r['stats_pass_all_alive']['median_ms'] / r['lcpm_count_pass']['median_ms'], 2)
		rec[name] = r
	rec['lcpm_count_kernel_ms_in_front_half_json'] = 0.052
	rec['reference_qc_reads_cpu'] = reference_seconds(x, args.reference)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	json.dump(rec, open(args.out, 'w'), indent=1)
	print(json.dumps(rec))


if __name__ == '__main__':
	main()
