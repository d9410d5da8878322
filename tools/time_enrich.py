"""Gene-set enrichment on the device (normalisr_amd/enrich.py), in ONE process after warm-up, timed with device events.  Writes one JSON record
(profiles/enrich.json).
  sizes      15 000 genes x 10 000 synthetic sets (sizes log-uniform in 5 .. 2000, members drawn without replacement, every gene in the background), for
             one study of 100 genes and for a whole binary network of density 0.02 as 15 000 studies (one per gene)
  call       enrich(..., device_out=True) on a study already in HBM with the sets bound and uploaded before: the four launches and the read-back of the
             studies' top records
  stages     from the engine's trace: pack, overlap (with the set sizes), fisher, top
  yardstick  a scipy.stats.fisher_exact loop on THIS machine's CPU over the 10 000 pairs of the one study, from the device's own counts -- the size it
             finishes in seconds; the whole network is 15 000 times that many tests.  Another processor, not a speed-up of the same code.  null without scipy.
Nothing is promised in advance: the record holds what was measured.

Usage: time_enrich.py [--reps R] [--warmup W] [--out profiles/enrich.json] [--genes G] [--sets T] [--no-network]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ('enrich_pack', 'enrich_overlap', 'enrich_fisher', 'enrich_top')


def synthetic_sets(ng, nsets, seed):
	from normalisr_amd import enrich
	rng = np.random.default_rng(seed)
	sizes = np.minimum(np.exp(rng.uniform(np.log(5), np.log(2000), nsets)).astype(np.int64), ng)
	rows = np.repeat(np.arange(nsets), sizes)
	cols = np.concatenate([rng.choice(ng, k, replace=False) for k in sizes])
	names = ['SET{:05d}'.format(t) for t in range(nsets)]
	bits = enrich.pack_bits(rows, cols, nsets, ng)
	bg = enrich.pack_bits(np.zeros(ng, dtype=np.int64), np.arange(ng), 1, ng)[0]
	return enrich.BoundSets(names, names, np.zeros(nsets, dtype=np.int64), np.arange(ng), bits, bg, np.arange(nsets)), sizes


def stats(ms):
	return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=10)
	ap.add_argument('--warmup', type=int, default=2)
	ap.add_argument('--out', default='profiles/enrich.json')
	ap.add_argument('--genes', type=int, default=15000)
	ap.add_argument('--sets', type=int, default=10000)
	ap.add_argument('--no-network', action='store_true')
	args = ap.parse_args()
	import torch
	from normalisr_amd import engine, enrich
	eng = engine.get_engine()
	ng, nsets = args.genes, args.sets
	bound, sizes = synthetic_sets(ng, nsets, 7)
	bound.device(eng)
	rec = dict(tool='time_enrich', device=torch.cuda.get_device_name(0), warmup=args.warmup, genes=ng, sets=nsets, set_size_median=int(np.median(sizes)),
			   set_size_max=int(sizes.max()))

	def measure(study, reps):
		call = lambda: enrich.enrich(study, bound, device_out=True)
		for _ in range(args.warmup):
			call()
		whole, per = [], {k: [] for k in STAGES}
		for _ in range(reps):
			eng.trace = []
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record()
			res = call()
			b.record()
			b.synchronize()
			whole.append(a.elapsed_time(b))
			for k, e0, e1 in eng.trace:
				if k in per:
					per[k].append(e0.elapsed_time(e1))
			eng.trace = None
		return res, dict(call=stats(whole), stages={k: stats(v) for k, v in per.items() if v})

	one = torch.zeros((1, ng), dtype=torch.uint8, device=eng.device)
	one[0, torch.from_numpy(np.random.default_rng(8).choice(ng, 100, replace=False)).to(eng.device)] = 1
	res, r = measure(one, args.reps)
	r.update(studies=1, study_genes=100, tests=nsets)
	rec['one_study'] = r
	k, K, p = res.k.cpu().numpy()[0], res.K.cpu().numpy(), res.p.cpu().numpy()[0]
	try:
		from scipy.stats import fisher_exact
		t0 = time.perf_counter()
		ref = np.array([fisher_exact([[int(k[t]), 100 - int(k[t])], [int(K[t]) - int(k[t]), ng - int(K[t]) - 100 + int(k[t])]])[1] for t in range(nsets)])
		rec['scipy_fisher_exact_cpu'] = dict(seconds=round(time.perf_counter() - t0, 3), tests=nsets, size='1 study of 100 genes x {} sets, {} genes'.format(nsets, ng),
											 largest_relative_difference=float(np.max(np.abs(ref - p) / ref)),
											 note='one CPU thread of the machine this record was made on: another processor, not a speed-up')
	except ImportError:
		rec['scipy_fisher_exact_cpu'] = None
	if not args.no_network:
		gen = torch.Generator(device=eng.device).manual_seed(9)
		net = torch.rand((ng, ng), generator=gen, device=eng.device) < 0.02
		res, r = measure(net, max(2, args.reps // 3))
		r.update(studies=ng, study_genes_median=int(res.n.median().item()), tests=ng * nsets, bit_products=ng * nsets * ng, studies_with_a_top_set=int((res.top >= 0).sum()))
		rec['whole_network'] = r
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	json.dump(rec, open(args.out, 'w'), indent=1)
	print(json.dumps(rec))


if __name__ == '__main__':
	main()
