"""The design of BASELINE configs[3] (1000 groupings x 50 000 cells, 1 % set, fp32) handed over dense and handed over sparse.  Writes one JSON record
(profiles/design_csr.json).  Four legs, each in a process of its own, the processes alternating (dense, sparse, dense, sparse, ...) for --rounds rounds:
  lists_dense   de_sparse.Lists(eng, dense tensor in HBM): nrm_design_count / _plan / _fill, two sweeps of the 200 MB matrix -- the yardstick
  lists_csr     de_sparse.Lists.from_csr(eng, DesignCSR): nrm_design_csr_count / nrm_design_plan / nrm_design_csr_fill over the stored entries
                both with device events around the call, which contains the one read-back of the sizes; after warm-up, --reps calls
  de_dense      the public norm.de(dg, dt, dc) on a design the engine has not seen, dg a dense numpy matrix: host clock around the call (it ends in downloads)
  de_scipy      the same call with dg a scipy.sparse CSR matrix
                --genes expression rows (fp32), 5 covariates with an intercept; a fresh design object per call, so that its lists are built inside the call
The two de legs also record a digest of the P-values: the record says whether they are the same bytes.

Usage: time_design_csr.py [--rounds R] [--reps N] [--warmup W] [--genes G] [--out profiles/design_csr.json]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NX, N, DENSITY, NC, SEED = 1000, 50000, 0.01, 5, 33
LEGS = ('lists_dense', 'lists_csr', 'de_dense', 'de_scipy')


def design():
	rng = np.random.default_rng(SEED)
	return (rng.random((NX, N)) < DENSITY).astype(np.float32)


def stats(ms):
	return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4), reps=len(ms))


def leg(name, args):
	import scipy.sparse
	import torch
	from normalisr_amd import de_sparse, engine
	import normalisr_amd.normalisr as norm
	eng = engine.get_engine()
	dg = design()
	rec = dict(stored_entries=int(np.count_nonzero(dg)))
	if name.startswith('lists'):
		src = eng.upload(dg) if name == 'lists_dense' else de_sparse.DesignCSR.from_scipy(scipy.sparse.csr_matrix(dg))
		build = (lambda: de_sparse.Lists(eng, src)) if name == 'lists_dense' else (lambda: de_sparse.Lists.from_csr(eng, src))
		for _ in range(args.warmup):
			build()
		ms = []
		for _ in range(args.reps):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record()
			lists = build()
			b.record()
			b.synchronize()
			ms.append(a.elapsed_time(b))
		rec.update(stats(ms), nnz=lists.nnz, padded=lists.padded,
				   input_bytes=int(dg.nbytes) if name == 'lists_dense' else int(sum(t.numel() * t.element_size() for t in (src.indptr, src.indices, src.data))))
	else:
		rng = np.random.default_rng(SEED + 1)
		dt = rng.standard_normal((args.genes, N), dtype=np.float32)
		dt[:8] += 0.5 * dg[0]
		dc = np.vstack([rng.normal(size=(NC - 1, N)), np.ones((1, N))])
		fresh = (lambda: dg.copy()) if name == 'de_dense' else (lambda: scipy.sparse.csr_matrix(dg))
		for _ in range(args.warmup):
			norm.de(fresh(), dt, dc)
		ms = []
		for _ in range(args.reps):
			d = fresh()
			torch.cuda.synchronize()
			t0 = time.perf_counter()
			out = norm.de(d, dt, dc)
			ms.append(1e3 * (time.perf_counter() - t0))
		rec.update(stats(ms), genes=args.genes, path=eng._tls.path, p_sha1=hashlib.sha1(np.ascontiguousarray(out[0]).tobytes()).hexdigest())
	print('LEG ' + json.dumps(rec), flush=True)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--rounds', type=int, default=2)
	ap.add_argument('--reps', type=int, default=20)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--genes', type=int, default=5000)
	ap.add_argument('--out', default='profiles/design_csr.json')
	ap.add_argument('--leg', choices=LEGS, default=None)
	args = ap.parse_args()
	if args.leg:
		return leg(args.leg, args)
	rec = dict(tool='time_design_csr', design=dict(groupings=NX, cells=N, density=DENSITY, dtype='float32'), covariates=NC, rounds=args.rounds, warmup=args.warmup, legs={k: [] for k in LEGS})
	for _ in range(args.rounds):
		for name in LEGS:  # (alternating: every leg once per round, a process each)
			reps = args.reps if name.startswith('lists') else max(3, args.reps // 5)
			r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, '--reps', str(reps), '--warmup', str(args.warmup if name.startswith('lists') else 1),
								'--genes', str(args.genes)], capture_output=True, text=True, timeout=600)
			if r.returncode != 0:
				raise SystemExit('leg {} failed ({}):\n{}'.format(name, r.returncode, r.stderr[-3000:]))
			rec['legs'][name].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('LEG ')][-1][4:]))
	med = lambda name: float(np.median([r['median_ms'] for r in rec['legs'][name]]))
	rec['summary'] = dict(lists_dense_ms=round(med('lists_dense'), 4), lists_csr_ms=round(med('lists_csr'), 4), de_dense_ms=round(med('de_dense'), 2), de_scipy_ms=round(med('de_scipy'), 2),
						  same_lists=len({(r['nnz'], r['padded']) for k in ('lists_dense', 'lists_csr') for r in rec['legs'][k]}) == 1,
						  same_p_values=len({r['p_sha1'] for k in ('de_dense', 'de_scipy') for r in rec['legs'][k]}) == 1)
	import torch
	rec['device'] = torch.cuda.get_device_name(0)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	json.dump(rec, open(args.out, 'w'), indent=1)
	print(json.dumps(rec['summary']))


if __name__ == '__main__':
	main()
