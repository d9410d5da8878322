"""bh and binnet in their two forms, P and ln P (p_kind 0 and 1), on resident matrices, in the same run: bh over 1000 x 15 000 entries (the shape of tools/time_bh.py:
a screen's de result; ln P and P from the same seeded association_tests call, with and without logp=True) and binnet over 5000^2 and 20 000^2 (a seeded matrix with a
planted dense corner: ln P log-uniform, P its exponential), fp32 and fp64.  HIP events around the call, launches included; the P form goes through the entries that
existed before the ln form (nrm_bh, nrm_binnet), the ln form through nrm_bh_pk / nrm_binnet_pk.

One process measures one tree.  `--rounds 3 --parent DIR` starts that many processes per tree in turn -- DIR (a checkout of the parent commit, built), this tree, DIR, ...
-- and reports, per case, the medians of the rounds and their range, so that the P form of this tree can be read against the parent's own spread.  A tree
without the _pk entries measures the P form only.

Usage: time_bh_logp.py [--reps R] [--warmup W] [--rounds N] [--parent DIR] [--sizes 5000,20000] [--out profiles/bh_logp.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NX, NY, CELLS, SEED = 1000, 15000, 256, 23
QCUT = 0.05


def measure(args):
	sys.path.insert(0, args.tree)
	import torch
	from normalisr_amd import _lib, engine
	from normalisr_amd.association import association_tests
	eng = engine.get_engine()
	lib = eng.lib
	has_ln = hasattr(lib, 'nrm_bh_pk')
	rng = np.random.default_rng(SEED)
	rec = dict(tree=os.path.abspath(args.tree), device=torch.cuda.get_device_name(0), has_ln=has_ln, cases={})

	def timed(step):
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
		return round(float(np.median(ms)), 4)

	# ---- bh: de's own P-values and, where the tree has it, ln P of the same call
	design = (rng.random((NX, CELLS)) < 0.05).astype(np.float64)
	design[:, 0], design[:, 1] = 1, 0
	exp = rng.normal(size=(NY, CELLS))
	cov = np.vstack([np.ones(CELLS), rng.normal(size=CELLS)])
	p64 = association_tests(design, exp, cov, return_dot=False, device_out=True)[0]
	ln64 = association_tests(design, exp, cov, return_dot=False, device_out=True, logp=True)[0] if has_ln else None
	for name, tdt, code in (('fp32', torch.float32, _lib.NRM_F32), ('fp64', torch.float64, _lib.NRM_F64)):
		nbytes = int(lib.nrm_bh_workspace_bytes(NX * NY, code))
		work = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
		flags = torch.zeros(2, dtype=torch.int32, device=eng.device)
		d_p = p64.to(tdt)
		out = torch.empty_like(d_p)
		rec['cases']['bh {} P'.format(name)] = timed(lambda: _lib.check(lib.nrm_bh(d_p.data_ptr(), code, NX, NY, NY, out.data_ptr(), NY, work.data_ptr(), nbytes, flags.data_ptr(), eng._stream())))
		assert flags.tolist() == [0, 1]
		if has_ln:
			d_l = ln64.to(tdt)
			rec['cases']['bh {} lnP'.format(name)] = timed(lambda: _lib.check(lib.nrm_bh_pk(d_l.data_ptr(), code, NX, NY, NY, out.data_ptr(), NY, work.data_ptr(), nbytes, flags.data_ptr(), 1, eng._stream())))
			assert flags.tolist() == [0, 1]
		del work, out, d_p
	del p64, ln64
	# ---- binnet: ln P log-uniform in [-20, 0), a dense corner of strong pairs; P = exp(ln P)
	for ng in args.sizes:
		g = torch.Generator(device=eng.device)
		g.manual_seed(SEED + ng)
		ln = -20.0 * torch.rand((ng, ng), generator=g, device=eng.device, dtype=torch.float64) ** 4
		k = ng // 20
		ln[:k, :k] -= 30.0
		ln = torch.triu(ln, 1)
		ln = ln + ln.T
		ln.fill_diagonal_(float('-inf'))
		for name, tdt, code in (('fp32', torch.float32, _lib.NRM_F32), ('fp64', torch.float64, _lib.NRM_F64)):
			out = torch.empty((ng, ng), dtype=torch.uint8, device=eng.device)
			total = torch.zeros(1, dtype=torch.int64, device=eng.device)
			flags = torch.zeros(2, dtype=torch.int32, device=eng.device)
			d_p = torch.exp(ln).to(tdt)
			rec['cases']['binnet {} {} P'.format(ng, name)] = timed(lambda: _lib.check(lib.nrm_binnet(d_p.data_ptr(), code, ng, ng, QCUT, out.data_ptr(), ng, total.data_ptr(), flags.data_ptr(), eng._stream())))
			edges = int(total.item())
			assert flags.tolist()[0] == 0 and edges > 0
			rec['cases']['binnet {} {} edges'.format(ng, name)] = edges
			del d_p
			if has_ln:
				d_l = ln.to(tdt)
				rec['cases']['binnet {} {} lnP'.format(ng, name)] = timed(lambda: _lib.check(lib.nrm_binnet_pk(d_l.data_ptr(), code, ng, ng, QCUT, out.data_ptr(), ng, total.data_ptr(), flags.data_ptr(), 1, eng._stream())))
				assert flags.tolist()[0] == 0
				rec['cases']['binnet {} {} lnP edges'.format(ng, name)] = int(total.item())
				del d_l
			del out
		del ln
	print('RECORD ' + json.dumps(rec), flush=True)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--reps', type=int, default=20)
	ap.add_argument('--warmup', type=int, default=3)
	ap.add_argument('--rounds', type=int, default=1)
	ap.add_argument('--parent', default=None)
	ap.add_argument('--tree', default=os.path.dirname(HERE))
	ap.add_argument('--sizes', default='5000,20000', type=lambda s: [int(v) for v in s.split(',')])
	ap.add_argument('--out', default='profiles/bh_logp.json')
	ap.add_argument('--child', action='store_true')
	args = ap.parse_args()
	if args.child:
		return measure(args)
	trees = ([('parent', args.parent)] if args.parent else []) + [('this', args.tree)]
	runs = {label: [] for label, _ in trees}
	for r in range(args.rounds):
		for label, tree in trees:  # a fresh process per tree and round, in turn
			cmd = [sys.executable, os.path.abspath(__file__), '--child', '--tree', tree, '--reps', str(args.reps), '--warmup', str(args.warmup), '--sizes', ','.join(str(v) for v in args.sizes)]
			p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
			line = [l for l in p.stdout.splitlines() if l.startswith('RECORD ')]
			if p.returncode != 0 or not line:
				sys.exit('round {} of {} failed:\n{}'.format(r, label, p.stdout[-3000:]))
			runs[label].append(json.loads(line[0][7:]))
			print(label, r, json.dumps(runs[label][-1]['cases']), flush=True)
	rec = dict(tool='time_bh_logp', device=runs['this'][0]['device'], reps=args.reps, warmup=args.warmup, rounds=args.rounds, qcut=QCUT, bh_shape=[NX, NY], cases={},
			   note='ms per call, HIP events around the call (launches included); per case the median of every round (a process of its own, the trees in turn) and '
					'their range; "parent": the parent commit built in a checkout of its own, P form only')
	for label in runs:
		for case in runs[label][0]['cases']:
			v = [run['cases'][case] for run in runs[label]]
			rec['cases'].setdefault(case, {})[label] = v[0] if 'edges' in case else dict(rounds=v, min=min(v), max=max(v))
	print(json.dumps(rec))
	if args.out != '/dev/null':
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, 'w') as f:
			f.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
	main()
