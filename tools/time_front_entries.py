"""numpy in -> numpy out wall time of lcpm, compute_var and qc_reads at the front-half size of tools/time_front.py (5000 genes x 10 000 cells of int32 counts from
the same seed, 8 covariates), on the library's whole-problem entries (nrm_lcpm_host, nrm_compute_var_host, nrm_qc_reads_host; a process in which torch cannot be
imported) and on the torch engine's public calls -- the route host input took before the entries existed.  The two routes alternate in separate processes,
`--rounds` times in one run; a round's figure is the median of `--reps` calls after `--warmup`.  The kernels are the same on both routes, so an entry that is
slower than the torch route by more than the run's own spread points at an extra copy or a missing page-lock in the entry (`above_spread`).
Then the whole-command wall time of `normalisr lcpm` and `normalisr fitvar` on .npy files of the size of the G18 fixture (112 x 240), both ways (the command
line's default against NRM_HOST_ENTRY=0), alternating as well: the share of torch's import.  Writes one JSON record.

Usage: time_front_entries.py [--rounds 3] [--reps 5] [--warmup 2] [--out profiles/front_entries.json]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

import plan_timing as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NG, N, SEED = 5000, 10000, 18
QC_PARAMS = (50, 20, 0.002, 200, 50, 0.01)


def inputs():
	rng = np.random.default_rng(SEED)
	mu = np.exp(rng.normal(-1.0, 1.3, NG))
	depth = np.exp(rng.normal(0.0, 0.5, N))
	x = rng.poisson(mu[:, None] * depth[None, :]).astype(np.int32)
	empty = x.sum(axis=0) == 0
	x[0, empty] = 1
	batch = rng.integers(0, 4, N)
	onehot = (batch[None, :] == np.arange(4)[:, None]).astype(np.float64)
	return x, onehot


def child(args):
	if args.child == 'entries':
		sys.modules['torch'] = None  # `import torch` raises ImportError in this process: every call below takes the entries
	os.environ.pop('NRM_HOST_ENTRY', None)
	import normalisr_amd.lcpm as lcpm
	import normalisr_amd.norm as norm
	import normalisr_amd.qc as qc
	x, onehot = inputs()

	def timed(fn):
		for _ in range(args.warmup):
			out = fn()
		ms = []
		for _ in range(args.reps):
			del out
			t0 = time.perf_counter()
			out = fn()
			ms.append(1e3 * (time.perf_counter() - t0))
		return out, [round(v, 3) for v in ms]

	rec = {}
	(lc, _, _, cov), rec['lcpm'] = timed(lambda: lcpm.lcpm(x))
	dc = norm.normcov(np.vstack([onehot, cov]))
	w, rec['compute_var'] = timed(lambda: norm.compute_var(lc, dc))
	keep, rec['qc_reads'] = timed(lambda: qc.qc_reads(x, *QC_PARAMS))
	rec['check'] = dict(lcpm_sum=float(lc.sum()), w_max=float(w.max()), genes=int(keep[0].size), cells=int(keep[1].size))
	if args.child == 'entries':
		assert sys.modules['torch'] is None and not [m for m in sys.modules if m.startswith('torch.')]
	else:
		assert 'torch' in sys.modules
	return rec


def commands(rounds, tmp):
	"""Wall time of `python -m normalisr_amd lcpm | fitvar` as child processes on .npy files of the G18 size, the default route and NRM_HOST_ENTRY=0 alternating."""
	g = np.load(os.path.join(ROOT, 'tests', 'golden', 'G18_front.npz'))
	h = np.load(os.path.join(ROOT, 'tests', 'golden', 'G18_front_chain.npz'))
	f = lambda name: os.path.join(tmp, name)
	np.save(f('reads.npy'), g['reads'])
	np.save(f('lcpm.npy'), g['lcpm'])
	np.save(f('cov.npy'), h['normcov_c'])
	cmds = dict(lcpm=['lcpm', f('reads.npy'), f('lcpm_out.npy'), f('scale.npy'), f('cov_out.npy')], fitvar=['fitvar', f('lcpm.npy'), f('cov.npy'), f('w.npy')])
	base = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
	base.pop('NRM_HOST_ENTRY', None)
	out = {}
	for name, argv in cmds.items():
		t = dict(entries=[], torch=[])
		for _ in range(rounds + 1):  # (the first pair warms the file cache and is dropped)
			for route, env in (('entries', base), ('torch', dict(base, NRM_HOST_ENTRY='0'))):
				t0 = time.perf_counter()
				r = subprocess.run([sys.executable, '-m', 'normalisr_amd'] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
				if r.returncode != 0:
					raise RuntimeError('{} ({}) failed:\n{}'.format(name, route, r.stderr[-3000:]))
				t[route].append(round(time.perf_counter() - t0, 3))
		out[name] = dict(entries_s=t['entries'][1:], torch_s=t['torch'][1:], entries_median_s=float(np.median(t['entries'][1:])), torch_median_s=float(np.median(t['torch'][1:])))
		out[name]['saved_s'] = round(out[name]['torch_median_s'] - out[name]['entries_median_s'], 3)
	return out


def main():
	args = pt.arg_parser('profiles/front_entries.json', 400, warmup=2, steps=None).parse_args()
	if args.child:
		print(json.dumps(child(args)))
		return
	ts, es = pt.alternate(__file__, args, ('torch', 'entries'))
	rec = dict(shape=dict(genes=NG, cells=N, dtype='int32', covariates=8, seed=SEED, qc_params=QC_PARAMS), rounds=args.rounds, reps=args.reps, warmup=args.warmup,
			   what='numpy in -> numpy out wall time per call (time.perf_counter), one process per route and round', check=dict(entries=es[-1]['check'], torch=ts[-1]['check']))
	for op in ('lcpm', 'compute_var', 'qc_reads'):
		e, t = pt.side(es, op, 3), pt.side(ts, op, 3)
		spread = max(t['max_ms'] - t['min_ms'], e['max_ms'] - e['min_ms'])
		rec[op] = dict(entries=e, torch=t, spread_ms=round(spread, 3), above_spread=bool(e['median_ms'] > t['median_ms'] + spread))
	with tempfile.TemporaryDirectory() as tmp:
		rec['commands_g18_npy'] = commands(args.rounds, tmp)
	pt.write(rec, args.out)


if __name__ == '__main__':
	main()
