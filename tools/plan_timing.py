"""What the timing tools of the C-ABI plans and entries share (time_c_plan.py, time_de_plan.py, time_single1_c_plan.py, time_single4_c_plan.py, time_front_entries.py):
the command line, the child processes -- one on the GPU at a time, two kinds alternating --, a side's figures, the time of a plan's own kernels from a kernel trace,
and the yardstick / spread / margin part of the record.  A tool keeps its shapes and seeds, what its children do, and the keys of its record."""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile

import numpy as np


def arg_parser(out, child_timeout, warmup=5, steps=20, kernel_stats=False):
	"""--rounds 3, --reps 5, --warmup, --out, --child, --child-timeout; a tool that times steps of a plan (steps is not None) has --steps and --data too."""
	ap = argparse.ArgumentParser()
	ap.add_argument('--rounds', type=int, default=3)
	if steps is not None:
		ap.add_argument('--steps', type=int, default=steps)
	ap.add_argument('--reps', type=int, default=5)
	ap.add_argument('--warmup', type=int, default=warmup)
	ap.add_argument('--out', default=out)
	if kernel_stats:
		ap.add_argument('--kernel-stats', default=None, help='kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of the c_plan child')
	ap.add_argument('--child', default=None)
	if steps is not None:
		ap.add_argument('--data', default=None)
	ap.add_argument('--child-timeout', type=int, default=child_timeout)
	return ap


def run_child(script, kind, args):
	"""`script --child KIND` with the run's --data, --steps, --reps and --warmup: what it prints on its last line, as JSON."""
	cmd = [sys.executable, os.path.abspath(script), '--child', kind]
	for k in ('data', 'steps', 'reps', 'warmup'):
		if getattr(args, k, None) is not None:
			cmd += ['--' + k, str(getattr(args, k))]
	r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.child_timeout)
	if r.returncode != 0:
		raise RuntimeError('{} child failed ({}):\n{}'.format(kind, r.returncode, r.stderr[-3000:]))
	return json.loads(r.stdout.strip().splitlines()[-1])


def alternate(script, args, kinds, data=None):
	"""`--rounds` times one child of each kind, in the order given -> the list of runs per kind.  data: the children share files DIR/DATA.* in a directory that lives
	as long as the run."""
	runs = [[] for _ in kinds]
	with tempfile.TemporaryDirectory() as tmp:
		if data is not None:
			args.data = os.path.join(tmp, data)
		for _ in range(args.rounds):
			for k, kind in enumerate(kinds):
				runs[k].append(run_child(script, kind, args))
	return runs


def side(runs, key, digits=4):
	"""A round's figure is the median of its reps (ms): the rounds' figures, their median, minimum and maximum, and every rep."""
	fig = [float(np.median(r[key])) for r in runs]
	return dict(rounds_ms=[round(v, digits) for v in fig], median_ms=round(float(np.median(fig)), digits), min_ms=round(min(fig), digits), max_ms=round(max(fig), digits),
				reps_ms=[[round(v, digits) for v in r[key]] for r in runs])


def own_kernels_ms(path, kernels):
	"""Mean time per launch of the plan's own kernels (one launch of each per step) from a `rocprofv3 --kernel-trace --stats` CSV of the c_plan child."""
	per = {}
	with open(path) as f:
		for row in csv.DictReader(f):
			for k in kernels:
				if k + '<' in row['Name'] or k + '(' in row['Name']:
					per[k] = per.get(k, 0.0) + float(row['AverageNs']) / 1e6
	return per


def margin(y, c, kernels, stats):
	"""The verdict's part of a record: the plan's median is at most the yardstick's median plus the yardstick's own min-max spread in this run plus the time of the
	plan's own kernels (`kernels`, from the kernel trace `stats`; no verdict without one)."""
	spread = y['max_ms'] - y['min_ms']
	own = own_kernels_ms(stats, kernels) if stats else None
	own_ms = None if own is None else round(sum(own.values()), 4)
	return dict(yardstick_spread_ms=round(spread, 4), own_kernels_ms=own, own_kernels_from=stats, margin_ms=None if own_ms is None else round(spread + own_ms, 4),
				within_margin=None if own_ms is None else bool(c['median_ms'] <= y['median_ms'] + spread + own_ms))


def write(rec, out):
	os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
	with open(out, 'w') as f:
		f.write(json.dumps(rec, indent=1) + '\n')
	print(json.dumps(rec))
