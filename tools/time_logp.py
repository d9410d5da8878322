"""Time K3 (nrm_assoc_sweep_pk, symmetric, without row records) at BASELINE configs[1] size -- 5000 genes, 10 000 cells -- for P-values (p_kind 0) and for
their logarithms (p_kind 1), fp32 and fp64 outputs, between two device events.  Two inputs: independent rows (every R^2 far below 1/4: both forms take the
straight-line fast path, ln P pays one logarithm in place of the exponential) and rows with a common factor of weight 1 (every R^2 = 1/4 or above: P is 0 there
without evaluating anything, nrm_zero_above_quarter, while ln P goes through the general path pair by pair).

Usage: time_logp.py [--genes 5000] [--reps 20] [--out profiles/logp.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from normalisr_amd import _lib  # noqa: E402


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--genes', type=int, default=5000)
	ap.add_argument('--reps', type=int, default=20)
	ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'logp.json'))
	args = ap.parse_args()
	lib = _lib.load()
	ng, n = args.genes, 10000
	mp = (ng + 255) // 256 * 256
	s = torch.cuda.current_stream().cuda_stream
	rec = dict(shape=dict(genes=ng, cells=n), reps=args.reps, what='nrm_assoc_sweep_pk, symmetric, no row records; ms per launch between two device events', runs=[])
	for label, weight in (('independent rows', 0.0), ('common factor, R^2 >= 1/4', 1.0)):
		g = torch.Generator(device='cuda').manual_seed(3)
		x = torch.randn((ng, n), dtype=torch.float64, device='cuda', generator=g)
		if weight:
			x += weight * torch.randn((1, n), dtype=torch.float64, device='cuda', generator=g)
		dot = torch.zeros((mp, mp), dtype=torch.float64, device='cuda')
		dot[:ng, :ng] = x @ x.T
		ss = torch.zeros(mp, dtype=torch.float64, device='cuda')
		ss[:ng] = (x * x).sum(1)
		del x
		for tdt, code in ((torch.float32, _lib.NRM_F32), (torch.float64, _lib.NRM_F64)):
			p = torch.empty((ng, ng), dtype=tdt, device='cuda')
			st = torch.empty((ng, ng), dtype=tdt, device='cuda')
			flags = torch.zeros(4, dtype=torch.int32, device='cuda')
			for kind in (0, 1):
				def run():
					_lib.check(lib.nrm_assoc_sweep_pk(dot.data_ptr(), mp, ss.data_ptr(), ss.data_ptr(), ng, ng, n, float(n - 4), 1, 0, p.data_ptr(), st.data_ptr(), 0, 0, code,
													  ng, flags.data_ptr(), 0, 0, 0, 0.0, kind, s))
				for _ in range(3):
					run()
				e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
				e0.record()
				for _ in range(args.reps):
					run()
				e1.record()
				torch.cuda.synchronize()
				off = ~torch.eye(ng, dtype=torch.bool, device='cuda')
				v = p[off]
				rec['runs'].append(dict(rows=label, out_dtype=str(tdt).replace('torch.', ''), p_kind=kind, ms=round(e0.elapsed_time(e1) / args.reps, 4),
										zeros=int((v == 0).sum()), finite=int(torch.isfinite(v).sum()), pairs=int(v.numel()), flags=flags.cpu().tolist()))
				print(rec['runs'][-1], flush=True)
	os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
	with open(args.out, 'w') as fh:
		json.dump(rec, fh, indent=1)
		fh.write('\n')


if __name__ == '__main__':
	main()
