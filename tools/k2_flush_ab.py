"""K2 alone (nrm_gram_i8_band + fix-up, NS = 6), several builds of the library alternating in one process -- the protocol of tools/k2_fold_ab.py: seven
alternations (after one that is not recorded) of 20 launches on 5000, 4992 and 5100 genes x 10 000 cells symmetric, then five of 5 on one rectangular launch of the configs[4] slice
shape (1024 x 15104 x 50 000 cells, three flushes in mid-piece per tile).  Every build's output is compared bit for bit with the first's, except builds
whose name ends in '!' (timing-only ablations such as QI_EXP=8 of tools/build_exp.sh, whose outputs are garbage).  profiles/k2_flush_ab.txt.
Usage: k2_flush_ab.py name=lib.so [name=lib.so ...]   (the tree's own library: name=tree)"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, '.')
from normalisr_amd import _lib
lib = _lib.load()
libs = []
for arg in sys.argv[1:]:
	name, path = arg.split('=', 1)
	l = lib if path == 'tree' else ctypes.CDLL(path)
	if l is not lib:
		l.nrm_gram_i8_band.argtypes = lib.nrm_gram_i8_band.argtypes
		l.nrm_gram_i8_band.restype = lib.nrm_gram_i8_band.restype
	libs.append((name, l))
st = torch.cuda.current_stream().cuda_stream
work = torch.empty(int(lib.nrm_gram_workspace_bytes()) // 8, dtype=torch.float64, device='cuda')

def timeit(f, reps):
	for _ in range(3):
		f()
	e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	e0.record()
	for _ in range(reps):
		f()
	e1.record()
	torch.cuda.synchronize()
	return e0.elapsed_time(e1) / reps

def problem(rows, n, seed):
	mp, kp = (rows + 127) // 128 * 128, (n + 15) // 16 * 16
	g = torch.Generator(device='cuda').manual_seed(seed)
	a = torch.zeros((mp, kp), dtype=torch.float64, device='cuda')
	a[:rows, :n] = torch.randn((rows, n), dtype=torch.float64, device='cuda', generator=g) * torch.exp(torch.randn((rows, 1), dtype=torch.float64, device='cuda', generator=g))
	q = torch.empty(int(lib.nrm_quant_bytes(mp, kp, 6)), dtype=torch.uint8, device='cuda')
	ex = torch.empty(mp, dtype=torch.int32, device='cuda')
	_lib.check(lib.nrm_quantize_rows(a.data_ptr(), mp, kp, kp, 6, q.data_ptr(), ex.data_ptr(), 0, 0, st))
	torch.cuda.synchronize()
	del a
	return mp, kp, q, ex

def run(tag, call, shape, alt, reps, valid):
	"""valid(dot) -> the entries somebody reads, as a 1-d tensor"""
	outs, res = {}, {}
	for name, l in libs:
		dot = torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')
		call(l, dot)
		torch.cuda.synchronize()
		outs[name], res[name] = valid(dot), []
		del dot
	base = libs[0][0]
	for name, _ in libs[1:]:
		if name.endswith('!'):
			continue
		a, b = outs[name].view(torch.int64), outs[base].view(torch.int64)
		print('%s %s against %s: entries whose bits differ %d of %d, all finite %s' % (tag, name, base, int((a != b).sum().item()), a.numel(),
																				 bool(torch.isfinite(outs[name]).all().item())), flush=True)
	del outs
	dot = torch.empty(shape, dtype=torch.float64, device='cuda')
	for rep in range(alt + 1):  # (the first round is not recorded: whoever runs first on a new shape pays for the clocks to settle)
		for name, l in libs:
			t = timeit(lambda: call(l, dot), reps)
			if rep:
				res[name].append(t)
	for k, v in res.items():
		print('%s ms: %-9s min %.4f  median %.4f  max %.4f   runs %s' % (tag, k, min(v), float(np.median(v)), max(v), ' '.join('%.4f' % x for x in v)), flush=True)

for ng in (5000, 4992, 5100):
	mp, kp, q, ex = problem(ng, 10000, 1)
	def call(l, dot):
		_lib.check(l.nrm_gram_i8_band(q.data_ptr(), ex.data_ptr(), 0, q.data_ptr(), ex.data_ptr(), 0, mp, mp, kp, 6, dot.data_ptr(), mp, 1, ng, ng, 0, mp, work.data_ptr(), st))
	iu = torch.triu_indices(ng, ng, device='cuda')
	run('%d genes x 10000 cells, symmetric:' % ng, call, (mp, mp), 7, 20, lambda d: d[iu[0], iu[1]])
	del q, ex, iu

m, nb, n = 1024, 15104, 50000
mp, kp, q, ex = problem(nb, n, 3)
plane = (mp // 32) * ((kp + 31) // 32) * 1024
def call(l, dot):
	_lib.check(l.nrm_gram_i8_band(q.data_ptr(), ex.data_ptr(), plane, q.data_ptr(), ex.data_ptr(), plane, m, mp, kp, 6, dot.data_ptr(), mp, 0, m, nb, 0, m, work.data_ptr(), st))
run('1024 x 15104 x 50000 cells, rectangular:', call, (m, mp), 5, 5, lambda d: d[:, :nb].reshape(-1))
