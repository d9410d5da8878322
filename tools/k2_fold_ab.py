"""K2 alone (nrm_gram_i8_band + fix-up, NS = 6), alternating in one process: this tree's library with NRM_DEBUG=gram_fold=0 (the ragged last tile column on
tiles of its own) and as it ships (folded into the diagonal tiles), and -- when given -- another build of the library, e.g. the parent commit's.
5000, 4992 and 5100 genes x 10 000 cells symmetric, then one rectangular launch of the configs[4] slice shape.  profiles/r07_k2_edge_fold.txt.
Usage: k2_fold_ab.py [other_lib.so]"""
import ctypes, os, sys
import numpy as np
import torch
sys.path.insert(0, '.')
from normalisr_amd import _lib
lib = _lib.load()
par = ctypes.CDLL(sys.argv[1]) if len(sys.argv) > 1 else None
if par is not None:
	par.nrm_gram_i8_band.argtypes = lib.nrm_gram_i8_band.argtypes
	par.nrm_gram_i8_band.restype = lib.nrm_gram_i8_band.restype
st = torch.cuda.current_stream().cuda_stream
work = torch.empty(int(lib.nrm_gram_workspace_bytes()) // 8, dtype=torch.float64, device='cuda')
ALT = 7

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
	nrm = torch.sqrt((a * a).sum(dim=1))
	del a
	return mp, kp, q, ex, nrm

def report(tag, res):
	for k, v in res.items():
		print('%s %-8s  min %.4f  median %.4f  max %.4f   runs %s' % (tag, k, min(v), float(np.median(v)), max(v), ' '.join('%.4f' % x for x in v)), flush=True)

def variants(call):
	def p():
		call(par)
	def off():
		os.environ['NRM_DEBUG'] = 'gram_fold=0'
		call(lib)
	def on():
		os.environ.pop('NRM_DEBUG', None)
		call(lib)
	return ((('parent', p), ) if par is not None else ()) + (('fold=0', off), ('fold', on))

for ng in (5000, 4992, 5100):
	mp, kp, q, ex, nrm = problem(ng, 10000, 1)
	dots = {}
	def call(l):
		_lib.check(l.nrm_gram_i8_band(q.data_ptr(), ex.data_ptr(), 0, q.data_ptr(), ex.data_ptr(), 0, mp, mp, kp, 6, dot.data_ptr(), mp, 1, ng, ng, 0, mp, work.data_ptr(), st))
	res = {}
	for name, f in variants(call):
		dot = torch.full((mp, mp), float('nan'), dtype=torch.float64, device='cuda')
		f()
		torch.cuda.synchronize()
		dots[name] = dot
		res[name] = []
	iu = torch.triu_indices(ng, ng, device='cuda')
	sc = nrm[iu[0]] * nrm[iu[1]]
	base = 'parent' if par is not None else 'fold=0'
	for name in ('fold=0', 'fold'):
		d = (dots[name][iu[0], iu[1]] - dots[base][iu[0], iu[1]]).abs() / sc
		print('%d genes: %s against %s: max |diff| / |a_i||a_j| = %.3e, entries that differ %d of %d, all finite %s' % (
			ng, name, base, d.max().item(), int((d > 0).sum().item()), d.numel(), bool(torch.isfinite(dots[name][iu[0], iu[1]]).all().item())), flush=True)
	dot = dots['fold']
	for rep in range(ALT):
		for name, f in variants(call):
			res[name].append(timeit(f, 20))
	report('%d genes x 10000 cells, symmetric, ms:' % ng, res)
	del dots, dot, q, ex

# one rectangular launch of the configs[4] slice shape: 1024 rows against 15104 rows at 50 000 cells (the fold does not apply)
m, nb, n = 1024, 15104, 50000
mp, kp, q, ex, _ = problem(nb, n, 3)
dot = torch.empty((m, mp), dtype=torch.float64, device='cuda')
plane = (mp // 32) * ((kp + 31) // 32) * 1024
def call(l):
	_lib.check(l.nrm_gram_i8_band(q.data_ptr(), ex.data_ptr(), plane, q.data_ptr(), ex.data_ptr(), plane, m, mp, kp, 6, dot.data_ptr(), mp, 0, m, nb, 0, m, work.data_ptr(), st))
res = {name: [] for name, _ in variants(call)}
for rep in range(5):
	for name, f in variants(call):
		res[name].append(timeit(f, 5))
report('1024 x 15104 x 50000 cells, rectangular, ms:', res)
