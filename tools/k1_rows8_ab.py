"""K1 alone (nrm_residualize_q, NS = 6, digit planes + row records, no fp64 output), alternating in one process: this tree's library with
NRM_DEBUG=k1_rows8=0 (k_residualize_v4: four rows per workgroup, covariates from L2 inside the step) and with k1_rows8=1 (k_residualize_v8: eight rows, covariate
slices through LDS, also on rows shorter than the launcher sends it), and -- when given -- another build of the library, e.g. the parent commit's.  5000 x 10 000 fp32 with 3 covariates (the headline),
16 000 x 50 000 fp32 with 5, and the 3840 x 500 000 fp64 slice with 3.  Every output of the two kernels is compared as bytes first.
Usage: k1_rows8_ab.py [other_lib.so | -] [rows:cells:f32|f64:covariates ...]   (shapes of one's own, e.g. to find where the two kernels cross)"""
import ctypes, os, sys
import numpy as np
import torch
sys.path.insert(0, '.')
from normalisr_amd import _lib
from normalisr_amd.association import _prepare_covariates
lib = _lib.load()
par = ctypes.CDLL(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != '-' else None
if par is not None:
	par.nrm_residualize_q.argtypes = lib.nrm_residualize_q.argtypes
	par.nrm_residualize_q.restype = lib.nrm_residualize_q.restype
st = torch.cuda.current_stream().cuda_stream
ALT = 7

def x_bytes(dt):
	return 8 if dt == torch.float64 else 4

def timeit(f, reps):
	for _ in range(2):
		f()
	e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
	e0.record()
	for _ in range(reps):
		f()
	e1.record()
	torch.cuda.synchronize()
	return e0.elapsed_time(e1) / reps

SHAPES = [(5000, 10000, torch.float32, 3), (16000, 50000, torch.float32, 5), (3840, 500000, torch.float64, 3)]
if len(sys.argv) > 2:
	SHAPES = [(int(r), int(n), torch.float64 if d == 'f64' else torch.float32, int(c)) for r, n, d, c in (a.split(':') for a in sys.argv[2:])]
for rows, n, dt, nc in SHAPES:
	reps = max(3, min(20, int(2e9 / (rows * n * x_bytes(dt)))))
	g = torch.Generator(device='cuda').manual_seed(5)
	x = torch.randn((rows, n), dtype=dt, device='cuda', generator=g) * 2 + 3
	rp, kp = (rows + 127) // 128 * 128, (n + 15) // 16 * 16
	rng = np.random.default_rng(1)
	dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	dc64, dci, dcr = _prepare_covariates(dc)
	d_c, d_dci = torch.from_numpy(dc64).cuda(), torch.from_numpy(np.ascontiguousarray(dci)).cuda()
	d_cmax = d_c.abs().max(dim=1).values.contiguous()
	def outputs():
		return dict(q=torch.full((int(lib.nrm_quant_bytes(rp, kp, 6)), ), 0x5A, dtype=torch.uint8, device='cuda'), ex=torch.full((rp, ), -1, dtype=torch.int32, device='cuda'),
					ss=torch.full((rp, ), float('nan'), dtype=torch.float64, device='cuda'), fix=torch.full((rp, 8), float('nan'), dtype=torch.float64, device='cuda'))
	def call(l, o):
		_lib.check(l.nrm_residualize_q(x.data_ptr(), _lib.NRM_F64 if dt == torch.float64 else _lib.NRM_F32, rows, n, n, d_c.data_ptr(), nc, n, d_dci.data_ptr(), int(dcr), 0, 0,
									   rp, o['ss'].data_ptr(), 0, 6, o['q'].data_ptr(), o['ex'].data_ptr(), 0, d_cmax.data_ptr(), o['fix'].data_ptr(), st))
	def variants(o):
		def p():
			call(par, o)
		def off():
			os.environ['NRM_DEBUG'] = 'k1_rows8=0'
			call(lib, o)
		def on():
			os.environ['NRM_DEBUG'] = 'k1_rows8=1'
			call(lib, o)
		return ((('parent', p), ) if par is not None else ()) + (('rows8=0', off), ('rows8', on))
	outs = {}
	for name, _ in variants(None):
		o = outputs()
		dict(variants(o))[name]()
		torch.cuda.synchronize()
		outs[name] = o
	base = 'parent' if par is not None else 'rows8=0'
	for name in ('rows8=0', 'rows8'):
		print('%d x %d: %s against %s: %s' % (rows, n, name, base, ', '.join('%s %s' % (k, 'same bytes' if torch.equal(outs[name][k].view(torch.uint8), outs[base][k].view(torch.uint8)) else 'DIFFERENT') for k in outs[name])), flush=True)
	o = outs['rows8']
	del outs
	res = {name: [] for name, _ in variants(o)}
	for rep in range(ALT):
		for name, f in variants(o):
			res[name].append(timeit(f, reps))
	for k, v in res.items():
		print('%d x %d %s, %d covariates, ms: %-8s  min %.4f  median %.4f  max %.4f   runs %s' % (rows, n, str(dt)[6:], nc, k, min(v), float(np.median(v)), max(v), ' '.join('%.4f' % t for t in v)), flush=True)
	del x, o
os.environ.pop('NRM_DEBUG', None)
