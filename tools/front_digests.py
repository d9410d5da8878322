"""SHA-256 digests of everything the front half of the C library returns, from fixed seeds: nrm_lcpm_host and nrm_lcpm_csr_host (normalize 0 and 1, with and
without the covariate rows, fp32 and fp64 output), nrm_compute_var_host (stepmax 1 and 3), nrm_normvar_host (1, 8, 9 and 32 covariates: both routes; keepvar 0
and 1; gene 0 is a nearly flat weighted row, rho = 1e-6, which the rule of csrc/nrm_nv_scale.h marks for the rescale) and cplan.FrontPlan (0 and 4 user covariates,
fp32 and fp64, stepmax 1 and 3: the eager step, the captured one and a replay, each with the plan's info()).  Shapes 70 x 131 and 33 x 64: more than one row tile
of 32, a ragged last tile, ragged cells.  No torch.  Two builds of the library that compute the same bits print the same JSON:

    python tools/with_lib.py <other libnormalisr_hip.so> tools/front_digests.py --out a.json;  python tools/front_digests.py --out b.json

Usage: front_digests.py [--out FILE]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

sys.modules['torch'] = None  # `import torch` raises ImportError here
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from normalisr_amd import _lib, cplan  # noqa: E402

SHAPES = ((70, 131), (33, 64))
F = {np.dtype(np.float32): _lib.NRM_F32, np.dtype(np.float64): _lib.NRM_F64}


def vp(a):
	return None if a is None else ctypes.c_void_p(a.ctypes.data)


def sha(a):
	return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def counts(rows, n, seed):
	"""int32 counts with a read in every cell and a zero in most genes."""
	rng = np.random.default_rng(seed)
	x = rng.poisson(np.exp(rng.normal(0.3, 1.0, rows))[:, None] * np.exp(rng.normal(0.0, 0.4, n))[None, :]).astype(np.int32)
	x[0, x.sum(axis=0) == 0] = 1
	return x


def lcpm_digests(lib, x):
	rows, n = x.shape
	r, c = np.nonzero(x)
	indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int64)
	indices, data = c.astype(np.int32), np.ascontiguousarray(x[r, c])
	out = {}
	for csr in (0, 1):
		for normalize in (0, 1):
			for with_cov in (0, 1):
				for dt in (np.float32, np.float64):
					res, cov = np.empty((rows, n), dtype=dt), np.empty((3, n)) if with_cov else None
					zero, info = np.empty(rows, dtype=np.int64), np.zeros(2, dtype=np.int64)
					tail = (normalize, -1, vp(res), F[np.dtype(dt)], vp(cov), vp(zero), vp(info))
					if csr:
						_lib.check(lib.nrm_lcpm_csr_host(vp(indptr), vp(indices), vp(data), _lib.NRM_I32, rows, n, int(data.size), *tail))
					else:
						_lib.check(lib.nrm_lcpm_host(vp(x), _lib.NRM_I32, rows, n, *tail))
					key = '%s normalize=%d cov=%d %s' % ('csr' if csr else 'dense', normalize, with_cov, np.dtype(dt).name)
					out[key] = dict(lcpm=sha(res), cov=sha(cov) if with_cov else None, gene_zero=sha(zero), info=[int(v) for v in info])
	return out


def covariates(rng, nc, n):
	"""nc - 1 standard normal rows and the constant row."""
	return np.ascontiguousarray(np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))]))


def compute_var_digests(lib, rows, n, seed):
	rng = np.random.default_rng(seed)
	y = np.log1p(rng.poisson(3.0, (rows, n)) * np.exp(rng.normal(0.0, 0.5, n))[None, :])
	c = covariates(rng, 3, n)
	out = {}
	for stepmax in (1, 3):
		w, state = np.empty(n), np.zeros(2)
		_lib.check(lib.nrm_compute_var_host(vp(y), _lib.NRM_F64, rows, n, vp(c), 3, stepmax, 1e-6, vp(w), vp(state)))
		out['stepmax=%d' % stepmax] = dict(w=sha(w), state=sha(state), steps=int(state[1]))
	return out


def normvar_digests(lib, rows, n, seed):
	rng = np.random.default_rng(seed)
	y = np.log1p(rng.poisson(3.0, (rows, n)).astype(np.float64))
	lnw, wt = rng.normal(0.0, 0.3, n), rng.uniform(0.2, 1.0, rows)
	y[0] = 5.0 * (1.0 + 1e-6 * rng.normal(size=n)) * np.exp(-lnw * wt[0])  # y e = 5 (1 + 1e-6 z): both variance sums cancel
	out = {}
	for nc in (1, 8, 9, 32):
		c = covariates(rng, nc, n)
		for keepvar in (0, 1):
			res, zero = np.empty((rows, n)), ctypes.c_int64(-1)
			_lib.check(lib.nrm_normvar_host(vp(y), _lib.NRM_F64, rows, n, vp(lnw), vp(wt), vp(c), nc, 1e-8, keepvar, vp(res), _lib.NRM_F64, ctypes.byref(zero)))
			out['nc=%d keepvar=%d' % (nc, keepvar)] = dict(out=sha(res), zero_rank=int(zero.value))
	return out


def plan_digests(x, seed):
	rows, n = x.shape
	rng = np.random.default_rng(seed)
	user = np.vstack([(rng.random((2, n)) < 0.4).astype(np.float64), rng.normal(size=(2, n))])  # two rows normcov leaves alone, two it centres and scales
	out = {}
	for n_cov in (0, 4):
		for dt in (np.float32, np.float64):
			for stepmax in (1, 3):
				steps = []
				with cplan.FrontPlan(x, user[:n_cov] if n_cov else None, stepmax=stepmax, out_dtype=dt) as plan:
					for _ in range(3):  # eager, captured, replayed
						plan.step()
						near = plan.check()
						got = plan._fetch(dtn=True, dcn=True, w=True, wt=True, lcpm=True, cov=True)
						steps.append(dict({k: sha(v) for k, v in got.items()}, near_constant=near, info=plan.info()))
				out['cov=%d %s stepmax=%d' % (n_cov, np.dtype(dt).name, stepmax)] = steps
	return out


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument('--out', default=None)
	args = ap.parse_args()
	lib = _lib.load()
	rec = {}
	for i, (rows, n) in enumerate(SHAPES):
		x = counts(rows, n, 100 + i)
		rec['%dx%d' % (rows, n)] = dict(lcpm=lcpm_digests(lib, x), compute_var=compute_var_digests(lib, rows, n, 200 + i), normvar=normvar_digests(lib, rows, n, 300 + i),
										front_plan=plan_digests(x, 400 + i))
	assert sys.modules['torch'] is None
	text = json.dumps(rec, indent=1, sort_keys=True)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, 'w') as f:
			f.write(text + '\n')
	print(text)


if __name__ == '__main__':
	main()
