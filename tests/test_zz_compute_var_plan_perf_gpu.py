"""GPU, collected after the parity files: a ComputeVarPlan step against the public compute_var on the same resident tensor in the same process, at the front
half's shape (5 000 genes x 10 000 cells, fp32 logCPM, 8 covariates of rank 7: four one-hot batches, lcpm's three and the intercept).  The plan runs the
public call's three streaming passes and removes its host round trips, so it must be faster or it has no reason to exist: the margin is zero, on purpose, and
no absolute time is asserted.  The public call is the code of the commit before the plan, measured here, not a stored number."""
import time

import numpy as np
import pytest

from test_gpu_parity import close

pytestmark = pytest.mark.gpu

NG, N, SEED = 5000, 10000, 18


def test_plan_step_is_faster_than_the_public_call():
	import torch
	import normalisr_amd.normalisr as norm
	from normalisr_amd.norm import ComputeVarPlan
	rng = np.random.default_rng(SEED)
	mu = np.exp(rng.normal(-1.0, 1.3, NG))
	x = rng.poisson(mu[:, None] * np.exp(rng.normal(0.0, 0.5, N))[None, :]).astype(np.int32)
	x[0, x.sum(axis=0) == 0] = 1
	onehot = (rng.integers(0, 4, N)[None, :] == np.arange(4)[:, None]).astype(np.float64)
	lc32, _, _, cov = norm.lcpm(torch.as_tensor(x).cuda(), device_out=True, out_dtype=np.float32)
	dc = norm.normcov(np.vstack([onehot, cov]))
	assert lc32.dtype == torch.float32 and dc.shape == (8, N) and np.linalg.matrix_rank(dc) == 7
	plan = ComputeVarPlan(lc32, dc, stepmax=1)
	for _ in range(5):  # eager, capture, replays
		plan.step()
	assert plan._graph.graph is not None
	w = plan.results()
	pub = norm.compute_var(lc32, dc, stepmax=1)
	assert close(w, pub, 1e-9, floor=1.0)
	plan_ms, pub_ms = [], []
	for _ in range(30):
		torch.cuda.synchronize()
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		e0.record()
		plan.step()
		e1.record()
		torch.cuda.synchronize()
		plan_ms.append(e0.elapsed_time(e1))
	for _ in range(3):
		norm.compute_var(lc32, dc, stepmax=1)
	for _ in range(30):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		norm.compute_var(lc32, dc, stepmax=1)
		torch.cuda.synchronize()
		pub_ms.append((time.perf_counter() - t0) * 1e3)
	a, b = float(np.median(plan_ms)), float(np.median(pub_ms))
	print('ComputeVarPlan.step() (HIP events, graph replay): median %.4f ms, min %.4f; public compute_var (synchronised): median %.4f ms, min %.4f'
		  % (a, min(plan_ms), b, min(pub_ms)))
	assert plan.check()
	assert a < b
