"""CPU: the parts of norm.ComputeVarPlan that need no device.  nrm_fitvar_pinv_host runs, with one lane, the routine the plan's pseudo-inverse kernel runs in
LDS (csrc/nrm_jacobi_lanes.h: the same cyclic sequence of rotations), so its ranks and pseudo-inverses are held to inv_rank's here; and the plan refuses bad
arguments with the classes compute_var raises before anything touches a device."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import close
from normalisr_amd import _lib
from normalisr_amd.association import inv_rank

TOL = 1e-8
CELLS = 2000


def _pinv_host(m, tol=TOL):
	m = np.ascontiguousarray(m, dtype=np.float64)
	n = m.shape[0]
	inv, rank = np.full((n, n), np.nan), ctypes.c_int64(-1)
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	_lib.check(_lib.load().nrm_fitvar_pinv_host(vp(m), n, float(tol), vp(inv), ctypes.byref(rank)))
	return inv, rank.value


def _covariates(kind, n, rng):
	"""(n, CELLS) covariates and the rank they have by construction."""
	if kind == 'full':
		return rng.normal(size=(n, CELLS)), n
	if kind == 'onehot':  # n - 1 one-hot batches and the intercept, which is their sum
		if n == 1:
			return np.ones((1, CELLS)), 1
		batch = np.arange(CELLS) % (n - 1)
		rng.shuffle(batch)
		return np.vstack([(batch[None, :] == np.arange(n - 1)[:, None]).astype(np.float64), np.ones((1, CELLS))]), n - 1
	assert kind == 'duplicate'
	c = rng.normal(size=(n, CELLS))
	if n > 1:
		c[n - 1] = c[0]
	return c, max(n - 1, 1)


@pytest.mark.parametrize('n', [1, 2, 8, 9, 26, 63])
@pytest.mark.parametrize('kind', ['full', 'onehot', 'duplicate'])
@pytest.mark.parametrize('spread', [False, True])
def test_pinv_host_against_inv_rank(n, kind, spread):
	rng = np.random.default_rng(100 * n + 10 * len(kind) + spread)
	c, rank = _covariates(kind, n, rng)
	u = 10.0**rng.uniform(-1, 1, CELLS) if spread else np.ones(CELLS)  # (the weights 1 / scale of a later iteration: two decades)
	cu = c * u
	m = np.matmul(cu, cu.T)
	s = np.linalg.svd(m, compute_uv=False)
	assert not ((s > TOL * s[0] / 100) & (s < TOL * s[0] * 100)).any()  # no singular value near the threshold: the rule alone decides the rank
	ref, rref = inv_rank(m, tol=TOL)
	got, r = _pinv_host(m)
	print(n, kind, spread, 'rank', r, 'max scaled error %.3g' % np.abs((got - ref) * s[0]).max())
	assert r == rref == rank
	assert np.array_equal(got, got.T) and close(got * s[0], ref * s[0], 1e-9, floor=1.0)


def test_pinv_host_refuses_bad_arguments():
	with pytest.raises(ValueError):
		_pinv_host(np.eye(65))
	with pytest.raises(ValueError):
		_pinv_host(np.eye(3), tol=0.0)
	assert _pinv_host(np.eye(64))[1] == 64  # ([C;1][C;1]^T of 63 covariates)


def test_plan_workspace_is_sized_from_the_shape():
	lib = _lib.load()
	assert lib.nrm_fitvar_plan_workspace(0, 3) == 0 and lib.nrm_fitvar_plan_workspace(100, 0) == 0 and lib.nrm_fitvar_plan_workspace(100, 64) == 0
	small, big = lib.nrm_fitvar_plan_workspace(100, 3), lib.nrm_fitvar_plan_workspace(10000, 63)
	assert small >= 100 + 6 and big >= 10000 + 2016 * 40  # (the new scale and a triangle per 256 cells, at the least)


def test_plan_argument_validation_before_device():
	pytest.importorskip('torch')
	from normalisr_amd.norm import ComputeVarPlan, compute_var
	dt, dc = np.zeros((5, 20)), np.ones((2, 20))
	for call in (ComputeVarPlan, compute_var):
		for kw in (dict(eps=0.0), dict(eps=-1.0), dict(stepmax=0), dict(stepmax=-2)):
			with pytest.raises(ValueError):
				call(dt, dc, **kw)
		for bad in (np.ones((0, 20)), np.ones((64, 20))):
			with pytest.raises(NotImplementedError):
				call(dt, bad)
		with pytest.raises(ValueError):
			call(dt, np.ones((2, 19)))
		with pytest.raises(ValueError):
			call(dt, np.ones(20))
		with pytest.raises(ValueError):
			call(np.zeros((0, 20)), dc)
	with pytest.raises(ValueError):  # a host array: compute_var is the call for it
		ComputeVarPlan(dt, dc)
