"""GPU: nrm_chol_inverse (csrc/nrm_chol_inverse.hip) alone -- the inverse of one positive definite matrix by blocked Cholesky on the fp64 matrix cores -- held to
the criteria of tests/test_chol_inverse_cpu.py: in extended precision max |M N - I| / (|M|_inf |N|_inf) <= 4 r^2 u (Higham Thm 10.4, normwise; a cap, the observed
value is printed), symmetric bits, the same bits on a second run, pitches larger than r, the status rules, and no trace of a bad matrix in a following good call."""
import numpy as np
import pytest

from test_chol_inverse_cpu import U, residual, spd

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 128, 129, 130, 377, 1024)


@pytest.fixture(scope='module')
def torch():
	import torch
	return torch


def residual_cap(m, n):
	"""The residual of test_chol_inverse_cpu.residual, or an upper bound of it.  Up to 400 rows: the extended-precision value itself.  Beyond (numpy's longdouble
	product of two 1024 x 1024 matrices takes 12 s): the fp64 product's value plus that product's own rounding, |fl(M N) - M N|_ij <= gamma_r sum_k |M_ik| |N_kj|
	<= (r + 2) u |M|_inf |N|_inf (Higham, eq. 3.13) -- never below the extended-precision value, so the assertion asks no less."""
	r = m.shape[0]
	if r <= 400:
		return residual(m, n)
	return float(np.abs(m @ n - np.eye(r)).max() / (np.abs(m).sum(axis=1).max() * np.abs(n).sum(axis=1).max())) + (r + 2) * U


class Inverse:
	"""One workspace and one status pair for every call of a size, as a plan holds them."""

	def __init__(self, torch, r, ldm=None, ldi=None):
		from normalisr_amd import _lib
		self.torch, self.lib, self.check = torch, _lib.load(), _lib.check
		self.r, self.ldm, self.ldi = r, ldm or r, ldi or r
		self.ws = torch.full((int(self.lib.nrm_chol_inverse_workspace(r)), ), np.nan, dtype=torch.float64, device='cuda')
		self.status = torch.zeros((2, ), dtype=torch.int32, device='cuda')

	def __call__(self, m):
		torch, r = self.torch, self.r
		d_m = torch.full((r, self.ldm), np.nan, dtype=torch.float64, device='cuda')
		d_m[:, :r] = torch.as_tensor(np.ascontiguousarray(m)).cuda()
		keep = d_m.clone()
		d_inv = torch.full((r, self.ldi), np.nan, dtype=torch.float64, device='cuda')
		self.check(self.lib.nrm_chol_inverse(d_m.data_ptr(), self.ldm, r, d_inv.data_ptr(), self.ldi, self.ws.data_ptr(), self.status.data_ptr(),
											 torch.cuda.current_stream().cuda_stream))
		torch.cuda.synchronize()
		assert torch.equal(torch.nan_to_num(d_m, nan=-7.0), torch.nan_to_num(keep, nan=-7.0))  # the input is not modified
		inv = d_inv.cpu().numpy()
		assert np.isnan(inv[:, r:]).all()  # nothing beyond column r
		return inv[:, :r]

	def counts(self):
		s = self.status.cpu().numpy().copy()
		self.status.zero_()
		return list(s)


@pytest.mark.parametrize('r', SIZES)
def test_device_inverse_within_the_cholesky_bound(torch, r):
	rng = np.random.default_rng(2300 + r)
	run = Inverse(torch, r)
	for cond in (1.0, 1e4):
		m = spd(rng, r, cond)
		inv = run(m)
		res = residual_cap(m, inv)
		print('r', r, 'cond', cond, 'residual', res, 'bound', 4 * r * r * U)
		assert run.counts() == [0, 0] and np.isfinite(inv).all()
		assert res <= 4 * r * r * U
		assert np.array_equal(inv, inv.T)  # symmetric bits
		assert np.array_equal(run(m), inv)  # the same bits on a second run
		assert run.counts() == [0, 0]


def test_device_inverse_asymmetric_check(torch):
	"""An inverse with a known, unsymmetric-looking structure: M = D + rank one, D a ramp -- a row / column swap in a tile's write would survive a random
	matrix's residual only by luck; here every element is compared with numpy's inverse."""
	r = 200
	d = np.linspace(1.0, 3.0, r)
	v = np.cos(np.arange(r) * 0.37) * 0.2
	m = np.diag(d) + np.outer(v, v)
	inv = Inverse(torch, r)(m)
	ref = np.linalg.inv(m)
	assert np.abs(inv - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize('r', (65, 130))
def test_device_inverse_takes_pitches(torch, r):
	rng = np.random.default_rng(2311 + r)
	m = spd(rng, r, 1e4)
	inv = Inverse(torch, r, ldm=r + 7, ldi=r + 3)(m)
	assert np.array_equal(inv, Inverse(torch, r)(m))


@pytest.mark.parametrize('r', (2, 65, 129, 377))
def test_bad_matrices_leave_no_trace(torch, r):
	rng = np.random.default_rng(2320 + r)
	run = Inverse(torch, r)
	good = spd(rng, r, 1e4)
	want = run(good)
	assert run.counts() == [0, 0]
	q = np.linalg.qr(rng.normal(size=(r, r)))[0]
	lam = np.ones(r)
	lam[r // 2] = -0.5
	bad = (q * lam) @ q.T
	inv = run((bad + bad.T) / 2)
	assert (inv == 0).all() and run.counts() == [1, 0]  # an indefinite matrix: a pivot that is not positive
	assert np.array_equal(run(good), want) and run.counts() == [0, 0]
	for where in ((0, 0), (r - 1, 0), (r - 1, r - 1), (0, r - 1)):
		m = good.copy()
		m[where] = np.nan
		assert (run(m) == 0).all() and run.counts() == [0, 1], where
		assert np.array_equal(run(good), want) and run.counts() == [0, 0]
	m = good.copy()
	m[r - 1, r - 1] = np.inf
	assert (run(m) == 0).all()
	assert (run((bad + bad.T) / 2) == 0).all()
	assert run.counts() == [1, 1]  # the counters add up over calls
	assert np.array_equal(run(good), want) and run.counts() == [0, 0]


def test_device_and_host_twin_agree(torch):
	"""Not the same bits (the matrix cores' inner order is the hardware's), the same inverse: both within the bound of the same matrix, and of each other."""
	from test_chol_inverse_cpu import host_inverse
	r = 129
	m = spd(np.random.default_rng(2340), r, 1e4)
	dev, host = Inverse(torch, r)(m), host_inverse(m)[0]
	assert np.abs(dev - host).max() <= 4 * r * r * U * 1e4 * np.abs(host).max()  # forward error <= condition x backward error
