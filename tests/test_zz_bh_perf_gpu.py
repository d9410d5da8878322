"""GPU, collected after the parity files: nrm_bh on a resident P-value vector against the only route there was for one before it -- download, then the host bh
(numpy.unique over every entry) -- in the same process on the same bytes, at 2^20 fp64 log-uniform P-values.  The device path exists to keep the result in HBM and
to be faster by orders of magnitude, so the margin is zero, on purpose, and no absolute time is asserted; tools/time_bh.py records the figures (profiles/bh.json)."""
import time

import numpy as np
import pytest

from normalisr_amd import _lib
from normalisr_amd import binnet as nb

pytestmark = pytest.mark.gpu

N, SEED = 1 << 20, 29


def test_bh_resident_is_faster_than_download_and_host_bh():
	from normalisr_amd import engine
	eng = engine.get_engine()
	torch, lib = eng.torch, eng.lib
	pv = 10.0 ** (-300 * np.random.default_rng(SEED).random(N))
	d_p = eng.upload(pv)
	out = torch.empty_like(d_p)
	nbytes = int(lib.nrm_bh_workspace_bytes(N, _lib.NRM_F64))
	work = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
	flags = torch.zeros(2, dtype=torch.int32, device=eng.device)

	def step():
		_lib.check(lib.nrm_bh(d_p.data_ptr(), _lib.NRM_F64, 1, N, N, out.data_ptr(), N, work.data_ptr(), nbytes, flags.data_ptr(), eng._stream()))
	dev_ms = []
	for i in range(7):  # 2 warm-ups, 5 timed
		torch.cuda.synchronize()
		e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
		e0.record()
		step()
		e1.record()
		torch.cuda.synchronize()
		if i >= 2:
			dev_ms.append(e0.elapsed_time(e1))
	host_ms = []
	for _ in range(3):
		torch.cuda.synchronize()
		t0 = time.perf_counter()
		q_host = nb.bh(eng.download(d_p))
		host_ms.append((time.perf_counter() - t0) * 1e3)
	a, b = float(np.median(dev_ms)), float(min(host_ms))
	print('nrm_bh resident, 2^20 fp64 (HIP events): median %.4f ms, min %.4f; download + host bh: best of 3 %.2f ms' % (a, min(dev_ms), b))
	assert flags.tolist() == [0, 1] and np.array_equal(out.cpu().numpy().view(np.uint8), q_host.view(np.uint8))
	assert a < b
