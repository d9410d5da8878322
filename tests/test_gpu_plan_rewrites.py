"""Resident plans whose inputs are rewritten IN PLACE between steps (permutation nulls, batches of one shape, the normvar -> coex -> binnet chain).

A plan decides on its first step and replays one captured HIP graph afterwards; a graph captured before a rewrite only comes back on the step after
the rewrite, or after the plan has decided again -- so every case here runs at least four steps past the rewrite.  After each of them the plan's
results are compared with the public call (or a fresh plan) on the tensors as they are now, bit for bit where the neighbouring tests hold that, and
with the fp64 oracle at the neighbouring tests' tolerances.  Where the rewrite makes the plan decide again, the graph it replays afterwards must be a
new one; that is asserted right after the step that decides, before any step that could replay the old graph."""
import numpy as np
import pytest

import oracle
from test_gpu_parity import I8_FLOOR, R_FLOOR, close, gamma_close, p_close

pytestmark = pytest.mark.gpu


def _raw_write(t):
	"""A view of `t` whose writes torch does not count in t._version -- as a kernel of another library writing through the pointer would: nothing on
	the Python side can see such a write, only the device counters of the step that reads it."""
	return t.data


# ---- Single4Plan -----------------------------------------------------------------------------------------------------------------------------------------------


def _s4_problem(dtype, seed):
	rng = np.random.default_rng(seed)
	nx, ny, n, nc = 48, 90, 6000, 4
	dx = (rng.random((nx, n)) < 0.02).astype(dtype)
	dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	dy = (rng.normal(size=(ny, n)) + 0.4 * dx[3] + 0.3 * dc[0]).astype(dtype)
	return dx, dy, dc


def _s4_matches(plan, d_x, d_y, dc, dtype):
	"""The plan's results against association_tests_single4 on the tensors as they are now (bit for bit) and the oracle's per-grouping loop."""
	from normalisr_amd.single4 import association_tests_single4
	got = plan.results()
	pub = association_tests_single4(d_x, d_y, dc, return_dot=False)
	for a, b in zip(got, pub):
		assert (a is None and b is None) or np.array_equal(a, b)
	want = oracle.association_tests(d_x.cpu().numpy().astype(np.float64), d_y.cpu().numpy().astype(np.float64), dc, single=4, return_dot=False)
	tol = 1e-6 if dtype == np.float32 else 1e-9
	ok = want[0] > (1e-30 if dtype == np.float32 else 1e-290)  # (fp32 outputs end at 1e-38)
	assert p_close(got[0][ok], want[0][ok], 1e-6) and close(got[1], want[1], tol, 1e-12) and close(got[3], want[3], tol) and close(got[4], want[4], tol)


def _s4_after_rewrite(plan, d_x, d_y, dc, dtype, g0, decides=1, steps=5):
	"""Steps past a rewrite: the public call on the new values, then the step that decides anew (step `decides`) -- whose graph must not be g0, asserted
	BEFORE the step that would replay it -- then the lean steps (eager, capture, replay)."""
	for k in range(steps):
		plan.step()
		if k == decides:
			assert plan.lean is True and plan._graph.graph is None and plan._graph.graph is not g0
		assert plan.check() and plan.fallbacks == 0
		_s4_matches(plan, d_x, d_y, dc, dtype)
	assert plan._graph.graph is not None and plan._graph.graph is not g0
	return plan._graph.graph


def _s4_plan(dtype, seed):
	import torch
	from normalisr_amd.single4 import Single4Plan
	dx, dy, dc = _s4_problem(dtype, seed)
	d_x, d_y = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
	plan = Single4Plan(d_x, d_y, dc, return_dot=False)
	for _ in range(4):
		plan.step()
	assert plan.lean is True and plan._graph.graph is not None and plan.check()
	return plan, d_x, d_y, dc


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('rewrite', ['y_rows', 'x_entries_added', 'x_row_permuted', 'y_then_x'])
def test_single4_plan_decides_again_after_an_in_place_rewrite(dtype, rewrite, monkeypatch):
	"""Single4Plan: a write to dx or dy sends the next step through the public call and the one after decides anew (entry lists, covariates, flags and the
	Newton-Schulz step count of the new values) -- with a graph of its own: the graph of the old decision points at buffers torch has taken back."""
	import torch
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')  # (the size rule would leave so small a screen to K1 + K2)
	plan, d_x, d_y, dc = _s4_plan(dtype, 700 + len(rewrite))
	g0 = plan._graph.graph
	nnz0 = int((d_x != 0).sum())
	if rewrite in ('y_rows', 'y_then_x'):
		d_y[7] += 2.0 * d_x[5]
		d_y[20:23] = torch.flip(d_y[20:23], dims=(1, ))
	if rewrite == 'y_then_x':
		plan.step()  # the public call on the new genes; the design is written to before the plan has decided again: the next step decides
		assert plan.lean is None
		_s4_matches(plan, d_x, d_y, dc, dtype)
	if rewrite in ('x_entries_added', 'y_then_x'):
		free = torch.nonzero(d_x.sum(dim=0) == 0).flatten()[:40]
		d_x[3, free] = 1.0
		assert int((d_x != 0).sum()) == nnz0 + 40
	if rewrite == 'x_row_permuted':
		g = torch.Generator(device='cpu').manual_seed(7)
		d_x[5] = d_x[5][torch.randperm(d_x.shape[1], generator=g).cuda()]
		assert int((d_x != 0).sum()) == nnz0
	g1 = _s4_after_rewrite(plan, d_x, d_y, dc, dtype, g0, decides=0 if rewrite == 'y_then_x' else 1)
	if rewrite != 'y_then_x':
		return
	# after the re-decision: a value that is not finite lands in the genes unseen by torch -- the replayed graph's counters must say so, and the step
	# is then what the public call makes of these tensors (its exception, or its bits)
	_raw_write(d_y)[11, 17] = float('nan')
	plan.step()
	assert plan._graph.graph is g1
	assert plan.check() is False and plan.fallbacks == 1
	from normalisr_amd.single4 import association_tests_single4
	try:
		pub = association_tests_single4(d_x, d_y, dc, return_dot=False)
	except Exception as e:  # noqa: BLE001 -- whatever the public call raises, results() raises
		with pytest.raises(type(e)):
			plan.results()
	else:
		got = plan.results()
		for a, b in zip(got, pub):
			assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)


# ---- DePlan ------------------------------------------------------------------------------------------------------------------------------------------------------


def _de_problem(seed, nx, ny, n, nc):
	rng = np.random.default_rng(seed)
	dx = (rng.random((nx, n)) < 0.02).astype(np.float32)
	dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))]).astype(np.float32)
	dy = (rng.normal(size=(ny, n)) - 4).astype(np.float32)
	dy[:25] += 0.4 * dx[0]
	dy[25:40] += 0.3 * dx[1]
	return dx, dy, dc


def _de_matches(plan, d_x, d_y, dc, monkeypatch, i8):
	"""A step of the plan against a fresh plan run eagerly (NRM_GRAPH=0) on the tensors as they are now, bit for bit, and against the oracle."""
	from normalisr_amd.distributed import DePlan
	got = plan.results()
	monkeypatch.setenv('NRM_GRAPH', '0')
	eager = DePlan(d_x, d_y, dc)
	monkeypatch.delenv('NRM_GRAPH')
	eager.step()
	want = eager.results()
	for a, b in zip(got, want):
		assert np.array_equal(a, b)
	p, g, vx, vy = got
	po, go, ao, vgo, vto = oracle.de(d_x.cpu().numpy().astype(np.float64), d_y.cpu().numpy().astype(np.float64), dc.astype(np.float64))
	assert close(p, po, 1e-6, 1e-38) and close(vx, vgo, 1e-6) and close(vy, vto[0], 1e-6)
	assert gamma_close(g, vx, vy, go, vgo, vto[0], I8_FLOOR if i8 else R_FLOOR)  # (as r: rows rescaled by 1e3 keep its floor where it was)


def _de_plan(dx, dy, dc):
	import torch
	from normalisr_amd.distributed import DePlan
	d_x, d_y = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
	plan = DePlan(d_x, d_y, dc)
	for _ in range(3):
		plan.step()
	assert plan._graph.graph is not None
	plan.results()
	return plan, d_x, d_y


def _de_steps(plan, d_x, d_y, dc, monkeypatch, g0, decides, i8, steps=4):
	for k in range(steps):
		plan.step()
		if decides:  # eager on the first step past the write, captured again on the second
			assert plan._graph.graph is not g0 and (plan._graph.graph is None) == (k == 0)
		_de_matches(plan, d_x, d_y, dc, monkeypatch, i8)
	assert plan._graph.graph is not None
	if decides:
		assert plan._graph.graph is not g0
	else:
		assert plan._graph.graph is g0  # (nothing to decide: the graph reads the rows where they are)


@pytest.mark.parametrize('rewrite', ['x_permuted', 'x_entries_added', 'x_dense', 'y_rows'])
def test_de_plan_sparse_design_rebuilds_its_lists_after_a_design_rewrite(rewrite, monkeypatch):
	"""DePlan on the sparse-design path: the captured graph holds the ENTRY LISTS of the design (cells and values, built from the design as it was), so a
	write to the design must drop graph and lists; the expression rows are read where they are and need nothing."""
	import torch
	monkeypatch.setenv('NRM_DE_SPARSE', 'force')
	nx, ny, n, nc = 40, 300, 4500, 3
	dx, dy, dc = _de_problem(810 + len(rewrite), nx, ny, n, nc)
	plan, d_x, d_y = _de_plan(dx, dy, dc)
	assert not plan.streaming() and plan._state['sparse'][2].ok
	g0 = plan._graph.graph
	lists0 = plan._state['sparse'][2]
	nnz0 = int((d_x != 0).sum())
	g = torch.Generator(device='cpu').manual_seed(11)
	if rewrite == 'x_permuted':  # a permutation null: every design row's cells shuffled, the same entries
		for i in range(nx):
			d_x[i] = d_x[i][torch.randperm(n, generator=g).cuda()]
		assert int((d_x != 0).sum()) == nnz0
	elif rewrite == 'x_entries_added':
		free = torch.nonzero(d_x.sum(dim=0) == 0).flatten()[:60]
		d_x[0, free] = 1.0
		d_x[2, free[:30]] = 1.0
	elif rewrite == 'x_dense':  # a quarter of the entries set: no lists, K1 + the Gram engines
		d_x.copy_((torch.rand((nx, n), generator=g) < 0.25).to(torch.float32).cuda())
	else:
		d_y[3] *= 3.0
		d_y[50:60] += 0.5 * d_x[4]
	_de_steps(plan, d_x, d_y, dc, monkeypatch, g0, rewrite != 'y_rows', n >= 2048 and rewrite == 'x_dense')
	lists = plan._state['sparse'][2]
	if rewrite == 'x_dense':
		assert not lists.ok
	elif rewrite == 'y_rows':
		assert lists is lists0
	else:
		assert lists is not lists0 and lists.ok and lists.nnz == int((d_x != 0).sum())


@pytest.mark.parametrize('path', ['streaming', 'dense'])
@pytest.mark.parametrize('rewrite', ['y_times_1e3', 'y_times_1e-3', 'x_rewritten'])
def test_de_plan_after_rescaled_genes_and_a_new_design(path, rewrite, monkeypatch):
	"""DePlan on the streaming kernel (nx + nc <= 32) and on K1 + the integer Gram engine (NRM_DE_SPARSE=0, n >= 2048): expression rows rescaled in place by
	1e3 and 1e-3 -- K1's fixed-point scale of those rows changes, and the replayed graph must take it from the rows as they are --, and a new design."""
	import torch
	monkeypatch.setenv('NRM_DE_SPARSE', '0')
	nx = 4 if path == 'streaming' else 40
	ny, n, nc = 300, 4500, 3
	dx, dy, dc = _de_problem(830 + nx + len(rewrite), nx, ny, n, nc)
	dx = np.maximum(dx, (np.random.default_rng(5).random(dx.shape) < 0.2)).astype(np.float32)
	plan, d_x, d_y = _de_plan(dx, dy, dc)
	assert plan.streaming() == (path == 'streaming')
	g0 = plan._graph.graph
	if rewrite == 'y_times_1e3':
		d_y[:30] *= 1e3
		d_y[100:110] *= 1e3
	elif rewrite == 'y_times_1e-3':
		d_y[:30] *= 1e-3
		d_y[200:210] *= 1e-3
	else:
		g = torch.Generator(device='cpu').manual_seed(13)
		d_x.copy_((torch.rand((nx, n), generator=g) < 0.3).to(torch.float32).cuda())
	_de_steps(plan, d_x, d_y, dc, monkeypatch, g0, rewrite == 'x_rewritten', path == 'dense')


# ---- Single1Plan -------------------------------------------------------------------------------------------------------------------------------------------------


def _s1_matches(plan, d_dx, d_y, dc):
	from normalisr_amd.single1 import association_tests_single1
	dx, dy = d_dx.cpu().numpy(), d_y.cpu().numpy()
	got = plan.results()
	pub = association_tests_single1(dx, dy, dc, return_dot=False, lowmem=False)
	for a, b in zip(got, pub):
		assert (a is None and b is None) or np.array_equal(a, b)
	want = oracle.association_tests(dx, dy, dc, single=1, return_dot=False, lowmem=False)
	assert p_close(got[0], want[0], 1e-6) and close(got[1], want[1], 1e-9, 1e-12) and close(got[3], want[3], 1e-9) and close(got[4], want[4], 1e-9)
	assert close(got[2], want[2], 1e-8, 1e-9)


def test_single1_plan_after_design_and_gene_rewrites():
	"""Single1Plan: the design written to in place -> lists, buffers and graph built anew (four steps past it, each the public call's bits); the genes
	written to -> the same graph reads them; after the rebuild, a value that is not finite in the genes raises from results() what the public call raises."""
	import torch
	from normalisr_amd.single1 import Single1Plan, association_tests_single1
	rng = np.random.default_rng(850)
	nx, ny, n, nc = 40, 70, 6000, 3
	dx = (rng.random((nx, n)) < 1.0 / nx).astype(np.float64)
	dy = rng.normal(size=(ny, n))
	dy[:5] += 0.5 * dx[0]
	dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	d_dx, d_y = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
	plan = Single1Plan(d_dx, d_y, dc, return_dot=False, lowmem=False)
	for _ in range(4):
		plan.step()
	g0 = plan._graph.graph
	assert g0 is not None
	_s1_matches(plan, d_dx, d_y, dc)
	free = torch.nonzero(d_dx.sum(dim=0) == 0).flatten()[:40]
	d_dx[3, free] = 1.0
	d_dx[7] = d_dx[7][torch.randperm(n, generator=torch.Generator(device='cpu').manual_seed(3)).cuda()]
	for _ in range(4):
		plan.step()
		assert plan._graph.graph is not g0
		assert plan.n_kept == int(((d_dx.cpu().numpy() != 0).sum(axis=0) == 1).sum())
		_s1_matches(plan, d_dx, d_y, dc)
	g1 = plan._graph.graph
	assert g1 is not None and g1 is not g0
	d_y[9] += 2.0 * d_dx[3]
	d_y[30:33] = torch.flip(d_y[30:33], dims=(1, ))
	for _ in range(4):
		plan.step()
		_s1_matches(plan, d_dx, d_y, dc)
	assert plan._graph.graph is g1
	d_y[11, 17] = float('nan')
	plan.step()
	try:
		pub = association_tests_single1(d_dx.cpu().numpy(), d_y.cpu().numpy(), dc, return_dot=False, lowmem=False)
	except Exception as e:  # noqa: BLE001 -- whatever the public call raises, results() raises
		with pytest.raises(type(e)):
			plan.results()
	else:
		got = plan.results()
		assert all((a is None and b is None) or np.array_equal(a, b, equal_nan=True) for a, b in zip(got, pub))


# ---- NormvarPlan -------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_normvar_plan_after_in_place_rewrites(dtype):
	"""NormvarPlan: rows rewritten, then the whole matrix replaced by the next batch of the same shape (copy_); four steps past each, every one the bits
	of normvar(..., device_out=True) on the matrix as it is now and within 1e-6 of the oracle's scale."""
	import torch
	import normalisr_amd.normalisr as norm
	from normalisr_amd.norm import NormvarPlan
	rng = np.random.default_rng(870)
	nt, ns, nc = 70, 3001, 4
	dt = (rng.normal(size=(nt, ns)) - 9).astype(dtype)
	dc = np.vstack([rng.normal(size=(nc - 1, ns)), np.ones((1, ns))])
	w, wt = np.exp(0.3 * rng.normal(size=ns)), rng.uniform(0, 1.5, nt)
	d_dt = torch.from_numpy(dt).cuda()
	plan = NormvarPlan(d_dt, dc, w, wt)
	assert plan.lean
	for _ in range(3):
		plan.step()
	assert plan._graph.graph is not None and plan.check()

	def four_steps():
		for _ in range(4):
			out = plan.step()
			pub = norm.normvar(d_dt, dc, w, wt, device_out=True)
			assert torch.equal(out, pub[0]) and np.array_equal(plan.dcn, pub[1])
			ref = oracle.normvar(d_dt.cpu().numpy().astype(np.float64), dc, w, wt)
			got = plan.results()
			assert np.abs(got[0] - ref[0]).max() < 1e-6 * np.abs(ref[0]).max() and close(got[1], ref[1], 1e-12, 1e-15)
	d_dt[3] += 0.25 * torch.from_numpy(dc[0]).cuda().to(d_dt.dtype)
	d_dt[10:14] *= 1.5
	four_steps()
	d_dt.copy_(torch.from_numpy((rng.normal(size=(nt, ns)) * 2 - 6).astype(dtype)).cuda())  # the next batch
	four_steps()


# ---- CoexPlan ----------------------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_coex_plan_after_rescaled_and_rewritten_rows(dtype):
	"""CoexPlan (one rank): K1 overwrites the previous step's digit planes in place (CoexPlan._into).  Rows rescaled by 1e3 (their fixed-point scale
	changes) and one row rewritten to another distribution: four steps past each, every one the bits of a fresh plan and the oracle's results."""
	import torch
	from normalisr_amd.distributed import CoexPlan
	rng = np.random.default_rng(890)
	ng, n, nc = 120, 4500, 3
	lat = rng.normal(size=(1, n))
	dt = (rng.normal(size=(ng, n)) + 0.5 * rng.normal(size=(ng, 1)) * lat).astype(dtype)
	dc = np.vstack([rng.normal(size=(nc - 1, n)), np.ones((1, n))])
	x = torch.from_numpy(dt).cuda()
	plan = CoexPlan(x, dc)
	for _ in range(2):
		plan.step()

	def four_steps():
		for _ in range(4):
			plan.step()
			plan._flags_ok_everywhere()
			P, D, V = (np.array(a) for a in plan.assemble())
			fresh = CoexPlan(x, dc)
			fresh.step()
			fresh._flags_ok_everywhere()
			for a, b in zip((P, D, V), fresh.assemble()):
				assert np.array_equal(a, b)
			po, do, vo = oracle.coex(x.cpu().numpy().astype(np.float64), dc)
			s, so = np.sqrt(V.astype(np.float64)), np.sqrt(vo)
			r, ro = D / s[:, None] / s[None, :], do / so[:, None] / so[None, :]  # (as r: the 1e3 rows keep the floor where it was)
			if dtype == np.float32:
				assert close(P, po, 1e-6, 1e-38) and close(r, ro, 1e-6, 1e-7) and close(V, vo, 1e-6)
			else:
				assert p_close(P, po) and close(r, ro, floor=1e-13) and close(V, vo, 1e-12)
	x[:10] *= 1e3
	x[60:63] *= 1e3
	four_steps()
	x[20] = torch.from_numpy(np.log1p(rng.poisson(3.0, n)).astype(dtype) * 50.0).cuda()
	four_steps()
