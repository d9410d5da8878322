"""Problems and the judge of the wide single=1 kernels (9 .. 32 covariates: nrm_single1_group_stats_wide, nrm_single1_group_info_wide and its host twin) --
TEST INFRASTRUCTURE ONLY, beside s1_reference.py, whose references (group_stats, group_info(gram=...), gram_from_parts, judge_group_info) work for any nc."""
import ctypes

import numpy as np

import s1_reference as s1
from s1_reference import F64, GB, HEAD, U, ULD, ld

GI_NC = [9, 16, 17, 32]
GI_NX = [1, 65]
GI_VARIANTS = ['plain', 'duplicate', 'zero covariate', 'one-hot', 'nearly dependent', 'no shared cells']
GS_NC = [9, 12, 16, 17, 31, 32]


def n_pairs(nc):
	nb = (nc + 7) // 8
	return nb * (nb + 1) // 2


def gi_problem(nx, nc, variant, seed=0):
	"""s1_reference.gi_problem for more than 8 covariates: grouping i owns 2 + i % 5 cells, 3 nc + 10 cells are shared (or none: dof <= 0 everywhere), and gpart
	has every block pair (bi <= bj) of 8 x 8 covariates, each as GB partial blocks that ONLY ADD UP to the block -- a kernel that drops a block pair or a partial
	sum misses the matrix.  The entries of the padding (covariates nc .. 8 nb) hold values that add up to nothing in particular: no kernel may read them.
	'plain' with nx >= 4: row 1 keeps nothing (vx 0 -> 1; flagged), row 2 takes a single value (not flagged with shared cells), row 3 has an infinite Gram entry.
	'one-hot': min(6, nc - 1) batches and the intercept, which is their sum (rank nc - 1)."""
	rng = np.random.default_rng([seed, nx, nc, 53])
	lens = [2 + i % 5 for i in range(nx)]
	n_common = 0 if variant == 'no shared cells' else 3 * nc + 10
	n = n_common + sum(lens)
	C = rng.normal(size=(nc, n))
	C[0] = 1.0
	if variant == 'duplicate':
		C[nc - 1] = C[0]
	if variant == 'zero covariate':
		C[1] = 0.0
	if variant == 'one-hot':
		k = min(6, nc - 1)
		batch = rng.permutation(n) % k
		C[1:1 + k] = batch[None] == np.arange(k)[:, None]
	if variant == 'nearly dependent':
		C[nc - 1] = C[nc - 2] + 1e-3 * rng.normal(size=n)
	seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
	cells = (n_common + np.arange(sum(lens))).astype(np.int64)
	xe = rng.uniform(0.25, 1.0, size=sum(lens))
	gs = np.asarray(s1.group_stats(seg, cells, xe, C, nc)[0], F64)
	nb = (nc + 7) // 8
	full = np.zeros((nb * 8, nb * 8))
	full[:nc, :nc] = C[:, :n_common] @ C[:, :n_common].T
	pad = np.arange(nb * 8) >= nc
	gpart = rng.normal(size=(n_pairs(nc), GB, 64)) * 1e-3 * (n_common > 0)
	q = 0
	for bi in range(nb):
		for bj in range(bi, nb):
			blk = full[bi * 8:bi * 8 + 8, bj * 8:bj * 8 + 8].ravel()
			live = ~(pad[bi * 8:bi * 8 + 8, None] | pad[None, bj * 8:bj * 8 + 8]).ravel()
			gpart[q, 0, live] += (blk - gpart[q].sum(axis=0))[live]
			gpart[q][:, ~live] = rng.normal(size=(GB, int((~live).sum()))) + 3.0
			q += 1
	rowinfo = np.array([[lens[i], xe[seg[i]:seg[i + 1]].min(), xe[seg[i]:seg[i + 1]].max()] for i in range(nx)])
	npair = nc * (nc + 1) // 2
	if variant == 'plain' and nx >= 4:
		gs[1, :] = 0.0
		rowinfo[1] = (0, np.inf, -np.inf)
		rowinfo[2, 1:] = 0.5
		gs[3, 0] = np.inf
	if variant == 'no shared cells' and nx >= 4:
		rowinfo[2, 1:] = 0.5  # the single value: flagged, no shared cell adds a 0
	return dict(gs=gs, gpart=gpart, rowinfo=rowinfo, n_common=n_common, nc=nc, nx=nx, npair=npair, dimreduce=1 if variant == 'plain' else 0)


def gi_reference(pb):
	return s1.group_info(pb['gs'], None, pb['rowinfo'], pb['n_common'], pb['nc'], pb['dimreduce'], gram=s1.gram_from_parts(pb['gpart'], pb['nc']))


def gi_host(lib, check, pb, extra_pitch=5, prefill=(0, 0, 0, 0, 0, -7, -7, -7)):
	"""nrm_single1_group_info_wide_host on the problem: (info (nx, record), varx, flags); the pitch padding must stay NaN."""
	nx, nc = pb['nx'], pb['nc']
	width = HEAD + nc + nc * nc
	pitch = width + extra_pitch
	info, varx, flags = np.full((nx, pitch), np.nan), np.full(nx, np.nan), np.array(prefill, np.int32)
	sel = np.full(8, -7, np.int64)
	sel[3] = pb['n_common']
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	gs, gp, rows = (np.ascontiguousarray(pb[k], dtype=F64) for k in ('gs', 'gpart', 'rowinfo'))
	check(lib.nrm_single1_group_info_wide_host(vp(gs), vp(gp), vp(rows), vp(sel), nc, nx, pb['dimreduce'], vp(info), pitch, vp(varx), vp(flags)))
	assert np.isnan(info[:, width:]).all(), 'written into the pitch padding'
	return info[:, :width].copy(), varx, flags


def gi_judge(info, varx, flags, pb, ref, plans):
	"""judge_group_info's outputs plus the plan columns bit for bit (plans: dof -> (len, 24), nrm_pvalue_plan_fill_many) and dof itself through ns and the rank."""
	ws = s1.judge_group_info(info, varx, flags, ref, pb['nc'])
	ws['plan (dof)'] = s1.bits(info[:, 2:HEAD].copy(), plans(ref['dof']), 'rec[2..25] == nrm_pvalue_plan_fill_many(dof)')
	return ws


def gs_problem(nc, exact, seed=0):
	"""Segments of s1.GS_LENS cells; ce (entries, nc) in segment order as nrm_single1_select writes it, and the (C, cells) that the reference gathers it from."""
	pb = s1.gs_problem(nc, seed, exact)
	pb['ce'] = np.ascontiguousarray(pb['C'][:, pb['cells']].T)
	return pb


def gs_reference(pb):
	"""The longdouble sums, and the bound of k_s1_group_stats_wide: every output is ONE chain of len fma over the segment's cells in their order, starting from 0
	(the comment above the kernel) -- len additions, so (len + 1) u sum |terms|; 16 x 2^-64 of the absolute sum for the reference itself."""
	nc, seg = pb['nc'], pb['seg']
	ref, _ = s1.group_stats(seg, pb['cells'], pb['xe'], pb['C'], nc)
	ab = np.zeros(ref.shape, s1.LD)
	iu = np.triu_indices(nc)
	for i in range(len(seg) - 1):
		a, b = int(seg[i]), int(seg[i + 1])
		cv, x = np.abs(ld(pb['ce'][a:b].T)), np.abs(ld(pb['xe'][a:b]))
		ab[i] = np.concatenate([(cv @ cv.T)[iu], cv @ x, [x @ x]])
	depth = (np.diff(seg) + 1).astype(F64)[:, None]
	return ref, depth * U * ab + 16 * ULD * ab
