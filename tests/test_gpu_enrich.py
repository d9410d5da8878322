"""GPU checks of the gene-set enrichment (normalisr_amd/enrich.py, csrc/nrm_enrich.hip): the pack and overlap kernels bit for bit against integer numpy on the
shapes where they can go wrong (rows ragged in the 64-bit word, in the 8-word step of the pack kernel and in the 16-word step and the 64 x 64 tile of the overlap
kernel; a pitch; byte values other than 1; a background), the Fisher kernel against the exact integer oracle of tests/enrich_numpy.py within 8 L u and bit for
bit against the host export, the three routes of enrich against one another and against the numpy restatement, and a planted pathway through top_pathway and
pccovt.  Nothing here is compared with goatools."""
import numpy as np
import pytest

import enrich_numpy as en
from normalisr_amd import _lib, enrich

pytestmark = pytest.mark.gpu


def _engine():
	from normalisr_amd import engine
	return engine.get_engine()


def _case(G, S, T, seed):
	"""A study byte matrix with pitch G + 7 whose padding is 255 and whose ones are 1, 2 or 255; sets as booleans; a background without every third gene."""
	rng = np.random.default_rng(seed)
	ld = G + 7
	buf = np.full((S, ld), 255, dtype=np.uint8)
	buf[:, :G] = np.where(rng.random((S, G)) < 0.4, rng.choice(np.array([1, 2, 255], dtype=np.uint8), (S, G)), 0)
	buf[:, 0] = 2  # (gene 0 is outside the background and present in every study row)
	if S > 1:
		buf[S - 1, :G] = 0  # one all-zero study
	member = rng.random((T, G)) < 0.3
	member[0] = True  # one all-ones set
	bg = np.arange(G) % 3 != 0
	if G == 2:
		bg = np.array([False, True])
	return buf, member, bg


def _pack_rows(mask):
	rows, cols = np.nonzero(mask)
	return enrich.pack_bits(rows, cols, mask.shape[0], mask.shape[1])


@pytest.mark.parametrize('G', [2, 63, 64, 65, 129, 1000])
def test_pack_and_overlap_bit_for_bit(G):
	eng = _engine()
	torch, lib = eng.torch, eng.lib
	for S in (1, 3, 70):
		for T in (1, 5, 257):
			buf, member, bg = _case(G, S, T, 1000 * G + 10 * S + T)
			W = (G + 63) // 64
			d_buf = eng.upload(buf)
			d_x = d_buf[:, :G]
			assert d_x.stride(0) == G + 7
			d_sets, d_bg = eng.upload(_pack_rows(member).view(np.int64)), eng.upload(_pack_rows(bg[None, :])[0].view(np.int64))
			words = torch.full((S, W), -1, dtype=torch.int64, device=eng.device)
			n = torch.full((S, ), -1, dtype=torch.int32, device=eng.device)
			K = torch.full((T, ), -1, dtype=torch.int32, device=eng.device)
			k = torch.full((S, T), -1, dtype=torch.int32, device=eng.device)
			_lib.check(lib.nrm_enrich_pack(d_x.data_ptr(), S, G, d_x.stride(0), d_bg.data_ptr(), words.data_ptr(), n.data_ptr(), eng._stream()))
			_lib.check(lib.nrm_enrich_overlap(words.data_ptr(), S, d_sets.data_ptr(), T, G, d_bg.data_ptr(), k.data_ptr(), K.data_ptr(), eng._stream()))
			study = (buf[:, :G] != 0) & bg
			assert np.array_equal(words.cpu().numpy().view(np.uint64), _pack_rows(study)), (G, S, T)  # (pad bits zero, the background applied)
			assert np.array_equal(n.cpu().numpy(), study.sum(axis=1)), (G, S, T)
			assert np.array_equal(K.cpu().numpy(), (member & bg).sum(axis=1)), (G, S, T)
			assert np.array_equal(k.cpu().numpy(), study.astype(np.int64) @ (member & bg).astype(np.int64).T), (G, S, T)
			if S > 1:
				assert n[S - 1].item() == 0 and (k[S - 1] == 0).all()
			# without a background: every gene counts
			_lib.check(lib.nrm_enrich_pack(d_x.data_ptr(), S, G, d_x.stride(0), None, words.data_ptr(), n.data_ptr(), eng._stream()))
			_lib.check(lib.nrm_enrich_overlap(words.data_ptr(), S, d_sets.data_ptr(), T, G, None, k.data_ptr(), K.data_ptr(), eng._stream()))
			assert np.array_equal(n.cpu().numpy(), (buf[:, :G] != 0).sum(axis=1)) and K[0].item() == G
			assert np.array_equal(k.cpu().numpy(), (buf[:, :G] != 0).astype(np.int64) @ member.astype(np.int64).T), (G, S, T)
			assert np.array_equal(d_buf.cpu().numpy(), buf)


def _fisher_device(eng, N, K, n, k):
	"""p and odds of the kernel for k (S, T), n (S), K (T)."""
	torch = eng.torch
	S, T = k.shape
	d_k, d_n, d_K = (eng.upload(np.ascontiguousarray(a, dtype=np.int32)) for a in (k, n, K))
	p = torch.full((S, T), -1.0, dtype=torch.float64, device=eng.device)
	odds = torch.full((S, T), -1.0, dtype=torch.float64, device=eng.device)
	_lib.check(eng.lib.nrm_enrich_fisher(d_k.data_ptr(), d_n.data_ptr(), d_K.data_ptr(), S, T, int(N), p.data_ptr(), odds.data_ptr(), eng._stream()))
	return p.cpu().numpy(), odds.cpu().numpy()


def _fisher_host(tab):
	cols = [np.ascontiguousarray(tab[:, i]) for i in range(4)]
	out = np.full(len(tab), np.nan)
	assert _lib.load().nrm_fisher_host(*(c.ctypes.data for c in cols), len(tab), out.ctypes.data) == 0
	return out


def test_fisher_kernel_on_every_small_table():
	"""Every table with N <= 12: per N, launches over all (n, K) with k = lo + c for c = 0 .. N (clamped to the support), gathered into one value per table."""
	eng = _engine()
	tab, exact, length = en.tables('small')
	got = {}
	for N in range(1, 13):
		a = np.arange(N + 1)
		lo, hi = np.maximum(0, a[:, None] + a[None, :] - N), np.minimum(a[:, None], a[None, :])
		for c in range(N + 1):
			k = np.minimum(lo + c, hi)
			p, odds = _fisher_device(eng, N, a, a, k)
			with np.errstate(divide='ignore', invalid='ignore'):
				want = np.where((a[:, None] > 0) & (a[None, :] > 0), (k / a[:, None]) / (a[None, :] / N), 0.0)
			assert np.array_equal(odds, want)
			for n in a:
				for K in a:
					key = (N, int(K), int(n), int(k[n, K]))
					assert got.setdefault(key, p[n, K]) == p[n, K]
	dev = np.array([got[tuple(row)] for row in tab.tolist()])
	assert len(got) == len(tab)
	assert np.array_equal(dev, _fisher_host(tab))  # the same header on the host: the same bits
	err = np.array([en.relative_error(v, ex) for v, ex in zip(dev, exact)])
	print('small: largest error {:.3g} L u'.format((err / (length * en.UNIT)).max()))
	assert (err <= 8 * length * en.UNIT).all(), tab[np.argmax(err / length)]


def test_fisher_kernel_on_the_large_tables():
	eng = _engine()
	tab, exact, length = en.tables('large')
	dev = np.array([_fisher_device(eng, N, np.array([K]), np.array([n]), np.array([[k]]))[0][0, 0] for N, K, n, k in tab.tolist()])
	assert np.array_equal(dev, _fisher_host(tab))
	err = np.array([en.relative_error(v, ex) for v, ex in zip(dev, exact)])
	print('large: errors in L u', err / (length * en.UNIT))
	assert (err <= 8 * length * en.UNIT).all()


def _same(a, b):
	return all(np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f))) for f in ('k', 'K', 'n', 'p', 'odds', 'top', 'top_records')) and a.N == b.N


def test_routes_agree_to_the_bit_and_with_numpy(monkeypatch):
	"""G = 129, T = 40, S = 70 (two tiles of studies): a numpy matrix, the same matrix in HBM, and the whole-problem entry."""
	eng = _engine()
	G, T, S = 129, 40, 70
	rng = np.random.default_rng(129)
	names = np.array(['gene{}'.format(i) for i in range(G)])
	member = rng.random((T, G)) < rng.uniform(0.05, 0.5, (T, 1))
	member[7] = member[3]  # two equal sets: a tie in p that goes to the lower index
	x = (rng.random((S, G)) < 0.2).astype(np.uint8)
	x[:20] |= (member[rng.integers(0, T, 20)] & (rng.random((20, G)) < 0.8)).astype(np.uint8)  # studies that do overlap a set
	x[S - 1] = 0
	bgmask = rng.random(G) < 0.9
	sets = enrich.GeneSets(['set{}'.format(t) for t in range(T)], ['label{}'.format(t) for t in range(T)], np.arange(T), [(t, names[g]) for t, g in zip(*np.nonzero(member))])
	bound = sets.bind(names, bg=bgmask)
	assert len(bound) == T and bound.N == int(bgmask.sum())
	monkeypatch.delenv('NRM_HOST_ENTRY', raising=False)
	a = enrich.enrich(x, bound, nmin=3)
	assert isinstance(a.p, np.ndarray) and a.p.shape == (S, T) and a.k.dtype == np.int32 and a.top.dtype == np.int64
	b = enrich.enrich(eng.upload(x), bound, nmin=3)
	c = enrich.enrich(x.astype(bool), sets, namet=names, bg=bgmask, nmin=3)
	d = enrich.enrich(eng.upload(x), bound, nmin=3, device_out=True)
	assert d.p.is_cuda and d.k.is_cuda and isinstance(d.top, np.ndarray)
	d.k, d.K, d.n, d.p, d.odds = (t.cpu().numpy() for t in (d.k, d.K, d.n, d.p, d.odds))
	monkeypatch.setenv('NRM_HOST_ENTRY', '1')
	h = enrich.enrich(x, bound, nmin=3)
	monkeypatch.delenv('NRM_HOST_ENTRY')
	again = enrich.enrich(x, bound, nmin=3)
	assert _same(a, b) and _same(a, c) and _same(a, d) and _same(a, h) and _same(a, again)  # three routes, two runs: identical bits
	k, K, n, N, p, odds, top = en.enrich_numpy(x, member, bgmask, nmin=3)
	assert np.array_equal(a.k, k) and np.array_equal(a.K, K) and np.array_equal(a.n, n) and a.N == N
	assert np.array_equal(a.top, top) and (top >= 0).sum() >= 10 and top[S - 1] == -1
	assert np.array_equal(a.p, p) and np.array_equal(a.odds, odds)  # (the restatement is the same arithmetic in Python floats)
	# independent of that arithmetic: every P-value within 8 L u of the exact integer oracle, and the oracle's own selection
	exact = {}
	rounded = lambda *tab: float(exact.setdefault(tab, en.fisher_exact_fraction(*tab)))
	assert np.array_equal(en.enrich_numpy(x, member, bgmask, nmin=3, pvalue=rounded)[6], a.top)
	assert len(exact) > 1000
	for s_, t_ in np.argwhere((n[:, None] > 0) & (K[None, :] > 0)).tolist():
		tab = (N, int(K[t_]), int(n[s_]), int(k[s_, t_]))
		lo, hi = en.support(*tab[:3])
		assert en.relative_error(a.p[s_, t_], exact[tab]) <= 8 * (hi - lo + 1) * en.UNIT, tab
	assert np.array_equal(a.top_records['p'][top >= 0], p[np.arange(S), top][top >= 0]) and np.array_equal(a.top_records['k'][top >= 0], k[np.arange(S), top][top >= 0])
	assert np.array_equal(a.p_bonferroni, np.minimum(1.0, p * T))
	s = int(np.flatnonzero(top >= 0)[0])
	rows = a.table(s)
	assert [r[7] for r in rows] == [sets.names[t] for t in np.argsort(p[s], kind='stable')] and rows == h.table(s)
	t0 = int(top[s])
	row = next(r for r in rows if r[7] == sets.names[t0])
	assert row[8].split(',') == names[(x[s] != 0) & member[t0] & bgmask].tolist() and row[5] == '{}/{}'.format(k[s, t0], n[s]) and row[6] == '{}/{}'.format(K[t0], N)
	assert a.genes(t0).tolist() == names[member[t0] & bgmask].tolist()
	# one study as a list of names, of rows, and of rows in HBM
	idx = np.flatnonzero(x[s])
	one = enrich.enrich(names[idx].tolist(), bound, nmin=3)
	assert np.array_equal(one.p[0], a.p[s]) and one.top[0] == a.top[s] and one.top_sets(0) == sets.names[t0]
	for form in (idx, eng.upload(idx)):
		assert np.array_equal(enrich.enrich(form, bound, nmin=3).p, one.p)
	with pytest.raises(ValueError, match='No GO enrichment found for given criteria.'):
		a.top_sets(S - 1)


def _planted(tmp_path):
	names = np.array(['g{:02d}'.format(i) for i in range(60)])
	net = np.zeros((60, 60), dtype=bool)
	net[:20, :] = True
	net[:, :20] = True
	net[np.arange(60), np.arange(60)] = False
	rng = np.random.default_rng(60)
	lines = []
	for d in range(9):
		if d == 4:
			lines.append('A\tthe planted pathway\t' + '\t'.join(names[[11, 3, 7, 0, 9, 1, 5, 10, 2, 8, 6, 4]]))
		genes = names if d == 0 else names[np.concatenate([rng.choice(20, 3 if d == 1 else 0, replace=False), 20 + rng.choice(40, 12, replace=False)])]
		lines.append('decoy{}\tnothing\t'.format(d) + '\t'.join(genes))
	(tmp_path / 'sets.gmt').write_text('\n'.join(lines) + '\n')
	return names, net, str(tmp_path / 'sets.gmt')


def test_planted_pathway_through_top_pathway_and_pccovt(tmp_path):
	from normalisr_amd import gocovt
	eng = _engine()
	names, net, gmt = _planted(tmp_path)
	sets = enrich.read_gmt(gmt)
	assert len(sets) == 10
	principals, res, top, genes = enrich.top_pathway(net, names, sets, n=15)
	assert principals == names[:20].tolist() and top == 'A' and genes == names[:12].tolist()  # (namet order, not the file's)
	assert res.n.tolist() == [20] and res.N == 60 and res.k[0, sets.names.index('A')] == 12 and res.top_records['K'][0] == 12
	assert res.odds[0, 0] == 1.0 and res.table(0)[0][7] == 'A' and res.table(0)[0][8] == ','.join(genes)
	again = enrich.top_pathway(eng.upload(net), names, sets.bind(names), n=15)  # the network in HBM, the sets bound once
	assert again[0] == principals and again[2:] == (top, genes) and np.array_equal(again[1].p, res.p)
	with pytest.raises(ValueError, match='No GO enrichment found for given criteria.'):
		enrich.top_pathway(net, names, sets, n=15, nmin=13)
	rng = np.random.default_rng(1)
	dt = rng.normal(size=(60, 200))
	dt[:12] += rng.normal(size=200)[None, :]
	dc = np.ones((1, 200))
	out = gocovt.pccovt(dt, dc, names, genes)
	assert out.shape == (2, 200) and np.isfinite(out).all() and np.array_equal(out[0], dc[0])


def test_command_line_writes_the_pathway_for_pccovt(tmp_path):
	"""`normalisr enrich` in this process: through the whole-problem entry, the files it writes."""
	from normalisr_amd import run
	names, net, gmt = _planted(tmp_path)
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('net.tsv'), net.astype(int), delimiter='\t', fmt='%i')
	run.file_write_txtlist(f('genes.txt'), names)
	run.enrich(dict(net_in=f('net.tsv'), genes_in=f('genes.txt'), pathway_out=f('pathway.txt'), gmt=gmt, go=None, key='id', n=15, nmin=5, master_out=f('master.txt'),
					goe_out=f('goe.tsv'), go_out=f('go.txt')))
	assert run.file_read_txtlist(f('pathway.txt')).tolist() == names[:12].tolist() and run.file_read_txtlist(f('master.txt')).tolist() == names[:20].tolist()
	assert run.file_read_txtlist(f('go.txt')).tolist() == ['A']
	table = [line.split('\t') for line in open(f('goe.tsv')).read().splitlines()]
	assert tuple(table[0]) == enrich.COLUMNS and len(table) == 11 and table[1][7] == 'A' and table[1][5:7] == ['12/20', '12/60']
