"""CPU checks of the gene-set enrichment (normalisr_amd/enrich.py, csrc/nrm_enrich.hip, csrc/nrm_fisher.h): the Fisher recurrence through the library's host
export against an exact integer oracle and against scipy, the readers on files written here, the selection rule, and the boundary (symbols, argument checks
before any device call, the parser).  No kernel is launched.  Nothing here is compared with goatools: the contract is the module's own."""
import ctypes
import os

import numpy as np
import pytest

import enrich_numpy as en
from conftest import ROOT
from normalisr_amd import _lib, enrich


def _fisher_host(tab):
	tab = np.ascontiguousarray(tab, dtype=np.int64)
	cols = [np.ascontiguousarray(tab[:, i]) for i in range(4)]
	out = np.full(len(tab), np.nan)
	rc = _lib.load().nrm_fisher_host(*(c.ctypes.data for c in cols), len(tab), out.ctypes.data)
	assert rc == 0, _lib.load().nrm_last_error()
	return out


_tables = en.tables


@pytest.mark.parametrize('name', ['small', 'seeded', 'large'])
def test_fisher_host_against_the_exact_oracle(name):
	"""Relative error <= 8 L u, L the support's length: a recurrence step rounds at most four times and the sums are of positive terms."""
	tab, exact, length = _tables(name)
	if name == 'seeded':
		assert len(tab) == 3000 and (tab[:, 0] < 400).all() and (tab[::5, 0] % 2 == 0).all() and (tab[::5, 1] * 2 == tab[::5, 0]).all()
	p = _fisher_host(tab)
	err = np.array([en.relative_error(v, ex) for v, ex in zip(p, exact)])
	print('{}: {} tables, largest error {:.3g} L u'.format(name, len(tab), (err / (length * en.UNIT)).max()))
	assert (p > 0).all() and (p <= 1).all()
	assert (err <= 8 * length * en.UNIT).all(), tab[np.argmax(err / length)]


def test_fisher_host_is_the_plain_recurrence():
	"""The Python restatement (IEEE doubles, no fused multiply-add) gives the library's bits: the header's arithmetic is what it says."""
	for name in ('small', 'large'):
		tab = _tables(name)[0]
		assert np.array_equal(_fisher_host(tab), np.array([en.fisher_recurrence(*row) for row in tab.tolist()]))


@pytest.mark.parametrize('name', ['small', 'seeded', 'large'])
def test_fisher_host_against_scipy(name):
	from scipy.stats import fisher_exact
	tab = _tables(name)[0]
	ref = np.array([fisher_exact([[k, n - k], [K - k, N - K - n + k]])[1] for N, K, n, k in tab.tolist()])
	np.testing.assert_allclose(_fisher_host(tab), ref, rtol=1e-9, atol=0)


def test_fisher_host_rejects_what_is_no_table():
	lib = _lib.load()
	out = np.zeros(1)
	for bad in ((10, 11, 3, 2), (10, 3, 11, 2), (10, 5, 5, 6), (10, 8, 8, 5), (0, 0, 0, 0), (10, -1, 3, 0), (2**31, 5, 5, 1)):
		cols = [np.array([v], dtype=np.int64) for v in bad]
		assert lib.nrm_fisher_host(*(c.ctypes.data for c in cols), 1, out.ctypes.data) == _lib.NRM_E_ARG, bad
	assert lib.nrm_fisher_host(None, None, None, None, 1, out.ctypes.data) == _lib.NRM_E_ARG
	assert lib.nrm_fisher_host(None, None, None, None, 0, None) == 0
	assert _fisher_host([(10, 0, 4, 0), (10, 4, 0, 0), (10, 10, 4, 4), (7, 3, 7, 3)]).tolist() == [1.0, 1.0, 1.0, 1.0]


def test_fisher_host_at_the_largest_gene_count():
	"""2^31 - 1 genes, the most the entries take: the mode's (n + 1)(K + 1) is a 62-bit product.  Supports short enough for the exact oracle, held to the same
	8 L u; the P-value is symmetric in (K, n) to the bit."""
	big = 2**31 - 1
	tab = np.array([(big, big - 5, big - 5, big - 7), (big, big - 5, big - 5, big - 10), (big, big - 1, big - 1, big - 2), (big, big, big, big), (big, 1, big, 1),
					(big, 1, big - 1, 0), (big, 3, big - 2, 2)], dtype=np.int64)
	p = _fisher_host(tab)
	assert np.array_equal(p, _fisher_host(tab[:, [0, 2, 1, 3]]))
	for (N, K, n, k), v in zip(tab.tolist(), p):
		lo, hi = en.support(N, K, n)
		assert 0 < v <= 1 and en.relative_error(v, en.fisher_exact_fraction(N, K, n, k)) <= 8 * (hi - lo + 1) * en.UNIT, (N, K, n, k, v)


# ---- readers --------------------------------------------------------------------------------------------------------------------------------------------------
OBO = """format-version: 1.2

[Term]
id: GO:1
name: root
namespace: biological_process

[Term]
id: GO:2
name: left
namespace: biological_process
alt_id: GO:20
is_a: GO:1 ! root

[Term]
id: GO:3
name: right
namespace: biological_process
is_a: GO:1 ! root

[Term]
id: GO:4
name: bottom
namespace: biological_process
is_a: GO:2 ! left
is_a: GO:3 ! right
relationship: part_of GO:9 ! not followed

[Term]
id: GO:5
name: deep
namespace: biological_process
is_a: GO:4

[Term]
id: GO:9
name: gone
namespace: biological_process
is_obsolete: true

[Typedef]
id: part_of
name: part of
"""


def _gaf(rows):
	lines = ['!gaf-version: 2.2', '!a comment']
	for gid, symbol, qualifier, term, evidence in rows:
		lines.append('\t'.join(['DB', gid, symbol, qualifier, term, 'REF:1', evidence, '', 'P', '', '', 'protein', 'taxon:1', '20200101', 'DB']))
	return '\n'.join(lines) + '\n'


GAF_ROWS = [
	('P1', 'g1', 'involved_in', 'GO:2', 'IDA'),
	('P1', 'g1', 'involved_in', 'GO:3', 'IMP'),  # under both branches of the diamond: once in the root
	('P2', 'g2', 'involved_in', 'GO:4', 'EXP'),
	('P3', 'g3', 'involved_in', 'GO:20', 'IPI'),  # an alt_id of GO:2
	('P4', 'g4', 'NOT|involved_in', 'GO:2', 'IDA'),  # a NOT qualifier
	('P5', 'g5', 'involved_in', 'GO:2', 'IEA'),  # an evidence code outside the set
	('P6', 'g6', 'involved_in', 'GO:9', 'IDA'),  # an obsolete term
	('P7', 'g7', 'involved_in', 'GO:5', 'ISS'),
]


def _go_files(tmp_path, obo=OBO, rows=GAF_ROWS):
	(tmp_path / 'go.obo').write_text(obo)
	(tmp_path / 'goa.gaf').write_text(_gaf(rows))
	return str(tmp_path / 'go.obo'), str(tmp_path / 'goa.gaf')


def _members(sets):
	return {name: sorted(g for t, g in sets.pairs if sets.names[t] == name) for name in sets.names}


def test_read_go_propagates_over_is_a(tmp_path):
	sets = enrich.read_go(*_go_files(tmp_path))
	assert sets.names == ['GO:1', 'GO:2', 'GO:3', 'GO:4', 'GO:5'] and sets.labels == ['root', 'left', 'right', 'bottom', 'deep']
	assert sets.depth.dtype == np.int64 and sets.depth.tolist() == [0, 1, 1, 2, 3]
	assert _members(sets) == {'GO:1': ['P1', 'P2', 'P3', 'P7'], 'GO:2': ['P1', 'P2', 'P3', 'P7'], 'GO:3': ['P1', 'P2', 'P7'], 'GO:4': ['P2', 'P7'], 'GO:5': ['P7']}
	assert sets.pairs == sorted(set(sets.pairs)) and sum(1 for t, g in sets.pairs if (t, g) == (0, 'P1')) == 1  # the diamond: once in the common ancestor
	sym = enrich.read_go(*_go_files(tmp_path), key='symbol')
	assert _members(sym) == {k: [g.replace('P', 'g') for g in v] for k, v in _members(sets).items()}
	wide = enrich.read_go(*_go_files(tmp_path), evidence_set=enrich.EVIDENCE_SET | {'IEA'})
	assert _members(wide)['GO:2'] == ['P1', 'P2', 'P3', 'P5', 'P7'] and 'P4' not in _members(wide)['GO:1'] and 'P6' not in _members(wide)['GO:1']
	assert enrich.EVIDENCE_SET == {'EXP', 'IDA', 'IPI', 'IMP', 'IGI', 'HTP', 'HDA', 'HMP', 'HGI', 'IBA', 'IBD', 'IKR', 'IRD', 'ISS', 'ISO', 'ISA', 'ISM'}
	with pytest.raises(ValueError):
		enrich.read_go(*_go_files(tmp_path), key='name')


def test_read_go_longest_path_and_cycle(tmp_path):
	obo = OBO + '\n[Term]\nid: GO:6\nname: short ! cut\nnamespace: molecular_function\nis_a: GO:1\nis_a: GO:5 ! deep\n'
	sets = enrich.read_go(*_go_files(tmp_path, obo, GAF_ROWS + [('P8', 'g8', '', 'GO:6', 'IDA')]))
	assert sets.depth[sets.names.index('GO:6')] == 4  # the longest path from the root, not the shortest
	assert sets.labels[-1] == 'short ! cut' and sets.namespace == ['biological_process'] * 5 + ['molecular_function']  # only is_a and alt_id carry a trailing comment
	cyc = OBO.replace('id: GO:1\nname: root\n', 'id: GO:1\nname: root\nis_a: GO:5\n')
	with pytest.raises(ValueError, match='cycle'):
		enrich.read_go(*_go_files(tmp_path, cyc))


def test_read_gmt_and_bind(tmp_path):
	(tmp_path / 's.gmt').write_text('A\tfirst\tg1\tg2\tzz\tg2\nB\tsecond\tg3\n\nC\tthird\tzz\tyy\nD\tfourth\tg4\tg1\n')
	sets = enrich.read_gmt(str(tmp_path / 's.gmt'))
	assert sets.names == ['A', 'B', 'C', 'D'] and sets.labels == ['first', 'second', 'third', 'fourth'] and sets.depth.tolist() == [0, 0, 0, 0] and sets.namespace is None
	assert sets.pairs == [(0, 'g1'), (0, 'g2'), (0, 'zz'), (1, 'g3'), (2, 'yy'), (2, 'zz'), (3, 'g1'), (3, 'g4')]
	namet = np.array(['g4', 'g3', 'g2', 'g1', 'g0'])
	b = sets.bind(namet)  # zz, yy are outside namet: C is dropped
	assert b.names == ['A', 'B', 'D'] and b.source.tolist() == [0, 1, 3] and b.N == 5 and b.bits.dtype == np.uint64 and b.bits.shape == (3, 1)
	assert b.bits[:, 0].tolist() == [0b01100, 0b00010, 0b01001] and int(b.bg[0]) == 0b11111
	assert b.genes(0).tolist() == ['g2', 'g1'] and b.genes('D').tolist() == ['g4', 'g1']
	b = sets.bind(namet, bg=['g1', 'g2', 'g0', 'nowhere'])  # a background smaller than namet: B has no gene in it
	assert b.names == ['A', 'D'] and b.N == 3 and int(b.bg[0]) == 0b11100 and b.genes('D').tolist() == ['g1']
	assert b.bits[:, 0].tolist() == [0b01100, 0b01001]  # (the bits keep the genes outside the background: the kernels mask them)
	assert sets.bind(namet, bg=np.array([False, False, True, True, True])).names == ['A', 'D'] and sets.bind(namet, bg=[2, 3, 4]).N == 3
	with pytest.raises(ValueError):
		sets.bind(namet, bg=['nowhere'])


@pytest.mark.parametrize('ng', [63, 64, 65])
def test_bind_pad_bits_are_zero(ng):
	names = ['g{}'.format(i) for i in range(ng)]
	sets = enrich.GeneSets(['all', 'last', 'ends'], ['', '', ''], [0, 0, 0], [(0, g) for g in names] + [(1, names[-1])] + [(2, names[0]), (2, names[-1]), (2, 'outside')])
	b = sets.bind(names)
	w = (ng + 63) // 64
	assert b.bits.shape == (3, w) and b.bg.shape == (w, ) and b.N == ng
	full = [(1 << min(64, ng - 64 * i)) - 1 for i in range(w)]
	assert [int(v) for v in b.bits[0]] == full and [int(v) for v in b.bg] == full
	assert enrich.unpack_bits(b.bits[1], ng).tolist() == [ng - 1] and enrich.unpack_bits(b.bits[2], ng).tolist() == [0, ng - 1]
	assert sum(bin(int(v)).count('1') for v in b.bits[0]) == ng


# ---- selection ------------------------------------------------------------------------------------------------------------------------------------------------
def _top_host(k, K, p, odds, nmin):
	k, K = np.ascontiguousarray(k, dtype=np.int32), np.ascontiguousarray(K, dtype=np.int32)
	p, odds = np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(odds, dtype=np.float64)
	top = np.empty(k.shape[0], dtype=enrich.TOP_DTYPE)
	rc = _lib.load().nrm_enrich_top_host(k.ctypes.data, K.ctypes.data, p.ctypes.data, odds.ctypes.data, k.shape[0], k.shape[1], nmin, top.ctypes.data)
	assert rc == 0
	return top


def test_selection_rule():
	K = [9, 9, 9, 9, 9]
	k = [[6, 6, 6, 2, 6], [6, 6, 6, 2, 6], [1, 1, 1, 1, 1], [6, 6, 6, 6, 6]]
	p = [[.2, .1, .1, .01, .1], [.2, .1, .1, .01, .001], [.5, .5, .5, .5, .5], [.3, .3, .3, .3, .3]]
	odds = [[2, 2, 2, 2, 2], [2, 2, 2, 2, 1.0], [3, 3, 3, 3, 3], [1, .5, 0, 1, 1]]
	top = _top_host(k, K, p, odds, 5)
	assert top['index'].tolist() == [1, 1, -1, -1]  # a tie in p: the lower index; k < nmin and odds <= 1 are excluded; nothing qualifies: -1
	assert (top['k'][0], top['K'][0], top['p'][0]) == (6, 9, .1) and (top['k'][2], top['K'][2], top['p'][2]) == (0, 0, 1.0)
	assert _top_host(k, K, p, odds, 2)['index'].tolist() == [3, 3, -1, -1]
	assert _top_host(k, K, p, odds, 0)['index'].tolist() == [3, 3, 0, -1] and _top_host(k, K, p, odds, -3)['index'].tolist() == [3, 3, 0, -1]  # nmin < 1 means 1
	sets = enrich.GeneSets(list('abcde'), [''] * 5, [0] * 5, [(t, 'g{}'.format(t)) for t in range(5)]).bind(['g{}'.format(t) for t in range(5)])
	res = enrich.EnrichResult(sets, np.array(k, dtype=np.int32), np.array(K, dtype=np.int32), np.array([8, 8, 8, 8], dtype=np.int32), 5, np.array(p), np.array(odds, dtype=float), top,
							  np.zeros((4, 1), dtype=np.uint64))
	assert res.top.tolist() == [1, 1, -1, -1] and res.top_sets(0) == 'b' and res.top_sets(1) == 'b'
	for s in (2, 3, None):
		with pytest.raises(ValueError, match='No GO enrichment found for given criteria.'):
			res.top_sets(s)
	assert res.ntest == 5 and np.array_equal(res.p_bonferroni, np.minimum(1, np.array(p) * 5))
	rows = res.table(0)
	assert [r[7] for r in rows] == ['d', 'b', 'c', 'e', 'a'] and rows[0][2:4] == (.01, .05) and rows[0][5:7] == ('2/8', '9/5')  # sorted by p, equal p by index
	assert len(enrich.COLUMNS) == len(rows[0]) == 9 and enrich.COLUMNS[0] == 'name' and enrich.COLUMNS[-1] == 'study_items'
	# the numpy restatement states the same rule
	kk, KK, n, N, pp, oo, tt = en.enrich_numpy(np.eye(3, 6), np.ones((2, 6)), nmin=1)
	assert tt.tolist() == [-1, -1, -1] and (oo == 1).all()


# ---- boundary -------------------------------------------------------------------------------------------------------------------------------------------------
NEW = ('nrm_enrich_pack', 'nrm_enrich_overlap', 'nrm_enrich_fisher', 'nrm_enrich_top', 'nrm_enrich_host', 'nrm_fisher_host', 'nrm_enrich_top_host')


def test_library_declares_the_enrich_entries():
	lib = _lib.load()
	hdr = open(os.path.join(ROOT, 'include', 'normalisr_hip.h')).read()
	for name in NEW:
		assert name in _lib.exported_symbols() and hasattr(lib, name) and name + '(' in hdr
	assert os.path.exists(os.path.join(ROOT, 'normalisr_amd', 'csrc', 'nrm_enrich.hip')) and os.path.exists(os.path.join(ROOT, 'normalisr_amd', 'csrc', 'nrm_fisher.h'))


def test_bad_arguments_are_refused_before_any_device_call():
	"""Every entry answers NRM_E_ARG from its own checks: there is no device here, and the buffers are host memory no kernel may see."""
	lib = _lib.load()
	buf = np.zeros(4096, dtype=np.uint64)
	a = buf.ctypes.data
	E = _lib.NRM_E_ARG
	big = 2**31
	pack = lambda x=a, S=3, G=70, ld=70, bg=a, w=a, n=a: lib.nrm_enrich_pack(x, S, G, ld, bg, w, n, None)
	for ka in (dict(x=None), dict(w=None), dict(n=None), dict(ld=69), dict(S=0), dict(G=0), dict(S=-1), dict(G=big, ld=big), dict(w=a + 4), dict(bg=a + 1), dict(n=a + 2)):
		assert pack(**ka) == E, ka
	over = lambda x=a, S=3, s=a, T=5, G=70, bg=a, k=a, K=a: lib.nrm_enrich_overlap(x, S, s, T, G, bg, k, K, None)
	for ka in (dict(x=None), dict(s=None), dict(k=None), dict(K=None), dict(S=0), dict(T=0), dict(G=0), dict(G=big), dict(x=a + 4), dict(s=a + 4), dict(bg=a + 4), dict(k=a + 2)):
		assert over(**ka) == E, ka
	fish = lambda k=a, n=a, K=a, S=3, T=5, N=70, p=a, o=a: lib.nrm_enrich_fisher(k, n, K, S, T, N, p, o, None)
	for ka in (dict(k=None), dict(n=None), dict(K=None), dict(p=None), dict(o=None), dict(S=0), dict(T=0), dict(N=0), dict(N=big), dict(p=a + 4), dict(o=a + 4)):
		assert fish(**ka) == E, ka
	top = lambda k=a, K=a, p=a, o=a, S=3, T=5, r=a: lib.nrm_enrich_top(k, K, p, o, S, T, 5, r, None)
	for ka in (dict(k=None), dict(K=None), dict(p=None), dict(o=None), dict(r=None), dict(S=0), dict(T=0), dict(p=a + 4), dict(r=a + 4)):
		assert top(**ka) == E, ka
	N = ctypes.c_int64(0)
	host = lambda x=a, S=3, G=70, ld=70, s=a, T=5, bg=a, k=a, out=a: lib.nrm_enrich_host(x, S, G, ld, s, T, bg, 5, k, a, a, a, a, out, ctypes.byref(N))
	for ka in (dict(x=None), dict(s=None), dict(k=None), dict(out=None), dict(ld=69), dict(S=0), dict(T=0), dict(G=0), dict(G=big, ld=big), dict(s=a + 4), dict(bg=a + 4)):
		assert host(**ka) == E, ka
	assert host() == E and b'background is empty' in lib.nrm_last_error()  # (bg all zero)
	with pytest.raises(ValueError):
		_lib.check(pack(ld=3))


def test_study_forms_and_checks_without_a_device():
	names = ['g{}'.format(i) for i in range(70)]
	b = enrich.GeneSets(['s'], [''], [0], [(0, 'g3'), (0, 'g69')]).bind(names)
	x = enrich._study_matrix(['g69', 'g0'], b)
	assert x.shape == (1, 70) and x.dtype == np.uint8 and np.flatnonzero(x[0]).tolist() == [0, 69]
	assert np.array_equal(enrich._study_matrix(np.array([69, 0]), b), x) and np.array_equal(enrich._study_matrix(x != 0, b), x)
	assert np.array_equal(enrich._study_matrix(np.where(x, 7.5, 0.0), b), x)
	for bad in (['g1', 'nowhere'], [70], np.zeros((2, 69), dtype=bool), [], np.zeros((0, 70), dtype=bool)):
		with pytest.raises(ValueError):
			enrich._study_matrix(bad, b)
	with pytest.raises(ValueError, match='namet is needed'):
		enrich.enrich(['g1'], enrich.GeneSets(['s'], [''], [0], [(0, 'g3')]))
	with pytest.raises(ValueError, match='bind again'):
		enrich.enrich(['g1'], b, bg=['g1'])
	with pytest.raises(ValueError, match='No enrichment found'):
		enrich.enrich(['g1'], enrich.GeneSets(['s'], [''], [0], [(0, 'elsewhere')]), namet=names)
	with pytest.raises(ValueError, match='Wrong shape for net or namet.'):
		enrich.top_pathway(np.zeros((4, 5), dtype=bool), names[:4], b)
	with pytest.raises(ValueError, match='Wrong shape for net or namet.'):
		enrich.top_pathway(np.zeros((4, 4), dtype=bool), names[:3], b)
	with pytest.raises(ValueError, match='Number of principal genes'):
		enrich.top_pathway(np.zeros((4, 4), dtype=bool), names[:4], b, n=4)


def test_parser_accepts_enrich_and_still_rejects_gocovt(capsys):
	from normalisr_amd.__main__ import build_parser
	from normalisr_amd import run
	p = build_parser()
	ns = vars(p.parse_args(['enrich', 'net', 'genes', 'out', '--gmt', 's.gmt']))
	assert (ns['cmd'], ns['net_in'], ns['genes_in'], ns['pathway_out'], ns['gmt'], ns['go'], ns['key'], ns['n'], ns['nmin']) == ('enrich', 'net', 'genes', 'out', 's.gmt', None, 'id', 100, 5)
	assert ns['master_out'] is None and ns['goe_out'] is None and ns['go_out'] is None
	ns = vars(p.parse_args(['enrich', 'net', 'genes', 'out', '--go', 'go.obo', 'goa.gaf', '--key', 'symbol', '-n', '20', '-m', '3', '--master_out', 'a', '--goe_out', 'b', '--go_out', 'c']))
	assert (ns['go'], ns['gmt'], ns['key'], ns['n'], ns['nmin'], ns['master_out'], ns['goe_out'], ns['go_out']) == (['go.obo', 'goa.gaf'], None, 'symbol', 20, 3, 'a', 'b', 'c')
	for bad in (['enrich', 'net', 'genes', 'out'], ['enrich', 'net', 'genes', 'out', '--gmt', 's', '--go', 'a', 'b'], ['enrich', 'net', 'genes', 'out', '--gmt', 's', '--key', 'alias'],
				['gocovt', 'e', 'c', 'n', 'g', 'go', 'goa', 'o']):
		with pytest.raises(SystemExit):
			p.parse_args(bad)
	capsys.readouterr()
	text = ' '.join(p.format_help().split())
	assert 'gocovt is not provided' in text and 'goatools' in text and 'enrich' in text
	assert 'The sub-command gocovt is not provided: its GO enrichment needs goatools and a web service.' in text
	assert callable(run.enrich) and not hasattr(run, 'gocovt')
	import normalisr_amd.gocovt as gocovt
	assert not hasattr(gocovt, 'gotop') and not hasattr(gocovt, 'goe')


def test_command_line_checks_before_any_device_call(tmp_path):
	from normalisr_amd import run
	f = lambda name: str(tmp_path / name)
	np.savetxt(f('net.tsv'), np.zeros((4, 4), dtype=int), delimiter='\t', fmt='%i')
	run.file_write_txtlist(f('three.txt'), ['a', 'b', 'c'])
	run.file_write_txtlist(f('four.txt'), ['a', 'b', 'c', 'd'])
	(tmp_path / 's.gmt').write_text('A\t\ta\tb\n')
	args = dict(net_in=f('net.tsv'), genes_in=f('three.txt'), pathway_out=f('o.txt'), gmt=f('s.gmt'), go=None, key='id', n=2, nmin=1, master_out=f('m.txt'), goe_out=None, go_out=None)
	with pytest.raises(ValueError, match='Wrong shape'):
		run.enrich(args)
	with pytest.raises(ValueError, match='Number of principal genes'):
		run.enrich(dict(args, genes_in=f('four.txt'), n=4))
	with pytest.raises(RuntimeError, match='Not enough principal genes'):
		run.enrich(dict(args, genes_in=f('four.txt')))
	assert not os.path.exists(f('o.txt')) and not os.path.exists(f('m.txt'))
