"""Gene-set enrichment on the device: what stands between gocovt.principal_genes and gocovt.pccovt in the reference's gocovt (its goe, gocovt.py:44-213), as
arithmetic alone.  The reference hands this step to goatools and converts gene names through a web service; neither is used here.  An enrichment study is overlap
counts between study sets and gene sets, a two-sided Fisher exact test per pair and a selection rule, with the gene sets read from local files.

NOT VERIFIED AGAINST goatools: goatools is not available to this project's tests, so nothing here claims its output.  The contract is the one written in this
module (and in DESIGN.md, "Gene-set enrichment"):
  sets      read_gmt: one set per line, name<TAB>description<TAB>gene<TAB>gene...   read_go: an OBO ontology and a GAF 2.x annotation file; obsolete terms dropped,
            alt_id mapped to its primary term, is_a edges only, NOT-qualified annotations skipped, evidence codes filtered (the reference's default set), every
            annotation propagated to all is_a ancestors, depth = the longest path from a root.  Genes are matched by GAF column 2 (key='id') or column 3
            (key='symbol': gene names as they are, instead of the web service).
  bind      gene names -> rows of the user's gene list; names outside it and sets without a gene in the background are dropped
  counts    n = study genes in the background, K = set genes in the background, k = genes in both, N = background genes
  test      the two-sided Fisher exact P-value of (k, n - k, K - k, N - K - n + k): the sum of the hypergeometric weights <= w(k) (1 + 1e-7) over the sum of all,
            by a recurrence anchored at the mode (csrc/nrm_fisher.h; relative error <= 8 L u for a support of L values, u = 2^-53)
  odds      (k / n) / (K / N), 0 (and p = 1) when n or K is 0
  top       the set of smallest p among those with odds > 1 and k >= nmin, the lower index of equals; -1 when none qualifies
  p_bonferroni = min(1, p T) with T the number of bound sets (each has K >= 1).  This count is this project's own rule; goatools counts differently.
Kernels: csrc/nrm_enrich.hip -- nrm_enrich_pack (byte matrix -> bit words), nrm_enrich_overlap (AND + popcount tiled through LDS), nrm_enrich_fisher (a lane per
pair), nrm_enrich_top (a record per study).  Done in batch -- one study per row of a byte matrix, such as a whole binary network -- the same kernels annotate
every gene's neighbourhood at once."""
import logging

import numpy as np

from . import engine as _engine

# the reference's default evidence codes (gocovt.py:51-53): not expression based, to avoid circular reasoning
EVIDENCE_SET = frozenset(['EXP', 'IDA', 'IPI', 'IMP', 'IGI', 'HTP', 'HDA', 'HMP', 'HGI', 'IBA', 'IBD', 'IKR', 'IRD', 'ISS', 'ISO', 'ISA', 'ISM'])
COLUMNS = ('name', 'depth', 'p_uncorrected', 'p_bonferroni', 'odds_ratio', 'ratio_in_study', 'ratio_in_pop', 'id', 'study_items')  # (gocovt.py:182-184; GO -> id)
TOP_DTYPE = np.dtype([('index', '<i8'), ('k', '<i8'), ('K', '<i8'), ('p', '<f8')])  # the record of nrm_enrich_top



class GeneSets:
	"""Gene sets as read from files: names (identifiers: GO ids, GMT names), labels (term names, GMT descriptions), depth (int64; zeros for GMT) and pairs, the
	membership as sorted unique (set index, gene name) tuples.  namespace: every set's GO namespace as read_go finds it, None where there is none (read_gmt); it
	is carried for the user and plays no part in the test."""

	def __init__(self, names, labels, depth, pairs, namespace=None):
		self.names, self.labels = list(names), list(labels)
		self.namespace = None if namespace is None else list(namespace)
		self.depth = np.asarray(depth, dtype=np.int64)
		self.pairs = sorted(set((int(t), str(g)) for t, g in pairs))
		if not (len(self.names) == len(self.labels) == len(self.depth)) or (self.namespace is not None and len(self.namespace) != len(self.names)):
			raise ValueError('names, labels and depth must have one entry per set.')
		if self.pairs and not 0 <= self.pairs[0][0] <= self.pairs[-1][0] < len(self.names):
			raise ValueError('A pair names a set that is not there.')

	def __len__(self):
		return len(self.names)

	def bind(self, namet, bg=None):
		"""The sets on the rows of a gene list.  namet: the gene names of the rows (of equal names the last one is taken, as pccovt does).  bg: the background -- None for
		all of namet, or names, or integer rows, or a bool mask of len(namet).  Names outside namet are dropped, and so are sets without a gene in the background.
		Returns a BoundSets whose membership is a (T, W) matrix of 64-bit words, W = ceil(G / 64), bit g % 64 of word g / 64 for gene g; bits at or beyond G are zero."""
		# Propagation (read_go) and this packing stay on the host: they run once per ontology, are O(annotations x depth) dictionary work on strings, and their
		# result -- a few MB of bits -- is what every later call uploads.
		namet = np.asarray(namet)
		if namet.ndim != 1 or namet.size == 0:
			raise ValueError('namet must be a non-empty one-dimensional list of gene names.')
		ng = int(namet.size)
		if ng > 2**31 - 1:
			raise ValueError('At most 2^31 - 1 genes.')
		where = dict(zip((str(x) for x in namet), range(ng)))
		mask = np.ones(ng, dtype=bool)
		if bg is not None:
			b = np.asarray(bg)
			mask = np.zeros(ng, dtype=bool)
			if b.dtype == np.bool_:
				if b.shape != (ng, ):
					raise ValueError('A bool background must have one entry per gene.')
				mask = b.copy()
			elif b.dtype.kind in 'iu':
				mask[b] = True
			else:
				mask[[where[str(x)] for x in b if str(x) in where]] = True
		if not mask.any():
			raise ValueError('Empty background.')
		rows = np.array([t for t, g in self.pairs if g in where], dtype=np.int64)
		cols = np.array([where[g] for t, g in self.pairs if g in where], dtype=np.int64)
		inbg = mask[cols] if cols.size else np.zeros(0, dtype=bool)
		keep = np.unique(rows[inbg])  # (rising: the sets keep their order)
		new = np.full(len(self.names), -1, dtype=np.int64)
		new[keep] = np.arange(keep.size)
		sel = new[rows] >= 0
		bits = pack_bits(new[rows[sel]], cols[sel], int(keep.size), ng)
		return BoundSets([self.names[t] for t in keep], [self.labels[t] for t in keep], self.depth[keep], namet, bits, pack_bits(np.zeros(int(mask.sum()), dtype=np.int64),
						 np.flatnonzero(mask), 1, ng)[0], keep)


def pack_bits(rows, cols, nrow, ng):
	"""(nrow, ceil(ng / 64)) uint64 with bit cols[i] % 64 of word cols[i] / 64 set in row rows[i]."""
	bits = np.zeros((nrow, (ng + 63) // 64), dtype=np.uint64)
	cols = np.asarray(cols, dtype=np.int64)
	np.bitwise_or.at(bits, (np.asarray(rows, dtype=np.int64), cols >> 6), np.uint64(1) << (cols & 63).astype(np.uint64))
	return bits


def unpack_bits(words, ng):
	"""The rising gene rows whose bit is set in a (W, ) word vector."""
	w = np.ascontiguousarray(words, dtype='<u8')
	return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder='little')[:ng])


class BoundSets:
	"""Gene sets bound to a gene list (GeneSets.bind): names, labels, depth, namet, bits (T, W) uint64, bg (W, ) uint64, N = genes in the background, source = the
	index of every set in the GeneSets it came from."""

	def __init__(self, names, labels, depth, namet, bits, bg, source):
		self.names, self.labels, self.depth, self.namet, self.bits, self.bg, self.source = names, labels, depth, namet, np.ascontiguousarray(bits), np.ascontiguousarray(bg), source
		self.ng = int(len(namet))
		self.N = int(unpack_bits(self.bg, self.ng).size)
		self._dev = {}

	def __len__(self):
		return len(self.names)

	def genes(self, t):
		"""The background genes of set t (an index, or a name) in namet order: what pccovt takes."""
		if not isinstance(t, (int, np.integer)):
			t = self.names.index(t)
		return self.namet[unpack_bits(self.bits[t] & self.bg, self.ng)]

	def device(self, eng):
		"""(bits, bg) in HBM as int64 tensors, uploaded once per device."""
		key = eng.device.index
		if key not in self._dev:
			self._dev[key] = (eng.upload(self.bits.view(np.int64)), eng.upload(self.bg.view(np.int64)))
		return self._dev[key]


# ---- readers ------------------------------------------------------------------------------------------------------------------------------------------------------

def _open_text(path):
	if str(path).endswith('.gz'):
		import gzip
		return gzip.open(path, 'rt')
	return open(path, 'r')


def read_gmt(path):
	"""Gene sets from a GMT file: one set per line, name<TAB>description<TAB>gene<TAB>gene...  Empty lines are skipped, a set named twice is one set."""
	names, labels, index, pairs = [], [], {}, []
	with _open_text(path) as fh:
		for line in fh:
			f = line.rstrip('\r\n').split('\t')
			if not f[0].strip():
				continue
			name = f[0].strip()
			if name not in index:
				index[name] = len(names)
				names.append(name)
				labels.append(f[1].strip() if len(f) > 1 else '')
			pairs.extend((index[name], g.strip()) for g in f[2:] if g.strip())
	return GeneSets(names, labels, np.zeros(len(names), dtype=np.int64), pairs)


def read_obo(path):
	"""The [Term] stanzas of an OBO file: {id: dict(name, namespace, alt_id list, is_a list, obsolete)}."""
	terms, cur, on = {}, None, False
	with _open_text(path) as fh:
		for line in fh:
			line = line.strip()
			if line.startswith('['):
				on = line == '[Term]'
				cur = dict(id=None, name='', namespace='', alt_id=[], is_a=[], obsolete=False) if on else None
				continue
			if not on or ':' not in line:
				continue
			key, val = line.split(':', 1)
			val = val.strip()
			if key == 'id':
				cur['id'] = val
				terms[val] = cur
			elif key in ('name', 'namespace'):
				cur[key] = val  # (as it stands: a name may hold ' ! ')
			elif key in ('alt_id', 'is_a') and val:
				cur[key].append(val.split()[0])  # (the identifier alone: 'GO:1 ! root' carries the parent's name as a comment)
			elif key == 'is_obsolete':
				cur['obsolete'] = val.lower().split()[:1] == ['true']
	return terms


def _ancestors_and_depth(parents):
	"""For a DAG {term: [parents]}: every term's ancestors (itself included) and its depth, the longest path from a root.  ValueError for a cycle."""
	anc, depth, state = {}, {}, {}
	for start in parents:
		if start in anc:
			continue
		stack = [(start, iter(parents[start]))]
		state[start] = 1
		while stack:
			node, it = stack[-1]
			for par in it:
				if state.get(par, 0) == 1:
					raise ValueError('The is_a relations form a cycle through {}.'.format(par))
				if par not in anc:
					state[par] = 1
					stack.append((par, iter(parents[par])))
					break
			else:
				stack.pop()
				state[node] = 2
				a = {node}
				for par in parents[node]:
					a |= anc[par]
				anc[node] = a
				depth[node] = 1 + max((depth[par] for par in parents[node]), default=-1)
	return anc, depth


def read_go(obo_path, gaf_path, key='id', evidence_set=EVIDENCE_SET):
	"""Gene sets from a GO ontology (OBO) and an annotation file (GAF 2.x), by the contract in the module docstring.  key='id': genes by GAF column 2 (where the
	reference's route ends after its web conversion); key='symbol': by column 3, which matches gene names directly.  evidence_set: the codes of column 7 to keep
	(None: all).  Terms without a gene are left out; the sets are in the order of their ids."""
	if key not in ('id', 'symbol'):
		raise ValueError("key must be 'id' or 'symbol'.")
	col = 1 if key == 'id' else 2
	terms = read_obo(obo_path)
	live = {t: v for t, v in terms.items() if not v['obsolete']}
	primary = {t: t for t in live}
	for t, v in live.items():
		for a in v['alt_id']:
			primary.setdefault(a, t)
	parents = {t: [primary[p] for p in v['is_a'] if p in primary] for t, v in live.items()}
	anc, depth = _ancestors_and_depth(parents)
	member = set()
	with _open_text(gaf_path) as fh:
		for line in fh:
			if line.startswith('!'):
				continue
			f = line.rstrip('\r\n').split('\t')
			if len(f) < 7:
				continue
			if 'NOT' in f[3].upper().split('|'):
				continue
			if evidence_set is not None and f[6] not in evidence_set:
				continue
			term = primary.get(f[4].strip())
			gene = f[col].strip()
			if term is None or not gene:
				continue
			member.update((a, gene) for a in anc[term])
	ids = sorted(set(t for t, g in member))
	index = {t: i for i, t in enumerate(ids)}
	return GeneSets(ids, [live[t]['name'] for t in ids], [depth[t] for t in ids], [(index[t], g) for t, g in member], namespace=[live[t]['namespace'] for t in ids])


# ---- the study ----------------------------------------------------------------------------------------------------------------------------------------------------

class EnrichResult:
	"""What enrich returns.  For S studies and T sets: k (S, T) int32 genes in both, K (T) int32 set sizes and n (S) int32 study sizes in the background, N the
	background's size, p (S, T) fp64 two-sided Fisher exact P-values, odds (S, T) fp64, top (S) int64 the index of every study's top set (-1: none) with
	top_records (index, k, K, p).  numpy arrays, or -- device_out=True -- torch CUDA tensors for k, K, n, p, odds (top is read back: S records)."""

	def __init__(self, sets, k, K, n, N, p, odds, top_records, words):
		self.sets, self.k, self.K, self.n, self.N, self.p, self.odds, self.top_records, self._words = sets, k, K, n, int(N), p, odds, top_records, words
		self.top = top_records['index'].copy()
		self.ntest = len(sets)  # every bound set has K >= 1 and counts as a test (this project's rule)

	@property
	def p_bonferroni(self):
		"""min(1, p T), T = the number of bound sets."""
		if _engine.is_dev(self.p):
			return (self.p * self.ntest).clamp_(max=1.0)
		return np.minimum(1.0, self.p * self.ntest)

	def top_sets(self, s=None):
		"""The name of the top set of study s, or of every study.  ValueError for a study without one."""
		idx = self.top if s is None else self.top[[s]]
		if (idx < 0).any():
			raise ValueError('No GO enrichment found for given criteria.')
		ans = [self.sets.names[t] for t in idx]
		return ans if s is None else ans[0]

	def genes(self, t):
		"""The background genes of set t (an index, or a name) in namet order: what pccovt takes."""
		return self.sets.genes(t)

	def _row(self, a, s):
		return np.asarray(a[s].cpu().numpy() if _engine.is_dev(a) else a[s])

	def table(self, s=0):
		"""The enrichment of study s as a list of rows (tuples in the order of COLUMNS, the columns the reference writes) sorted by p, equal p by set index."""
		k, p, odds = self._row(self.k, s), self._row(self.p, s), self._row(self.odds, s)
		K = np.asarray(self.K.cpu().numpy() if _engine.is_dev(self.K) else self.K)
		n = int(self._row(self.n, s))
		study = np.ascontiguousarray(self._row(self._words, s)).view(np.uint64)
		pb = np.minimum(1.0, p * self.ntest)
		rows = []
		for t in np.argsort(p, kind='stable'):
			items = self.sets.namet[unpack_bits(study & self.sets.bits[t], self.sets.ng)]
			rows.append((self.sets.labels[t], int(self.sets.depth[t]), float(p[t]), float(pb[t]), float(odds[t]), '{}/{}'.format(int(k[t]), n),
						 '{}/{}'.format(int(K[t]), self.N), self.sets.names[t], ','.join(str(x) for x in items)))
		return rows


def _study_matrix(study, bound):
	"""The study as an (S, G) byte matrix, numpy or a torch CUDA tensor: a matrix as it is, a list of names or rows as one row."""
	ng = bound.ng
	if _engine.is_dev(study) and study.dim() == 2:
		import torch
		if study.dtype not in (torch.bool, torch.uint8):
			raise TypeError('study must be bool or uint8.')
		if study.shape[1] != ng or study.shape[0] < 1:
			raise ValueError('A study matrix must have one column per gene.')
		x = study if study.stride(1) == 1 and study.stride(0) >= ng else study.contiguous()
		return x.view(torch.uint8) if x.dtype == torch.bool else x
	if _engine.is_dev(study):  # integer rows in HBM (principal_genes(..., device_out=True))
		import torch
		if study.dim() != 1 or study.dtype not in (torch.int32, torch.int64):
			raise ValueError('A study in HBM is an (S, G) bool / uint8 matrix or a one-dimensional list of integer rows.')
		if study.numel() and (int(study.min()) < 0 or int(study.max()) >= ng):
			raise ValueError('Genes not found: rows outside the gene list.')
		x = torch.zeros((1, ng), dtype=torch.uint8, device=study.device)
		x[0, study.long()] = 1
		return x
	a = np.asarray(study.cpu() if hasattr(study, 'data_ptr') else study)
	if a.ndim == 2:
		if a.shape[1] != ng or a.shape[0] < 1:
			raise ValueError('A study matrix must have one column per gene.')
		if a.dtype != np.bool_ and a.dtype != np.uint8:
			a = a != 0
		return np.ascontiguousarray(a).view(np.uint8)
	from .gocovt import _gene_rows
	if a.ndim != 1 or a.size == 0:
		raise ValueError('A study is an (S, G) matrix or a non-empty one-dimensional list of gene names or rows.')
	idx = _gene_rows(ng, None if a.dtype.kind in 'iu' else bound.namet, a if a.dtype.kind in 'iu' else [str(x) for x in a])
	x = np.zeros((1, ng), dtype=np.uint8)
	x[0, idx] = 1
	return x


def _enrich_host(x, bound, nmin):
	"""Through nrm_enrich_host: numpy buffers in and out, no torch."""
	import ctypes
	from . import _lib
	lib = _lib.load()
	S, T = int(x.shape[0]), len(bound)
	k, K, n = np.empty((S, T), dtype=np.int32), np.empty(T, dtype=np.int32), np.empty(S, dtype=np.int32)
	p, odds, top = np.empty((S, T)), np.empty((S, T)), np.empty(S, dtype=TOP_DTYPE)
	N = ctypes.c_int64(0)
	vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
	_lib.check(lib.nrm_enrich_host(vp(x), S, bound.ng, x.strides[0], vp(bound.bits), T, vp(bound.bg), int(nmin), vp(k), vp(K), vp(n), vp(p), vp(odds), vp(top), ctypes.byref(N)))
	assert N.value == bound.N
	words = pack_bits(*np.nonzero(x), S, bound.ng) & bound.bg
	return EnrichResult(bound, k, K, n, N.value, p, odds, top, words)


def _enrich_engine(x, bound, nmin, device_out):
	from . import _lib
	eng = _engine.get_engine(x.device.index if _engine.is_dev(x) else None)
	S, T, ng = int(x.shape[0]), len(bound), bound.ng
	with eng.lock:
		torch = eng.torch
		with torch.cuda.device(eng.device):
			d_x = x if _engine.is_dev(x) else eng.upload(x)
			d_bits, d_bg = bound.device(eng)
			dev = dict(device=eng.device)
			words = torch.empty((S, d_bits.shape[1]), dtype=torch.int64, **dev)
			n = torch.empty((S, ), dtype=torch.int32, **dev)
			K = torch.empty((T, ), dtype=torch.int32, **dev)
			k = torch.empty((S, T), dtype=torch.int32, **dev)
			p = torch.empty((S, T), dtype=torch.float64, **dev)
			odds = torch.empty((S, T), dtype=torch.float64, **dev)
			top = torch.empty((S, 4), dtype=torch.int64, **dev)
			stream = eng._stream()
			with _engine._Span(eng, 'enrich_pack'):
				_lib.check(eng.lib.nrm_enrich_pack(d_x.data_ptr(), S, ng, d_x.stride(0), d_bg.data_ptr(), words.data_ptr(), n.data_ptr(), stream))
			with _engine._Span(eng, 'enrich_overlap'):
				_lib.check(eng.lib.nrm_enrich_overlap(words.data_ptr(), S, d_bits.data_ptr(), T, ng, d_bg.data_ptr(), k.data_ptr(), K.data_ptr(), stream))
			with _engine._Span(eng, 'enrich_fisher'):
				_lib.check(eng.lib.nrm_enrich_fisher(k.data_ptr(), n.data_ptr(), K.data_ptr(), S, T, bound.N, p.data_ptr(), odds.data_ptr(), stream))
			with _engine._Span(eng, 'enrich_top'):
				_lib.check(eng.lib.nrm_enrich_top(k.data_ptr(), K.data_ptr(), p.data_ptr(), odds.data_ptr(), S, T, int(nmin), top.data_ptr(), stream))
			rec = np.ascontiguousarray(top.cpu().numpy()).view(TOP_DTYPE).reshape(S)  # (the one read-back of a resident loop: S records)
			if device_out:
				return EnrichResult(bound, k, K, n, bound.N, p, odds, rec, words)
			return EnrichResult(bound, eng.download(k), K.cpu().numpy(), n.cpu().numpy(), bound.N, eng.download(p), eng.download(odds), rec, words.cpu().numpy().view(np.uint64))


def enrich(study, sets, namet=None, bg=None, nmin=5, device_out=False, device=None):
	"""Enrichment of study sets in gene sets, on the device.
	study: a list of gene names, or of integer rows of the gene list (one study: what principal_genes returns, on the host or in HBM), or an (S, G) bool / uint8
	matrix, numpy or a torch CUDA tensor with any pitch (a binary network as binnet(..., device_out=True) returns it is one study per gene: every gene's
	neighbourhood).  Any non-zero byte counts once.
	sets: a GeneSets (read_gmt, read_go) with namet, the names of the G genes, and bg, the background (None: all of namet; see GeneSets.bind) -- or a BoundSets, which
	carries both (bind once, call often).
	nmin: the fewest study genes a top set must hold (below 1 means 1).  device: the GPU's index.
	Returns an EnrichResult; with device_out=True its k, K, n, p and odds stay in HBM.  With torch it runs on the engine; in a process without torch, or with
	NRM_HOST_ENTRY=1, through the library's whole-problem entry nrm_enrich_host."""
	if isinstance(sets, BoundSets):
		if bg is not None or (namet is not None and (len(namet) != sets.ng or any(str(a) != str(b) for a, b in zip(namet, sets.namet)))):
			raise ValueError('A BoundSets carries its gene list and background: bind again for others.')
		bound = sets
	else:
		if namet is None:
			raise ValueError('namet is needed to bind the gene sets.')
		bound = sets.bind(namet, bg)
	if len(bound) == 0:
		raise ValueError('No enrichment found. Check your input ID type.')  # (the reference's words for an empty study, gocovt.py:168)
	x = _study_matrix(study, bound)
	with _engine.use_device(device):
		from .association import _use_host_entry
		if not _engine.is_dev(x) and not device_out and _use_host_entry():
			res = _enrich_host(x, bound, nmin)
		else:
			res = _enrich_engine(x, bound, nmin, device_out)
	logging.debug('enrich: {} studies, {} sets, {} background genes.'.format(x.shape[0], len(bound), bound.N))
	return res


def top_pathway(net, namet, sets, n=100, nmin=5):
	"""The reference's gotop (gocovt.py:216-269) without its file parsing: the principal genes of a binary network (gocovt.principal_genes), their enrichment with
	all of namet as the background, the top set's name and its genes in namet order (what pccovt takes).  Returns (principals, result, top_name, genes).
	ValueError for a wrong net or n comes from principal_genes, unchanged; namet, which principal_genes does not take, must name the net's rows;
	'No GO enrichment found for given criteria.' when no set qualifies."""
	from . import gocovt
	namet = np.asarray(namet)
	if namet.ndim != 1 or len(net.shape) < 1 or namet.shape[0] != net.shape[0]:
		raise ValueError('Wrong shape for net or namet.')
	sel = gocovt.principal_genes(net, n=n)
	res = enrich(sel, sets, namet=None if isinstance(sets, BoundSets) else namet, nmin=nmin, device=net.device.index if _engine.is_dev(net) else None)
	name = res.top_sets(0)
	return [str(x) for x in namet[sel]], res, name, [str(x) for x in res.genes(int(res.top[0]))]


assert __name__ != "__main__"
