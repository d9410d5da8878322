"""User API facade: `import normalisr_amd.normalisr as norm` (reference normalisr.py:3-9).
The pipeline from read counts to the network is provided: lcpm (+ scaling_factor) -> normcov -> compute_var -> normvar -> de / coex -> binnet.  The
quality-control steps qc_reads and qc_outlier (and subset) live in normalisr_amd.qc and behind the command line, and so do pccovt and principal_genes (the
selection inside the reference's gotop) in normalisr_amd.gocovt; this facade does not export them yet.  The reference's GO enrichment (goe, and gotop around it)
is outside this build's scope: it needs goatools and a web service."""
from .de import de
from .coex import coex
from .binnet import binnet
from .norm import normvar, normcov, compute_var
from .lcpm import lcpm, scaling_factor

_OUT_OF_SCOPE = ('qc_reads', 'qc_outlier', 'gotop', 'pccovt')


def __getattr__(name):
	if name in _OUT_OF_SCOPE:
		if name in ('qc_reads', 'qc_outlier'):
			raise NotImplementedError('{0} is not exported by this facade: call normalisr_amd.qc.{0} (or `normalisr {0}` on the command line).'.format(name))
		if name == 'pccovt':
			raise NotImplementedError('pccovt is not exported by this facade: call normalisr_amd.gocovt.pccovt (or `normalisr pccovt` on the command line).')
		raise NotImplementedError('normalisr_amd provides the pipeline from lcpm to binnet; '
								  '{} is not part of this build.'.format(name))
	raise AttributeError(name)


assert __name__ != "__main__"
