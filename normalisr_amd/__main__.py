"""`python -m normalisr_amd <cmd>` / `normalisr <cmd>`: command line of the pipeline from read counts to the network.
Same sub-commands, positionals and flags as the reference CLI for `lcpm` (__main__.py:164-216), `normcov` (:222-245), `fitvar` (:251-272), `normvar` (:311-352),
`de` (:358-436), `coex` (:442-492) and `binnet` (:498-509), and for the quality-control steps `qc_reads` (:24-113), `subset` (:120-158) and `qc_outlier`
(:275-305); global -v (:14-17), help on stderr + exit 1 without arguments (:649-651).  `principal` and `pccovt` are sub-commands of this build's own: the two
numerical parts of the reference's `gocovt` (:512-597), whose GO enrichment between them is not provided; `enrich`, also this build's own, does that step
from local gene-set files (normalisr_amd/enrich.py) and writes the pathway's genes for `pccovt`; `bh`, this build's own too, turns de's P-value matrix into
Benjamini-Hochberg q-values over all its entries (the reference has the function, binnet.py:77-131, and no command for it)."""
import argparse
import logging
import sys


def build_parser():
	p0 = argparse.ArgumentParser(prog='normalisr', description='Normalisr on AMD MI355X: quality control (qc_reads, subset, qc_outlier), normalisation (lcpm, normcov, '
								 'fitvar, normvar), association testing (de, coex), network binarisation (binnet), q-values over a result matrix (bh) and the covariate of a pathway\'s top principal component '
								 '(principal, pccovt).  The sub-command gocovt is not provided: its GO enrichment needs goatools and a web service.  Run principal, find the '
								 'enriched pathway among its genes with any tool, and hand the pathway\'s genes to pccovt.  The sub-command enrich does the first two of these steps on the '
								 'device from local gene-set files (GMT, or GO as OBO + GAF): Fisher exact tests by this build\'s own contract, not goatools\' output.')
	p0.add_argument('-v', dest='verbose', action='store_true', help='Verbose mode.')
	sub = p0.add_subparsers(help='sub-commands', dest='cmd')

	p = sub.add_parser('qc_reads', help='Quality control of genes and cells by lower bounds on read counts; the defaults suit 10x datasets.')
	p.add_argument('reads_in', help='Input read-count matrix (genes x cells) without row or column names: TSV if dense (default), Matrix Market (.mtx, .mtx.gz) with -s.')
	p.add_argument('genes_in', help='Input text file of the gene names (rows of reads_in), one per line.')
	p.add_argument('cells_in', help='Input text file of the cell names (columns of reads_in), one per line.')
	p.add_argument('genes_out', help='Output text file of the names of the genes that pass, same format.')
	p.add_argument('cells_out', help='Output text file of the names of the cells that pass, same format.')
	p.add_argument('--gene_read_count', dest='n_gene', action='store', type=int, default='0', help='Reads a gene needs. 0 disables. Default: 0.')
	p.add_argument('--gene_cell_count', dest='nc_gene', action='store', type=int, default='50', help='Cells that must express a gene. 0 disables. Default: 50.')
	p.add_argument('--gene_cell_prop', dest='ncp_gene', action='store', type=float, default='0.02', help='Share of the cells that must express a gene. 0 disables. Default: 0.02.')
	p.add_argument('--cell_read_count', dest='n_cell', action='store', type=int, default='500', help='Reads a cell needs. 0 disables. Default: 500.')
	p.add_argument('--cell_gene_count', dest='nt_cell', action='store', type=int, default='100', help='Genes a cell must express. 0 disables. Default: 100.')
	p.add_argument('--cell_gene_prop', dest='ntp_cell', action='store', type=float, default='0', help='Share of the genes a cell must express. 0 disables. Default: 0.')
	p.add_argument('-s', dest='sparse', action='store_true', help='Read reads_in as a sparse Matrix Market (COO) file; needs scipy. The counts stay sparse on the device.')

	p = sub.add_parser('subset', help='Cut a matrix down to the rows and columns named; removes genes and cells after quality control.')
	p.add_argument('matrix_in', help='Input matrix without row or column names: TSV if dense (default), Matrix Market (.mtx, .mtx.gz) with -s.')
	p.add_argument('matrix_out', help='Output matrix after subsetting, TSV.')
	p.add_argument('-r', nargs=2, metavar=('row_before', 'row_after'), help='Text files of the row names before and after subsetting, one per line.')
	p.add_argument('-c', nargs=2, metavar=('col_before', 'col_after'), help='Text files of the column names before and after subsetting, one per line.')
	p.add_argument('--nodummy', dest='nodummy', action='store_true', help='Drop single-valued columns / rows when subsetting only the rows / columns.')
	p.add_argument('-s', dest='sparse', action='store_true', help='Read matrix_in as a sparse Matrix Market (COO) file; needs scipy.')

	p = sub.add_parser('qc_outlier', help='Find outlier cells from the fitted variance.')
	p.add_argument('weights_in', help='Input vector of the fitted weight of each cell (weights_out of fitvar), TSV.')
	p.add_argument('cells_in', help='Input text file of the cell names, one per line.')
	p.add_argument('cells_out', help='Output text file of the names of the cells that pass, same format.')
	p.add_argument('--pcut', dest='pcut', action='store', type=float, default='1E-10', help='Bonferroni P-value cutoff for outliers. Default: 1E-10.')
	p.add_argument('--outrate', dest='outrate', action='store', type=float, default='0.02',
				   help='Largest share of outliers on either tail of the variance distribution: sets the start and bounds the result. Default: 0.02.')

	p = sub.add_parser('de', help='Differential expression analysis.')
	p.add_argument('design_in', help='Design/predictor matrix (predictors x cells), TSV without row or column names.')
	p.add_argument('exp_in', help='Normalized expression matrix (genes x cells), TSV.')
	p.add_argument('cov_in', help='Covariate matrix (covariates x cells), TSV.')
	p.add_argument('pv_out', help='Output P-value matrix (predictors x genes), TSV.')
	p.add_argument('lfc_out', help='Output log fold change matrix (predictors x genes), TSV.')
	p.add_argument('-m', dest='method', action='store', default='ignore',
				   help='Treatment of the other predictors when testing one: "ignore" (default), "single" (only cells with all other '
				   'predictors == 0; low-MOI screens), "covariate" (other predictors as covariates; high-MOI screens).')
	p.add_argument('-n', dest='nth', action='store', type=int, default='0', help='Number of CPU cores (kept for compatibility; the GPU path ignores it).')
	p.add_argument('-b', dest='bs', action='store', type=int, help='Batch size (kept for compatibility; results do not depend on it).')
	p.add_argument('-d', dest='dimr', action='store', type=int, help='Extra dimension loss in the expression data due to preprocessing. Default: 0.')
	p.add_argument('--clfc_out', dest='clfc_out', action='store', help='Output covariate log fold changes, (predictors, genes*covariates) row-major, TSV.')
	p.add_argument('--vard_out', dest='vard_out', action='store', help='Output variance of each predictor unexplained by covariates, TSV.')
	p.add_argument('--vart_out', dest='vart_out', action='store', help='Output variance of expression unexplained by covariates (predictors x genes), TSV.')
	p.add_argument('--logp', dest='logp', action='store_true', default=None,
				   help='Write the natural logarithm of the P-values into pv_out: finite where a P-value underflows to 0 (method "ignore", one GPU).')
	p.add_argument('--gpus', dest='gpus', action='store', type=int, default=1, help='GPUs of this node to shard the problem over (one process per GPU, RCCL); every rank reads only its gene rows of exp_in. Default: 1.')

	p = sub.add_parser('coex', help='Co-expression analysis.')
	p.add_argument('exp_in', help='Normalized expression matrix (genes x cells), TSV.')
	p.add_argument('cov_in', help='Covariate matrix (covariates x cells), TSV.')
	p.add_argument('pv_out', help='Output P-value matrix (genes x genes), TSV.')
	p.add_argument('-n', dest='nth', action='store', type=int, default='0', help='Number of CPU cores (kept for compatibility; the GPU path ignores it).')
	p.add_argument('-b', dest='bs', action='store', type=int, help='Batch size (kept for compatibility; results do not depend on it).')
	p.add_argument('-d', dest='dimr', action='store', type=int, help='Extra dimension loss in the expression data due to preprocessing. Default: 0.')
	p.add_argument('--var_out', dest='var_out', action='store', help='Output variance of each gene unexplained by covariates, TSV.')
	p.add_argument('--dot_out', dest='dot_out', action='store',
				   help='Output covariance of gene pairs after covariate removal (inner product / cell count), TSV. Pearson R = dot/sqrt(var_i var_j).')
	p.add_argument('--logp', dest='logp', action='store_true', default=None,
				   help='Write the natural logarithm of the P-values into pv_out: finite where a P-value underflows to 0; -INF on the diagonal (one GPU).')
	p.add_argument('--gpus', dest='gpus', action='store', type=int, default=1, help='GPUs of this node to shard the problem over (one process per GPU, RCCL); every rank reads only its gene rows of exp_in. Default: 1.')
	p = sub.add_parser('lcpm', help='Compute Bayesian expectation of logCPM and cellular summary covariates from read counts.')
	p.add_argument('reads_in', help='Input read-count matrix (genes x cells) without row or column names: TSV if dense (default), Matrix Market (.mtx, .mtx.gz) with -s.')
	p.add_argument('lcpm_out', help='Output Bayesian logCPM matrix (genes x cells), always dense, TSV.')
	p.add_argument('scale_out', help='Output vector of the variance-normalisation scaling factor of each gene, TSV.')
	p.add_argument('cov_out', help='Output matrix of the 3 cellular summary covariates (after the rows of -c, if given), TSV.')
	p.add_argument('-s', dest='sparse', action='store_true', help='Read reads_in as a sparse Matrix Market (COO) file; needs scipy.')
	p.add_argument('-r', dest='rseed', action='store', type=int, help='Initial random seed (kept for compatibility; the posterior expectation draws nothing).')
	p.add_argument('-n', dest='nth', action='store', type=int, default='0', help='Number of CPU cores (kept for compatibility; the GPU path ignores it).')
	p.add_argument('-c', dest='cov_in', help='Input matrix of existing covariates (covariates x cells), TSV; the new covariates are appended after them in cov_out.')
	p.add_argument('--var_out', help='Output matrix of the variance of the posterior distribution of logCPM (genes x cells), TSV.')

	p = sub.add_parser('normcov', help='Normalize continuous covariates and include constant 1 covariate as intercept.')
	p.add_argument('cov_in', help='Input covariate matrix (covariates x cells), TSV; can be cov_out of lcpm.')
	p.add_argument('cov_out', help='Output matrix of normalized covariates, same format.')
	p.add_argument('--no1', dest='no1', action='store_true', default=False, help='Do not add the constant 1 covariate (only if this is not the last normcov step).')

	p = sub.add_parser('fitvar', help='Fit lognormal distribution of variance with covariates.')
	p.add_argument('lcpm_in', help='Input Bayesian logCPM matrix (genes x cells), TSV.')
	p.add_argument('cov_in', help='Input covariate matrix (covariates x cells), TSV.')
	p.add_argument('weights_out', help='Output vector of the fitted weight (variance**-0.5) of each cell, TSV.')

	p = sub.add_parser('normvar', help='Normalize variances of gene expressions and covariates.')
	p.add_argument('lcpm_in', help='Input Bayesian logCPM matrix (genes x cells), TSV.')
	p.add_argument('weights_in', help='Input vector of the fitted weight of each cell, TSV.')
	p.add_argument('cov_in', help='Input covariate matrix (covariates x cells), TSV.')
	p.add_argument('scale_in', help='Input vector of the variance-normalisation scaling factor of each gene, TSV.')
	p.add_argument('exp_out', help='Output normalized expression matrix, same format as lcpm_in.')
	p.add_argument('cov_out', help='Output normalized covariate matrix.')
	p.add_argument('-n', dest='nth', action='store', type=int, default='0', help='Number of CPU cores (kept for compatibility; ignored).')
	p.add_argument('-b', dest='bs', action='store', type=int, help='Batch size (kept for compatibility; ignored).')

	p = sub.add_parser('binnet', help='Binarize P-value co-expression network.')
	p.add_argument('pv_in', help='Input P-value matrix of gene pairwise co-expression (genes x genes), TSV.')
	p.add_argument('net_out', help='Output binary co-expression network (genes x genes, 0/1), TSV.')
	p.add_argument('qcut', type=float, help='Q-value cutoff for binary network.')
	p.add_argument('--logp', dest='logp', action='store_true', default=None,
				   help='pv_in holds the natural logarithms of the P-values (pv_out of coex --logp; -INF on the diagonal): the network is cut on ln q.')

	p = sub.add_parser('bh', help='Benjamini-Hochberg q-values over all entries of a P-value matrix (pv_out of de); a sub-command of this build\'s own.')
	p.add_argument('pv_in', help='Input P-value matrix or vector, TSV.')
	p.add_argument('q_out', help='Output q-values in the same shape, TSV.')
	p.add_argument('--logp', dest='logp', action='store_true', default=None,
				   help='pv_in holds the natural logarithms of the P-values (pv_out of de --logp); q_out receives ln q, finite where q underflows to 0.')

	p = sub.add_parser('principal', help='List the principal genes of a binary co-expression network: the genes with the most co-expressed genes (the selection of '
					   'the reference\'s gocovt, without its GO enrichment).')
	p.add_argument('net_in', help='Input binary co-expression network (genes x genes, 0/1), TSV; net_out of binnet.')
	p.add_argument('genes_in', help='Input text file of the gene names (rows of net_in), one per line.')
	p.add_argument('master_out', help='Output text file of the names of the principal genes, same format.')
	p.add_argument('-n', dest='n', action='store', type=int, default='100', help='Number of top principal genes; genes that tie with the last one are kept too. Default: 100.')

	p = sub.add_parser('enrich', help='Find the gene set most enriched among the principal genes of a binary co-expression network, from local gene-set files, and '
					   'write its genes for pccovt.')
	p.add_argument('net_in', help='Input binary co-expression network (genes x genes, 0/1), TSV; net_out of binnet.')
	p.add_argument('genes_in', help='Input text file of the gene names (rows of net_in), one per line; all of them are the background.')
	p.add_argument('pathway_out', help='Output text file of the names of the genes of the top enriched set, one per line: pathway_in of pccovt.')
	g = p.add_mutually_exclusive_group(required=True)
	g.add_argument('--gmt', dest='gmt', action='store', help='Gene sets as a GMT file: name<TAB>description<TAB>gene<TAB>gene... per line.')
	g.add_argument('--go', dest='go', nargs=2, metavar=('go_obo', 'goa_gaf'), help='Gene sets from a GO ontology (OBO) and an annotation file (GAF 2.x).')
	p.add_argument('--key', dest='key', action='store', default='id', choices=('id', 'symbol'),
				   help='With --go: match genes by the annotation file\'s object id ("id", column 2; default) or symbol ("symbol", column 3).')
	p.add_argument('-n', dest='n', action='store', type=int, default='100', help='Number of top principal genes; genes that tie with the last one are kept too. Default: 100.')
	p.add_argument('-m', dest='nmin', action='store', type=int, default='5', help='Fewest principal genes the top set must hold. Default: 5.')
	p.add_argument('--master_out', dest='master_out', action='store', help='Output text file of the names of the principal genes, one per line.')
	p.add_argument('--goe_out', dest='goe_out', action='store', help='Output enrichment table, TSV with a header line, sorted by P-value.')
	p.add_argument('--go_out', dest='go_out', action='store', help='Output text file holding the name (GO id) of the top enriched set.')

	p = sub.add_parser('pccovt', help='Append the top principal component of the chosen genes (a pathway) as a covariate.')
	p.add_argument('exp_in', help='Normalized expression matrix (genes x cells), TSV.')
	p.add_argument('cov_in', help='Covariate matrix (covariates x cells), TSV.')
	p.add_argument('genes_in', help='Input text file of the gene names (rows of exp_in), one per line.')
	p.add_argument('pathway_in', help='Input text file of the names of the genes whose top principal component is taken, one per line.')
	p.add_argument('cov_out', help='Output covariate matrix with the new covariate as its last row, same format as cov_in.')
	p.add_argument('--nocond', dest='nocond', action='store_true', help='Do not remove the existing covariates from the expression before taking the component.')

	p = sub.add_parser('coex_levels', help='Run the co-expression loop (coex, binnet, enrich, pccovt, once per level) in one process with the problem resident on '
					   'the device: every level appends the top principal component of the top enriched gene set as a covariate.')
	p.add_argument('exp_in', help='Normalized expression matrix (genes x cells), TSV.')
	p.add_argument('cov_in', help='Covariate matrix of level 0 (covariates x cells), TSV.')
	p.add_argument('genes_in', help='Input text file of the gene names (rows of exp_in), one per line; all of them are the background.')
	p.add_argument('qcut', type=float, help='Q-value cutoff for the binary networks.')
	p.add_argument('out_dir', help='Output directory: lv{k}_net, lv{k}_master.txt, lv{k}_go.txt, lv{k}_pathway.txt, lv{k}_goe.tsv and lv{k+1}_cov per level k.')
	g = p.add_mutually_exclusive_group(required=True)
	g.add_argument('--gmt', dest='gmt', action='store', help='Gene sets as a GMT file: name<TAB>description<TAB>gene<TAB>gene... per line.')
	g.add_argument('--go', dest='go', nargs=2, metavar=('go_obo', 'goa_gaf'), help='Gene sets from a GO ontology (OBO) and an annotation file (GAF 2.x).')
	p.add_argument('--key', dest='key', action='store', default='id', choices=('id', 'symbol'),
				   help='With --go: match genes by the annotation file\'s object id ("id", column 2; default) or symbol ("symbol", column 3).')
	p.add_argument('-l', dest='lvmax', action='store', type=int, default='5', help='Last level; levels 0 to this one are run. Default: 5.')
	p.add_argument('-n', dest='n', action='store', type=int, default='100', help='Number of top principal genes; genes that tie with the last one are kept too. Default: 100.')
	p.add_argument('-m', dest='nmin', action='store', type=int, default='5', help='Fewest principal genes the top set must hold. Default: 5.')
	p.add_argument('-d', dest='dimr', action='store', type=int, default=None, help='Degrees of freedom removed by preprocessing. Default: 0.')
	p.add_argument('--ext', dest='ext', action='store', default='.tsv', choices=('.tsv', '.tsv.gz', '.npy'), help='Suffix (and format) of the matrix files. Default: .tsv.')
	p.add_argument('--pv', dest='pv', action='store_true', help='Also write the P-value matrix of every level, lv{k}_pv.')
	p.add_argument('--dot', dest='dot', action='store_true', help='Also write the covariance matrix of every level, lv{k}_dot.')
	p.add_argument('--var', dest='var', action='store_true', help='Also write the variances of every level, lv{k}_var.')
	return p0


def main(argv=None):
	argv = sys.argv[1:] if argv is None else argv
	p0 = build_parser()
	if len(argv) == 0:
		p0.print_help(sys.stderr)
		return 1
	args = vars(p0.parse_args(argv))
	logging.basicConfig(format='%(levelname)s:%(process)d:%(asctime)s:%(pathname)s:%(lineno)d:%(message)s',
						level=logging.DEBUG if args['verbose'] else logging.WARNING)
	if args['cmd'] is None:
		p0.print_help(sys.stderr)
		return 1
	if args.get('gpus', 1) < 1:
		raise ValueError('--gpus must be positive')
	if args.get('gpus', 1) > 1 and args.get('logp'):
		raise NotImplementedError('--logp is available on one GPU only (the sharded paths return P-values).')
	if args.get('gpus', 1) > 1:  # one process per GPU, started before anything in this process touches a GPU
		from . import launch
		return launch.run_sharded(args['cmd'], args)
	from . import run
	getattr(run, args['cmd'])(args)
	return 0


if __name__ == '__main__':
	sys.exit(main())
