"""`python -m normalisr_amd <cmd>` / `normalisr <cmd>`: command line of the pipeline from read counts to the network.
Same sub-commands, positionals and flags as the reference CLI for `lcpm` (__main__.py:164-216), `normcov` (:222-245), `fitvar` (:251-272), `normvar` (:311-352),
`de` (:358-436), `coex` (:442-492) and `binnet` (:498-509), global -v (:14-17), help on stderr + exit 1 without arguments (:649-651)."""
import argparse
import logging
import sys


def build_parser():
	p0 = argparse.ArgumentParser(prog='normalisr', description='Normalisr on AMD MI355X: normalisation (lcpm, normcov, fitvar, normvar), association testing '
								 '(de, coex) and network binarisation (binnet).  The quality-control and post-processing sub-commands are not provided by this build.')
	p0.add_argument('-v', dest='verbose', action='store_true', help='Verbose mode.')
	sub = p0.add_subparsers(help='sub-commands', dest='cmd')

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
	if args.get('gpus', 1) > 1:  # one process per GPU, started before anything in this process touches a GPU
		from . import launch
		return launch.run_sharded(args['cmd'], args)
	from . import run
	getattr(run, args['cmd'])(args)
	return 0


if __name__ == '__main__':
	sys.exit(main())
