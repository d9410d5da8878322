/*
 * normalisr_hip.h -- C ABI of libnormalisr_hip.so: the MI355X (gfx950) implementation of Normalisr's
 * linear-association hot path (covariate residualisation -> Gram contraction -> R^2 -> p-value).
 *
 * The reference (lingfeiwang/normalisr v1.0.0) is pure Python and has no FFI; the seams this ABI
 * replaces are named per function below as file:line under /root/reference/src/normalisr/.
 * Conventions:
 *   - every function returns 0 on success or a negative NRM_E_* code; nrm_last_error() gives the text;
 *   - all matrices are row-major with cells contiguous (association.py:163-170); `ld*` are row pitches
 *     in ELEMENTS; dtype codes: NRM_F32 = 0, NRM_F64 = 1;
 *   - pointers named d_* are DEVICE pointers (HBM) owned by the caller; the library never frees or
 *     retains them past return; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     kernels are enqueued asynchronously on it;
 *   - pointers named h_* are HOST pointers (numpy buffers); those entry points synchronise.
 * No torch / Python types cross this boundary.  Bound from Python with ctypes (normalisr_amd/_lib.py),
 * see INTEGRATION.md for the stub a maintainer of the reference would add.
 */
#ifndef NORMALISR_HIP_H
#define NORMALISR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRM_F32 0
#define NRM_F64 1

#define NRM_OK 0
#define NRM_E_ARG -1      /* bad shape/argument  -> ValueError   (association.py:199-216)  */
#define NRM_E_DEVICE -2   /* HIP runtime failure -> RuntimeError                           */
#define NRM_E_NUMERIC -3  /* non-finite / out-of-range result -> AssertionError (association.py:248-259) */
#define NRM_E_UNSUPPORTED -4  /* the call is outside what a whole-problem host entry covers (nrm_last_error says why): use another path -> NotImplementedError */

/* Tile geometry the padded device buffers must honour (rows multiple of NRM_ROW_TILE, pitch and
 * cell count multiple of NRM_K_TILE). */
#define NRM_ROW_TILE 128
#define NRM_K_TILE 16

/* Number of u-polynomial coefficients of the p-value fast path (see nrm_pvalue_plan). */
#define NRM_PCOEF 20

int nrm_version(void);
const char* nrm_last_error(void);
/* hipGetDeviceCount / hipSetDevice wrappers so that a pure-C host needs no HIP headers. */
int nrm_device_count(int* count);
int nrm_set_device(int device);
/* Result buffers on the host (the caller's numpy arrays, filled where the reference's gather loop fills them,
 * association.py:1005-1034): nrm_host_pin faults the pages of [ptr, ptr+bytes) in with `threads` host threads
 * (0 = choose; contents are preserved) and page-locks the range so device->host copies run at the PCIe rate;
 * nrm_copy_to_host queues such a copy on `stream`; nrm_host_unpin releases the lock (after the stream is synchronised). */
int nrm_host_pin(void* ptr, int64_t bytes, int threads);
int nrm_host_unpin(void* ptr);
int nrm_copy_to_host(void* h_dst, const void* d_src, int64_t bytes, void* stream);
/* Page-locked host memory owned by the library's caller (hipHostMalloc / hipHostFree): the Python host keeps a pool of such
 * blocks behind the numpy result arrays it returns, so that repeated calls neither fault in nor register fresh pages. */
int nrm_host_alloc(void** ptr, int64_t bytes);
int nrm_host_free(void* ptr);
/* a rectangle (rows x row_bytes, pitches in bytes) of a device matrix -> the same rectangle of a host matrix, queued on `stream` */
/* Host side of a symmetric result that arrives by rows: h[0:a, a:b] = h[a:b, 0:a]^T for a row-major matrix of 4- or 8-byte elements
 * (`threads` host threads, 0 = one per 4 hardware threads up to 32).  The numpy-out coex path ships only the rows a..b up to column b over
 * PCIe and mirrors them here while later rows are in flight (the reference mirrors on the host too: association.py:1049-1057). */
int nrm_host_mirror_rows(void* h, int64_t ld_bytes, int elem_bytes, int64_t a, int64_t b, int threads);
int nrm_copy_rect_to_host(void* h_dst, int64_t dst_pitch, const void* d_src, int64_t src_pitch, int64_t row_bytes, int64_t rows, void* stream);
/* Device-side assembly of the padded operand buffers (zero padding, stacking [C; X~] for the streaming path, gathering sums of
 * squares of row chunks): asynchronous on `stream`; pitches and row_bytes in BYTES. */
int nrm_fill_zero(void* d_dst, int64_t bytes, void* stream);
int nrm_fill_i32(void* d_dst, int32_t value, int64_t count, void* stream);  /* count int32 words = value */
int nrm_copy_rows(void* d_dst, int64_t dst_pitch, const void* d_src, int64_t src_pitch, int64_t row_bytes, int64_t rows, void* stream);

/*
 * K1 -- residualise rows against covariates and take their sums of squares.
 * Replaces association.py:224-233 (ccx = dci@(dc@dx.T); dx1 = dx - ccx@dc; mean of squares) and
 * removes the per-tile recomputation (the reference redoes this inside every 500x500 tile).
 *   d_x     (rows, n) input rows, dtype x_dtype, pitch ldx
 *   d_c     (nc, n) fp64 covariates, pitch ldc;  d_dci (nc, nc) fp64 pseudo-inverse of C C^T
 *           (computed on the host in fp64: inv_rank, association.py:4-134); rank = integer rank;
 *           rank == 0 or nc == 0 -> rows are copied unchanged (association.py:224).
 *   d_out   (rows_pad, ldo) fp64 residualised rows, zero-filled for cells >= n and rows >= rows
 *   d_ss    (rows_pad) fp64  sum_k out[i,k]^2   (variance * n; the 0 -> 1 rule is applied later)
 *   d_coef  (rows, nc) fp64 or NULL: the OLS coefficients ccx, needed only for alpha (lowmem=False)
 */
int nrm_residualize(const void* d_x, int x_dtype, int64_t rows, int64_t n, int64_t ldx,
					const double* d_c, int64_t nc, int64_t ldc, const double* d_dci, int rank,
					double* d_out, int64_t ldo, int64_t rows_pad,
					double* d_ss, double* d_coef, void* stream);

/* K1 with fixed-point output for the integer Gram engine (see nrm_quantize_rows below): the residuals are rounded and cut into
 * digit planes inside K1 (a second sweep over the rows, which are in L2 by then), so the fp64 residuals need not travel through
 * HBM at all: d_out may be NULL.  Needs 16-byte aligned rows and rows_pad % NRM_ROW_TILE == 0; d_q holds
 * nrm_quant_bytes(rows_pad, round_up(n, 16), nslices) bytes, d_exp rows_pad int32.  plane_pitch_bytes != 0: the rows are a
 * block of 32-row groups of a larger quantised matrix (d_q points at the block's first group, the pitch is the larger matrix's:
 * rows that arrive chunk by chunk fill one set of planes).  d_cmax (nc) = max_k |C[c,k]| of every covariate row, or NULL: with it
 * the fixed-point scale of a row comes from the bound max|x| + sum_c |b_c| max|C_c| >= max|residual| and the rows are swept twice
 * instead of three times -- as long as that bound lies within 12x of the residuals' rms (estimated in the first sweep); rows whose
 * mean dwarfs their spread, or whose covariates nearly cancel, are swept for their true maximum so that the overestimate never
 * costs more than a few of the 8 * nslices - 2 bits.
 * d_fix (rows_pad, NRM_FIX_STRIDE) fp64 or NULL: one record per row for K3 (nrm_assoc_sweep* below): the digit sums of the planes
 * whose products the integer engine leaves out (K3 adds the product of the digit means back exactly) and the two numbers of the
 * accuracy guard, c = sqrt(max digit variance / |q|^2) and g = sqrt(n) / (2 |q|); see csrc/nrm_fix.h.  The reference computes this
 * contraction in fp64 (association.py:224-235); the records are what lets the integer engine certify, pair by pair, that its
 * P-values agree with that to the stated tolerance.  Rows of fewer than 2^22 cells. */
#define NRM_FIX_STRIDE 8
int nrm_residualize_q(const void* d_x, int x_dtype, int64_t rows, int64_t n, int64_t ldx,
					  const double* d_c, int64_t nc, int64_t ldc, const double* d_dci, int rank,
					  double* d_out, int64_t ldo, int64_t rows_pad, double* d_ss, double* d_coef,
					  int nslices, void* d_q, int32_t* d_exp, int64_t plane_pitch_bytes, const double* d_cmax, double* d_fix, void* stream);
/* Profiling aid, not part of the product path: d_stamps = a device buffer of 6 int64 per row of nrm_binnet* (time stamps: start, row loaded,
 * threshold found, mask written; counting passes; spare) that later launches fill; NULL switches it off (tools/time_binnet.py). */
int nrm_binnet_debug_buffer(void* d_stamps);
/* The same with the digit planes cut along the cells into chunks of 32 * chunk_ksteps cells: chunk c is a dense quantised operand
 * of its own (nslices planes of rows_pad / 32 * chunk_ksteps KB) at d_q + c * nrm_quant_bytes(rows_pad, 32 * chunk_ksteps, nslices);
 * all chunks share d_exp; the last chunk is zero padded.  The sharded coex path (normalisr_amd/distributed.py; the N > 1 form of
 * association.py:890-909) sends the chunks to the other GPUs one after another and contracts each as it lands. */
int nrm_residualize_q_chunked(const void* d_x, int x_dtype, int64_t rows, int64_t n, int64_t ldx,
							  const double* d_c, int64_t nc, int64_t ldc, const double* d_dci, int rank,
							  int64_t rows_pad, double* d_ss, int nslices, void* d_q, int32_t* d_exp,
							  int64_t chunk_ksteps, const double* d_cmax, double* d_fix, void* stream);

/*
 * K2 -- Gram contraction dot[i,j] = sum_k A[i,k] B[j,k] on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64, 128x128 workgroup tiles staged through LDS).
 * Replaces np.matmul(dy1, dx1.T) at association.py:234 for ALL tiles of the problem at once.
 *   d_a (m_pad, lda), d_b (n_pad, ldb) fp64, zero padded; m_pad, n_pad multiples of NRM_ROW_TILE;
 *   k_pad multiple of NRM_K_TILE; d_dot (m_pad, ldd) fp64.
 *   symmetric != 0 (coex: d_b == d_a): only tiles on or above the block diagonal are computed and
 *   written (association.py:893-894); the strictly-lower tiles of d_dot are left untouched, and inside
 *   diagonal tiles only 16x16 sub-blocks on or above the diagonal are guaranteed.
 *   m_rows, n_rows: valid (unpadded) row counts (0 = all): 16-row sub-blocks that are pure padding are skipped
 *   and their outputs left unwritten.
 */
int nrm_gram_f64(const double* d_a, const double* d_b, int64_t m_pad, int64_t n_pad, int64_t k_pad,
				 int64_t lda, int64_t ldb, double* d_dot, int64_t ldd, int symmetric,
				 int64_t m_rows, int64_t n_rows, void* d_work, void* stream);
/* The same for the output rows [row0, row1) only (cut at multiples of 8 * NRM_ROW_TILE, or at m_pad): lets the caller
 * pipeline K2 -> K3 -> copy-out band by band, as the reference hands finished tiles to the gather loop
 * (association.py:997-1034).  Consecutive bands on one stream may share d_work. */
int nrm_gram_f64_band(const double* d_a, const double* d_b, int64_t m_pad, int64_t n_pad, int64_t k_pad,
					  int64_t lda, int64_t ldb, double* d_dot, int64_t ldd, int symmetric,
					  int64_t m_rows, int64_t n_rows, int64_t row0, int64_t row1, void* d_work, void* stream);
/* Size of the device scratch nrm_gram_f64 needs in d_work (partial tiles of the stream-K tail; summed in a fixed
 * order, so results are bitwise reproducible).  Independent of the problem size. */
int64_t nrm_gram_workspace_bytes(void);

/*
 * K2, integer engine -- the same contraction computed EXACTLY on the int8 matrix cores from fixed-point operands
 * (csrc/nrm_gram_i8.hip): every row is scaled by a power of two, rounded once to 8 * nslices - 2 bits (nslices = 6: 46 bits,
 * 1.4e-14 of the row's largest entry; 5: 38 bits) and cut into nslices balanced base-256 digits; the digit products are
 * accumulated in int32 without rounding and combined in fp64.  About 2.5x (6 slices) / 3.4x (5) the rate of the fp64 kernel.
 *   nrm_quantize_rows: d_x (rows_pad, ldx) fp64 rows as written by nrm_residualize (rows_pad % 32 == 0 -- % NRM_ROW_TILE for
 *       nrm_gram_i8 operands --, k_pad % 16 == 0, zero padded) -> d_q (nrm_quant_bytes() bytes: digit planes in the kernel's tiled layout) and d_exp (rows_pad) int32 with
 *       x = q * 2^exp.
 *   nrm_gram_i8_band: as nrm_gram_f64_band with quantised operands (d_qb == d_qa, d_eb == d_ea for symmetric problems).
 *       plane_*_bytes: distance between an operand's digit planes, 0 = dense (m_pad / 32 * ceil(k_pad / 32) KB); an operand may be
 *       a block of 32-row groups of a larger quantised matrix: pass the pointer of its first group and the larger matrix's pitch.
 *       d_ea 16-byte aligned (the kernel reads four row exponents at a time; any 32-row group of an aligned array is), ldd < 2^27.
 */
int64_t nrm_quant_bytes(int64_t rows_pad, int64_t k_pad, int nslices);
int nrm_quantize_rows(const double* d_x, int64_t rows_pad, int64_t k_pad, int64_t ldx, int nslices, void* d_q, int32_t* d_exp,
					  double* d_fix /* row records as in nrm_residualize_q, or NULL */, int64_t n_cells /* valid cells (<= k_pad), for d_fix */, void* stream);
int nrm_gram_i8_band(const void* d_qa, const int32_t* d_ea, int64_t plane_a_bytes, const void* d_qb, const int32_t* d_eb,
					 int64_t plane_b_bytes, int64_t m_pad, int64_t n_pad, int64_t k_pad, int nslices, double* d_dot, int64_t ldd,
					 int symmetric, int64_t m_rows, int64_t n_rows, int64_t row0, int64_t row1, void* d_work, void* stream);
/* One cell chunk (k_pad = its cells) of a contraction whose operands arrive in chunks: accumulate != 0 adds the chunk's exact
 * partial dot products to d_dot in fp64 instead of overwriting it.  b_block_rows != 0: operand B is n_pad / b_block_rows blocks
 * (cyclically from block b_first of b_count) of a gathered buffer, block b a dense quantised operand of b_block_rows padded rows
 * at d_qb + b * b_block_stride_bytes with its exponents at d_eb + b * b_block_rows: all full partner blocks of a rank in one
 * launch (the N > 1 form of the x0 <= y0 tile loop, association.py:890-909). */
int nrm_gram_i8_chunk(const void* d_qa, const int32_t* d_ea, int64_t plane_a_bytes, const void* d_qb, const int32_t* d_eb,
					  int64_t plane_b_bytes, int64_t m_pad, int64_t n_pad, int64_t k_pad, int nslices, double* d_dot, int64_t ldd,
					  int symmetric, int64_t m_rows, int64_t n_rows, int accumulate, int64_t b_block_rows, int64_t b_block_stride_bytes,
					  int b_first, int b_count, void* d_work, void* stream);

/*
 * P-value plan: host-side constants of p = I_{1-R^2}(dof/2, 1/2) for one dof
 * (scipy.stats.beta.cdf call at association.py:249).  dof is uniform per call for single=0:
 * dof = n_cell - 1 - rank - dimreduce.
 */
typedef struct nrm_pvalue_plan {
	double a;                /* dof / 2                                                   */
	double alpha;            /* a - 1/4                                                   */
	double ln_front;         /* ln( Gamma(a+1/2) / (Gamma(a) sqrt(pi)) )                  */
	double umax;             /* fast path used for -ln(1-R^2) <= umax (0 = never)         */
	double coef[NRM_PCOEF];  /* fast path: p = exp(-alpha u)(erfcx(sqrt(alpha u)) + sqrt(alpha u) sum_j coef[j] u^j) */
} nrm_pvalue_plan;
int nrm_pvalue_plan_init(nrm_pvalue_plan* plan, double dof);
/* The same for `count` dofs (single=1: one dof per grouping, association.py:374): record j = the 24 doubles of the plan
 * for dof[j], written at out + j * pitch (pitch in doubles, >= 24). */
int nrm_pvalue_plan_init_many(const double* dof, int64_t count, double* out, int64_t pitch);
/* The same records from the double-precision form the device builds its plans with (csrc/nrm_pvalue_plan.h, here compiled for the host). */
int nrm_pvalue_plan_fill_many(const double* dof, int64_t count, double* out, int64_t pitch);

/* Elementwise p-values from R^2 (device arrays); kernel-level entry for the table tests. */
int nrm_pvalues_from_r2(const double* d_r2, int64_t count, double dof, double* d_p, void* stream);
/* The same for ln p (csrc/nrm_pvalue.h: nrm_logpvalue): finite for every 0 < fl(1 - R^2) < 1, whatever dof and R^2 -- at 100 000 cells an
 * R^2 of 0.0022 has ln p = -110, and every R^2 >= 1/4 a p that is 0 in double precision --, 0 where p = 1, -inf where fl(1 - R^2) <= 0. */
int nrm_logpvalues_from_r2(const double* d_r2, int64_t count, double dof, double* d_lnp, void* stream);

/*
 * K3 -- per-pair sweep: R^2 = dot^2/(ssx_i ssy_j) -> p-value, effect size, optional Pearson r and t.
 * Replaces association.py:231-235,248-249 and the gather/symmetrise steps :1037-1057.
 *   d_dot (.., ldd) from nrm_gram_f64;  d_ssx (nx), d_ssy (ny) from nrm_residualize
 *   n_cells, dof as above.  zero sums of squares are replaced by n_cells (variance 0 -> 1, :231-233).
 *   symmetric != 0: coex -- pair (i,j) reads dot[min(i,j), max(i,j)], diagonal outputs are exactly 0
 *                   (association.py:1050-1057); requires nx == ny and d_ssx == d_ssy.
 *   stat_kind: 0 -> covariance x~.y~/n ("dot", association.py:1039,1048); 1 -> gamma = x~.y~/ssx (:234)
 *   outputs (nx, ldo) of dtype out_dtype; d_r / d_t may be NULL (north-star extras: Pearson r, t statistic)
 *   d_flags: int32[4] device counters, incremented for non-finite inputs [0] and R^2 > 1+1e-8 [1]
 *            (the reference's assertions at association.py:248,252); may be NULL when fix_nslices == 0.
 *   fix_nslices != 0 (5 or 6: d_dot came from the integer engine with that many digit planes): d_fixx (nx, NRM_FIX_STRIDE) and
 *            d_fixy (ny, ..) are the row records K1 wrote.  Every dot product first receives the exact correction for the coherent
 *            part of the digit products the engine left out; then, guard_tol > 0, the pair is checked: d_flags[2] counts the pairs
 *            whose P-value the engine's remaining error (a rigorous bound, csrc/nrm_fix.h) could move by more than guard_tol
 *            (relative) -- the host redoes such a call on nrm_gram_f64 -- and d_flags[3] receives the largest error estimate seen
 *            (bits of a float).
 */
int nrm_assoc_sweep(const double* d_dot, int64_t ldd, const double* d_ssx, const double* d_ssy,
					int64_t nx, int64_t ny, int64_t n_cells, double dof, int symmetric, int stat_kind,
					void* d_p, void* d_stat, void* d_r, void* d_t, int out_dtype, int64_t ldo,
					int32_t* d_flags, int fix_nslices, const double* d_fixx, const double* d_fixy, double guard_tol, void* stream);
/* The same for the x rows [row0, row1) (multiples of 64, or nx).  Symmetric problems: the band reads only dot rows
 * < row1 and, once the bands [0, row1) have run in order, output rows [0, row1) are complete (mirrored halves included). */
int nrm_assoc_sweep_band(const double* d_dot, int64_t ldd, const double* d_ssx, const double* d_ssy,
						 int64_t nx, int64_t ny, int64_t n_cells, double dof, int symmetric, int stat_kind,
						 void* d_p, void* d_stat, void* d_r, void* d_t, int out_dtype, int64_t ldo,
						 int32_t* d_flags, int64_t row0, int64_t row1, int fix_nslices, const double* d_fixx, const double* d_fixy,
						 double guard_tol, void* stream);

/* The same for an off-diagonal RECTANGLE of a symmetric (coex) problem: rows [r0, r0 + mx) against columns [c0, c0 + my),
 * c0 + my <= r0; d_dot (mx, ldd) holds that rectangle of the Gram matrix, d_ssx / d_ssy the sums of squares of its rows / columns.
 * Every pair is computed once and written at (r0 + i, c0 + j) AND (c0 + j, r0 + i) of the (ng, ldo) outputs (covariance in d_stat),
 * so a coex whose rows arrive chunk by chunk can finish and ship all pairs of a chunk at once (association.py:1049-1057). */
int nrm_assoc_sweep_mirror(const double* d_dot, int64_t ldd, const double* d_ssx, const double* d_ssy, int64_t mx, int64_t my,
						   int64_t n_cells, double dof, void* d_p, void* d_stat, int out_dtype, int64_t ldo, int64_t r0, int64_t c0,
						   int32_t* d_flags, int fix_nslices, const double* d_fixx, const double* d_fixy, double guard_tol, void* stream);

/* The three sweeps with the form of their first result as an argument: p_kind 0 = p (the entries above, which forward here), 1 = ln p,
 * rounded once to out_dtype.  ln p = 0 where p = 1, -inf exactly where p is a 0 that is no underflow (fl(1 - R^2) <= 0, and the diagonal of a
 * symmetric problem), finite for every other pair; NaN propagates and d_flags[0], [1] count as for p.  Everything else a sweep writes is the
 * same bytes for either p_kind (of a whole call: unless the guard below certifies it in one form and not in the other -- nrm_association_tests_host_pk).  The guard of the integer engine (fix_nslices != 0) in this form: a pair is uncertified when the bound on
 * |d ln p| exceeds guard_tol * max(1, |ln p|), and only pairs with fl(1 - R^2) <= 0 are exempt (csrc/nrm_fix.h). */
int nrm_assoc_sweep_pk(const double* d_dot, int64_t ldd, const double* d_ssx, const double* d_ssy,
					   int64_t nx, int64_t ny, int64_t n_cells, double dof, int symmetric, int stat_kind,
					   void* d_p, void* d_stat, void* d_r, void* d_t, int out_dtype, int64_t ldo,
					   int32_t* d_flags, int fix_nslices, const double* d_fixx, const double* d_fixy, double guard_tol, int p_kind, void* stream);
int nrm_assoc_sweep_band_pk(const double* d_dot, int64_t ldd, const double* d_ssx, const double* d_ssy,
							int64_t nx, int64_t ny, int64_t n_cells, double dof, int symmetric, int stat_kind,
							void* d_p, void* d_stat, void* d_r, void* d_t, int out_dtype, int64_t ldo,
							int32_t* d_flags, int64_t row0, int64_t row1, int fix_nslices, const double* d_fixx, const double* d_fixy,
							double guard_tol, int p_kind, void* stream);
int nrm_assoc_sweep_mirror_pk(const double* d_dot, int64_t ldd, const double* d_ssx, const double* d_ssy, int64_t mx, int64_t my,
							  int64_t n_cells, double dof, void* d_p, void* d_stat, int out_dtype, int64_t ldo, int64_t r0, int64_t c0,
							  int32_t* d_flags, int fix_nslices, const double* d_fixx, const double* d_fixy, double guard_tol, int p_kind, void* stream);

/*
 * alpha[i,j,c] = by[j,c] - gamma[i,j] * bx[i,c]  (association.py:238-243), fp64 coefficients in, out_dtype out.
 * The reference computes alpha from gamma whatever return_dot says (return_dot only rescales the returned
 * statistic afterwards, association.py:1044-1048), so d_stat may hold either form of K3's output:
 *   stat_kind 1: d_stat = gamma;  stat_kind 0: d_stat = covariance x~.y~/n, turned back into gamma with
 *   d_ssx (nx, sums of squares from nrm_residualize; 0 -> n_cells as in K3) and n_cells.
 */
int nrm_alpha(const void* d_stat, int stat_dtype, int64_t ldg, int stat_kind, const double* d_ssx, int64_t n_cells,
			  const double* d_bx, const double* d_by, int64_t nx, int64_t ny, int64_t nc, void* d_alpha, int out_dtype,
			  void* stream);

/*
 * K2s + sweep -- streaming path for de with few design rows (nx + nc <= 32): HBM-bound, every expression
 * value is read once, raw (fp32/fp64), never materialised as an fp64 residual (see csrc/nrm_gram_skinny.hip).
 *   nrm_gram_skinny:  G[y,:] = sum_k Y[y,k] Z[:,k] (rows_pad, 32) and ss[y] = sum_k Y[y,k]^2, with
 *       d_z (32, ldz) fp64 = [C (nc rows); X~ (nx rows, residualised by nrm_residualize); zero rows],
 *       zero padded to k_pad cells (multiple of 128); rows_pad multiple of 256.  d_a rows must be 16-byte aligned (lda % (16/itemsize) == 0).
 *   nrm_de_small_sweep: |y~|^2 = ss - (y C^T) dci (C y^T), y~.x~ = y.x~  ->  R^2, p, gamma|cov (association.py:226-235,249);
 *       d_ssy (ny) receives |y~|^2; d_by (ny, nc) or NULL receives the OLS coefficients ccy (for alpha).
 */
/*
 * The OLS products a = x C^T of the design rows of the streaming de path (first half of association.py:224-227 for dx): rows <= 32
 * design rows against nc <= 32 covariate rows, spread along the cells, partial sums added in a fixed order.
 *   d_ga (rows, 32): a[r][c] at d_ga[r * 32 + c]; the last covariate in column 31 when const_last != 0 (the layout
 *   nrm_residualize_wide reads).  d_work: nrm_design_products_workspace_doubles(rows, n_cells) doubles.
 */
int64_t nrm_design_products_workspace_doubles(int64_t rows, int64_t n_cells);
int nrm_design_products(const void* d_x, int x_dtype, int64_t rows, int64_t n_cells, int64_t ldx, const double* d_c, int64_t nc, int64_t ldc,
						double* d_ga, double* d_work, int const_last, void* stream);

/* Residualise <= 32 rows with the work spread along the cells (used for the design rows of the streaming path):
 * d_ga (rows, 32) holds x C^T in its first nc columns (from nrm_gram_skinny against Z = [C; 0]); out (rows, ldo) fp64,
 * zero padded up to ldo; d_ss (rows) sums of squares; d_coef (rows, nc) or NULL the OLS coefficients.  A row the covariates explain to twenty digits
 * (|x~|^2 < 1e-22 |x|^2) is explained exactly: its row of d_out is cleared, its sum of squares 0 (variance 0 -> 1, P = 1). */
int nrm_residualize_wide(const void* d_x, int x_dtype, int64_t rows, int64_t n, int64_t ldx, const double* d_c, int64_t nc,
						 int64_t ldc, const double* d_ga, const double* d_dci, int rank, double* d_out, int64_t ldo,
						 double* d_ss, double* d_coef, double* d_work /* 64 * ceil(ldo/1024) doubles */,
						 int const_last /* != 0: the LAST covariate is the constant row: its product sits in column 31 of d_ga */, void* stream);
int nrm_gram_skinny(const void* d_a, int a_dtype, int64_t rows, int64_t n, int64_t lda, const double* d_z, int64_t ldz,
					int64_t k_pad, double* d_g, double* d_ss, int64_t rows_pad, int64_t nz /* used rows of Z (<= 32); <= 16 selects the half-width variant */,
					double const_row_value /* != 0: G[:, 31] = value * sum_k Y[y,k], the product with a constant covariate row (the
					intercept) that the caller left out of Z: a vector-ALU sum instead of a 4-row matrix-core group; 0: none */,
					void* d_work, void* stream);
int64_t nrm_gram_skinny_workspace_bytes(void);  /* scratch for d_work (deterministic combination of partial pieces) */
int nrm_de_small_sweep(const double* d_g, const double* d_ssraw, const double* d_dci, int64_t nc, int rank, const double* d_ssx,
					   int64_t nx, int64_t ny, int64_t n_cells, double dof, int stat_kind, void* d_p, void* d_stat, void* d_r,
					   void* d_t, int out_dtype, int64_t ldo, double* d_ssy, double* d_by, int32_t* d_flags,
					   int const_last /* as above: covariate nc-1 in column 31, the design rows from column nc-1 on */, void* stream);
/* The same with p_kind (0 = p, 1 = ln p in d_p: nrm_assoc_sweep_pk above). */
int nrm_de_small_sweep_pk(const double* d_g, const double* d_ssraw, const double* d_dci, int64_t nc, int rank, const double* d_ssx,
						  int64_t nx, int64_t ny, int64_t n_cells, double dof, int stat_kind, void* d_p, void* d_stat, void* d_r,
						  void* d_t, int out_dtype, int64_t ldo, double* d_ssy, double* d_by, int32_t* d_flags, int const_last, int p_kind, void* stream);

/*
 * single=4 sweep (competition-aware DE, association.py:421-576 in closed form).
 * Inputs from one multiple regression of every gene on A = [dx; dc] (m = nx + nc rows):
 *   d_bt  (ny, ldb) fp64: Bt[y,k] = coefficient of row k of A for gene y      (B = (A A^T)^-1 A Y^T)
 *   d_pt  (ny, ldb) fp64: Pt[y,k] = A_k . y                                   (prody^T, association.py:952-967)
 *   d_yy  (ny) fp64: sum_k y^2 (association.py:968);  d_dxx (nx) fp64: 1/(n (AA^T)^-1_ii) = variance of x_i
 *   unexplained by all other rows (association.py:539-540).
 * Outputs (nx, ldo) of out_dtype: p, gamma (association.py:550) or gamma*varx when return_dot, vary (:548).
 * dof = n - 1 - (m - 1) - dimreduce is uniform for full-rank A A^T.  d_work: ny doubles of scratch.
 */
int nrm_single4_sweep(const double* d_bt, const double* d_pt, int64_t ldb, const double* d_yy, const double* d_dxx,
					  int64_t nx, int64_t ny, int64_t m, int64_t n_cells, double dof, int return_dot,
					  void* d_p, void* d_stat, void* d_vary, int out_dtype, int64_t ldo, double* d_work, int32_t* d_flags,
					  void* stream);
/* single=4 with the products Y~ X~^T from the integer Gram engine (normalisr_amd/single4.py: the regression is taken on rows
 * residualised against the covariates -- Frisch-Waugh -- so that K1's digit planes, K2's exact contraction and the row records of
 * nrm_residualize_q serve it as they serve single=0; replaces association.py:926-980,421-576 for full-rank designs).
 *   nrm_gram_i8_fix_dot: adds the engine's exact mean-product correction (csrc/nrm_fix.h) to a raw dot matrix in place, from the row
 *       records of its rows and of its columns -- what K3 does inside its sweeps, for callers that need the products themselves.
 *   nrm_single4_sweep_guarded: nrm_single4_sweep plus the accuracy guard: d_fix_y (ny, NRM_FIX_STRIDE) the genes' records, d_kappa (nx)
 *       = sum_j |x~_j| |N_ji| / sqrt(N_ii), cstar / gstar the largest c and g among the design rows' records; a pair whose P-value the
 *       products' error bound could move by more than `budget` (relative) is counted in d_flags[2], the largest estimate kept in
 *       d_flags[3] (float bits); d_flags has 4 entries.  The caller redoes the genes with hits (or the whole call) on the fp64 Gram kernel. */
int nrm_gram_i8_fix_dot(double* d_dot, int64_t ldd, const double* d_fix_rows, const double* d_fix_cols, int64_t rows, int64_t cols,
						int nslices, int64_t n_cells, void* stream);
int nrm_single4_sweep_guarded(const double* d_bt, const double* d_pt, int64_t ldb, const double* d_yy, const double* d_dxx,
							  int64_t nx, int64_t ny, int64_t m, int64_t n_cells, double dof, int return_dot, void* d_p,
							  void* d_stat, void* d_vary, int out_dtype, int64_t ldo, double* d_work, int32_t* d_flags,
							  const double* d_fix_y, const double* d_kappa, double cstar, double gstar, int nslices, double budget,
							  int32_t* d_gene_hits /* (ny) zeroed by the caller, or NULL: 1 for every gene with a counted pair */, void* stream);

/*
 * The small steps around single=4's on-device inverse of M~ = X~ X~^T (normalisr_amd/single4.py: Newton-Schulz iteration X <- X (2 I - M X), its
 * two products per step on nrm_gram_f64; replaces the per-grouping SVDs of association.py:527-528 for full-rank designs).  All matrices
 * (nxp, nxp) fp64 row-major, nxp a multiple of 128 >= nx; every reduction in a fixed order.
 *   nrm_spd_prepare: d_m (.., ldm) as a symmetric nrm_gram_f64 launch leaves it (entries i <= j valid) -> d_mp, the full symmetric matrix,
 *       its padding rows carrying mean(diag) on the diagonal; d_scal[0] = ||M||_1, d_scal[1] = mean(diag); d_work: 2 nxp doubles.
 *   nrm_spd_start: d_x = diag(1 / M_ii) (diagonal != 0) or I / ||M||_1.
 *   nrm_spd_transpose_residual: d_tt = d_t^T, d_res[0] = ||I - d_t||_F; d_work: (nxp / 32)^2 doubles.
 *   nrm_spd_update: d_x = 2 d_x - d_xt (both 16-byte aligned: anything else is refused).
 *   nrm_spd_finish: d_n = (d_x + d_x^T) / 2 inside nx x nx, 0 in the padding; d_small (3, nx) = diag(N), sum_j |N_ij| sqrt(d_ss[j]), sum_j |N_ij|.
 */
int nrm_spd_prepare(const double* d_m, int64_t ldm, int64_t nx, int64_t nxp, double* d_mp, double* d_scal, double* d_work, void* stream);
int nrm_spd_start(const double* d_mp, int64_t nxp, int diagonal, const double* d_scal, double* d_x, void* stream);
int nrm_spd_transpose_residual(const double* d_t, int64_t nxp, double* d_tt, double* d_res, double* d_work, void* stream);
int nrm_spd_update(double* d_x, const double* d_xt, int64_t count, void* stream);
int nrm_spd_finish(const double* d_x, int64_t nx, int64_t nxp, const double* d_ss, double* d_n, double* d_small, void* stream);
/* What the single=4 sweep needs of N~ (d_small (3, nx) of nrm_spd_finish) without the host: d_dxx[i] = 1 / (n_cells N~_ii) (association.py:539-540 in closed form),
 * d_varx the same with the reference's 0 -> 1 (:546-547); d_flags[5] (int32[8]) += design rows whose N~_ii is not a positive finite number. */
int nrm_single4_design_scalars(const double* d_small, int64_t nx, int64_t n_cells, double* d_dxx, double* d_varx, int32_t* d_flags, void* stream);

/*
 * single=1 sweep (every grouping tested on its own subset of cells, association.py:263-390).
 *   d_g  (ny, ldg): Gram of the expression rows with the masked rows W_i = [1_Si C (nc rows); 1_Si x_i], i = 0..nx-1,
 *        column i*(nc+1)+c;  d_g2 (ny, ldg2): Gram of the squared expression rows with the masks 1_Si.
 *   d_info (nx, info_pitch) fp64 per grouping: [ns_i, vx_i, the 24 doubles of struct nrm_pvalue_plan, ccx_i (nc), M_i^+ (nc*nc)]
 *        prepared on the host (inv_rank of C_S C_S^T stays on the host: integer rank).
 * Outputs (nx, ldo): p, gamma (or gamma*vx when return_dot), vary; d_alpha (nx, ny, nc) or NULL.
 */
int nrm_single1_sweep(const double* d_g, int64_t ldg, const double* d_g2, int64_t ldg2, const double* d_info, int64_t info_pitch,
					  int64_t nc, int64_t nx, int64_t ny, int return_dot, void* d_p, void* d_stat, void* d_vary, void* d_alpha,
					  int out_dtype, int64_t ldo, int32_t* d_flags, void* stream);

/*
 * The same single=1 statistics for designs with entries >= 0 (gRNA incidence), without the masked Gram contractions and without a
 * transposed copy of the expression matrix (association.py:263-390,911-925).  Every cell has a code (int32): a cell where every grouping
 * is 0 is NRM_S1_COMMON (-2); a cell where exactly one grouping is not 0 carries its position (>= 0) in the list of such cells ordered
 * by grouping (d_seg[i] .. d_seg[i+1] are the positions of grouping i); any other cell is NRM_S1_SKIP (-1).
 *   nrm_single1_stream reads d_y (ny, ldy) once, where it lies (y_dtype), with d_c (nc, ldc) fp64 covariates, and leaves
 *     d_common (nc + 1, ny) fp64: rows c < nc = the sums of y C_c over the common cells, row nc = the sum of y^2 over them;
 *     d_ye (cells with a position, ldye) in y_dtype: the expression values at those cells, transposed (ldye: a multiple of 8, >= ny;
 *     64-byte aligned; columns ny .. ldye are scratch).  nc <= 32 (more than 8 covariates: further passes over d_y).
 *   nrm_single1_cells finishes every (grouping, gene) pair from d_common, d_ye, d_ce (cells with a position, nc) fp64 covariates and
 *     d_xe (the same cells) fp64 own value of the grouping; d_info, outputs and flags as nrm_single1_sweep.
 */
#define NRM_S1_COMMON (-2)
#define NRM_S1_SKIP (-1)
int nrm_single1_stream(const void* d_y, int y_dtype, int64_t ldy, const double* d_c, int64_t ldc, int64_t nc, const int32_t* d_code,
					   int64_t n, int64_t ny, double* d_common, void* d_ye, int64_t ldye, void* stream);
int nrm_single1_cells(const void* d_ye, int y_dtype, int64_t ldye, const double* d_ce, const double* d_xe, const int64_t* d_seg,
					  const double* d_common, const double* d_info, int64_t info_pitch, int64_t nc, int64_t nx, int64_t ny, int return_dot,
					  void* d_p, void* d_stat, void* d_vary, void* d_alpha, int out_dtype, int64_t ldo, int32_t* d_flags, void* stream);
/* The groupings' own statistics over their own cells (association.py:350-364): d_seg (nx + 1) delimits grouping i's entries of d_cells (cell
 * indices, int64) / d_xe (its value there); d_out (nx, nc (nc + 1) / 2 + nc + 1): the sums of C_c C_d (c <= d, row by row), of C_c x, of x x.  nc <= 8. */
int nrm_single1_group_stats(const int64_t* d_seg, const int64_t* d_cells, const double* d_xe, const double* d_c, int64_t ldc, int64_t nc, int64_t nx,
							double* d_out, void* stream);
/* The grouping side of association_test_2's loop body (association.py:350-374) on the device, a lane per grouping: M_i = (the shared cells' covariate
 * Gram matrix, d_gram_part of nrm_single1_select added up in block order) + (the grouping's own, d_gs of nrm_single1_group_stats); its pseudo-inverse and
 * INTEGER rank by the rule of inv_rank (association.py:77-80; the Jacobi code the host's nrm_small_pinv runs); ccx_i, vx_i (0 -> 1), dof_i = ns_i - 1 -
 * rank_i - dimreduce and the P-value plan for it -- written as the records nrm_single1_cells reads (d_info (nx, info_pitch >= 26 + nc + nc nc)) -- and
 * d_varx (nx) fp64.  What the reference asserts or raises there is counted into d_flags (int32[8], zeroed by the caller; [0], [1] are the sweep's):
 * [2] groupings with a single value on their selected cells (:917-918), [3] groupings with dof <= 0, [4] groupings whose M_i is not finite.  nc <= 8. */
int nrm_single1_group_info(const double* d_gs, const double* d_gram_part, const double* d_rowinfo, const int64_t* d_sel_info, int64_t nc, int64_t nx,
						   int dimreduce, double* d_info, int64_t info_pitch, double* d_varx, int32_t* d_flags, void* stream);
/* The same two steps for 1 <= nc <= 32 covariates, a wave per grouping (association.py:350-374).
 *   nrm_single1_group_stats_wide: d_out in the packing of nrm_single1_group_stats, from d_ce (d_seg[nx], nc) -- the covariates at the groupings' own cells
 *     in segment order, as nrm_single1_select writes them; it takes the place of (d_cells, d_c, ldc): nothing is gathered -- and d_xe.  Every output is one
 *     fma chain over the segment's cells in their order, starting from 0 (len roundings): the same bits every run.  Empty segments give zeros.
 *   nrm_single1_group_info_wide: the arguments, records (d_info (nx, info_pitch >= 26 + nc + nc nc)), d_varx and counters d_flags[2], [3], [4] of
 *     nrm_single1_group_info.  M_i = (the shared cells' matrix: all nb (nb + 1) / 2 blocks of d_gram_part, nb = ceil(nc / 8), each added up over its
 *     partial sums in block order) + (the grouping's own, d_gs); pseudo-inverse and INTEGER rank by cyclic Jacobi with the lanes of the wave sharing a
 *     rotation, |eigenvalue| >= 1e-8 x the largest kept (association.py:77-80,350-351); ccx_i, vx_i (0 -> 1, :362-364), dof_i = ns_i - 1 - rank_i -
 *     dimreduce and its P-value plan (:372-374).  A non-finite M_i counts into d_flags[4] and continues on the identity.
 *   nrm_single1_group_info_wide_host: the same routine with one lane on HOST arrays (flags int32[8], counted into) -- no device, no HIP call. */
int nrm_single1_group_stats_wide(const int64_t* d_seg, const double* d_xe, const double* d_ce, int64_t nc, int64_t nx, double* d_out, void* stream);
int nrm_single1_group_info_wide(const double* d_gs, const double* d_gram_part, const double* d_rowinfo, const int64_t* d_sel_info, int64_t nc, int64_t nx,
								int dimreduce, double* d_info, int64_t info_pitch, double* d_varx, int32_t* d_flags, void* stream);
int nrm_single1_group_info_wide_host(const double* gs, const double* gram_part, const double* rowinfo, const int64_t* sel_info, int64_t nc, int64_t nx,
									 int dimreduce, double* info, int64_t pitch, double* varx, int32_t* flags);

/*
 * binnet -- binarise a (ng, ng) co-expression P-value matrix at a per-row Benjamini-Hochberg q-value cutoff
 * (reference binnet.py:134-173 with bh :77-131; the consumer of coex's p-matrix).  d_out (ng, ldo) bytes 0/1, diagonal 0;
 * *d_total receives the number of selected entries (0 -> the reference raises "Empty binary network");
 * d_flags[0] counts rows with entries outside [0,1] / non-finite (reference assertions :151-152).
 */
int nrm_binnet(const void* d_p, int p_dtype, int64_t ng, int64_t ldp, double qcut, unsigned char* d_out, int64_t ldo,
			   unsigned long long* d_total, int32_t* d_flags, void* stream);
/* The same for a block of gene rows [row0, row0 + rows) of the (ng, ng) matrix: d_p (rows, ldp) and d_out (rows, ldo) hold only
 * that block (row i of the block is gene row0 + i; its diagonal entry is column row0 + i).  Rows are independent in the reference
 * (binnet.py:159 maps bh over the rows), so a GPU that owns a row block of a sharded coex binarises it without the other blocks;
 * *d_total counts this block's selected entries (the caller sums the blocks before the "Empty binary network" test). */
int nrm_binnet_rows(const void* d_p, int p_dtype, int64_t rows, int64_t ng, int64_t ldp, int64_t row0, double qcut,
					unsigned char* d_out, int64_t ldo, unsigned long long* d_total, int32_t* d_flags, void* stream);
/* The two entries with the form of the matrix as an argument: p_kind = 0, P-values, is what the entries above pass; p_kind = 1: d_p holds ln P (what the
 * p_kind = 1 sweeps write, nrm_assoc_sweep_pk).  Valid entries are <= 0 and no NaN; -inf is the exact zero of the linear form (coex's diagonal) and both zeros are
 * ln 1; d_flags[0] counts the rows with other entries.  Row i's edges are { j != i : lnp_ij <= tau* }, tau* = max{ v : v + (ln m - ln c_v) <= ln qcut }, m = ng - 1,
 * c_v = #{off-diagonal entries <= v}, evaluated in fp64 for both dtypes.  d_out, d_total as above. */
int nrm_binnet_pk(const void* d_p, int p_dtype, int64_t ng, int64_t ldp, double qcut, unsigned char* d_out, int64_t ldo,
				  unsigned long long* d_total, int32_t* d_flags, int p_kind, void* stream);
int nrm_binnet_rows_pk(const void* d_p, int p_dtype, int64_t rows, int64_t ng, int64_t ldp, int64_t row0, double qcut,
					   unsigned char* d_out, int64_t ldo, unsigned long long* d_total, int32_t* d_flags, int p_kind, void* stream);

/*
 * bh -- Benjamini-Hochberg q-values over ALL entries of a P-value matrix that lies in HBM (reference binnet.py:77-131 with weight=None; csrc/nrm_bh.hip): what
 * a screen's de step delivers, computed where de left its P-values.  Contract: for N valid entries (finite, in [0, 1]) with u the sorted distinct values (-0.0
 * counts as 0.0) and c(u) the exact number of entries <= u:  w = fl(c / N), q(u) = fl(u / w), a non-finite q -> 1, clipped to [0, 1], q(u) <- min over u' >= u
 * of q(u'); the output is q of every entry, in the input's dtype, and equals the reference's BIT FOR BIT: fp64 divides in IEEE fp64, fp32 divides in fp64 and
 * rounds each quotient once to fp32 (the correctly rounded fp32 quotient while c and N are exact in fp32, N <= 2^24).  Departure: beyond 2^24 fp32 entries the
 * reference's fp32 cumsum of ones stalls at 2^24; the counts here stay exact.  Weighted bh is not provided (the reference's sequential sums have no parallel form).
 *   nrm_bh_workspace_bytes: bytes of d_work for n entries (two key buffers, the q array, the histogram tables, the look-up's sampled keys: about 3.1 n elements); a negative NRM_E_* code for n <= 0 (NRM_E_ARG:
 *       the reference asserts size > 0), n > 2^31 - 1 (NRM_E_UNSUPPORTED) or a bad dtype.
 *   nrm_bh_tile:   keys per workgroup of the sort and scan kernels (the tests size themselves by it).
 *   nrm_bh:        d_p (rows, cols) of p_dtype with pitch ldp, flattened row-major (a vector: rows = 1) -> d_q (rows, cols) with pitch ldq, same dtype; d_q may equal
 *       d_p when the pitches are equal.  d_work: 256-byte aligned.  d_flags int32[2], zeroed by the call itself on `stream`: [0] = entries that are NaN, infinite,
 *       < 0 or > 1 (the reference's assertion :104; d_q is then meaningless, no access leaves the buffers), [1] = 1 when there is more than one distinct value, else 0
 *       (the reference warns "Identical p-value in all entries.").  Does not synchronise and reads nothing back: the launch sequence depends on (n, dtype) only, so
 *       the call can be queued behind a plan's step and captured into a HIP graph.  No kernel waits for another workgroup.
 *   nrm_bh_layout: byte offsets into d_work of what a finished call leaves there: [0] the sorted keys (the entries' bit patterns: uint32 / uint64), [1] c per sorted
 *       position (uint32), [2] q per sorted position after the suffix minimum (p_dtype), [3] 0.  For the stage tests.
 *   nrm_bh_host:   the whole problem from host buffers (as nrm_binnet_host: no torch, the library's scratch pool, the device of nrm_set_device): h_p (n) -> h_q (n);
 *       *identical = 1 when every entry holds the same value; NRM_E_NUMERIC "P-values must be finite and within [0, 1]" for entries that are not.
 *   nrm_bh_pk, nrm_bh_host_pk: the same with the form of the entries as an argument; p_kind = 0 is what nrm_bh and nrm_bh_host pass.  p_kind = 1: the entries are
 *       ln P.  Valid: <= 0 and no NaN (-inf is the exact zero of the linear form; +0.0 and -0.0 are both ln 1); d_flags[0] counts the others.  With u over the
 *       distinct values and c(u) the exact number of entries <= u:  ln q(u) = min(0, u + (ln N - ln c(u))), then the minimum over u' >= u, in fp64 for both dtypes;
 *       an fp32 result is that value rounded once at the store.  -inf gives -inf, c = N leaves u itself, equal entries get equal bytes, the output is
 *       non-decreasing in the input.  Keys are the complemented bit patterns of |ln P|; workspace, layout ([2] then holds ln q) and launch sequence are those of the
 *       linear form: the sequence depends on (n, dtype, p_kind) only.
 * Threads: the device-pointer entries keep no state (any thread, the caller orders work by its streams and owns d_work for the duration); the host entry takes the
 * lock all whole-problem entries share -- one such call at a time per process.
 */
int64_t nrm_bh_workspace_bytes(int64_t n, int p_dtype);
int64_t nrm_bh_tile(void);
int nrm_bh(const void* d_p, int p_dtype, int64_t rows, int64_t cols, int64_t ldp, void* d_q, int64_t ldq, void* d_work, int64_t work_bytes,
		   int32_t* d_flags /* [2] */, void* stream);
int nrm_bh_layout(int64_t n, int p_dtype, int64_t offsets[4]);
int nrm_bh_host(const void* h_p, int p_dtype, int64_t n, void* h_q, int32_t* identical);
int nrm_bh_pk(const void* d_p, int p_dtype, int64_t rows, int64_t cols, int64_t ldp, void* d_q, int64_t ldq, void* d_work, int64_t work_bytes,
			  int32_t* d_flags /* [2] */, int p_kind, void* stream);
int nrm_bh_host_pk(const void* h_p, int p_dtype, int64_t n, void* h_q, int32_t* identical, int p_kind);

/*
 * normvar (reference norm.py:131-289): per-gene weighted covariate removal, e_gk = w_k^wt_g.
 *   nrm_normvar_weights: U = e^2, V = e^2 * y  (fp64, (rows_pad, ldo), zero padded) for the two Gram contractions
 *       M_g = U P^T (P = products C_c*C_c') and a_g = V C^T on nrm_gram_f64;  s1 = sum_k y e, s2 = sum_k (y e)^2.
 *       d_lnw (n) = ln w, d_wt (rows) = wt.
 *   nrm_normvar_apply:   out_gk = scale_g * e_gk * (y_gk - sum_c b_gc C_ck),  b_g = M_g^+ a_g from the host (integer rank), or the rows of the basis
 *       B as d_c with b_g from nrm_normvar_chol.  1 <= nc <= nrm_wide_covariates(): beyond 64 the coefficient table is in dynamic LDS.
 */
int nrm_normvar_weights(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_lnw, const double* d_wt,
						double* d_u, double* d_v, int64_t ldo, int64_t rows_pad, double* d_s1, double* d_s2, void* stream);
int nrm_normvar_apply(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_lnw, const double* d_wt,
					  const double* d_c, int64_t nc, int64_t ldc, const double* d_b, const double* d_scale, void* d_out, int out_dtype,
					  int64_t ldo, int32_t* d_flags /* int32[4] or NULL: [1] += waves that wrote a non-finite value (norm.py:286) */, void* stream);
/* d_out[i] = exp(d_x[i]) as the normvar kernels compute their per-gene cell weights w_k^wt_g = exp(wt_g ln w_k) (norm.py:245): a table of 2^(j/64) and a
 * polynomial of degree 5 instead of the library's exp (csrc/nrm_normvar.hip: nv_exp).  A probe for the tests. */
int nrm_normvar_exp_probe(const double* d_x, int64_t count, double* d_out, void* stream);
/* Round 5: b_g, scale_g and the integer rank of every gene WITHOUT leaving the device, for 1 .. nrm_normvar_device_covariates() covariates: one pass
 * over d_y sums the per-gene moments (M_g = sum_k e_gk^2 C_k C_k^T, a_g = sum_k e_gk^2 y_gk C_k, sum y e, sum (y e)^2) in registers -- no U, V, no Gram
 * launches --, a thread per gene takes M_g^+ by the rank rule of inv_rank (association.py:77-80; the Jacobi iteration of nrm_small_pinv: same integer
 * ranks) and the variance-keeping scale (norm.py:248-259; keepvar = 0: 1).  d_mom: rows (nc (nc + 1) / 2 + nc + 2) doubles of scratch; d_flags[0] +=
 * genes of rank 0 (norm.py:158-159 raises for them).  Then nrm_normvar_apply. */
int64_t nrm_normvar_device_covariates(void);
int nrm_normvar_solve(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_lnw, const double* d_wt, const double* d_c, int64_t nc,
					  int64_t ldc, double tol, int keepvar, double* d_mom, double* d_b, double* d_scale, int64_t* d_rank, int32_t* d_flags, void* stream);
/* The variance-keeping scale is (dv / dv2)^wt_g with dv^2 = s2 / n - mean^2 and dv2^2 = (s2 - a . b) / n: differences of one-pass sums.  Where either difference is
 * below 2^-20 of its minuend (a nearly flat weighted row, or one the covariates explain almost completely), keepvar != 0 and wt_g != 0, nrm_normvar_solve and the host
 * route of nrm_normvar_host leave -1.0 in d_scale[g] (no computed scale is negative), and this entry replaces it by the scale from the reference's two-pass form,
 * sum (y e - mean)^2 and sum (e (y - b . c))^2 over the row itself: a workgroup per gene that leaves at once when its gene is not marked.  Every other d_scale[g] keeps
 * its bits.  Call it between the solve and nrm_normvar_apply, on the same stream; 1 <= nc <= nrm_wide_covariates(). */
int nrm_normvar_rescale(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_lnw, const double* d_wt, const double* d_c, int64_t nc,
						int64_t ldc, const double* d_b, double* d_scale, void* stream);
/*
 * normvar with 64 .. nrm_wide_covariates() covariates (csrc/nrm_normvar_wide.hip), replacing the reference's per-gene pseudo-inverse and projection
 * (norm.py:154-163, called per gene from norm.py:232-259).  The host gives an orthonormal basis B (r, n) of the covariates' row space (normalisr_amd/norm.py:
 * _wide_basis); M_g = B diag(e_g^2) B^T is then positive definite and b_g solves M_g b_g = a_g, a_g = B (e_g^2 o y_g).
 *   nrm_wide_covariates: the largest covariate count of nrm_fitvar_* and nrm_normvar_apply, and the largest r here.
 *   nrm_normvar_pairs:   d_p (rows_pad, ldp) = rows [pair0, pair0 + count) of P, P_(i,j) = B_i o B_j for i <= j in the order of numpy's triu_indices(r);
 *       rows count .. rows_pad and cells n .. ldp are written as zeros.  A panel of the operand of  M = U P^T  (nrm_normvar_weights, nrm_gram_f64_whole).
 *   nrm_normvar_chol:    a workgroup per gene: blocked Cholesky factorisation of the packed upper triangle d_m[g] (ldm >= r (r + 1) / 2; row i holds columns
 *       i .. r - 1; overwritten by the factor), the two triangular solves for d_b[g] (r), and d_scale[g] = (dv / dv2)^wt_g with dv2^2 = (s2 - a . b) / n
 *       (norm.py:248-259; keepvar = 0: 1).  d_status (genes, or NULL): 0, 1 = a pivot that is not positive, 2 = a value that is not finite; such a gene gets
 *       zeros in d_b and d_scale, and d_flags[0] / d_flags[1] count them.
 *   nrm_gram_f64_whole:  nrm_gram_f64 (not symmetric) with every tile computed whole by one workgroup: an entry's bits do not depend on the launch's shape.
 */
int64_t nrm_wide_covariates(void);
int nrm_normvar_pairs(const double* d_b, int64_t r, int64_t n, int64_t ldb, int64_t pair0, int64_t count, double* d_p, int64_t rows_pad, int64_t ldp, void* stream);
int nrm_normvar_chol(double* d_m, int64_t ldm, const double* d_a, int64_t lda, int64_t genes, int64_t r, const double* d_s1, const double* d_s2, const double* d_wt,
					 int64_t n, int keepvar, double* d_b, double* d_scale, int32_t* d_status, int32_t* d_flags /* int32[4] */, void* stream);
int nrm_gram_f64_whole(const double* d_a, const double* d_b, int64_t m_pad, int64_t n_pad, int64_t k_pad, int64_t lda, int64_t ldb, double* d_dot, int64_t ldd,
					   int64_t m_rows, int64_t n_rows, void* stream);
/* normvar1 with explicit per-gene cell weights w2 (rows, ldw) (norm.py:150-153: row g is residualised against dc * w2[g]):
 * out_gk = y_gk - w2_gk * sum_c b_gc C_ck, with b_g = (sum_k w2_gk^2 C_k C_k^T)^+ (sum_k w2_gk y_gk C_k) from the host. */
int nrm_normvar_apply_w2(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_w2, int64_t ldw,
						 const double* d_c, int64_t nc, int64_t ldc, const double* d_b, void* d_out, int out_dtype, int64_t ldo, void* stream);

/*
 * Whole-problem host entry (numpy in / numpy out): the seam association_tests(dx, dy, dc, ...)
 * -> (p, dot|gamma, alpha|None, varx|None, vary) at association.py:761-771,1093 for single=0.
 * All pointers are HOST buffers owned by the caller.  h_dy == NULL means dy = dx (coex).
 *   h_dci (nc,nc) fp64 and rank from the host inv_rank;  dimreduce int (association.py:213).
 *   h_p, h_stat (nx,ny) of dtype out_dtype; h_varx (nx) / h_vary (ny) of out_dtype (h_varx may be
 *   NULL); h_alpha (nx,ny,nc) or NULL (lowmem); h_r / h_t optional extras or NULL.
 *   return_dot: 1 -> covariance, 0 -> gamma (association.py:769).
 * Runs on the current device (nrm_set_device) and synchronises before returning.
 */
/* Frees the device scratch nrm_association_tests_host keeps between calls (it is reused best-fit; calls are
 * serialised per process). */
int nrm_release_cache(void);
/* The pool's own accounting: *held = bytes of device memory the pool holds, *in_use = those of them taken by a running entry or a live plan (either may be NULL). */
int nrm_cache_bytes(int64_t* held, int64_t* in_use);
/* Verdict of the integer engine's accuracy guard for the last nrm_association_tests_host call of this thread: *hits = pairs it could
 * not certify on the integer pass (> 0: the call was redone on the fp64 Gram kernel before returning), *worst = largest relative
 * error estimate of a P-value among the pairs it looked at.  NRM_I8_GUARD_TOL sets the tolerance (default 2.5e-7; 0 = no guard). */
int nrm_last_guard(int64_t* hits, double* worst);
int nrm_association_tests_host(const void* h_dx, int x_dtype, int64_t nx,
							   const void* h_dy, int y_dtype, int64_t ny,
							   const void* h_dc, int c_dtype, int64_t nc, int64_t n_cells,
							   const double* h_dci, int rank, int dimreduce, int return_dot,
							   void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary,
							   void* h_r, void* h_t, int out_dtype);
/* The same with p_kind: 1 writes ln p into h_p (nrm_assoc_sweep_pk above) on every route the entry takes -- dense, streaming de, sparse design,
 * the fp64 rerun after a guard hit; 0 is nrm_association_tests_host.  When the integer pass is not certified for ln P, ln P comes from the fp64 pass and
 * the other results from the call with p_kind 0, its own rerun included (up to four passes).  A call certified for ln P but not for P keeps the integer
 * engine's other results, where p_kind 0 returns the fp64 kernel's (1e-13 apart): the one case in which they are not the same bytes. */
int nrm_association_tests_host_pk(const void* h_dx, int x_dtype, int64_t nx,
								  const void* h_dy, int y_dtype, int64_t ny,
								  const void* h_dc, int c_dtype, int64_t nc, int64_t n_cells,
								  const double* h_dci, int rank, int dimreduce, int return_dot,
								  void* h_p, void* h_stat, void* h_alpha, void* h_varx, void* h_vary,
								  void* h_r, void* h_t, int out_dtype, int p_kind);

/* (Round 5) nrm_association_tests_host streams the raw expression rows (nrm_gram_skinny, as the Python engine does) when dy is given and nx + nc <= 32 --
 * case-control DE, BASELINE configs[2]; NRM_DEBUG="de_path=general" keeps K1 + K2 -- and takes the sparse-design path below by itself when dy is given and the design matrix qualifies -- at most
 * 1/16 of its entries set, >= 32 design rows, >= 64 expression rows, >= 2048 cells, nx n >= 2^22, <= 32 covariates; NRM_DE_SPARSE=0 switches that
 * off, =force takes it whatever the size -- and hands calls whose rows are too close to the span of the covariates back to its dense fp64 path.
 *
 * The other two CLI methods of `normalisr de` at the same seam (association_tests(..., single=1 | 4), association.py:911-980), numpy buffers in
 * and out, no torch.  Outputs as the reference returns them: h_p, h_stat (gamma, or gamma * varx when return_dot), h_vary (nx, ny), h_varx (nx),
 * h_alpha (nx, ny, nc) or NULL -- all of out_dtype.  NRM_E_UNSUPPORTED (nrm_last_error says why) for calls outside what the entry covers:
 *   nrm_association_tests_single1_host (`-m single`, association.py:263-390,911-925): design entries >= 0 of which at most a quarter are set,
 *     at most 32 covariates (the gRNA incidence of a screen; the package's masked-Gram path takes the rest); the groupings' statistics stay on the device
 *     at every covariate count (nrm_single1_group_stats[_wide] + nrm_single1_group_info[_wide]), NRM_DEBUG="single1_stats=host" finishes them on the host
 *     from 9 covariates as before, and NRM_DEBUG="s1_trace=1" says on stderr which of the two a call with 9 .. 32 covariates took;
 *   nrm_association_tests_single4_host (`-m covariate`, association.py:421-576,926-980): the closed form for full-rank designs -- rank == nc
 *     (h_dci, rank from the host's inv_rank of C C^T) and A A^T certified full rank at `tol` (association.py:77) from norms at hand; a sparse design
 *     goes through the sparse-design kernels, any other through nrm_residualize + nrm_gram_f64;
 *   nrm_association_tests_single4_pinv_host: the same closed form for covariates of any rank 0 < rank <= nc (one-hot batches and an intercept:
 *     rank < nc), the rows residualised with h_dci = inv_rank's pseudo-inverse of C C^T and dof = n - nx - rank - dimreduce, when every grouping's
 *     matrix in the reference's loop certainly has the rank nx - 1 + rank at `tol` (single4.py: pinv_rank_certificate, from norms at hand).
 * nrm_binnet_host (binnet.py:134-173): h_p (ng, ng) -> h_net (ng, ng) bytes 0 / 1, *total = selected entries (0: the reference raises).
 */
int nrm_association_tests_single1_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc, int c_dtype,
									   int64_t nc, int64_t n_cells, int dimreduce, int return_dot, void* h_p, void* h_stat, void* h_alpha, void* h_varx,
									   void* h_vary, int out_dtype);
int nrm_association_tests_single4_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc, int c_dtype,
									   int64_t nc, int64_t n_cells, const double* h_dci, int rank, int dimreduce, int return_dot, double tol, void* h_p,
									   void* h_stat, void* h_alpha, void* h_varx, void* h_vary, int out_dtype);
int nrm_association_tests_single4_pinv_host(const void* h_dx, int x_dtype, int64_t nx, const void* h_dy, int y_dtype, int64_t ny, const void* h_dc, int c_dtype,
											int64_t nc, int64_t n_cells, const double* h_dci, int rank, int dimreduce, int return_dot, double tol, void* h_p,
											void* h_stat, void* h_alpha, void* h_varx, void* h_vary, int out_dtype);
int nrm_binnet_host(const void* h_p, int p_dtype, int64_t ng, double qcut, unsigned char* h_net, int64_t* total);
/* p_kind = 1: h_p holds ln P (nrm_binnet_pk); 0 is what nrm_binnet_host passes */
int nrm_binnet_host_pk(const void* h_p, int p_dtype, int64_t ng, double qcut, unsigned char* h_net, int64_t* total, int p_kind);
/* (Round 6) What the package needs to follow the reference's per-grouping algorithm of single=4 without torch where the closed form of
 * nrm_association_tests_single4_host does not apply (rank-deficient A A^T, mpc / method / qr, dy=None): the Gram matrices association.py:926-968 forms with
 * numpy.matmul, on the fp64 Gram kernel -- h_out (ra, rb) fp64 = A B^T over n cells (h_b == NULL: B = A), optionally the rows' sums of squares -- and the
 * P-value function of association.py:563 for host arrays.  The small pseudo-inverses of the algorithm stay in numpy (normalisr_amd/single4.py). */
int nrm_gram_host(const void* h_a, int a_dtype, int64_t ra, const void* h_b, int b_dtype, int64_t rb, int64_t n, double* h_out, double* h_ssa, double* h_ssb);
int nrm_pvalues_host(const double* h_r2, int64_t count, double dof, double* h_p);
/* (Round 5) normvar's expression side at the same kind of seam (norm.py:166-289; `normalisr normvar`): h_y (rows, n) fp32 / fp64, h_lnw (n) = ln w, h_wt (rows), h_c (nc, n)
 * fp64 -> h_out (rows, n) of out_dtype = gene g times w^wt_g, the covariates C w^wt_g removed, the variance kept (keepvar != 0, norm.py:248-259); tol: the rank rule of
 * inv_rank (association.py:77).  1 .. nrm_normvar_device_covariates() covariates entirely on the device; up to 32 through two launches of the fp64 Gram kernel and the host's
 * threaded Jacobi stack (round 6; NRM_E_UNSUPPORTED beyond 32).  *zero_rank = genes whose covariates have rank 0 (the
 * reference raises RuntimeError, norm.py:158-159; h_out is not written then); NRM_E_NUMERIC for non-finite results (norm.py:286).  The covariates' own scaling
 * (norm.py:261-273) is element-wise on (nc, n) and stays with the caller. */
int nrm_normvar_host(const void* h_y, int y_dtype, int64_t rows, int64_t n, const double* h_lnw, const double* h_wt, const double* h_c, int64_t nc, double tol,
					 int keepvar, void* h_out, int out_dtype, int64_t* zero_rank);
/* eigenvalues (ascending) of a small symmetric matrix, n <= 32 (host only) */
int nrm_small_eigvals(const double* m, int64_t n, double* w);

/*
 * de with a SPARSE design matrix (a CRISPR screen's gRNA incidence), association.py:224-235 without the dense contraction: a residual is
 * orthogonal to the covariates, so x~_i . y~ = x_i . y - (y C^T) . b_i and |y~|^2 = |y|^2 - (y C^T) . b_y -- the raw expression rows are
 * read ONCE, and of each only the values at the cells where a design row is not zero are added up.
 *   d_y (ny, ldy) raw expression rows (y_dtype); d_common (nc + 1, ny) fp64 their products with the covariates and (row nc) sums of
 *   squares, as nrm_single1_stream leaves them when every cell has the code NRM_S1_COMMON; d_dci (nc, nc) the pseudo-inverse of C C^T,
 *   nc <= nrm_de_sparse_max_covariates() (nc = 0: no covariates, or covariates of rank 0).
 *   The design matrix as lists: its rows are slots 0 .. 64 * ngroups - 1 (d_slot2x: slot -> design row, -1 for an empty slot); the cells
 *   are cut into chunks of nrm_de_sparse_chunk().  In every chunk the slots are dealt anew to the 64 * ngroups POSITIONS of the workgroup's
 *   lanes, d_sig[c * 64 * ngroups + p] = the slot position p gathers for in chunk c (a permutation inside every block of 1024 positions:
 *   one pass of the kernel; sorted by the slots' number of entries in the chunk, so that the 64 lists a wave walks in step are equally
 *   long).  For chunk c and the 64 positions of group g, d_w[c * ngroups + g] is the length of the longest list among them rounded up to a
 *   multiple of 8, and d_base[c * ngroups + g] the start of their block in d_ell: entry j of position 64 g + l at
 *   d_base[..] + (64 (j / 8) + l) 8 + j % 8 (8 consecutive entries of a position side by side: one 16-byte load) = the offset of the cell
 *   inside its chunk, or nrm_de_sparse_chunk() for padding; d_ellv: the entries' values likewise (fp64), or NULL
 *   when every entry is 1.  d_bx (design rows, ldb) the design rows' coefficients b_i from K1.
 * Out: d_dot[i * ldd + y] = x~_i . y~_y (by_gene != 0: d_dot[y * ldd + i], the layout single=4 reads); d_ssy (ny) = |y~|^2; d_coefy (ny, nc)
 *   = b_y or NULL; d_flags (int32[4], as nrm_assoc_sweep's) or NULL: [2] counts the expression rows whose residual is so small a part
 *   of the row (|y~|^2 < 1e-4 |y|^2) that these differences have lost four digits -- redo such a call on nrm_residualize + nrm_gram_f64.
 *   Then nrm_assoc_sweep as for K2's output.
 */
int64_t nrm_de_sparse_chunk(void);
int64_t nrm_de_sparse_max_covariates(void);
/*   d_ct != NULL (round 5): the rows' products with the covariates and their sums of squares are taken INSIDE the kernel, on the fp64 matrix
 *   cores, from the chunk of rows it holds in LDS anyway -- ONE pass over the expression matrix -- and left in d_common ((nc + 1, ny), then
 *   an output; nrm_single1_stream need not run).  d_c (nc, ldc) the covariates; const_idx: a covariate that is constant (the intercept, value
 *   const_val) or -1 -- it needs no operand; at most nrm_de_sparse_fused_covariates() others; d_ct: nrm_de_sparse_ct_doubles() doubles of scratch. */
int64_t nrm_de_sparse_fused_covariates(void);
int64_t nrm_de_sparse_ct_doubles(int64_t n, int64_t nc, int64_t const_idx);
int nrm_de_sparse(const void* d_y, int y_dtype, int64_t ny, int64_t n, int64_t ldy, double* d_common, int64_t nc, const double* d_dci,
				  const int16_t* d_ell, const double* d_ellv, const int64_t* d_base, const int32_t* d_w, const int32_t* d_sig, int64_t ngroups,
				  const int32_t* d_slot2x, const double* d_bx, int64_t ldb, double* d_dot, int64_t ldd, int by_gene, double* d_ssy, double* d_coefy,
				  int32_t* d_flags, const double* d_c, int64_t ldc, int64_t const_idx, double const_val, double* d_ct, void* stream);

/*
 * The design rows' own statistics from their entries (association.py:224-230 for a sparse design row): d_row_ptr (nx + 1), d_cells (int32),
 * d_vals (fp64, or NULL: every entry 1) list the entries of design row i at [d_row_ptr[i], d_row_ptr[i + 1]); d_c (nc, ldc), d_dci as above.
 * d_ss (nx) = |x~_i|^2 = |x_i|^2 - (x_i C^T) . b_i, d_coef (nx, nc) = b_i.  d_flags (int32[4]) or NULL: [2] counts the design rows whose
 * residual is so small a part of the row (|x~|^2 < 1e-4 |x|^2: a gRNA that all but coincides with a covariate) that this difference, and the
 * products nrm_de_sparse forms with the row, have lost four digits -- the same hand-back to nrm_residualize + nrm_gram_f64 as on the
 * expression side.
 */
int nrm_design_stats(const int64_t* d_row_ptr, const int32_t* d_cells, const double* d_vals, const double* d_c, int64_t ldc, int64_t nc,
					 const double* d_dci, int64_t nx, double* d_ss, double* d_coef, int32_t* d_flags, void* stream);

/*
 * The lists above built from the design matrix itself, by kernels of the library (csrc/nrm_design_lists.hip) -- the design side of
 * association.py:224-235 for a sparse design, and what association.py:914-918 selects cells from.  d_x (nx, ldx) the design matrix in HBM
 * (NRM_F32 / NRM_F64); nslots = nx rounded up to a multiple of 64; nch = ceil(n / nrm_de_sparse_chunk()) chunks of cells.
 *   nrm_design_count: ONE pass over d_x.  d_cnt (nch, nslots) int32: low 16 bits = entries (values != 0, NaN included) of design row `slot` in
 *     chunk c, above them bits NRM_DESIGN_* describing those entries; d_info (int64[8]) is zeroed by the call.
 *   nrm_design_plan: from the counts -- d_row_ptr (nx + 1) the CSR offsets, d_coff (nch, nslots) int32 the entries of a row before each chunk,
 *     d_slot2x (nslots) or NULL; with d_sig != NULL also the dealing d_sig / d_pos (nch, nslots: position -> slot and slot -> position, sorted
 *     by the entries of the chunk inside every block of 1024 slots, most first, ties in row order), the widths d_w (nch, nslots / 64) and
 *     offsets d_base of the ELL blocks as nrm_de_sparse reads them.  d_info[0] = entries in all, d_info[1] = entries of the ELL form, padding included,
 *     d_info[2] = the NRM_DESIGN_* bits of all entries.
 *   nrm_design_fill: the second pass over d_x writes the entries (cells ascending inside a row; no atomics: the same lists run to run) into
 *     d_cells / d_row_vals (CSR; d_cells may be NULL) and d_ell / d_ellv (ELL, padding included; d_ell may be NULL); binary != 0: every entry
 *     is 1 (d_info[2] has no NRM_DESIGN_NOTONE) and the value arrays are not written.
 * The caller reads d_info (one small copy) between plan and fill to size d_cells (d_info[0]) and d_ell (d_info[1]).
 */
#define NRM_DESIGN_NOTONE 1     /* an entry that is neither 0 nor 1 */
#define NRM_DESIGN_NEG 2        /* an entry < 0 */
#define NRM_DESIGN_GT1 4        /* an entry > 1 */
#define NRM_DESIGN_HAS1 8       /* an entry == 1 */
#define NRM_DESIGN_NAN 16       /* a NaN (an infinite entry sets NRM_DESIGN_GT1 or NRM_DESIGN_NEG) */
int nrm_design_count(const void* d_x, int x_dtype, int64_t nx, int64_t n, int64_t ldx, int32_t* d_cnt, int64_t nslots, int64_t* d_info, void* stream);
int nrm_design_plan(const int32_t* d_cnt, int64_t nx, int64_t n, int64_t nslots, int32_t* d_sig, int32_t* d_pos, int32_t* d_w, int64_t* d_base,
					int64_t* d_row_ptr, int32_t* d_coff, int32_t* d_slot2x, int64_t* d_info, void* stream);
int nrm_design_fill(const void* d_x, int x_dtype, int64_t nx, int64_t n, int64_t ldx, int64_t nslots, const int32_t* d_pos, const int32_t* d_w,
					const int64_t* d_base, const int64_t* d_row_ptr, const int32_t* d_coff, int16_t* d_ell, double* d_ellv, int32_t* d_cells,
					double* d_row_vals, int binary, void* stream);
/*
 * The same lists from a design that is SPARSE already (csrc/nrm_design_csr.hip): the design side of association.py:224-235, and what association.py:914-918
 * selects cells from, without the dense (groupings x cells) matrix anywhere.  The design is canonical CSR over its rows, in HBM: d_indptr (nx + 1) int64,
 * d_indices int32 (the cell of every stored entry, strictly increasing inside a row), d_data (NRM_F32 / NRM_F64 by data_dtype) or NULL: every stored entry is 1.
 * A stored zero is legal and is NOT an entry; a NaN is one (value != 0, as nrm_design_count counts).
 *   nrm_design_csr_count: d_cnt (nch, nslots) exactly as nrm_design_count writes it for the same design given dense; d_info (int64[8]) is zeroed by the call.
 *     It also checks the structure -- d_indptr[0] == 0, d_indptr[nx] == nnz, d_indptr does not decrease, every column lies in [0, n) and increases strictly
 *     inside a row -- and sets d_info[NRM_DESIGN_CSR_BAD] (a slot neither nrm_design_plan nor nrm_single1_select writes) to non-zero for a violation.  Nothing
 *     is addressed through an unchecked value: the row bounds are clamped to [0, nnz] and a column outside [0, n) is not used.  A malformed matrix is the
 *     caller's error to report (its counts mean nothing): do not go on to fill.
 *   nrm_design_plan as above, unchanged: it reads d_cnt only.
 *   nrm_design_csr_fill: the second pass, for a matrix nrm_design_csr_count accepted.  d_cells / d_row_vals (the library's CSR form: stored zeros dropped)
 *     and d_ell / d_ellv (padding included) as nrm_design_fill writes them, either of d_cells / d_ell may be NULL; no atomics: the same bits run to run.
 *     d_coff is taken for the likeness of the two argument lists and not read.  Every store is checked against the sizes the plan allotted.
 *   nrm_design_csr_dense: d_out (nx, ldo), NRM_F32 / NRM_F64 by out_dtype, is zeroed (padding too) and the stored entries are written into it -- for the
 *     routes that read the design as a matrix.  For a matrix nrm_design_csr_count accepted; columns outside [0, n) are skipped.
 * For every canonical CSR design every array these entries and nrm_design_plan produce is byte for byte what the dense entries produce from the densified matrix.
 */
#define NRM_DESIGN_CSR_BAD 5    /* index into d_info: non-zero for a malformed CSR design */
int nrm_design_csr_count(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int data_dtype, int64_t nx, int64_t n, int64_t nnz,
						 int32_t* d_cnt, int64_t nslots, int64_t* d_info, void* stream);
int nrm_design_csr_fill(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int data_dtype, int64_t nx, int64_t n, int64_t nslots,
						const int32_t* d_pos, const int32_t* d_w, const int64_t* d_base, const int64_t* d_row_ptr, const int32_t* d_coff, int16_t* d_ell,
						double* d_ellv, int32_t* d_cells, double* d_row_vals, int binary, void* stream);
int nrm_design_csr_dense(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int data_dtype, int64_t nx, int64_t n, void* d_out,
						 int out_dtype, int64_t ldo, void* stream);
/*
 * single=1's cell selection (association.py:914-918) for a design with entries >= 0, from its CSR form: cell k is selected for grouping i
 * when i's entry is the only one of the cell, and for every grouping when the cell has none.
 *   d_cnt (n) int32 scratch (entries per cell); d_code (n): the cell codes nrm_single1_stream reads; d_seg (nx + 1): grouping i owns the
 *   positions [d_seg[i], d_seg[i + 1]) of d_idx (cell, int64) / d_xe (its value there) / d_ce (position, nc: the covariates there) -- arrays
 *   with room for nnz positions; d_rowinfo (nx, 3): positions of grouping i, smallest and largest value among them (+-inf: none);
 *   d_gram_part (nb (nb + 1) / 2, nrm_single1_select_gram_blocks(), 64), nb = ceil(nc / 8): partial sums of the covariate Gram matrix over
 *   the cells without entries, by 8 x 8 blocks of covariates (block pairs bi <= bj row by row): the caller adds the partials of a pair in order.
 *   d_info (int64[8]): [3] = cells without entries, [4] = positions in all.
 */
int64_t nrm_single1_select_gram_blocks(void);
int nrm_single1_select(const int64_t* d_row_ptr, const int32_t* d_cells, const double* d_vals, int64_t nx, int64_t n, int64_t nnz, const double* d_c,
					   int64_t ldc, int64_t nc, int32_t* d_cnt, int32_t* d_code, int64_t* d_seg, int64_t* d_idx, double* d_xe, double* d_ce,
					   double* d_rowinfo, double* d_gram_part, int64_t* d_info, void* stream);
/* The last step of nrm_single1_select by itself (d_gram_part from d_cnt as the selection left it): a caller that passes d_gram_part = NULL to
 * nrm_single1_select runs it where it likes -- beside nrm_single1_stream, which needs the cell codes only, on another stream. */
int nrm_single1_common_gram(const int32_t* d_cnt, int64_t n, const double* d_c, int64_t ldc, int64_t nc, double* d_gram_part, void* stream);

/*
 * Pseudo-inverses and ranks of a stack of small symmetric matrices (host only): what single=1 needs per grouping (association.py:350-351)
 * and normvar per gene (norm.py:232-246), by the reference's rule (association.py:77-80: singular values below tol x the largest count as
 * zero) -- Jacobi iteration per matrix, the stack dealt to `threads` host threads (0 = choose).  m, inv (count, n, n) fp64; n <= 32.
 */
int nrm_small_pinv(const double* m, int64_t count, int64_t n, double tol, double* inv, int64_t* rank, int threads);

/*
 * The covariates' side of a single=0 call for a binder without LAPACK (host only): h_dci (nc, nc) fp64 = the pseudo-inverse of C C^T and *rank its integer rank,
 * what association.py:899-903 takes from inv_rank(np.matmul(dc, dc.T)) (:77-80: singular values below tol x the largest count as zero; the reference's tol is 1e-8).
 * C C^T is summed in fp64 cell by cell, in a fixed order; the eigenvalues come from the Jacobi iteration behind nrm_small_pinv.  All-zero covariates are rank 0 with
 * a zero h_dci (the reference crashes there).  h_dc (nc, n_cells) of c_dtype; nc == 0: rank 0, nothing written; nc > 32: NRM_E_UNSUPPORTED.
 */
int nrm_covariates_pinv(const void* h_dc, int c_dtype, int64_t nc, int64_t n_cells, double tol, double* h_dci, int* rank);

/*
 * Host -> device copy of a caller's (pageable) array through a ring of page-locked staging blocks the library owns: host threads fill
 * the next block while the previous block's DMA runs, so the copy runs at the DMA's rate without page-locking the caller's memory.
 * Returns once the last block has been handed to the DMA engine (completion is in stream order; h_src may be reused at once).
 * threads: host threads per block, 0 = choose.  nrm_upload_release frees the ring.
 */
int nrm_upload(const void* h_src, void* d_dst, int64_t bytes, int threads, void* stream);
int nrm_upload_release(void);

/*
 * Minimum, maximum and number of NaNs of a host array in one threaded pass (host only): what the reference's assertions on its results
 * (de.py:124-131, norm.py:286-289: finite, within range) need.  out[0] = minimum, out[1] = maximum (NaNs left out), out[2] = NaN count.
 */
int nrm_host_minmax(const void* p, int dtype, int64_t count, int threads, double* out);

/*
 * Text matrices of the command line (host only): the reference reads with numpy.loadtxt(delimiter='\t') and writes with
 * numpy.savetxt(fmt='%.8G') (run.py:20-35).  Same text in, same text out, parsed / printed by `threads` host threads (0 = choose).
 *   nrm_tsv_shape: rows = lines with data ('#' comments and blank lines skipped), cols = fields of the first such line.
 *   nrm_tsv_parse: the matrix into out (rows, ld), NRM_F32 or NRM_F64; a field that is not a number, or a row with another number of
 *     fields: NRM_E_ARG (ValueError, as numpy.loadtxt), the place in nrm_last_error().
 *   nrm_tsv_format: rows x cols as text; kind 0 = '%.8G' (NRM_F32 / NRM_F64), kind 1 = '%i' (NRM_TSV_I64 / _I32 / _U8).  Rows are dealt in
 *     order to `parts` threads; part t writes at out + t * part_cap, its length to lens[t];
 *     part_cap >= ceil(rows / parts) * max(cols, 1) * nrm_tsv_width(kind).
 */
#define NRM_TSV_I64 16
#define NRM_TSV_I32 17
#define NRM_TSV_U8 18
int nrm_tsv_shape(const char* buf, int64_t len, int delim, int threads, int64_t* rows, int64_t* cols);
int nrm_tsv_parse(const char* buf, int64_t len, int delim, int threads, void* out, int out_dtype, int64_t rows, int64_t cols, int64_t ld);
int64_t nrm_tsv_width(int kind);
int nrm_tsv_format(const void* data, int dtype, int64_t rows, int64_t cols, int64_t ld, int delim, int kind, char* out, int64_t part_cap,
				   int64_t* lens, int parts);

/*
 * lcpm and scaling_factor (reference lcpm.py:21-283): Bayesian logCPM from a read-count matrix, the first stage of the pipeline.  With the reference's default
 * arguments lcpm[g,k] = T[x_gk] - t1[k] with T[x] = psi(1 + x) - psi(sum(x) + 2) and t1[k] = ln sum_g exp(T[x_gk]) - ln 1e6 (lcpm.py:96-160): three streaming
 * passes over d_x (rows, ld) of integer counts -- dtype NRM_I64, NRM_I32, NRM_I16 or NRM_U8 -- and two tables of (largest count + 1) doubles.
 *   nrm_lcpm_count:   d_cell_total[k] += sum_g x_gk and d_cell_nnz[k] += #{g: x_gk != 0} (lcpm.py:194-200: the covariates), d_gene_zero[g] += #{k: x_gk == 0}
 *       (lcpm.py:258: scaling_factor's default variable), d_info[0] = sum(x) (lcpm.py:94), d_info[1] = max(x) (lcpm.py:100), d_info[2] = 1
 *       for a negative entry (lcpm.py:85-86 raises).  All int64; d_gene_zero zeroed by the caller (integer atomics, exact); the per-cell sums and d_info go
 *       through d_partial -- one slab per row tile, one record per workgroup -- and are folded in a fixed order (counts below 2^53).
 *   nrm_lcpm_digamma: HOST: h_psi[x] = psi(1 + x), x = 0 .. xmax, and *h_psi_t0 = psi(t0) (scipy.special.digamma in lcpm.py:96,101-107): -gamma + H_x by
 *       recurrence below 12, the asymptotic series (after an upward shift) from there.  xmax < nrm_lcpm_table_cap(), NRM_E_ARG beyond.
 *   nrm_lcpm_colsum:  d_t1[k] = ln sum_g d_exp_table[x_gk] - ln 1e6 (lcpm.py:158; d_exp_table = exp(T): exp once per table entry).  d_partial:
 *       ceil(rows / nrm_lcpm_row_tile()) x n doubles of scratch: one partial sum per row tile, added in a fixed order (no floating-point atomics).
 *   nrm_lcpm_write:   d_out[g,k] = d_table[x_gk] - d_t1[k] (lcpm.py:150,159; d_t1 == NULL: normalize=False), out_dtype NRM_F32 / NRM_F64: one rounding.
 * A count outside [0, table_len) reads the nearest end of the table.
 */
#define NRM_I64 16
#define NRM_I32 17
#define NRM_U8 18
#define NRM_I16 19
int64_t nrm_lcpm_row_tile(void);
int64_t nrm_lcpm_table_cap(void);
int64_t nrm_lcpm_count_workspace(int64_t rows, int64_t n);
int nrm_lcpm_count(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_gene_zero,
				   int64_t* d_info /* int64[4] */, int64_t* d_partial /* nrm_lcpm_count_workspace(rows, n) words of scratch */, void* stream);
int nrm_lcpm_digamma(int64_t xmax, double t0, double* h_psi, double* h_psi_t0);
int nrm_lcpm_colsum(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, const double* d_exp_table, int64_t table_len, double* d_partial,
					double* d_t1, void* stream);
int nrm_lcpm_write(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, const double* d_table, int64_t table_len, const double* d_t1, void* d_out,
				   int out_dtype, int64_t ldo, void* stream);

/*
 * The same three passes over a SPARSE count matrix (the reference accepts scipy.sparse input, lcpm.py:118-137, and densifies it; these never form the dense
 * counts): canonical CSR over genes -- d_indptr int64[rows + 1] from 0 to nnz, d_indices int32[nnz] (the cell; strictly increasing inside a row), d_data[nnz]
 * of dtype NRM_I64 / NRM_I32 / NRM_I16 / NRM_U8; stored zeros are legal and count as zeros.  Outputs and layouts as the dense entries'.
 *   nrm_lcpm_csr_count:  d_cell_total, d_cell_nnz, d_info[0..2] as nrm_lcpm_count (lcpm.py:94,100,85-86,194-200); d_gene_zero[g] = n - #{stored entries of g
 *       that are not 0} (lcpm.py:258; written, not added to).  d_info[3] = 1 for a malformed matrix: a column outside [0, n), a row whose columns do not
 *       strictly increase, d_indptr not 0 = p[0] <= ... <= p[rows] = nnz.  No entry reads or writes out of bounds for such a matrix (indptr is clamped, a
 *       column outside its chunk is skipped); its results mean nothing.  d_partial: nrm_lcpm_csr_workspace(rows, n) int64 words of scratch.
 *   nrm_lcpm_csr_colsum: d_t1[k] = ln(rows * E[0] + sum over the stored entries of cell k of (E[x] - E[0])) - ln 1e6 (lcpm.py:158), E = d_exp_table.  The
 *       terms are added as 64-bit fixed-point integers (exact, in any order: the same bits every run; no floating-point atomics), scaled per cell by the
 *       power of two that puts d_cell_total[k] * unit below 2^62; unit = max over x >= 1 of (E[x] - E[0]) / x.  d_cell_total from nrm_lcpm_csr_count;
 *       d_partial as there.
 *   nrm_lcpm_csr_write:  d_out[g,k] = d_table[x_gk] - d_t1[k] for every cell, d_table[0] - d_t1[k] where nothing is stored (lcpm.py:150,159); each element
 *       stored once.  d_t1 == NULL: normalize=False.  out_dtype NRM_F32 / NRM_F64: one rounding.
 */
int64_t nrm_lcpm_csr_workspace(int64_t rows, int64_t n);
int nrm_lcpm_csr_count(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
					   int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_gene_zero, int64_t* d_info /* int64[4] */, int64_t* d_partial, void* stream);
int nrm_lcpm_csr_colsum(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
						const double* d_exp_table, int64_t table_len, double unit, const int64_t* d_cell_total, int64_t* d_partial, double* d_t1, void* stream);
int nrm_lcpm_csr_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
					   const double* d_table, int64_t table_len, const double* d_t1, void* d_out, int out_dtype, int64_t ldo, void* stream);

/*
 * Quality control on read counts (reference qc.py:4-85) and the subsetting after it, on a count matrix that stays in HBM.  The matrix is not rewritten between
 * the iterations of qc_reads: two byte masks, d_gene_alive[rows] and d_cell_alive[n] (0 = removed), say what is left.  Integer arithmetic only: every result is
 * exact and the same on every run (integer atomics and fixed-order folds; no floating-point atomics).
 *   nrm_qc_stats:     dense d_x (rows, ld) of dtype NRM_I64 / NRM_I32 / NRM_I16 / NRM_U8.  d_gene_total[g] = sum and d_gene_nnz[g] = number of entries > 0 of an
 *       alive gene over the alive cells; d_cell_total[k], d_cell_nnz[k] likewise of an alive cell over the alive genes (qc.py:56-71 on the matrix as subset so
 *       far).  All int64; the value at a removed index is unspecified.  d_info int64[2]: [0] = 1 for a negative alive entry, [1] = 0.  A row tile without an
 *       alive gene and a chunk of 1024 cells without an alive cell are not loaded.  d_work: nrm_qc_stats_workspace words of scratch.
 *   nrm_qc_csr_stats: the same over canonical CSR (the format of nrm_lcpm_csr_count; stored zeros are legal and count as zeros).  Only the rows of alive genes
 *       are walked.  d_info[1] = 1 for a malformed matrix -- d_indptr not 0 = p[0] <= ... <= p[rows] = nnz, or, in a walked row, a column outside [0, n) or
 *       columns that do not strictly increase.  Such a matrix is never read or written out of bounds; its results mean nothing.
 *   nrm_qc_decide:    h_thresholds int64[6] on the HOST = (n_gene, nc_gene, nc_gene_prop, n_cell, nt_cell, nt_cell_prop), 0 = disabled.  An alive gene is
 *       removed when d_gene_total < n_gene or d_gene_nnz < nc_gene or d_gene_nnz < nc_gene_prop, an alive cell likewise; both read the statistics of ONE pass
 *       (qc.py:52-75).  d_out int64[2] = the genes and the cells still alive.
 *   nrm_subset_dense: d_out[i, j] = d_x[d_row_idx[i], d_col_idx[j]] for elements of elem = 1, 2, 4 or 8 bytes, ld and ldo in elements.  The lists are int64, in
 *       any order, with repeats; NULL keeps the axis as it is.  The caller checks the lists: an index outside the matrix reads its nearest edge.
 *   nrm_subset_csr_count, nrm_subset_csr_scan, nrm_subset_csr_write: a CSR matrix cut down to the alive genes and cells (both in their order), in three steps.
 *       count: d_row_count[g] = stored entries of row g at alive cells (0 for a removed row); d_info[1] as nrm_qc_csr_stats, over every row.  scan (one workgroup): d_row_count
 *       becomes, in place, the first output position of every row; d_out_indptr (room for rows + 1) the new indptr; d_cell_map[k] = alive cells before k, the
 *       new column of an alive cell; d_out int64[3] = (rows kept, cells kept, stored entries kept).  write: the kept entries in their order, columns through
 *       d_cell_map, values of elem bytes copied (stored zeros stay stored); out_nnz bounds every store.  The result is canonical CSR.
 */
int64_t nrm_qc_stats_workspace(int64_t rows, int64_t n);
int nrm_qc_stats(const void* d_x, int dtype, int64_t rows, int64_t n, int64_t ld, const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, int64_t* d_gene_total,
				 int64_t* d_gene_nnz, int64_t* d_cell_total, int64_t* d_cell_nnz, int64_t* d_info /* int64[2] */, int64_t* d_work, void* stream);
int nrm_qc_csr_stats(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int dtype, int64_t rows, int64_t n, int64_t nnz,
					 const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, int64_t* d_gene_total, int64_t* d_gene_nnz, int64_t* d_cell_total, int64_t* d_cell_nnz,
					 int64_t* d_info /* int64[2] */, int64_t* d_work, void* stream);
int nrm_qc_decide(const int64_t* d_gene_total, const int64_t* d_gene_nnz, const int64_t* d_cell_total, const int64_t* d_cell_nnz, int64_t rows, int64_t n,
				  const int64_t* h_thresholds /* int64[6], host */, uint8_t* d_gene_alive, uint8_t* d_cell_alive, int64_t* d_out /* int64[2] */, void* stream);
int nrm_subset_dense(const void* d_x, int elem, int64_t rows, int64_t n, int64_t ld, const int64_t* d_row_idx, int64_t rows_out, const int64_t* d_col_idx,
					 int64_t n_out, void* d_out, int64_t ldo, void* stream);
int nrm_subset_csr_count(const int64_t* d_indptr, const int32_t* d_indices, int64_t rows, int64_t n, int64_t nnz, const uint8_t* d_gene_alive,
						 const uint8_t* d_cell_alive, int64_t* d_row_count, int64_t* d_info /* int64[2] */, void* stream);
int nrm_subset_csr_scan(int64_t* d_row_count, int64_t rows, const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, int64_t n, int64_t* d_out_indptr,
						int32_t* d_cell_map, int64_t* d_out /* int64[3] */, void* stream);
int nrm_subset_csr_write(const int64_t* d_indptr, const int32_t* d_indices, const void* d_data, int elem, int64_t rows, int64_t n, int64_t nnz,
						 const uint8_t* d_gene_alive, const uint8_t* d_cell_alive, const int64_t* d_row_off, const int32_t* d_cell_map, int32_t* d_out_indices,
						 void* d_out_data, int64_t out_nnz, void* stream);

/*
 * The covariate of the top principal component of chosen genes (reference gocovt.py: the row degrees of gotop, :257-266; pccovt, :271-321, with pc1, :4-25).
 * The rows are gathered (nrm_subset_dense), residualised against [covariates; 1] by K1, twice (nrm_residualize: the fp64 residual rows Zres (m, ldz), zero padded, and
 * their sums of squares ss) and contracted by K2 (nrm_gram_f64, symmetric: G = Zres Zres^T, upper tiles only).  The entries below do the rest.  Every sum is
 * taken in a fixed order (no floating-point atomics): the same bits on every run.
 *   nrm_net_degree:     d_deg[g] (int64) = the number of non-zero bytes of row g of the (ng, ng) byte matrix d_net with pitch ld >= ng bytes -- net.sum(axis=1) of
 *       a binary network (gocovt.py:258), any non-zero byte counted once.  One read of the matrix: 16-byte loads from the first aligned address of a row on,
 *       single bytes before it and in the tail; any base address and pitch.  Exact.
 *   nrm_pc_correlation: a_g = 1 / (sqrt(ss_g / n) + 1e-200) (pc1's scaling, gocovt.py:21) into d_a (m), and the correlation matrix of the scaled rows
 *       d_r[g, h] = (G[lo, hi] * a_lo) * a_hi / n with lo = min(g, h), hi = max(g, h): both triangles from the upper one, symmetric to the bit.  A row of
 *       exact zeros has G = 0 and a = 1e200 and gives a zero row of d_r (the products are taken in that order), not NaN.
 *   nrm_pc_power:       `iters` steps of the power iteration on d_r (m, ldr): w = R v (a wave per row), lambda = v.w, residual = |w - lambda v|,
 *       v <- w / |w| (v stays when w == 0); d_v (m) is updated in place, d_w (m) is scratch, d_stat[0..2] = lambda, residual, |w| of the LAST step.
 *       Replaces the randomized TruncatedSVD of gocovt.py:22-23 (5 power iterations from a random sketch) by the exact component.
 *   nrm_pc_score:       the sign of svd_flip(u_based_decision=False): the entry of v of largest magnitude (the first of equals) is positive; then
 *       d_out[j] = sum_g (+-v_g a_g) Zres[g, j], the score Z^T v of gocovt.py:23, as NRM_F64 or NRM_F32 (rounded once).  d_z 16-byte aligned, ldz even and
 *       >= n rounded up to 2.  The genes are split over workgroups where the cells alone do not fill the device; the partial sums are added in the order of the
 *       splits.  d_work: nrm_pc_score_workspace(m, n) doubles.  d_sign (int64[2]) = the index of that entry and the sign applied (+-1).
 */
int nrm_net_degree(const uint8_t* d_net, int64_t ng, int64_t ld, int64_t* d_deg, void* stream);
int nrm_pc_correlation(const double* d_g, int64_t ldg, int64_t m, int64_t n, const double* d_ss, double* d_r, int64_t ldr, double* d_a, void* stream);
int nrm_pc_power(const double* d_r, int64_t ldr, int64_t m, double* d_v, double* d_w, double* d_stat /* double[3] */, int iters, void* stream);
int64_t nrm_pc_score_workspace(int64_t m, int64_t n);
int nrm_pc_score(const double* d_z, int64_t ldz, int64_t m, int64_t n, const double* d_v, const double* d_a, void* d_out, int out_dtype, double* d_work,
				 int64_t* d_sign /* int64[2] */, void* stream);

/*
 * compute_var (reference norm.py:56-128, `normalisr fitvar`): one iteration of the fit with cell weights u (n) -- all ones in the first, 1 / (fitted scale) of
 * the previous one after it (norm.py:98-99).  The reference's two regressions are used for their fitted values only, so the first is b_g = M^+ a_g with
 * M = sum_k u_k^2 C_k C_k^T (its pseudo-inverse d_mi (nc, nc) from the caller: inv_rank) and a_g = sum_k u_k^2 y_gk C_k.  1 <= nc <= nrm_wide_covariates() (1024):
 * up to 63 the workgroup's coefficient table is a static array, beyond it lies in dynamic LDS (4 x nc doubles) and d_mi is read as symmetric.
 *   nrm_fitvar_moments: d_a (rows, nc) = Y Cw^T with d_cw (nc, ldc) = u^2 C                                                       (norm.py:100)
 *   nrm_fitvar_genes:   d_b (rows, nc) = a M^+;  r_gk = u_k (y_gk - sum_c b_gc C_ck);  d_mean[g] = mean_k r_gk,  d_sc[g] = sqrt(mean_k (r_gk - mean)^2)
 *       (norm.py:101-107);  d_flags[0] += genes with d_sc == 0 or not finite (the reference divides by it, norm.py:108, and fails norm.py:125)
 *   nrm_fitvar_cells:   d_v[k] = mean_g ((r_gk - mean_g) / sc_g)^2 (norm.py:108, before its sqrt and log).  d_partial: ceil(rows / nrm_fitvar_row_tile()) x n
 *       doubles of scratch, one partial sum per row tile, added in a fixed order (no floating-point atomics).
 * The residual is recomputed in every pass and never stored.
 */
int64_t nrm_fitvar_row_tile(void);
int nrm_fitvar_moments(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_cw, int64_t nc, int64_t ldc, double* d_a, void* stream);
int nrm_fitvar_genes(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_u, const double* d_c, int64_t nc, int64_t ldc,
					 const double* d_a, const double* d_mi, double* d_b, double* d_mean, double* d_sc, int32_t* d_flags, void* stream);
int nrm_fitvar_cells(const void* d_y, int y_dtype, int64_t rows, int64_t n, int64_t ldy, const double* d_u, const double* d_c, int64_t nc, int64_t ldc,
					 const double* d_b, const double* d_mean, const double* d_sc, double* d_partial, double* d_v, void* stream);

/*
 * compute_var with nothing on the host (norm.ComputeVarPlan; csrc/nrm_fitvar_plan.hip): what the reference does between the passes above, on device pointers only,
 * so that all stepmax iterations are one enqueue.  A state record is four doubles {bestv, steps taken, the last t1, 0}; iteration i reads d_state and writes
 * d_state_next.  Once `bestv > eps` (the loop test of norm.py:98) fails, the entries below leave the scale, best, u, cw and M^+ as they are and copy the record.
 * d_ws: nrm_fitvar_plan_workspace doubles of scratch, the same block for every call of one plan.  Sums over cells are per-chunk partial sums added in a fixed order.
 *   nrm_fitvar_plan_start: d_s = 1 (norm.py:93), d_best = NaN (`best is None`), the first record {1e300, 0, NaN, 0} (norm.py:94-96)
 *   nrm_fitvar_design:     d_u = 1 / d_s, d_cw (nc, n) = C u^2, the chunks' upper triangles of sum_k (u_k C_k)(u_k C_k)^T                      (norm.py:99-100)
 *   nrm_fitvar_pinv:       d_mi (nc, nc) = the pseudo-inverse of that sum by the rule of inv_rank (association.py:77-80), *d_rank its rank; one workgroup,
 *       the cyclic Jacobi iteration of csrc/nrm_jacobi_lanes.h with both matrices in LDS                                                         (norm.py:100)
 *   nrm_fitvar_update:     after nrm_fitvar_cells: l = log sqrt v, new = exp(fit of l on [C;1]) s with d_m2i ((nc + 1)^2) the pseudo-inverse of [C;1][C;1]^T
 *       from the caller, new /= min(new), t1 = max |new - s| / s, s = new, best = new and bestv = t1 if t1 < bestv, steps + 1                  (norm.py:109-120)
 *   nrm_fitvar_weights:    d_w = 1 / d_best, d_w /= min(d_w); d_flags[1] += weights that are not finite and positive                            (norm.py:123-127)
 *   nrm_fitvar_pinv_host:  nrm_fitvar_pinv's routine on one host matrix m (n, n), n <= 64, one lane: the same sequence of rotations
 */
int64_t nrm_fitvar_plan_workspace(int64_t n, int64_t nc);
int nrm_fitvar_plan_start(int64_t n, double* d_s, double* d_best, double* d_state, void* stream);
int nrm_fitvar_design(const double* d_c, int64_t nc, int64_t ldc, int64_t n, const double* d_s, const double* d_state, double eps, double* d_u, double* d_cw, double* d_ws,
					  void* stream);
int nrm_fitvar_pinv(int64_t n, int64_t nc, double tol, const double* d_state, double eps, const double* d_ws, double* d_mi, int64_t* d_rank, void* stream);
int nrm_fitvar_update(const double* d_v, const double* d_c, int64_t nc, int64_t ldc, int64_t n, const double* d_m2i, double* d_s, double* d_best, const double* d_state,
					  double* d_state_next, double eps, double* d_ws, void* stream);
int nrm_fitvar_weights(const double* d_best, int64_t n, double* d_ws, double* d_w, int32_t* d_flags, void* stream);
int nrm_fitvar_pinv_host(const double* m, int64_t n, double tol, double* inv, int64_t* rank);

/*
 * The inverse of one symmetric positive definite matrix on the device (csrc/nrm_chol_inverse.hip), replacing the pseudo-inverse of the weighted covariates' Gram
 * matrix that compute_var takes per iteration (reference norm.py:100 through association.py:4-134) where an orthonormal basis of the covariates' row space makes
 * that matrix positive definite (below).  Blocked right-looking Cholesky M = L L^T in block columns of 64, W = L^-1 block row by block row, N = W^T W; tile
 * products on the fp64 matrix cores.  The launch sequence (4 ceil(r / 64) - 1 launches on the one stream) depends on r only, every element is one workgroup's sum
 * in a fixed order (no floating-point atomics: the same bits every run and every graph replay), no workgroup waits for another.  1 <= r <= nrm_wide_covariates().
 *   nrm_chol_inverse_workspace: doubles of d_ws for r; 0 outside 1 .. nrm_wide_covariates()
 *   nrm_chol_inverse:      d_m (r, ldm) symmetric, row-major, read in full, not modified -> d_inv (r, ldi), the full symmetric inverse (inv[i][j] and inv[j][i] the
 *       same bits).  The first failure of a call decides: a value of d_m or a pivot that is not finite, d_status[1] += 1; a pivot that is not positive,
 *       d_status[0] += 1; in either case d_inv is written as zeros (every launch runs to its end: no loop depends on the data).
 *   nrm_chol_inverse_host: the same blocked algorithm, block boundaries and status rules on host buffers, one thread (not the matrix cores' bits)
 * NRM_E_ARG for r, a pitch or a pointer, before any device call.
 */
int64_t nrm_chol_inverse_workspace(int64_t r);
int nrm_chol_inverse(const double* d_m, int64_t ldm, int64_t r, double* d_inv, int64_t ldi, double* d_ws, int32_t* d_status /* int32[2] */, void* stream);
int nrm_chol_inverse_host(const double* m, int64_t ldm, int64_t r, double* inv, int64_t ldi, int32_t* status /* int32[2] */);

/*
 * compute_var's iteration with 64 .. nrm_wide_covariates() covariates and nothing on the host (norm.ComputeVarPlan; csrc/nrm_fitvar_plan.hip), replacing
 * reference norm.py:99-100 and norm.py:109-110.  The caller gives orthonormal bases B (r, n) of the covariates' row space and B1 (r1, n) of span([C;1])
 * (normalisr_amd/norm.py: _fitvar_bases).  B diag(u) spans what C diag(u) spans, so the first regression is nrm_fitvar_moments / genes / cells with d_c = B,
 * nc = r and d_mi = the inverse of M = (B u)(B u)^T from nrm_gram_f64_whole and nrm_chol_inverse; the second is the projection B1^T (B1 l).  State records, the
 * stop rule and d_flags as for the entries above; d_ws: nrm_fitvar_wide_workspace doubles, the same block for every call of one plan.
 *   nrm_fitvar_wide_workspace: 0 for sizes the two entries do not take (n <= r, r > nrm_wide_covariates(), r1 > nrm_wide_covariates() + 1)
 *   nrm_fitvar_wide_design:  d_u = 1 / d_s, d_bu (rows_pad, ldbu) = B u with rows r .. rows_pad and cells n .. ldbu zero (rows_pad a multiple of 128, ldbu of 16:
 *       the operand of nrm_gram_f64_whole), d_cw (r, n) = (B u) u: each one rounded operation, in the order of nrm_fitvar_design.  kappa = (max u / min u)^2 from
 *       per-chunk extrema; d_flags[2] += 1 when !(hi >= safety tol kappa && (full || lo < tol / (safety kappa))): no certificate that the reference's rank rule
 *       (association.py:77-80) keeps exactly the r directions of B for these weights (hi, lo: eigenvalues r and r + 1 of C C^T over the largest; full: r == nc).
 *   nrm_fitvar_wide_update:  after nrm_fitvar_cells: l = log sqrt v, coef = B1 l (per-chunk partial sums added in order), new = exp(B1^T coef) s, then as
 *       nrm_fitvar_update (norm.py:109-120).  The coefficients stay at d_ws + 2 ceil(n / 256) + ceil(n / 1024) r1 (tests).
 */
int64_t nrm_fitvar_wide_workspace(int64_t n, int64_t r, int64_t r1);
int nrm_fitvar_wide_design(const double* d_b, int64_t r, int64_t ldb, int64_t n, const double* d_s, const double* d_state, double eps, double hi, double lo, double tol,
						   double safety, int full, double* d_u, double* d_bu, int64_t rows_pad, int64_t ldbu, double* d_cw, double* d_ws, int32_t* d_flags, void* stream);
int nrm_fitvar_wide_update(const double* d_v, const double* d_b1, int64_t r1, int64_t ldb1, int64_t n, double* d_s, double* d_best, const double* d_state,
						   double* d_state_next, double eps, double* d_ws, void* stream);

/*
 * The front half of the pipeline as WHOLE-PROBLEM entries (csrc/nrm_host_front.hip): HOST buffers in, HOST buffers out, no torch -- the kernels above, sequenced
 * as normalisr_amd/lcpm.py, norm.py and qc.py sequence them, uploads and scratch inside the library.  One call at a time per process, on the device of
 * nrm_set_device.  Every argument is checked before any device call; the messages are the reference's.  The host arithmetic is csrc/nrm_host_math.h.
 *
 *   nrm_lcpm_host (lcpm.lcpm with varscale = 0, lcpm.py:21-208; scaling_factor's default variable, lcpm.py:258): h_x (rows, n) dense counts of dtype NRM_I64 /
 *       NRM_I32 / NRM_I16 / NRM_U8.  nrm_lcpm_count, one read-back, nrm_lcpm_digamma and exp() of the table on the host, nrm_lcpm_colsum (normalize != 0),
 *       nrm_lcpm_write, copy out.  ntot < 0: None (t0 = sum + 2, lcpm.py:94-95), else t0 = ntot + 2.  h_out (rows, n) of out_dtype NRM_F32 / NRM_F64, or NULL:
 *       the integer pass alone.  h_cov (3, n) fp64 or NULL: ln total, genes without a read, ln^2 total of every cell (lcpm.py:194-200).  h_gene_zero int64[rows]
 *       or NULL: the zero entries of every gene -- one upload serves lcpm and scaling_factor.  h_info int64[2] = sum, maximum.
 *       NRM_E_ARG: a negative entry when h_out or h_cov is given (lcpm.py:85-86), an empty matrix, a cell without a read when h_cov is given (lcpm.py:196), ntot == 0.  NRM_E_NUMERIC: no read
 *       at all (the assertion of lcpm.py:95).  NRM_E_UNSUPPORTED: a count at or beyond nrm_lcpm_table_cap.
 *   nrm_lcpm_csr_host: the same over canonical CSR host arrays (the format of nrm_lcpm_csr_count) through nrm_lcpm_csr_count / colsum / write: the dense counts
 *       are never formed.  NRM_E_ARG for a malformed matrix.
 *   nrm_compute_var_host (norm.compute_var, norm.py:56-128): h_y (rows, n) fp32 / fp64 logCPM, h_c (nc, n) fp64, 1 <= nc <= 63 (NRM_E_UNSUPPORTED outside,
 *       before any device call) -> h_w fp64[n], the weights >= 1.  The pseudo-inverse of [C;1][C;1]^T on rows of unit length comes from the Jacobi routine of
 *       nrm_fitvar_pinv_host on the host; then the device-only sequence: nrm_fitvar_plan_start, per iteration design, pinv, moments, genes, cells, update -- all
 *       stepmax iterations enqueued, iterations past `best change <= eps` leave the state as it is --, nrm_fitvar_weights, and ONE read-back of the counters,
 *       the last state record and the weights.  h_state double[2] = the best change (the reference's bestv) and the steps taken.  NRM_E_NUMERIC: a gene with a
 *       constant residual (norm.py:108,125), weights that are not finite and positive (norm.py:125-127).  NRM_E_ARG: stepmax <= 0, eps <= 0, covariates with
 *       infs or NaNs.
 *   nrm_qc_reads_host, nrm_qc_reads_csr_host (qc.qc_reads, qc.py:4-85): the reference's loop (qc.py:49-81) -- nrm_qc_stats / nrm_qc_csr_stats, the thresholds
 *       of the CURRENT numbers of genes and cells (ceil of the double; the proportional bounds of the current numbers), nrm_qc_decide, one read-back -- until
 *       neither count changes.  h_gene_alive[rows], h_cell_alive[n]: byte masks, 1 = kept.  h_info int64[3] = iterations, genes left, cells left; the loop stops
 *       where no gene or no cell is left and the entry returns NRM_OK: the caller raises qc.py:78-81 (genes first).  NRM_E_ARG: negative parameters,
 *       proportions above 1, a negative entry, a malformed matrix.
 */
int nrm_lcpm_host(const void* h_x, int dtype, int64_t rows, int64_t n, int normalize, int64_t ntot, void* h_out, int out_dtype, double* h_cov /* (3, n) or NULL */,
				  int64_t* h_gene_zero /* rows or NULL */, int64_t* h_info /* int64[2] */);
int nrm_lcpm_csr_host(const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int dtype, int64_t rows, int64_t n, int64_t nnz, int normalize, int64_t ntot,
					  void* h_out, int out_dtype, double* h_cov, int64_t* h_gene_zero, int64_t* h_info /* int64[2] */);
int nrm_compute_var_host(const void* h_y, int y_dtype, int64_t rows, int64_t n, const double* h_c, int64_t nc, int64_t stepmax, double eps, double* h_w,
						 double* h_state /* double[2] */);
int nrm_qc_reads_host(const void* h_x, int dtype, int64_t rows, int64_t n, double n_gene, double nc_gene, double ncp_gene, double n_cell, double nt_cell, double ntp_cell,
					  uint8_t* h_gene_alive, uint8_t* h_cell_alive, int64_t* h_info /* int64[3] */);
int nrm_qc_reads_csr_host(const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int dtype, int64_t rows, int64_t n, int64_t nnz, double n_gene,
						  double nc_gene, double ncp_gene, double n_cell, double nt_cell, double ntp_cell, uint8_t* h_gene_alive, uint8_t* h_cell_alive,
						  int64_t* h_info /* int64[3] */);

/*
 * Gene-set enrichment (normalisr_amd/enrich.py; csrc/nrm_enrich.hip): what stands between the principal genes and pccovt in the reference's gocovt, as
 * arithmetic alone.  S study sets against T gene sets over G genes, N of them in the background.  Bit matrices hold W = ceil(G / 64) 64-bit words per row with
 * pitch W, gene g at bit g % 64 of word g / 64, bits at or beyond G zero; word buffers are 8-byte aligned.  Every entry checks its arguments (null pointers,
 * S, T or G <= 0, ld < G, more than 2^31 - 1 genes, misaligned buffers: NRM_E_ARG) before any device call.  Counts are exact and every floating-point value
 * is computed by one lane alone: the same bits on every run.
 *   nrm_enrich_pack:    d_study (S, G) bytes with pitch ld >= G (a binary network: what nrm_binnet writes; any non-zero byte counts once; nothing at or beyond
 *       G in a row is read) -> d_words (S, W), ANDed with d_bg (W) when that is not NULL, and d_n[s] = popcount of row s.
 *   nrm_enrich_overlap: d_k[s * T + t] = popcount(d_study[s] & d_sets[t]) over W words (int32; both operands tiled through LDS, no matrix cores) and
 *       d_K[t] = popcount(d_sets[t] & d_bg) (d_bg NULL: every gene).  At most 65535 x 64 studies per call.
 *   nrm_enrich_fisher:  one lane per pair: d_p[s * T + t] = the two-sided Fisher exact P-value of the table (k, n - k, K - k, N - K - n + k) in fp64 by the
 *       recurrence of csrc/nrm_fisher.h (anchored at the mode with weight 1, walked both ways; p = the sum of the weights <= w(k) (1 + 1e-7) over the sum of
 *       all, at most 1; no lgamma, nothing overflows; relative error <= 8 L u for a support of L values), and d_odds = (k / n) / (K / N), 0 with p = 1 when n
 *       or K is 0.
 *   nrm_enrich_top:     per study the set of smallest p among those with odds > 1 and k >= nmin (nmin < 1 means 1), the lower index of equals; d_top (S) records
 *       of 32 bytes {int64 index (-1: none qualifies), int64 k, int64 K, double p}.
 *   nrm_enrich_top_host: nrm_enrich_top's rule (the same predicates, csrc/nrm_fisher.h) on host arrays, no device.
 *   nrm_fisher_host:    nrm_enrich_fisher's P-value for `count` tables on the host, no device: the same code, the same bits.  NRM_E_ARG for a table with
 *       K or n outside [0, N], N outside [1, 2^31 - 1] or k outside [max(0, n + K - N), min(n, K)].
 *   nrm_enrich_host:    the whole problem from host buffers, no torch (as nrm_binnet_host; runs on the device of nrm_set_device): h_study (S, G) bytes with
 *       pitch ld, h_sets (T, W), h_bg (W) or NULL -> h_k (S, T), h_K (T), h_n (S), h_p and h_odds (S, T), h_top (S) records, *h_N = popcount(h_bg) (G without).
 */
int nrm_enrich_pack(const uint8_t* d_study, int64_t S, int64_t G, int64_t ld, const uint64_t* d_bg, uint64_t* d_words, int32_t* d_n, void* stream);
int nrm_enrich_overlap(const uint64_t* d_study, int64_t S, const uint64_t* d_sets, int64_t T, int64_t G, const uint64_t* d_bg, int32_t* d_k, int32_t* d_K, void* stream);
int nrm_enrich_fisher(const int32_t* d_k, const int32_t* d_n, const int32_t* d_K, int64_t S, int64_t T, int64_t N, double* d_p, double* d_odds, void* stream);
int nrm_enrich_top(const int32_t* d_k, const int32_t* d_K, const double* d_p, const double* d_odds, int64_t S, int64_t T, int64_t nmin, void* d_top, void* stream);
int nrm_enrich_top_host(const int32_t* k, const int32_t* K, const double* p, const double* odds, int64_t S, int64_t T, int64_t nmin, void* top);
int nrm_fisher_host(const int64_t* N, const int64_t* K, const int64_t* n, const int64_t* k, int64_t count, double* out_p);
int nrm_enrich_host(const uint8_t* h_study, int64_t S, int64_t G, int64_t ld, const uint64_t* h_sets, int64_t T, const uint64_t* h_bg, int64_t nmin, int32_t* h_k,
					int32_t* h_K, int32_t* h_n, double* h_p, double* h_odds, void* h_top, int64_t* h_N);

/*
 * One more covariate for a co-expression problem whose Gram matrix stays in HBM (normalisr_amd/levels.py; csrc/nrm_coex_levels.hip): reference association.py:224-235
 * applied to an enlarged dc, without residualising again.  With q a unit vector orthogonal to the covariates already removed, the Gram matrix of the residual rows
 * G = X (I - P) X^T changes to G - a a^T with a = X q taken on the RAW rows (q is orthogonal to the covariates), and the sums of squares to ss - a^2.
 *   nrm_coex_project:  d_a[k * lda + i] = sum_c X[i, c] Q[k, c] for 1 <= k <= 8 directions per launch.  d_x (nt, ns) NRM_F32 or NRM_F64 with pitch ldx >= ns
 *       elements, aligned to its element only (a row may start anywhere); d_q (k, ns) fp64 with pitch ldq; d_a (k, nt) fp64 with pitch lda.  Every element of X is
 *       read once for all k.  Products are rounded to fp64; every sum is a compensated one (two-sum pairs) folded in a fixed order -- a lane over its cells, the
 *       lanes of a wave, the waves of the workgroup that owns the row: |error| <= 8 u sum_c |x_c q_c|, the same bits on every run, no floating-point atomics.
 *   nrm_coex_downdate: in place, d_g[i * ld + j] -= sum_k a_ki a_kj, the terms taken for k = 0 .. k - 1 in that order, each product with its rounding error (one fma)
 *       and every sum a two-sum, the entry rounded once at the end: within 2 u (|G| + sum_k |a_ki a_kj|) for any k, where a chain of k rounded fmas carries k
 *       roundings; d_ss[i] likewise with a_ki^2.  Every step is symmetric in (i, j) to the bit.  VALID AFTERWARDS: the
 *       64 x 64 tiles with column tile >= row tile, restricted to i, j < nt -- every (i, j) with j / 64 >= i / 64, which holds dot[min(i, j), max(i, j)], what
 *       nrm_assoc_sweep(symmetric != 0) reads; inside the diagonal tiles both (i, j) and (j, i) are updated and stay equal bit for bit.  Tiles below the diagonal
 *       and columns >= nt are not touched.  d_counters (int32[2], integer atomics) are incremented: [0] for every row whose new d_ss is not finite or <= 0,
 *       [1] for every row whose new d_ss < 2^-10 d_ss_ref[i] (d_ss_ref: the sums of squares of the last from-scratch build).
 */
int nrm_coex_project(const void* d_x, int x_dtype, int64_t nt, int64_t ns, int64_t ldx, const double* d_q, int64_t k, int64_t ldq, double* d_a, int64_t lda, void* stream);
int nrm_coex_downdate(double* d_g, int64_t nt, int64_t ld, double* d_ss, const double* d_ss_ref, const double* d_a, int64_t k, int64_t lda, int32_t* d_counters,
					  void* stream);

/*
 * Resident coex plan (csrc/nrm_coex_plan.hip): coex(dt, dc) -- reference coex.py:4-48, that is association_tests(dt, None, dc) at association.py:761-1093 with its
 * tile loop :890-909,997-1057 -- for a caller that repeats it on a matrix of one shape.  The problem stays in HBM; a step is K1 -> K2 -> K3 -> variances
 * (association.py:224-235,248-249,230-233) on one stream; nothing is allocated, copied or decided on the host between steps.  numpy and this library suffice.
 *   nrm_coex_plan_create: dt (ng, n_cells) of dt_dtype.  dt_on_device == 0: a contiguous HOST array (ld == n_cells, or 0); the plan owns a device copy, uploaded
 *       through nrm_upload.  dt_on_device != 0: a DEVICE pointer with row pitch ld elements, adopted: never copied, never freed, and the caller may rewrite it in
 *       place between steps (in stream order with them); create synchronises the device, so whatever filled it is through.  h_dc (nc, n_cells) of c_dtype, h_dci (nc, nc) fp64 and rank as nrm_association_tests_host takes them;
 *       h_dci == NULL: the library computes both (nrm_covariates_pinv at tol 1e-8; rank is ignored; nc <= 32).  Every argument check of nrm_association_tests_host
 *       is made, in the reference's words (association.py:199-216), before any device call: NRM_E_ARG.  The K2 engine is chosen once, by that entry's rule: 6 digit
 *       planes from 2048 cells (NRM_GRAM=i8|i8x5|f64 overrides) when the matrix has 16-byte aligned rows (base % 16 == 0 and ld % 4 == 0), the fp64 kernel otherwise.
 *       NRM_I8_GUARD_TOL is read here.  Every buffer a step needs is taken from the scratch pool here and given back by nrm_coex_plan_destroy.  The plan
 *       remembers its device (nrm_set_device's at create) and binds the calling thread to it on every entry.
 *   nrm_coex_plan_upload: new values (same shape and dtype) into the plan's own copy; NRM_E_ARG for an adopted matrix.
 *   nrm_coex_plan_step: stream == NULL: a non-blocking stream the plan created (the legacy stream cannot be captured).  The first step runs eagerly, the second is
 *       recorded by thread-local stream capture and instantiated, later steps are one hipGraphLaunch.  Does not synchronise.  If the capture fails it is ended and
 *       discarded, the plan stays eager and nrm_last_error says why (the step itself still runs: NRM_OK).  NRM_DEBUG="graph=0" keeps every step eager.
 *   nrm_coex_plan_check: synchronises the device (steps may have gone to any streams), reads and clears the step counters.  NRM_E_NUMERIC for the reference's assertions (association.py:248,252).  If the integer
 *       engine's guard could not certify a pair since the last check, the step is redone now, eagerly, on the fp64 Gram kernel from the matrix as it stands (fp64
 *       rows allocated for that one pass) and *guard_hits is the count (else 0); *guard_worst the largest relative error estimate of a P-value.  After NRM_OK what
 *       the plan holds is certified, as after nrm_association_tests_host.  Either pointer may be NULL.
 *   nrm_coex_plan_results: check, then P-values and covariances (ng, ng) and variances (ng) of out_dtype into the caller's HOST arrays (any may be NULL); large
 *       arrays are page-locked for the copy.
 *   nrm_coex_plan_device_results: the same three as DEVICE pointers (row pitch *ld elements), valid until destroy, written by every step: a consumer such as
 *       nrm_binnet queued on the step's stream (nrm_coex_plan_stream: the plan's own) reads them without anything leaving HBM.
 *   nrm_coex_plan_info: info[0] engine (0 fp64, 5 or 6 digit planes), [1] captured (0/1), [2] steps run, [3] fp64 reruns, [4] rank, [5] dof, [6] bytes resident, [7] 0.
 *   nrm_coex_plan_time: `steps` steps between two events on the plan's stream, *ms_per_step their mean (the eager first step and the capture run before, untimed).
 *   nrm_coex_plan_destroy: accepts NULL.
 * Threads: create, check, results and destroy take the lock of the whole-problem entries (they use the scratch pool); step, upload and time do not.  A plan is
 * used by one thread at a time; two plans in one process are fine.  nrm_release_cache leaves a live plan's buffers alone (they are taken, not idle).
 */
typedef struct nrm_coex_plan nrm_coex_plan;
int nrm_coex_plan_create(nrm_coex_plan** plan, const void* dt, int dt_dtype, int64_t ng, int64_t n_cells, int64_t ld, int dt_on_device, const void* h_dc, int c_dtype,
						 int64_t nc, const double* h_dci, int rank, int dimreduce, int out_dtype);
int nrm_coex_plan_upload(nrm_coex_plan* plan, const void* h_dt);
int nrm_coex_plan_step(nrm_coex_plan* plan, void* stream);
int nrm_coex_plan_check(nrm_coex_plan* plan, int64_t* guard_hits, double* guard_worst);
int nrm_coex_plan_results(nrm_coex_plan* plan, void* h_p, void* h_dot, void* h_var);
int nrm_coex_plan_device_results(nrm_coex_plan* plan, void** d_p, void** d_dot, void** d_var, int64_t* ld);
int nrm_coex_plan_stream(nrm_coex_plan* plan, void** stream);
int nrm_coex_plan_info(nrm_coex_plan* plan, int64_t info[8]);
int nrm_coex_plan_time(nrm_coex_plan* plan, int64_t steps, double* ms_per_step);
int nrm_coex_plan_destroy(nrm_coex_plan* plan);

/*
 * Resident de plan (csrc/nrm_de_plan.hip): de(dg, dt, dc) with single=0 -- reference de.py:4-132 over association.py:224-249 -- on the sparse-design kernels, for a
 * caller that repeats a screen of one shape.  The plan is the sparse-design route by declaration: no size or density threshold (what NRM_DE_SPARSE=force takes).
 * The design, the expression matrix, the covariates and every result stay in HBM; a step is launches on one stream, from the second step on one hipGraphLaunch.
 *   nrm_de_plan_create: the design (ng0, n_cells) by design_form.  0: a dense matrix dg of dg_dtype (NRM_F32 / NRM_F64) with row pitch ldg elements (0: n_cells), on
 *       the host (contiguous) or, dg_on_device != 0, in HBM.  1: canonical CSR as nrm_design_csr_count takes it -- indptr (ng0 + 1) int64, indices int32, dg the nnz
 *       values of dg_dtype or NULL for all ones -- host arrays (uploaded) or, dg_on_device != 0, device arrays; its structure is checked by nrm_design_csr_count and a
 *       malformed matrix is NRM_E_ARG.  Either way the design is read here only (and by nrm_de_plan_design): the plan keeps lists, not the matrix.
 *       de's row filter (de.py:93) runs on the device: a row is tested when it holds more than one distinct value among its n_cells cells (NaNs count as equal; a
 *       stored zero of a CSR matrix is not an entry; with n_cells < 2 no row varies).  The rows kept are compacted on the device (nrm_subset_dense; nrm_subset_csr_count
 *       / scan / write) and the lists are built from them by nrm_design_count / nrm_design_csr_count, nrm_design_plan and nrm_design_fill / nrm_design_csr_fill: the
 *       bytes de builds for the same input.  A row that is dropped reaches neither nrm_design_stats nor the guard.  No row left to test: NRM_E_ARG.
 *       dt (nt, n_cells) of dt_dtype: a contiguous HOST array (the plan owns a device copy; nrm_de_plan_upload re-fills it) or, dt_on_device != 0, a DEVICE pointer with
 *       row pitch ldt, adopted: never copied, rewritten in place by its owner between steps.  h_dc, c_dtype, nc, h_dci, rank as nrm_coex_plan_create takes them
 *       (h_dci == NULL: nrm_covariates_pinv, nc <= 32); more than nrm_de_sparse_max_covariates() covariates: NRM_E_UNSUPPORTED.  want_alpha: lowmem=False;
 *       want_q: Benjamini-Hochberg q-values of all ng0 * nt P-values by nrm_bh inside every step.  Every argument check, those of association.py:199-216 in the
 *       reference's words included, is made before any device call.  Every buffer of a step is taken from the scratch pool here, sized for ng0 rows.
 *   nrm_de_plan_design: another design of the same shape (any form) in place of the present one; drops the captured graph and a remembered hand-back.
 *   nrm_de_plan_upload: new values (same shape and dtype) into the plan's own copy of dt; NRM_E_ARG for an adopted matrix.
 *   nrm_de_plan_step: nrm_design_stats -> the products (nrm_de_sparse, behind nrm_single1_stream beyond nrm_de_sparse_fused_covariates()) -> nrm_assoc_sweep (gamma)
 *       -> nrm_alpha on request: the launches of the whole-problem entry; then the re-inflation of de.py:107-122 (rows not tested: p = 1, gamma = alpha = varg = 0),
 *       the variances ss / n with the 0 -> 1 rule, the count of entries outside the ranges de.py:124-131 asserts, and nrm_bh on request.  Nothing is read back,
 *       allocated or waited for.  stream == NULL: the plan's own.  The first step on a route runs eagerly, the second is captured (thread-local) and instantiated,
 *       later ones are one hipGraphLaunch; a failed capture leaves the plan eager with the reason in nrm_last_error (NRM_OK).  NRM_DEBUG="graph=0": always eager.
 *   nrm_de_plan_check: synchronises the device, reads and clears the counters.  NRM_E_NUMERIC for the reference's assertions (association.py:248,252; de.py:124-131).
 *       *handed_back: expression or design rows that have all but vanished against the covariates' span since the last check (else 0): the step was then redone, now,
 *       on K1 and the fp64 Gram kernel (nrm_residualize, nrm_gram_f64_band) on the compacted design written out dense from its lists, and that is the plan's route for later steps
 *       until the design is replaced.  The dense route's buffers are taken from the pool at this moment.
 *   nrm_de_plan_results: check, then de's outputs of the last step into HOST arrays of out_dtype, any of them NULL: P (ng0, nt), gamma (ng0, nt), alpha (ng0, nt, nc),
 *       varg (ng0), vart (ng0, nt: the genes' variances on every tested row, zero on the others, written out here from the vector and the mask), q (ng0, nt).
 *   nrm_de_plan_device_results: P, gamma, alpha, varg, q as full-size DEVICE arrays (row pitch *ld = nt), the vart vector (nt), the byte mask of tested rows (ng0);
 *       NULL for what the plan was created without.  Valid until destroy, written by every step.
 *   nrm_de_plan_info: info[0] route (0 sparse-design kernels, 1 K1 + fp64 Gram), [1] captured, [2] steps, [3] reruns, [4] rank, [5] dof, [6] bytes resident, [7] rows kept.
 *   nrm_de_plan_time: as nrm_coex_plan_time.  nrm_de_plan_destroy: accepts NULL.
 * Threads: create, design, check, results and destroy take the lock of the whole-problem entries; step, upload and time do not.  One thread at a time per plan.
 */
typedef struct nrm_de_plan nrm_de_plan;
int nrm_de_plan_create(nrm_de_plan** plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
					   int dg_on_device, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n_cells, int64_t ldt, int dt_on_device, const void* h_dc,
					   int c_dtype, int64_t nc, const double* h_dci, int rank, int dimreduce, int out_dtype, int want_alpha, int want_q);
int nrm_de_plan_design(nrm_de_plan* plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
					   int dg_on_device);
int nrm_de_plan_upload(nrm_de_plan* plan, const void* h_dt);
int nrm_de_plan_step(nrm_de_plan* plan, void* stream);
int nrm_de_plan_check(nrm_de_plan* plan, int64_t* handed_back);
int nrm_de_plan_results(nrm_de_plan* plan, void* h_p, void* h_gamma, void* h_alpha, void* h_varg, void* h_vart, void* h_q);
int nrm_de_plan_device_results(nrm_de_plan* plan, void** d_p, void** d_gamma, void** d_alpha, void** d_varg, void** d_q, void** d_vart, void** d_mask, int64_t* ld);
int nrm_de_plan_stream(nrm_de_plan* plan, void** stream);
int nrm_de_plan_info(nrm_de_plan* plan, int64_t info[8]);
int nrm_de_plan_time(nrm_de_plan* plan, int64_t steps, double* ms_per_step);
int nrm_de_plan_destroy(nrm_de_plan* plan);

/*
 * Resident single=1 plan (csrc/nrm_single1_plan.hip): de(dg, dt, dc, single=1), a low-MOI screen in which every grouping is tested on the cells that carry no other
 * grouping -- reference de.py:4-132 over association.py:263-390, 911-925 -- for a caller that repeats a screen of one shape.  Names, argument order and semantics are
 * those of nrm_de_plan_* wherever the two coincide; there is no h_dci / rank, because single=1 takes a pseudo-inverse per grouping, on the device.  The domain is that
 * of nrm_association_tests_single1_host: entries >= 0 with the largest equal to 1, at most a quarter of them set, at most 32 covariates.
 *   nrm_single1_plan_create: the design (ng0, n_cells) by design_form, dt, ldt, dt_on_device, h_dc, c_dtype, nc, out_dtype, want_alpha (lowmem=False) and want_q exactly as
 *       nrm_de_plan_create takes them; dimreduce a scalar >= 0.  Every argument check -- dtypes, sizes ("Incorrect dx/dy/dc size.", "Unmatching dx/dy/dc dimensions."),
 *       dimreduce, rows and cells <= 2^31 - 1, row pitches: NRM_E_ARG; nc > 32: NRM_E_UNSUPPORTED -- is made before any device call.  The design is then set on the
 *       device, in this order: de's row filter (de.py:93) and the row map; the rows kept compacted (nrm_subset_dense; nrm_subset_csr_count / scan / write); their entry
 *       lists as nrm_association_tests_single1_host builds them (no ELL form; filled while at most a quarter of the entries is set); nrm_single1_select once, whose count
 *       of cells that carry exactly one grouping is the only size read back; the stream kernel's transposed output, sized from that count.  A row de drops never reaches
 *       the selection (an all-ones row left in would leave no cell with exactly one grouping).  Refused, in the words of the host entry: the largest entry of the rows
 *       kept is not 1, or a NaN: NRM_E_NUMERIC (association.py:914); negative entries or more than a quarter of the entries set: NRM_E_UNSUPPORTED; a malformed CSR
 *       matrix or no row left to test: NRM_E_ARG.  Every buffer of a step is taken from the scratch pool here.
 *   nrm_single1_plan_design: another design of the same shape (any form) in place of the present one; drops the captured graph.  After a refusal the plan has no design.
 *   nrm_single1_plan_upload: new values (same shape and dtype) into the plan's own copy of dt; NRM_E_ARG for an adopted matrix.
 *   nrm_single1_plan_step: nrm_single1_select; then, on a side stream the plan owns (forked and joined by events, so that a capture records both branches),
 *       nrm_single1_common_gram and nrm_single1_group_stats + nrm_single1_group_info (nc <= 8) or their _wide forms (9 .. 32), beside nrm_single1_stream on the step's
 *       stream; after the join nrm_single1_cells (gamma, alpha on request); then one pass that puts the compact P, gamma, alpha and vary rows back among all ng0 rows
 *       (rows not tested: p = 1, gamma = alpha = varg = vart = 0; when every row is tested the sweep writes the full-size arrays itself), rounds varx once to out_dtype
 *       and counts the entries outside the ranges de.py:124-131 asserts; nrm_bh over all ng0 * nt P-values on request.  Nothing is read back, allocated or waited for.
 *       stream == NULL: the plan's own.  The first step on a design runs eagerly, the second is captured (thread-local) and instantiated, later ones are one
 *       hipGraphLaunch; a failed capture leaves the plan eager with the reason in nrm_last_error (NRM_OK).  NRM_DEBUG="graph=0": always eager.
 *   nrm_single1_plan_check: synchronises the device, reads and clears the counters, and answers in the reference's order: groupings with a single value on the cells
 *       selected for them (association.py:917-918): NRM_E_NUMERIC; "array must not contain infs or NaNs": NRM_E_ARG; "Insufficient number of cells ...": NRM_E_DEVICE;
 *       the result assertions (association.py:248,252) and de's (de.py:124-131): NRM_E_NUMERIC.  single=1 has no hand-back route.
 *   nrm_single1_plan_results: check, then de's outputs of the last step into HOST arrays of out_dtype, any of them NULL: P (ng0, nt), gamma (ng0, nt), alpha (ng0, nt, nc),
 *       varg (ng0), vart (ng0, nt: per grouping here), q (ng0, nt).
 *   nrm_single1_plan_device_results: the same arrays as full-size DEVICE pointers (row pitch *ld = nt; vart (ng0, nt)) and the byte mask of tested rows (ng0); NULL for
 *       what the plan was created without.  Valid until destroy, written by every step.
 *   nrm_single1_plan_info: info[0] 0, [1] captured, [2] steps, [3] cells kept by the selection, [4] covariates, [5] 0, [6] bytes resident, [7] rows kept.
 *   nrm_single1_plan_stream, nrm_single1_plan_time, nrm_single1_plan_destroy (accepts NULL): as nrm_de_plan_*.
 * Threads: create, design, check, results and destroy take the lock of the whole-problem entries; step, upload and time do not.  One thread at a time per plan.
 */
typedef struct nrm_single1_plan nrm_single1_plan;
int nrm_single1_plan_create(nrm_single1_plan** plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
							int dg_on_device, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n_cells, int64_t ldt, int dt_on_device, const void* h_dc,
							int c_dtype, int64_t nc, int dimreduce, int out_dtype, int want_alpha, int want_q);
int nrm_single1_plan_design(nrm_single1_plan* plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
							int dg_on_device);
int nrm_single1_plan_upload(nrm_single1_plan* plan, const void* h_dt);
int nrm_single1_plan_step(nrm_single1_plan* plan, void* stream);
int nrm_single1_plan_check(nrm_single1_plan* plan);
int nrm_single1_plan_results(nrm_single1_plan* plan, void* h_p, void* h_gamma, void* h_alpha, void* h_varg, void* h_vart, void* h_q);
int nrm_single1_plan_device_results(nrm_single1_plan* plan, void** d_p, void** d_gamma, void** d_alpha, void** d_varg, void** d_q, void** d_vart, void** d_mask,
									int64_t* ld);
int nrm_single1_plan_stream(nrm_single1_plan* plan, void** stream);
int nrm_single1_plan_info(nrm_single1_plan* plan, int64_t info[8]);
int nrm_single1_plan_time(nrm_single1_plan* plan, int64_t steps, double* ms_per_step);
int nrm_single1_plan_destroy(nrm_single1_plan* plan);

/*
 * Resident single=4 plan (csrc/nrm_single4_plan.hip): de(dg, dt, dc, single=4), a high-MOI screen in which every grouping is tested with all the others as
 * covariates -- reference de.py:4-132 over association.py:421-576, 926-980, in closed form -- for a caller that repeats a screen of one shape.  Names, argument
 * order and semantics are those of nrm_de_plan_* wherever the two coincide.  Nothing of the design side depends on the expression matrix, and the plan reads its
 * design only when it is set: M~ = X~ X~^T, its inverse N~, dxx, varx and the rank decision are taken ONCE PER DESIGN, and a step keeps what depends on dt.  The
 * domain is that of nrm_association_tests_single4_host / _pinv_host: designs for which the closed form has a certificate; scalar dimreduce; no mpc / method / qr.
 *   nrm_single4_plan_create: the design (ng0, n_cells) by design_form, dt, ldt, dt_on_device, h_dc, c_dtype, nc, h_dci, rank (h_dci == NULL: nrm_covariates_pinv at
 *       `tol`, nc <= 32), dimreduce, out_dtype, want_alpha (lowmem=False) and want_q exactly as nrm_de_plan_create takes them; tol, 0 < tol < 1: the threshold of the
 *       rank certificates (association.py:77; the reference's default is 1e-8).  Every argument check -- dtypes, sizes ("Incorrect dx/dy/dc size.", "Unmatching
 *       dx/dy/dc dimensions."), dimreduce, tol, rows and cells <= 2^31 - 1, row pitches, rank: NRM_E_ARG; more than nrm_de_sparse_max_covariates() covariates, or
 *       covariates of rank 0: NRM_E_UNSUPPORTED -- is made before any device call.  The design is then set on the device, in this order: de's row filter (de.py:93),
 *       the row map, the rows kept compacted and their lists with the ELL form (as nrm_de_plan_create); the rows kept written out dense once from the lists
 *       (nrm_design_csr_dense; returned to the pool afterwards); the design side, eagerly and with its read-backs: nrm_design_stats; M~ by nrm_de_sparse with the
 *       dense design rows in the place of the expression rows; N~ by Newton-Schulz iteration on nrm_gram_f64 (nrm_spd_*; the host's Cholesky factorisation when it
 *       does not converge); dxx = 1 / (n N~_ii), varx, ||M~||_1, ||N~||_1; the certificate (full-rank covariates: A A^T passes the reference's rank test;
 *       rank-deficient ones: every grouping has the rank nx - 1 + rank).  A design row all but inside the covariates' span sends the design side, and the plan, to K1
 *       + nrm_gram_f64 (route 1) at once.  Refused: n_cells <= rows kept + rank + dimreduce: "Insufficient number of cells ...", NRM_E_DEVICE; no certificate, or
 *       M~ not positive definite: NRM_E_UNSUPPORTED in the words of the host entry (the caller takes norm.de(..., single=4), which looks at the spectrum of A A^T and
 *       follows the per-grouping algorithm if need be); a malformed CSR matrix or no row left to test: NRM_E_ARG.
 *   nrm_single4_plan_design: another design of the same shape (any form) in place of the present one: all of the above again; drops the captured graph and a
 *       remembered hand-back.  After a refusal the plan has no design.
 *   nrm_single4_plan_upload: new values (same shape and dtype) into the plan's own copy of dt; NRM_E_ARG for an adopted matrix.
 *   nrm_single4_plan_step: G = Y~ X~^T, |y~|^2 and b_y on request (route 0: nrm_de_sparse, behind nrm_single1_stream beyond nrm_de_sparse_fused_covariates(); route
 *       1: nrm_residualize + nrm_gram_f64) -> B^T = G N~ (nrm_gram_f64) -> nrm_single4_sweep (gamma): the launches of the whole-problem entry; then alpha on request
 *       -- alpha_y = b_y - B_y b_x as an (nt, nc) fp64 matrix summed in a fixed order, then written to all ng0 rows (zeros for rows not tested) --, one pass that
 *       puts the compact P, gamma and vart rows back among all ng0 rows (rows not tested: p = 1, gamma = varg = vart = 0; when every row is tested the sweep writes
 *       the full-size arrays itself), rounds varx once to out_dtype and counts the entries outside the ranges de.py:124-131 asserts; nrm_bh over all ng0 * nt
 *       P-values on request.  Nothing is read back, allocated or waited for.  stream == NULL: the plan's own.  The first step on a route runs eagerly, the second
 *       is captured (thread-local) and instantiated, later ones are one hipGraphLaunch; a failed capture leaves the plan eager with the reason in nrm_last_error
 *       (NRM_OK).  NRM_DEBUG="graph=0": always eager.
 *   nrm_single4_plan_check: synchronises the device, reads and clears the counters.  *handed_back: expression rows with |y~|^2 < 1e-4 |y|^2 since the last check
 *       (else 0): the design side and the step were then redone, now, on route 1 -- whose residual rows are taken from the pool at this moment, each matrix in one
 *       piece; a refusal of the pool is reported as such --, and that is the plan's route until the design is replaced.  Then NRM_E_NUMERIC for the reference's
 *       assertions on what stands (association.py:557; de.py:124-131).
 *   nrm_single4_plan_results: check, then de's outputs of the last step into HOST arrays of out_dtype, any of them NULL: P (ng0, nt), gamma (ng0, nt), alpha (ng0, nt,
 *       nc), varg (ng0), vart (ng0, nt: per grouping), q (ng0, nt).
 *   nrm_single4_plan_device_results: the same arrays as full-size DEVICE pointers (row pitch *ld = nt) and the byte mask of tested rows (ng0); NULL for what the plan
 *       was created without.  Valid until destroy, written by every step.
 *   nrm_single4_plan_info: info[0] route (0 sparse-design kernels, 1 K1 + fp64 Gram), [1] captured, [2] steps, [3] reruns, [4] covariate rank, [5] dof = n_cells -
 *       rows kept - rank - dimreduce, [6] bytes resident, [7] rows kept.
 *   nrm_single4_plan_stream, nrm_single4_plan_time, nrm_single4_plan_destroy (accepts NULL): as nrm_de_plan_*.
 * Threads: create, design, check, results and destroy take the lock of the whole-problem entries; step, upload and time do not.  One thread at a time per plan.
 */
typedef struct nrm_single4_plan nrm_single4_plan;
int nrm_single4_plan_create(nrm_single4_plan** plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
							int dg_on_device, int64_t ng0, const void* dt, int dt_dtype, int64_t nt, int64_t n_cells, int64_t ldt, int dt_on_device, const void* h_dc,
							int c_dtype, int64_t nc, const double* h_dci, int rank, int dimreduce, int out_dtype, int want_alpha, int want_q, double tol);
int nrm_single4_plan_design(nrm_single4_plan* plan, int design_form, const void* dg, int dg_dtype, int64_t ldg, const int64_t* indptr, const int32_t* indices, int64_t nnz,
							int dg_on_device);
int nrm_single4_plan_upload(nrm_single4_plan* plan, const void* h_dt);
int nrm_single4_plan_step(nrm_single4_plan* plan, void* stream);
int nrm_single4_plan_check(nrm_single4_plan* plan, int64_t* handed_back);
int nrm_single4_plan_results(nrm_single4_plan* plan, void* h_p, void* h_gamma, void* h_alpha, void* h_varg, void* h_vart, void* h_q);
int nrm_single4_plan_device_results(nrm_single4_plan* plan, void** d_p, void** d_gamma, void** d_alpha, void** d_varg, void** d_q, void** d_vart, void** d_mask,
									int64_t* ld);
int nrm_single4_plan_stream(nrm_single4_plan* plan, void** stream);
int nrm_single4_plan_info(nrm_single4_plan* plan, int64_t info[8]);
int nrm_single4_plan_time(nrm_single4_plan* plan, int64_t steps, double* ms_per_step);
int nrm_single4_plan_destroy(nrm_single4_plan* plan);

/*
 * Resident front-half plan (csrc/nrm_front_plan.hip): read counts in HBM in, normvar's (dtn, dcn) in HBM out -- the reference's chain lcpm (lcpm.py:21-208) ->
 * normcov (norm.py:4-53) -> compute_var (norm.py:56-128) -> scaling_factor (lcpm.py:211-283) -> normvar (norm.py:166-289) with its default options: normalize=True,
 * varscale=0, cat=1, keepvar=True, normmean=False, c=True, the scaling variable nt0mean with v0=0 and v1='max'.  Nothing is decided, allocated or read back on
 * the host between the launches of a step: the totals, t0, the digamma and exp tables, lcpm's three covariate rows, normcov, the pseudo-inverse of compute_var's
 * second regression, ln w and the rescale are kernels on device memory, so a step is one enqueue on ONE stream (no parallel branches) and one hipGraphLaunch from
 * the second step on, and the graph stays valid when the counts are rewritten.  A coex / de plan of the same process adopts the output matrix.
 *   nrm_front_plan_create: reads (genes, n_cells) of dtype NRM_I64 / NRM_I32 / NRM_I16 / NRM_U8.  reads_on_device == 0: a contiguous HOST array (ld == n_cells, or 0);
 *       the plan owns a device copy that nrm_front_plan_upload rewrites.  reads_on_device != 0: a DEVICE pointer with row pitch ld, adopted: never copied, rewritten
 *       in place by its owner between steps (in stream order with them); create synchronises the device.  h_cov (n_cov, n_cells) fp64, n_cov >= 0: the raw user
 *       covariate rows a caller would stack in front of lcpm's three before normcov.  ntot (-1: the matrix total, lcpm.py:94-96), stepmax and eps (compute_var),
 *       tol (normvar's rank rule, norm.py:152-160), out_dtype NRM_F64 (the reference's) or NRM_F32 for lcpm and dtn, count_cap: the tables hold psi(1 + x) for
 *       x < count_cap, 2 <= count_cap <= nrm_lcpm_table_cap().  Every argument check is made before any device call (csrc/nrm_front_plan_args.h): NRM_E_ARG, in the
 *       reference's words where it has any ("reads must not be empty.", "eps and stepmax must be positive.", a user row that is not finite, a constant user row:
 *       "Detected constant covariate. ..." norm.py:34-37); n_cov + 3 + 1 > nrm_normvar_device_covariates(): NRM_E_UNSUPPORTED, the text names the bound.
 *       Every buffer of a step is taken from the scratch pool here and given back by nrm_front_plan_destroy.
 *   nrm_front_plan_create_csr: the same plan on SPARSE counts, canonical CSR over the genes as nrm_lcpm_csr_count takes it -- indptr (genes + 1) int64, indices
 *       int32 strictly increasing inside a row, data of one of the four count dtypes, stored zeros legal -- in arrays that hold nnz_cap >= max(nnz, 1) elements; no
 *       (genes, n_cells) matrix of counts is ever formed.  on_device == 0: HOST arrays of nnz stored entries; the plan owns three device buffers of capacity nnz_cap
 *       that nrm_front_plan_upload_csr rewrites.  on_device != 0: DEVICE arrays, adopted and rewritten in place by their owner, the pattern included; nnz is then
 *       only checked against nnz_cap, and every step reads the number of stored entries from indptr[genes].  The other arguments are nrm_front_plan_create's.  Checked
 *       before any device call as well: 0 <= nnz <= nnz_cap, nnz_cap >= 1, the arrays' alignment, and for host arrays 0 = indptr[0] <= ... <= indptr[genes] = nnz
 *       (NRM_E_ARG in the words of nrm_lcpm_csr_host's malformed matrix).  What needs every entry -- columns inside [0, n_cells) and strictly increasing -- is the
 *       count kernel's, at every step, and is reported by check.  No step reads outside the genes + 1 offsets and the nnz_cap entries, whatever the arrays hold.
 *   nrm_front_plan_upload: new counts (same shape and dtype) into the plan's own copy; NRM_E_ARG for an adopted matrix or a plan on CSR counts.
 *   nrm_front_plan_upload_csr: new CSR counts (same shape and dtype, any pattern, nnz <= nnz_cap, the offsets checked as in create_csr) into the plan's own arrays;
 *       NRM_E_ARG, before any copy, for an adopted matrix, for nnz > nnz_cap, and for a plan on a dense matrix.  The graph of the step stays as it is.
 *   nrm_front_plan_step: nrm_lcpm_count; t0 = sum + 2, len = max + 1 and lcpm's refusals counted (one workgroup); tab[x] = psi(1 + x) - psi(t0) and exp(tab[x]) for
 *       x < len, each entry on its own (csrc/nrm_digamma.h); nrm_lcpm_colsum and nrm_lcpm_write with table_len = count_cap (lcpm.py:107,158); lcpm's rows ln total,
 *       genes - nnz, ln^2 total (lcpm.py:194-200) and normcov on [user rows; those three] with the ones row appended, a workgroup per row, two-pass mean and spread
 *       in a fixed order; ([dc;1][dc;1]^T)^+ on unit-length rows by the lane Jacobi; the launches of nrm_compute_var_host; ln w and wt = (zeros / cells) / max
 *       (lcpm.py:258,268-283); dcn = the continuous rows and the ones row times w (norm.py:261-273); nrm_normvar_solve / rescale / apply.  stream == NULL: the
 *       plan's own.  Eager the first time, captured (thread-local) the second, one hipGraphLaunch afterwards; a failed capture leaves the plan eager with the reason
 *       in nrm_last_error (NRM_OK).  NRM_DEBUG="graph=0": always eager.  No floating-point atomics: the same input gives the same bits, eager or replayed.
 *       On CSR counts the three lcpm passes are nrm_lcpm_csr_count / colsum / write in the form that reads its data-dependent scalars on the device: the stored
 *       entries from indptr[genes], clamped to nnz_cap, and the fixed-point unit max (E[x] - E[0]) / x from a word a kernel fills from the table just written
 *       (an integer maximum on the bit patterns); from the covariate rows on, the step is the dense one.
 *   nrm_front_plan_check: synchronises the device, reads all counters once, clears them and answers in the order the reference would meet the conditions: a
 *       malformed CSR matrix (a word of its own beside the sixteen counters: NRM_E_ARG in the words of nrm_lcpm_csr_host, in front of everything else); a
 *       negative entry (lcpm.py:86, NRM_E_ARG); no read at all (the assertion t0 > 2, lcpm.py:97: NRM_E_NUMERIC); a cell without a read (lcpm.py:196, NRM_E_ARG);
 *       a count at or beyond count_cap (NRM_E_UNSUPPORTED, naming the cap and the count); a constant covariate row (norm.py:34-37, NRM_E_ARG); compute_var's two
 *       assertions (norm.py:108,125-127: NRM_E_NUMERIC); scaling_factor's (lcpm.py:278-282: NRM_E_NUMERIC); normvar's zero rank (norm.py:160: NRM_E_DEVICE) and
 *       non-finite results (norm.py:286: NRM_E_NUMERIC).  *near_constant (may be NULL): rows normcov would warn about (norm.py:44-47) since the last check.
 *       After a refusal the plan is usable again once its counts are good.
 *   nrm_front_plan_results: check, then into HOST arrays, any of them NULL: dtn (genes, n_cells) of out_dtype, dcn (n_cov + 4, n_cells) fp64, w (n_cells) and
 *       wt (genes) fp64, lcpm (genes, n_cells) of out_dtype, the normalised covariates (n_cov + 4, n_cells) fp64.
 *   nrm_front_plan_device_results: dtn, dcn and lcpm as DEVICE pointers (row pitch *ld = n_cells elements) and the plan's own stream; valid until destroy, written
 *       by every step.
 *   nrm_front_plan_info: info[0] captured, [1] steps, [2] iterations compute_var took in the last step checked, [3] the largest count of that step, [4] count_cap,
 *       [5] covariates in all (n_cov + 4), [6] bytes resident, [7] near-constant rows at the last check.
 *   nrm_front_plan_stream, nrm_front_plan_time, nrm_front_plan_destroy (accepts NULL): as nrm_coex_plan_*.
 * Threads: create, check, results and destroy take the lock of the whole-problem entries; step, upload and time do not.  One thread at a time per plan.
 */
typedef struct nrm_front_plan nrm_front_plan;
int nrm_front_plan_create(nrm_front_plan** plan, const void* reads, int dtype, int64_t genes, int64_t n_cells, int64_t ld, int reads_on_device, const double* h_cov,
						  int64_t n_cov, int64_t ntot, int64_t stepmax, double eps, double tol, int out_dtype, int64_t count_cap);
int nrm_front_plan_create_csr(nrm_front_plan** plan, const int64_t* indptr, const int32_t* indices, const void* data, int dtype, int64_t genes, int64_t n_cells, int64_t nnz,
							  int64_t nnz_cap, int on_device, const double* h_cov, int64_t n_cov, int64_t ntot, int64_t stepmax, double eps, double tol, int out_dtype,
							  int64_t count_cap);
int nrm_front_plan_upload(nrm_front_plan* plan, const void* h_reads);
int nrm_front_plan_upload_csr(nrm_front_plan* plan, const int64_t* h_indptr, const int32_t* h_indices, const void* h_data, int64_t nnz);
int nrm_front_plan_step(nrm_front_plan* plan, void* stream);
int nrm_front_plan_check(nrm_front_plan* plan, int64_t* near_constant);
int nrm_front_plan_results(nrm_front_plan* plan, void* h_dtn, double* h_dcn, double* h_w, double* h_wt, void* h_lcpm, double* h_cov);
int nrm_front_plan_device_results(nrm_front_plan* plan, void** d_dtn, void** d_dcn, void** d_lcpm, int64_t* ld, void** stream);
int nrm_front_plan_stream(nrm_front_plan* plan, void** stream);
int nrm_front_plan_info(nrm_front_plan* plan, int64_t info[8]);
int nrm_front_plan_time(nrm_front_plan* plan, int64_t steps, double* ms_per_step);
int nrm_front_plan_destroy(nrm_front_plan* plan);

#ifdef __cplusplus
}
#endif
#endif
