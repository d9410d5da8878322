"""ctypes binding of libnormalisr_hip.so (include/normalisr_hip.h).  No CPU fallback: if the HIP
library is missing or a call fails, this raises."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libnormalisr_hip.so')

NRM_F32, NRM_F64 = 0, 1
NRM_TSV_I64, NRM_TSV_I32, NRM_TSV_U8 = 16, 17, 18  # integer dtypes of nrm_tsv_format
NRM_I64, NRM_I32, NRM_U8, NRM_I16 = 16, 17, 18, 19  # count dtypes of nrm_lcpm_*
NRM_S1_COMMON, NRM_S1_SKIP = -2, -1  # cell codes of nrm_single1_stream (include/normalisr_hip.h)
DESIGN_NOTONE, DESIGN_NEG, DESIGN_GT1, DESIGN_HAS1, DESIGN_NAN = 1, 2, 4, 8, 16  # bits of nrm_design_count's d_info[2]
DESIGN_CSR_BAD = 5  # the slot of d_info nrm_design_csr_count flags a malformed CSR design in
NRM_E_ARG, NRM_E_DEVICE, NRM_E_NUMERIC, NRM_E_UNSUPPORTED = -1, -2, -3, -4
ROW_TILE, K_TILE, PCOEF, FIX_STRIDE = 128, 16, 20, 8

_i64, _i32, _vp, _dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double


class PvaluePlan(ctypes.Structure):
	_fields_ = [('a', _dbl), ('alpha', _dbl), ('ln_front', _dbl), ('umax', _dbl), ('coef', _dbl * PCOEF)]


_SIGNATURES = {
	'nrm_version': ([], _i32),
	'nrm_last_error': ([], ctypes.c_char_p),
	'nrm_device_count': ([ctypes.POINTER(_i32)], _i32),
	'nrm_set_device': ([_i32], _i32),
	'nrm_release_cache': ([], _i32),
	'nrm_last_guard': ([ctypes.POINTER(_i64), ctypes.POINTER(_dbl)], _i32),
	'nrm_host_pin': ([_vp, _i64, _i32], _i32),
	'nrm_host_unpin': ([_vp], _i32),
	'nrm_copy_to_host': ([_vp, _vp, _i64, _vp], _i32),
	'nrm_host_alloc': ([ctypes.POINTER(_vp), _i64], _i32),
	'nrm_host_free': ([_vp], _i32),
	'nrm_fill_zero': ([_vp, _i64, _vp], _i32),
	'nrm_fill_i32': ([_vp, _i32, _i64, _vp], _i32),
	'nrm_copy_rows': ([_vp, _i64, _vp, _i64, _i64, _i64, _vp], _i32),
	'nrm_residualize': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp], _i32),
	'nrm_residualize_q': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_binnet_debug_buffer': ([_vp], _i32),
	'nrm_residualize_q_chunked': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_gram_f64': ([_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp], _i32),
	'nrm_gram_f64_band': ([_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i32, _i64, _i64, _i64, _i64, _vp, _vp], _i32),
	'nrm_gram_workspace_bytes': ([], _i64),
	'nrm_quant_bytes': ([_i64, _i64, _i32], _i64),
	'nrm_quantize_rows': ([_vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp], _i32),
	'nrm_gram_i8_band': ([_vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i64, _i64, _vp, _vp], _i32),
	'nrm_gram_i8_chunk': ([_vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i64, _i64, _i32, _i32, _vp, _vp], _i32),
	'nrm_pvalue_plan_init': ([ctypes.POINTER(PvaluePlan), _dbl], _i32),
	'nrm_pvalue_plan_init_many': ([_vp, _i64, _vp, _i64], _i32),
	'nrm_pvalue_plan_fill_many': ([_vp, _i64, _vp, _i64], _i32),
	'nrm_pvalues_from_r2': ([_vp, _i64, _dbl, _vp, _vp], _i32),
	'nrm_logpvalues_from_r2': ([_vp, _i64, _dbl, _vp, _vp], _i32),
	'nrm_assoc_sweep': ([_vp, _i64, _vp, _vp, _i64, _i64, _i64, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _dbl, _vp], _i32),
	'nrm_assoc_sweep_band': ([_vp, _i64, _vp, _vp, _i64, _i64, _i64, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _vp], _i32),
	'nrm_assoc_sweep_mirror': ([_vp, _i64, _vp, _vp, _i64, _i64, _i64, _dbl, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _dbl, _vp], _i32),
	# the same three with p_kind (0 = P, 1 = ln P) before the stream
	'nrm_assoc_sweep_pk': ([_vp, _i64, _vp, _vp, _i64, _i64, _i64, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _dbl, _i32, _vp], _i32),
	'nrm_assoc_sweep_band_pk': ([_vp, _i64, _vp, _vp, _i64, _i64, _i64, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _dbl, _i32, _vp], _i32),
	'nrm_assoc_sweep_mirror_pk': ([_vp, _i64, _vp, _vp, _i64, _i64, _i64, _dbl, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _dbl, _i32, _vp], _i32),
	'nrm_host_mirror_rows': ([_vp, _i64, _i32, _i64, _i64, _i32], _i32),
	'nrm_copy_rect_to_host': ([_vp, _i64, _vp, _i64, _i64, _i64, _vp], _i32),
	'nrm_single4_sweep': ([_vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _dbl, _i32, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp], _i32),
	'nrm_gram_i8_fix_dot': ([_vp, _i64, _vp, _vp, _i64, _i64, _i32, _i64, _vp], _i32),
	'nrm_single4_sweep_guarded': ([_vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _dbl, _i32, _vp, _vp, _vp, _i32, _i64, _vp, _vp,
								  _vp, _vp, _dbl, _dbl, _i32, _dbl, _vp, _vp], _i32),
	'nrm_spd_prepare': ([_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_spd_start': ([_vp, _i64, _i32, _vp, _vp, _vp], _i32),
	'nrm_spd_transpose_residual': ([_vp, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_spd_update': ([_vp, _vp, _i64, _vp], _i32),
	'nrm_spd_finish': ([_vp, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_single4_design_scalars': ([_vp, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_design_products_workspace_doubles': ([_i64, _i64], _i64),
	'nrm_design_products': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _vp], _i32),
	'nrm_residualize_wide': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _vp], _i32),
	'nrm_gram_skinny': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _dbl, _vp, _vp], _i32),
	'nrm_gram_skinny_workspace_bytes': ([], _i64),
	'nrm_de_small_sweep': ([_vp, _vp, _vp, _i64, _i32, _vp, _i64, _i64, _i64, _dbl, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _i32, _vp], _i32),
	'nrm_de_small_sweep_pk': ([_vp, _vp, _vp, _i64, _i32, _vp, _i64, _i64, _i64, _dbl, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _i32, _i32, _vp], _i32),
	'nrm_single1_sweep': ([_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp], _i32),
	'nrm_de_sparse_chunk': ([], _i64),
	'nrm_de_sparse_max_covariates': ([], _i64),
	'nrm_de_sparse_fused_covariates': ([], _i64),
	'nrm_de_sparse_ct_doubles': ([_i64, _i64, _i64], _i64),
	'nrm_de_sparse': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _dbl, _vp, _vp], _i32),
	'nrm_design_count': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp], _i32),
	'nrm_design_plan': ([_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_design_fill': ([_vp, _i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp], _i32),
	'nrm_design_csr_count': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp], _i32),
	'nrm_design_csr_fill': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp], _i32),
	'nrm_design_csr_dense': ([_vp, _vp, _vp, _i32, _i64, _i64, _vp, _i32, _i64, _vp], _i32),
	'nrm_single1_select_gram_blocks': ([], _i64),
	'nrm_single1_select': ([_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_single1_common_gram': ([_vp, _i64, _vp, _i64, _i64, _vp, _vp], _i32),
	'nrm_design_stats': ([_vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_upload': ([_vp, _vp, _i64, _i32, _vp], _i32),
	'nrm_upload_release': ([], _i32),
	'nrm_host_minmax': ([_vp, _i32, _i64, _i32, _vp], _i32),
	'nrm_small_pinv': ([_vp, _i64, _i64, _dbl, _vp, _vp, _i32], _i32),
	'nrm_tsv_shape': ([_vp, _i64, _i32, _i32, _vp, _vp], _i32),
	'nrm_tsv_parse': ([_vp, _i64, _i32, _i32, _vp, _i32, _i64, _i64, _i64], _i32),
	'nrm_tsv_width': ([_i32], _i64),
	'nrm_tsv_format': ([_vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _i32], _i32),
	'nrm_single1_group_stats': ([_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp], _i32),
	'nrm_single1_group_info': ([_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_single1_group_stats_wide': ([_vp, _vp, _vp, _i64, _i64, _vp, _vp], _i32),
	'nrm_single1_group_info_wide': ([_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_single1_group_info_wide_host': ([_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp], _i32),
	'nrm_single1_stream': ([_vp, _i32, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _vp], _i32),
	'nrm_single1_cells': ([_vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp], _i32),
	'nrm_binnet': ([_vp, _i32, _i64, _i64, _dbl, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_binnet_rows': ([_vp, _i32, _i64, _i64, _i64, _i64, _dbl, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_binnet_pk': ([_vp, _i32, _i64, _i64, _dbl, _vp, _i64, _vp, _vp, _i32, _vp], _i32),
	'nrm_binnet_rows_pk': ([_vp, _i32, _i64, _i64, _i64, _i64, _dbl, _vp, _i64, _vp, _vp, _i32, _vp], _i32),
	'nrm_bh_workspace_bytes': ([_i64, _i32], _i64),
	'nrm_bh_tile': ([], _i64),
	'nrm_bh': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp], _i32),
	'nrm_bh_layout': ([_i64, _i32, ctypes.POINTER(_i64)], _i32),
	'nrm_bh_host': ([_vp, _i32, _i64, _vp, ctypes.POINTER(_i32)], _i32),
	'nrm_bh_pk': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _vp], _i32),
	'nrm_bh_host_pk': ([_vp, _i32, _i64, _vp, ctypes.POINTER(_i32), _i32], _i32),
	'nrm_normvar_weights': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp], _i32),
	'nrm_normvar_apply': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i64, _vp, _vp], _i32),
	'nrm_normvar_device_covariates': ([], _i64),
	'nrm_normvar_exp_probe': ([_vp, _i64, _vp, _vp], _i32),
	'nrm_normvar_solve': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_normvar_rescale': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp], _i32),
	'nrm_normvar_apply_w2': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _i64, _vp], _i32),
	'nrm_alpha': ([_vp, _i32, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp], _i32),
	'nrm_association_tests_single1_host': ([_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32], _i32),
	'nrm_association_tests_single4_host': ([_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _i32], _i32),
	'nrm_association_tests_single4_pinv_host': ([_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _i32], _i32),
	'nrm_binnet_host': ([_vp, _i32, _i64, _dbl, _vp, _vp], _i32),
	'nrm_binnet_host_pk': ([_vp, _i32, _i64, _dbl, _vp, _vp, _i32], _i32),
	'nrm_gram_host': ([_vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _vp, _vp], _i32),
	'nrm_pvalues_host': ([_vp, _i64, _dbl, _vp], _i32),
	'nrm_normvar_host': ([_vp, _i32, _i64, _i64, _vp, _vp, _vp, _i64, _dbl, _i32, _vp, _i32, _vp], _i32),
	'nrm_small_eigvals': ([_vp, _i64, _vp], _i32),
	'nrm_association_tests_host': ([_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _i32, _i32, _i32,
									_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32], _i32),
	'nrm_association_tests_host_pk': ([_vp, _i32, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _i32, _i32, _i32,
									   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32], _i32),
	'nrm_lcpm_row_tile': ([], _i64),
	'nrm_lcpm_table_cap': ([], _i64),
	'nrm_lcpm_count_workspace': ([_i64, _i64], _i64),
	'nrm_lcpm_count': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_lcpm_digamma': ([_i64, _dbl, _vp, _vp], _i32),
	'nrm_lcpm_colsum': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_lcpm_write': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i32, _i64, _vp], _i32),
	'nrm_lcpm_csr_workspace': ([_i64, _i64], _i64),
	'nrm_lcpm_csr_count': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_lcpm_csr_colsum': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _i64, _dbl, _vp, _vp, _vp, _vp], _i32),
	'nrm_lcpm_csr_write': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i32, _i64, _vp], _i32),
	'nrm_qc_stats_workspace': ([_i64, _i64], _i64),
	'nrm_qc_stats': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_qc_csr_stats': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_qc_decide': ([_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_subset_dense': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp], _i32),
	'nrm_subset_csr_count': ([_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_subset_csr_scan': ([_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_subset_csr_write': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp], _i32),
	'nrm_net_degree': ([_vp, _i64, _i64, _vp, _vp], _i32),
	'nrm_pc_correlation': ([_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp], _i32),
	'nrm_pc_power': ([_vp, _i64, _i64, _vp, _vp, _vp, _i32, _vp], _i32),
	'nrm_pc_score_workspace': ([_i64, _i64], _i64),
	'nrm_pc_score': ([_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp], _i32),
	'nrm_fitvar_row_tile': ([], _i64),
	'nrm_wide_covariates': ([], _i64),
	'nrm_normvar_pairs': ([_vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp], _i32),
	'nrm_normvar_chol': ([_vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_gram_f64_whole': ([_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp], _i32),
	'nrm_fitvar_moments': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp], _i32),
	'nrm_fitvar_genes': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_cells': ([_vp, _i32, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_plan_workspace': ([_i64, _i64], _i64),
	'nrm_fitvar_plan_start': ([_i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_design': ([_vp, _i64, _i64, _i64, _vp, _vp, _dbl, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_pinv': ([_i64, _i64, _dbl, _vp, _dbl, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_update': ([_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _vp, _vp], _i32),
	'nrm_fitvar_weights': ([_vp, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_pinv_host': ([_vp, _i64, _dbl, _vp, _vp], _i32),
	'nrm_chol_inverse_workspace': ([_i64], _i64),
	'nrm_chol_inverse': ([_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp], _i32),
	'nrm_chol_inverse_host': ([_vp, _i64, _i64, _vp, _i64, _vp], _i32),
	'nrm_fitvar_wide_workspace': ([_i64, _i64, _i64], _i64),
	'nrm_fitvar_wide_design': ([_vp, _i64, _i64, _i64, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _dbl, _i32, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_fitvar_wide_update': ([_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _dbl, _vp, _vp], _i32),
	'nrm_lcpm_host': ([_vp, _i32, _i64, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp], _i32),
	'nrm_lcpm_csr_host': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _i64, _vp, _i32, _vp, _vp, _vp], _i32),
	'nrm_compute_var_host': ([_vp, _i32, _i64, _i64, _vp, _i64, _i64, _dbl, _vp, _vp], _i32),
	'nrm_qc_reads_host': ([_vp, _i32, _i64, _i64] + [_dbl] * 6 + [_vp, _vp, _vp], _i32),
	'nrm_qc_reads_csr_host': ([_vp, _vp, _vp, _i32, _i64, _i64, _i64] + [_dbl] * 6 + [_vp, _vp, _vp], _i32),
	'nrm_enrich_pack': ([_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_enrich_overlap': ([_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
	'nrm_enrich_fisher': ([_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp], _i32),
	'nrm_enrich_top': ([_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp], _i32),
	'nrm_enrich_top_host': ([_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp], _i32),
	'nrm_fisher_host': ([_vp, _vp, _vp, _vp, _i64, _vp], _i32),
	'nrm_enrich_host': ([_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_coex_project': ([_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp], _i32),
	'nrm_coex_downdate': ([_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp], _i32),
	'nrm_cache_bytes': ([ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
	'nrm_covariates_pinv': ([_vp, _i32, _i64, _i64, _dbl, _vp, ctypes.POINTER(_i32)], _i32),
	'nrm_coex_plan_create': ([ctypes.POINTER(_vp), _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i64, _vp, _i32, _i32, _i32], _i32),
	'nrm_coex_plan_upload': ([_vp, _vp], _i32),
	'nrm_coex_plan_step': ([_vp, _vp], _i32),
	'nrm_coex_plan_check': ([_vp, ctypes.POINTER(_i64), ctypes.POINTER(_dbl)], _i32),
	'nrm_coex_plan_results': ([_vp, _vp, _vp, _vp], _i32),
	'nrm_coex_plan_device_results': ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)], _i32),
	'nrm_coex_plan_stream': ([_vp, ctypes.POINTER(_vp)], _i32),
	'nrm_coex_plan_info': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_coex_plan_time': ([_vp, _i64, ctypes.POINTER(_dbl)], _i32),
	'nrm_coex_plan_destroy': ([_vp], _i32),
	'nrm_de_plan_create': ([ctypes.POINTER(_vp), _i32, _vp, _i32, _i64, _vp, _vp, _i64, _i32, _i64, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i64, _vp, _i32, _i32, _i32, _i32,
						   _i32], _i32),
	'nrm_de_plan_design': ([_vp, _i32, _vp, _i32, _i64, _vp, _vp, _i64, _i32], _i32),
	'nrm_de_plan_upload': ([_vp, _vp], _i32),
	'nrm_de_plan_step': ([_vp, _vp], _i32),
	'nrm_de_plan_check': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_de_plan_results': ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_de_plan_device_results': ([_vp] + [ctypes.POINTER(_vp)] * 7 + [ctypes.POINTER(_i64)], _i32),
	'nrm_de_plan_stream': ([_vp, ctypes.POINTER(_vp)], _i32),
	'nrm_de_plan_info': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_de_plan_time': ([_vp, _i64, ctypes.POINTER(_dbl)], _i32),
	'nrm_de_plan_destroy': ([_vp], _i32),
	'nrm_single1_plan_create': ([ctypes.POINTER(_vp), _i32, _vp, _i32, _i64, _vp, _vp, _i64, _i32, _i64, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i64, _i32, _i32, _i32, _i32],
								_i32),
	'nrm_single1_plan_design': ([_vp, _i32, _vp, _i32, _i64, _vp, _vp, _i64, _i32], _i32),
	'nrm_single1_plan_upload': ([_vp, _vp], _i32),
	'nrm_single1_plan_step': ([_vp, _vp], _i32),
	'nrm_single1_plan_check': ([_vp], _i32),
	'nrm_single1_plan_results': ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_single1_plan_device_results': ([_vp] + [ctypes.POINTER(_vp)] * 7 + [ctypes.POINTER(_i64)], _i32),
	'nrm_single1_plan_stream': ([_vp, ctypes.POINTER(_vp)], _i32),
	'nrm_single1_plan_info': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_single1_plan_time': ([_vp, _i64, ctypes.POINTER(_dbl)], _i32),
	'nrm_single1_plan_destroy': ([_vp], _i32),
	'nrm_single4_plan_create': ([ctypes.POINTER(_vp), _i32, _vp, _i32, _i64, _vp, _vp, _i64, _i32, _i64, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i64, _vp, _i32, _i32, _i32,
								_i32, _i32, _dbl], _i32),
	'nrm_single4_plan_design': ([_vp, _i32, _vp, _i32, _i64, _vp, _vp, _i64, _i32], _i32),
	'nrm_single4_plan_upload': ([_vp, _vp], _i32),
	'nrm_single4_plan_step': ([_vp, _vp], _i32),
	'nrm_single4_plan_check': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_single4_plan_results': ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_single4_plan_device_results': ([_vp] + [ctypes.POINTER(_vp)] * 7 + [ctypes.POINTER(_i64)], _i32),
	'nrm_single4_plan_stream': ([_vp, ctypes.POINTER(_vp)], _i32),
	'nrm_single4_plan_info': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_single4_plan_time': ([_vp, _i64, ctypes.POINTER(_dbl)], _i32),
	'nrm_single4_plan_destroy': ([_vp], _i32),
	'nrm_front_plan_create': ([ctypes.POINTER(_vp), _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _dbl, _dbl, _i32, _i64], _i32),
	'nrm_front_plan_create_csr': ([ctypes.POINTER(_vp), _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _dbl, _dbl, _i32, _i64], _i32),
	'nrm_front_plan_upload': ([_vp, _vp], _i32),
	'nrm_front_plan_upload_csr': ([_vp, _vp, _vp, _vp, _i64], _i32),
	'nrm_front_plan_step': ([_vp, _vp], _i32),
	'nrm_front_plan_check': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_front_plan_results': ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
	'nrm_front_plan_device_results': ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_vp)], _i32),
	'nrm_front_plan_stream': ([_vp, ctypes.POINTER(_vp)], _i32),
	'nrm_front_plan_info': ([_vp, ctypes.POINTER(_i64)], _i32),
	'nrm_front_plan_time': ([_vp, _i64, ctypes.POINTER(_dbl)], _i32),
	'nrm_front_plan_destroy': ([_vp], _i32),
}

_lib = None


def exported_symbols():
	return sorted(_SIGNATURES)


_prefer_host = False


def prefer_host_entry(on=True):
	"""The command line's default for de / coex / binnet on one GPU: numpy buffers through the library's whole-problem entries, torch not imported."""
	global _prefer_host
	prev, _prefer_host = _prefer_host, bool(on)
	return prev


def host_entry_preferred():
	v = os.environ.get('NRM_HOST_ENTRY', '')
	return v == '1' or (_prefer_host and v != '0')


def _preload_torch_hip():
	try:
		import importlib.util
		spec = importlib.util.find_spec('torch')  # (finds the package, does not import it)
		for d in (spec.submodule_search_locations or []) if spec is not None else []:
			f = os.path.join(d, 'lib', 'libamdhip64.so')
			if os.path.exists(f):
				ctypes.CDLL(f, mode=ctypes.RTLD_GLOBAL)
				return True
	except Exception:
		pass
	return False


def load():
	"""Load the HIP library; raises RuntimeError (never falls back) when it is not built."""
	global _lib
	if _lib is not None:
		return _lib
	if not os.path.exists(LIB_PATH):
		try:  # build in-tree once if a ROCm toolchain is present; never fall back to a CPU path
			from . import build as _build
			_build.build()
		except Exception as e:
			raise RuntimeError('libnormalisr_hip.so is not built ({}) and building it failed: {}. Run `python -m normalisr_amd.build` '
							   '(needs hipcc); there is no CPU fallback.'.format(LIB_PATH, e))
	# One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  If it is
	# loaded first our DT_NEEDED entry binds to it; the other order would load /opt/rocm's copy next to
	# torch's and the second runtime finds no device.  torch is the plumbing for device memory anyway.
	if 'torch' not in sys.modules and host_entry_preferred():
		# a process on the library's own whole-problem entries (the command line; NRM_HOST_ENTRY=1) never needs torch: its import alone is a
		# second of a 1.3 s `normalisr coex` call.  The HIP runtime torch bundles is loaded by itself instead, so that a later `import torch`
		# (a call the entries do not cover) still finds ONE runtime in the process.
		_preload_torch_hip()
	else:
		try:
			import torch  # noqa: F401
		except ImportError:
			pass
	lib = ctypes.CDLL(LIB_PATH)
	for name, (args, res) in _SIGNATURES.items():
		f = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
		f.argtypes = args
		f.restype = res
	_lib = lib
	return lib


def check(rc):
	"""Map a status code to the exception class the reference raises for the same condition."""
	if rc == 0:
		return
	msg = load().nrm_last_error().decode('utf-8', 'replace')
	if rc == NRM_E_ARG:
		raise ValueError(msg)
	if rc == NRM_E_NUMERIC:
		raise AssertionError(msg)
	if rc == NRM_E_UNSUPPORTED:
		raise NotImplementedError(msg)
	raise RuntimeError(msg)
