"""ctypes binding of libbayeslm_hip.so (include/bayeslm.h).

The product path has no CPU fallback: if the library is missing, was built for
another ABI, or a call fails, this module raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLM_LIB=/path/to/another/libbayeslm_hip.so selects a different BUILD of the same library (same-box A/B runs of
# tools/ab_lib.sh) without touching the in-tree file; it is still the HIP library or nothing -- there is no fallback
LIB_PATH = os.environ.get("BLM_LIB") or os.path.join(_HERE, "libbayeslm_hip.so")

ABI_VERSION = 1
TOPK_MAX = 256  # BLM_TOPK_MAX (include/bayeslm.h)
ROW_TEMPS_MAX = 8  # BLM_ROW_TEMPS_MAX
CACHE_THETAS_MAX = 8  # BLM_CACHE_THETAS_MAX
DYNEVAL_RMS_WS_FLOATS = 4096  # BLM_DYNEVAL_RMS_WS_FLOATS
EDIT_MAX_LEN = 1023  # BLM_EDIT_MAX_LEN
NBEST_GRID_MAX = 64  # BLM_NBEST_GRID_MAX
SWAG_RANK_MAX = 32  # BLM_SWAG_RANK_MAX
SWAG_DRAWS_MAX = 8  # BLM_SWAG_DRAWS_MAX
SWAG_SAMPLES_MAX = 64  # BLM_SWAG_SAMPLES_MAX
LAPLACE_SAMPLES_MAX = 32  # BLM_LAPLACE_SAMPLES_MAX
LAPLACE_LINKS = {"probit": 0, "expexp": 1}  # blm_laplace_row_stats' link; "mc" is blm_laplace_mc_rows
OK = 0
ERR_INVALID, ERR_ABI, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3, -4  # blm_status (include/bayeslm.h)
GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_MUL_DGELU, EPI_BAYES_WGRAD, EPI_GP_MIX, EPI_MUL_DGP_MIX = range(7)
GEMM_ACCUMULATE = 1
STREAM_WEIGHT = 0x10000000   # stream class in the top 4 bits, tensor / site id in the low 28: the classes cannot alias
STREAM_DROPOUT = 0x20000000
STREAM_LRT = 0x30000000      # pre-activation noise of local reparameterisation (ops.bayes_linear_lrt), + site id
STREAM_SWAG = 0x40000000     # a SWAG sample's noise: + 0 diagonal, + 1 low rank; the step is the sample id
STREAM_LAPLACE = 0x50000000  # the logit noise of the last-layer Laplace predictive; the step is the sample id
STREAM_SGMCMC = 0x60000000   # the Langevin noise of an SG-MCMC weight update; the step is the optimisation step

c_fp = C.POINTER(C.c_float)
c_i64p = C.POINTER(C.c_int64)


class Rng(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("stream", C.c_uint32), ("step", C.c_uint32)]


class Variational(C.Structure):
    _fields_ = [("lgstd", C.c_void_p), ("eps", C.c_void_p), ("row_lo", C.c_int32), ("srows", C.c_int32),
                ("rng", Rng)]


class VarItem(C.Structure):
    """blm_var_item: one tensor of a variational group (include/bayeslm.h)."""
    _fields_ = [("mu", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64), ("v", Variational), ("w_out", C.c_void_p),
                ("kl_weight", C.c_float), ("kl_minus", C.c_float), ("dw", C.c_void_p), ("dmu", C.c_void_p),
                ("dlgstd", C.c_void_p)]


VAR_GROUP_MAX = 16


class GemmArgs(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("op", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("A", C.c_void_p), ("lda", C.c_int64), ("B", C.c_void_p), ("ldb", C.c_int64),
                ("C", C.c_void_p), ("ldc", C.c_int64), ("alpha", C.c_float), ("flags", C.c_uint32),
                ("epilogue", C.c_int32), ("bias", C.c_void_p), ("aux", C.c_void_p), ("coef", C.c_void_p),
                ("var_b", Variational), ("C2", C.c_void_p), ("wg_mu", C.c_void_p), ("var_c", Variational),
                ("kl_lambda", C.c_float), ("kl_inv_n", C.c_float), ("drop_p", C.c_float), ("drop_rng", Rng),
                ("drop_B", C.c_int32), ("drop_col_offset", C.c_int32), ("drop_global_cols", C.c_int32),
                ("colsum_a", C.c_void_p)]


class Gpnn2Seq(C.Structure):
    """blm_gpnn2_seq (include/bayeslm.h)."""
    _fields_ = ([("abi_version", C.c_uint32), ("mode", C.c_int32), ("gate", C.c_int32), ("acts", C.c_int32)]
                + [(n, C.c_int32) for n in ("T", "B", "H", "M", "MP", "GP", "nF")]
                + [(n, C.c_void_p) for n in ("xw", "w_hh", "w_hh_t", "FT", "Fp", "cwp", "cwt", "hs", "cs", "ga", "z4", "pre", "feat",
                                             "sact", "gout", "dy", "dh", "dcs2", "dgates", "da", "ds", "df")])


class BeamPoolArgs(C.Structure):
    """blm_beam_pool (include/bayeslm.h)."""
    _fields_ = ([("abi_version", C.c_uint32), ("P", C.c_int32)]
                + [(n, C.c_void_p) for n in ("norm", "raw", "len", "step", "parent", "finished", "count", "inserted")])


class RowTemps(C.Structure):
    """blm_row_temps (include/bayeslm.h)."""
    _fields_ = [("abi_version", C.c_uint32), ("count", C.c_int32), ("beta", C.c_float * ROW_TEMPS_MAX)]


class CacheThetas(C.Structure):
    """blm_cache_thetas (include/bayeslm.h)."""
    _fields_ = [("abi_version", C.c_uint32), ("count", C.c_int32), ("theta", C.c_float * CACHE_THETAS_MAX)]


class NbestGrid(C.Structure):
    """blm_nbest_grid (include/bayeslm.h)."""
    _fields_ = [("abi_version", C.c_uint32), ("G", C.c_int32), ("lmwt", C.c_double * NBEST_GRID_MAX),
                ("nnweight", C.c_double * NBEST_GRID_MAX), ("wip", C.c_double * NBEST_GRID_MAX),
                ("pscale", C.c_double * NBEST_GRID_MAX)]


class SwagDraw(C.Structure):
    """blm_swag_draw (include/bayeslm.h)."""
    _fields_ = [("abi_version", C.c_uint32), ("count", C.c_int32), ("a", C.c_float), ("b", C.c_float), ("inv_n", C.c_float),
                ("var_floor", C.c_float), ("sample_id", C.c_uint32 * SWAG_DRAWS_MAX), ("rng", Rng)]


class GemmPlan(C.Structure):
    _fields_ = [("tile", C.c_int32), ("splits", C.c_int32), ("source", C.c_int32), ("model_us", C.c_float)]


# name -> (restype, argtypes); every symbol include/bayeslm.h declares
_vp, _i, _f, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
_rngp, _varp = C.POINTER(Rng), C.POINTER(Variational)
SIGNATURES = {
    "blm_abi_version": (C.c_uint32, []),
    "blm_last_error": (C.c_char_p, []),
    "blm_query": (_i, [_i, C.c_char_p, C.POINTER(_i), C.POINTER(_i)]),
    "blm_sample_weight": (_i, [_vp, _i64, _i64, _varp, _vp, _vp, _f, _vp]),
    "blm_sample_weight_bwd": (_i, [_vp, _i64, _i64, _varp, _vp, _vp, _vp]),
    "blm_variational_group_fwd": (_i, [C.POINTER(VarItem), _i, _vp, _vp]),
    "blm_variational_group_bwd": (_i, [C.POINTER(VarItem), _i, _vp, _vp]),
    "blm_philox_normal": (_i, [_vp, _i64, _rngp, _vp]),
    "blm_lrt_prepare": (_i, [_vp, _vp, _i64, _i, _vp]),
    "blm_lrt_combine": (_i, [_vp, _vp, _vp, _rngp, _i, _i, _i, _i, _i, _vp]),
    "blm_lrt_bwd_factor": (_i, [_vp, _vp, _vp, _vp, _rngp, _i, _i, _i, _i, _i, _vp]),
    "blm_lrt_mul": (_i, [_vp, _vp, _vp, _i64, _f, _i, _vp]),
    "blm_kl_mean_fwd": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _f, _vp, _vp]),
    "blm_kl_mean_bwd": (_i, [_vp, _i64, _vp, _i64, _i64, _vp, _f, _vp, _i64, _vp, _vp]),
    "blm_gemm": (_i, [C.POINTER(GemmArgs), _vp]),
    "blm_set_gemm_mode": (_i, [_i]),
    "blm_get_gemm_mode": (_i, []),
    "blm_gemm_plan_query": (_i, [C.POINTER(GemmArgs), C.POINTER(GemmPlan)]),
    "blm_gemm_plan_launch": (_i, [C.POINTER(GemmArgs), C.POINTER(GemmPlan)]),
    "blm_gemm_plan_model_us": (_i, [C.POINTER(GemmArgs), _i, _i, C.POINTER(C.c_float)]),
    "blm_gemm_plan_override": (_i, [_i, _i]),
    "blm_gemm_plan_set": (_i, [_i] * 8),
    "blm_gemm_plan_clear": (_i, [_i]),
    "blm_mfma_probe_ws_floats": (_i64, []),
    "blm_mfma_probe": (_i, [_vp, _i, C.POINTER(C.c_double), _vp]),
    "blm_set_option": (_i, [C.c_char_p, _i]),
    "blm_get_option": (_i, [C.c_char_p, C.POINTER(C.c_int)]),
    "blm_gemm_plan_set_cus": (_i, [_i]),
    "blm_gemm_plan_get_cus": (_i, []),
    "blm_gemm_plan_comm_window": (_i, [_f]),
    "blm_gemm_plan_comm_window_left": (_f, []),
    "blm_gemm_plan_set_comm": (_i, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "blm_embed_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i64, _f, _f, _rngp, _i, _i, _vp]),
    "blm_embed_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _f, _f, _rngp, _i, _i, _vp]),
    "blm_add_pe_dropout": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_dropout": (_i, [_vp, _vp, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_dropout_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_add_dropout_ln_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _rngp, _i, _i, _vp]),
    "blm_ln_bwd_ws_floats": (_i64, [_i, _i]),
    "blm_add_dropout_ln_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_attn_fwd": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_attn_fwd_rows": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _vp]),
    "blm_attn_fwd_tree": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "blm_attn_bwd": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_attn_bwd_ws": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _f, _rngp, _i, _i, _vp,
                            _i64, _vp]),
    "blm_attn_bwd_ws_floats": (_i64, [_i, _i, _i, _i]),
    "blm_attn_fwd_keep": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "blm_attn_bwd_keep": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "blm_attn_decode_ws_floats": (_i64, [_i, _i, _i, _i, _i]),
    "blm_attn_decode": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "blm_kv_append": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "blm_kv_gather": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "blm_embed_at": (_i, [_vp, _vp, _i64, _f, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "blm_log_softmax_rows": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp]),
    "blm_sample_rows": (_i, [_vp, _i64, _i, _i, _f, _rngp, _vp, _vp]),
    "blm_row_stats": (_i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blm_row_stats_temps": (_i, [_vp, _i64, _vp, _i, _i, C.POINTER(RowTemps), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blm_cache_scores": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(CacheThetas), _vp, _vp, _vp, _vp]),
    "blm_dyneval_accum": (_i, [_vp, _vp, _i64, _vp]),
    "blm_dyneval_rms": (_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp]),
    "blm_dyneval_update": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _f, _f, _f, _i, _vp]),
    "blm_swag_collect": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "blm_swag_sample": (_i, [_vp, _i64, _vp, _vp, _vp, _i64, _i, _vp, _i64, C.POINTER(SwagDraw), _vp]),
    "blm_logp_avg_accum": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "blm_sgmcmc_update": (_i, [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _f, _f, _rngp, _vp]),
    "blm_laplace_curvature": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp]),
    "blm_laplace_row_stats": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blm_laplace_mc_rows": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _i, _rngp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blm_edit_distance": (_i, [_vp, _i64, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "blm_nbest_select": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(NbestGrid), _vp, _vp]),
    "blm_nbest_mbr": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, C.POINTER(NbestGrid), _vp, _vp, _vp]),
    "blm_topk_rows": (_i, [_vp, _i64, _i, _i, _i, _vp, _vp, _vp]),
    "blm_beam_select": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp]),
    "blm_beam_select_pool": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i64, _i, _i, _i, _f, _f, _i, C.POINTER(BeamPoolArgs),
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blm_sample_rows_filtered": (_i, [_vp, _i64, _i, _i, _f, _i, _f, _rngp, _vp, _vp]),
    "blm_spec_accept": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _i, _f, _rngp, _vp, _vp, _vp, _vp, _vp]),
    "blm_ce_fwd_bwd": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "blm_ce_interp_fwd": (_i, [_vp, _vp, _i64, _f, _vp, _vp, _i, _i, _vp]),
    "blm_ce_soft_fwd_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "blm_ce_soft_topk_fwd_bwd": (_i, [_vp, _i64, _vp, _vp, _i64, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "blm_ce_soft_temp_fwd_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "blm_ce_soft_topk_temp_fwd_bwd": (_i, [_vp, _i64, _vp, _vp, _i64, _i, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i,
                                           _vp]),
    "blm_linear_nll_ws_floats": (_i64, [_i, _i]),
    "blm_linear_nll": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "blm_linear_mc_stats_ws_floats": (_i64, [_i, _i, _i]),
    "blm_linear_mc_stats": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "blm_linear_mc_logprobs_ws_floats": (_i64, [_i, _i, _i]),
    "blm_linear_mc_logprobs": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "blm_linear_nll2_wcat_floats": (_i64, [_i, _i, _i]),
    "blm_linear_nll2_ws_floats": (_i64, [_i, _i, _i, _i]),
    "blm_linear_nll2": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "blm_linear_nll_edges_ws_floats": (_i64, [_i, _i]),
    "blm_linear_nll_edges": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "blm_linear_nll2_edges_ws_floats": (_i64, [_i, _i, _i, _i]),
    "blm_linear_nll2_edges": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _vp, _i64, _vp, _i64, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i,
                                   _vp]),
    "blm_ce_bwd": (_i, [_vp, _i64, _vp, _vp, _vp, _f, _vp, _i, _i, _vp]),
    "blm_gp_coef_grad": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "blm_colsum": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp]),
    "blm_colsum2": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _vp]),
    "blm_init_multi": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "blm_sqnorm_ws_floats": (_i64, [_i]),
    "blm_sqnorm_multi": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "blm_clip_sgd_multi": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _f, _f, _f, _i, _f, _vp]),
    "blm_lstm_step_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_lstm_step_bwd": (_i, [_vp] * 10 + [_i, _i, _vp]),
    "blm_lstm_seq_fwd": (_i, [_vp] * 6 + [_i, _i, _i, _vp]),
    "blm_lstm_seq_bwd": (_i, [_vp] * 7 + [_i, _vp, _i, _i, _i, _i, _i, _vp]),
    "blm_lstm_seq_pair_fwd": (_i, [_vp] * 5 + [_i] + [_vp] * 5 + [_i, _i, _i, _vp]),
    "blm_lstm_step_fwd_gp": (_i, [_vp] * 8 + [_i, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_lstm_step_bwd_gp": (_i, [_vp] * 10 + [_i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_transpose": (_i, [_vp, _vp, _i, _i, _vp]),
    "blm_lstm_cell_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_lstm_cell_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_lstm_cell_bwd2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_lstm_cell_ovr_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_lstm_cell_ovr_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_gp_mix_fwd": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "blm_gp_mix_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_add_rowvec": (_i, [_vp, _vp, _i, _i, _vp]),
    "blm_axpy": (_i, [_vp, _vp, _i64, _f, _vp]),
    "blm_rows_gather_add": (_i, [_vp, _vp, _vp, _i64, _i, _i64, _vp]),
    "blm_mix2_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_mix2_partials": (_i64, [_i, _i, _i]),
    "blm_mix2_bwd": (_i, [_vp] * 8 + [_i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_mix2_gp_bwd": (_i, [_vp] * 11 + [_i, _i, _i, _f, _rngp, _i, _i, _vp]),
    "blm_lstm_search_cell_fwd": (_i, [_vp] * 7 + [_i, _i, _vp]),
    "blm_lstm_search_cell_partials": (_i64, [_i, _i]),
    "blm_lstm_search_cell_bwd": (_i, [_vp] * 10 + [_i, _i, _vp]),
    "blm_lstm_search_step_fwd": (_i, [_vp] * 8 + [_i, _i, _vp]),
    "blm_lstm_search_step_partials": (_i64, [_i, _i]),
    "blm_lstm_search_step_bwd": (_i, [_vp] * 11 + [_i, _i, _vp]),
    "blm_lstm_step_dh": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "blm_lstm_step_dh_ld": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "blm_lstm_step_dh_act": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _i, _f, _i, _vp]),
    "blm_gpnn2_actsum_fwd": (_i, [_vp, _vp, _i64, _i, _i, _i, _f, _i, _vp]),
    "blm_gpnn2_actsum_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _f, _i, _vp]),
    "blm_add_cols": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i, _vp]),
    "blm_gpnn2_sample_steps": (_i, [_vp, _vp, _vp, _rngp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "blm_gpnn2_freq_grad": (_i, [_vp, _vp, _vp, _rngp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "blm_lstm_gpnn2_seq_fwd": (_i, [C.POINTER(Gpnn2Seq), _vp]),
    "blm_lstm_gpnn2_seq_bwd": (_i, [C.POINTER(Gpnn2Seq), _vp]),
    "blm_lstm_cell_ovr_bwd2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "blm_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp]),
    "blm_clip_sgd_multi_wd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _f, _f, _f, _i, _f, _f, _vp]),
}

# The entries that return a VALUE (include/bayeslm.h); every other one returns a blm_status, which calls() checks
VALUE_RETURNING = frozenset((
    "blm_abi_version", "blm_last_error", "blm_get_gemm_mode", "blm_gemm_plan_get_cus", "blm_gemm_plan_comm_window_left",
    "blm_mfma_probe_ws_floats", "blm_ln_bwd_ws_floats", "blm_attn_bwd_ws_floats", "blm_attn_decode_ws_floats",
    "blm_linear_nll_ws_floats", "blm_linear_mc_stats_ws_floats", "blm_linear_mc_logprobs_ws_floats", "blm_linear_nll2_wcat_floats",
    "blm_linear_nll2_ws_floats", "blm_linear_nll_edges_ws_floats", "blm_linear_nll2_edges_ws_floats", "blm_sqnorm_ws_floats",
    "blm_mix2_partials", "blm_lstm_search_cell_partials", "blm_lstm_search_step_partials"))

_views = None  # (raw, checked): two CDLL instances of one dlopen handle, each with its own function objects
ROCTX_RANGES = [0]  # ranges pushed so far (BLM_ROCTX=1)


def _wrap_with_roctx(l):
    """BLM_ROCTX=1: every C-ABI call of this binding runs inside a roctx range named after the entry point
    (roctxRangePushA / roctxRangePop of librocprofiler-sdk-roctx, else libroctx64), so `rocprofv3 --marker-trace --kernel-trace` shows which call each kernel
    dispatch belongs to.  Off by default: a range costs two more foreign calls per entry point."""
    try:  # rocprofv3 (rocprofiler-sdk) intercepts this one; the roctracer library is the fallback for older tools
        rx = C.CDLL("librocprofiler-sdk-roctx.so")
    except OSError:
        rx = C.CDLL("libroctx64.so")
    rx.roctxRangePushA.argtypes, rx.roctxRangePushA.restype = [C.c_char_p], C.c_int
    rx.roctxRangePop.argtypes, rx.roctxRangePop.restype = [], C.c_int
    for name in SIGNATURES:
        fn = getattr(l, name)

        def ranged(*a, _fn=fn, _name=name.encode()):
            rx.roctxRangePushA(_name)
            ROCTX_RANGES[0] += 1
            try:
                return _fn(*a)
            finally:
                rx.roctxRangePop()
        setattr(l, name, ranged)


class BayesLMError(RuntimeError):
    status = None  # the blm_status of the failed call, where one failed


def _failure(what, rc, message):
    e = BayesLMError("%s failed (status %d): %s" % (what, rc, message.decode("utf-8", "replace")))
    e.status = rc
    return e


def _load():
    global _views
    if not os.path.exists(LIB_PATH):
        raise BayesLMError(
            "libbayeslm_hip.so is not built (%s). Build it with `make -C bayeslms_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback." % LIB_PATH)
    raw, checked = C.CDLL(LIB_PATH), C.CDLL(LIB_PATH)  # one dlopen handle, two sets of function objects
    last_error = checked.blm_last_error  # the function itself: a failure's message is not a range of its own under BLM_ROCTX=1

    def errcheck(rc, fn, args):
        if rc != OK:
            raise _failure(fn.__name__, rc, last_error())
        return rc
    for l in (raw, checked):
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
            if l is checked and name not in VALUE_RETURNING:
                fn.errcheck = errcheck
    if raw.blm_abi_version() != ABI_VERSION:
        raise BayesLMError("libbayeslm_hip.so ABI %d != binding ABI %d" % (raw.blm_abi_version(), ABI_VERSION))
    if os.environ.get("BLM_ROCTX", "0") == "1":
        _wrap_with_roctx(raw)
        _wrap_with_roctx(checked)
    _views = raw, checked
    return _views


def lib():
    """The loaded library, raw: an entry returns its blm_status (see check); raises if it is not built (no fallback)."""
    return (_views or _load())[0]


def calls():
    """The same library, checked (what ops calls): a non-zero blm_status raises BayesLMError with check()'s message."""
    return (_views or _load())[1]


def check(rc, what=""):
    if rc != OK:
        raise _failure(what or "libbayeslm_hip call", rc, lib().blm_last_error())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_dev_index = None


def stream():
    """Raw handle of torch's CURRENT stream on this process's GPU (one process per GPU: the device index is read once).
    ``torch.cuda.current_stream()`` costs ~17 us per call (device-index resolution); the raw query is < 1 us, and an
    op makes this call for every kernel it launches."""
    global _dev_index
    if _raw_stream is None:
        return torch.cuda.current_stream().cuda_stream
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()
    return _raw_stream(_dev_index)


def ptr(t):
    """Device address of a tensor (None -> NULL); plain integers (ops._P row addresses) pass through."""
    if t is None or isinstance(t, int):
        return t
    return t.data_ptr()


def dev_tensor(t, name="tensor", dtype=torch.float32):
    """Product-path guard: fp32 (or int64) contiguous tensor on the GPU."""
    if not t.is_cuda:
        raise BayesLMError("%s must live on the GPU: bayeslms_amd has no CPU path" % name)
    if _dev_index is not None and t.device.index != _dev_index:
        raise BayesLMError("%s lives on cuda:%d but this process launches on cuda:%d (one process per GPU: call "
                           "torch.cuda.set_device before the first kernel)" % (name, t.device.index, _dev_index))
    if t.dtype != dtype:
        raise BayesLMError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def rng(seed, stream_id, step):
    return Rng(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF)


_checked_arch = False


def require_gfx950():
    """Called once per process before the first kernel launch."""
    global _checked_arch
    if _checked_arch:
        return
    if not torch.cuda.is_available():
        raise BayesLMError("no GPU visible: bayeslms_amd runs on MI355X (gfx950) only")
    arch = C.create_string_buffer(32)
    ncu, lds = C.c_int(0), C.c_int(0)
    calls().blm_query(torch.cuda.current_device(), arch, C.byref(ncu), C.byref(lds))
    name = arch.value.decode()
    if not name.startswith("gfx950"):
        raise BayesLMError("libbayeslm_hip.so is built for gfx950 only, device is %s" % name)
    _checked_arch = True
