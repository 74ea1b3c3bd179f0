"""ctypes binding of the C-ABI in include/bdl_sgmcmc.h (libbdl_sgmcmc.so).

The shared library is built in-tree (`make -C bayesdll_amd/csrc`, or
`__graft_entry__.build()`).  There is no fallback: if the library is missing
or a call fails, a RuntimeError is raised.  The product path never computes
the update anywhere else.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np
import torch  # noqa: F401  — load torch's HIP runtime first so the .so binds to it

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BDL_SGMCMC_LIB", os.path.join(HERE, "libbdl_sgmcmc.so"))

# enums / bits — must match include/bdl_sgmcmc.h
BDL_OK = 0
CSGHMC, SGHMC, SGLD, SGHMC_GRAD, SGLD_GRAD, ADAM_SGHMC, ADAM_SGHMC_GRAD = range(7)
NOISE_NONE, NOISE_BUFFER, NOISE_PHILOX = 0, 1, 2
COLLECT_NONE, COLLECT_WELFORD_INIT, COLLECT_WELFORD, COLLECT_MEAN_INIT, COLLECT_MEAN = range(5)
MIX_BARE, MIX_PIPELINED, MIX_PACED = 0, 1, 2  # include/bdl_measure.h bdl_mix_schedule
ATTR_HEAD, ATTR_PRIOR, ATTR_SKIP, ATTR_GUNALIGNED = 0x1, 0x2, 0x4, 0x8
FLAG_FIRST_STEP, FLAG_RECIP_DIV, FLAG_MOMENTUM, FLAG_GRAD_READY = 0x1, 0x2, 0x4, 0x8
VAR_GIVEN, VAR_RAW_MOMENTS, VAR_WELFORD = 0, 1, 2
ABI_VERSION = 8

_fp = C.c_void_p


class Segment(C.Structure):
    _fields_ = [("offset", C.c_int64), ("numel", C.c_int64), ("attr", C.c_uint32),
                ("pad", C.c_uint32)]


class Run(C.Structure):
    _fields_ = [("end", C.c_int64), ("attr", C.c_uint32), ("pad", C.c_uint32)]


class StepArgs(C.Structure):
    _fields_ = [
        ("theta", _fp), ("grad", _fp), ("mom", _fp), ("prior_mean", _fp), ("noise", _fp),
        ("mom1", _fp), ("mom2", _fp), ("runs", _fp),
        ("nruns", C.c_int32), ("method", C.c_int32), ("noise_mode", C.c_int32),
        ("collect", C.c_int32), ("flags", C.c_int32), ("pad0", C.c_int32),
        ("n", C.c_int64),
        ("lr", C.c_float * 2), ("noise_scale", C.c_float * 2),
        ("one_minus_alpha", C.c_float), ("prior_sig", C.c_float), ("sigma2", C.c_float),
        ("n_data", C.c_float), ("mu", C.c_float), ("collect_a", C.c_float),
        ("collect_b", C.c_float), ("inv_sigma2", C.c_float), ("inv_n_data", C.c_float),
        ("inv_collect_a", C.c_float), ("inv_collect_b", C.c_float), ("pad1", C.c_float),
        ("seed", C.c_uint64), ("chain", C.c_uint64), ("step", C.c_uint64),
        ("grad_base", _fp), ("nonfinite", _fp), ("philox_offset", C.c_uint64),
        ("chain_groups", C.c_uint64),
    ]


class AdamArgs(C.Structure):
    _fields_ = [("adam_m", _fp), ("adam_v", _fp), ("sgd_buf", _fp),
                ("beta1", C.c_float), ("one_minus_beta1", C.c_float), ("beta2", C.c_float),
                ("one_minus_beta2", C.c_float), ("bias_corr1", C.c_float),
                ("bias_corr2", C.c_float), ("eps", C.c_float), ("two_alpha", C.c_float),
                ("nd", C.c_float), ("temperature", C.c_float), ("inv_bias_corr1", C.c_float),
                ("inv_bias_corr2", C.c_float), ("inv_temperature", C.c_float),
                ("pad2", C.c_float), ("grad_is_mom", C.c_int32)]


class MomentsArgs(C.Structure):
    _fields_ = [("theta", _fp), ("mom1", _fp), ("mom2", _fp), ("n", C.c_int64),
                ("collect", C.c_int32), ("flags", C.c_int32), ("collect_a", C.c_float),
                ("collect_b", C.c_float), ("inv_collect_a", C.c_float),
                ("inv_collect_b", C.c_float)]


class SampleArgs(C.Structure):
    _fields_ = [("out", _fp), ("mom1", _fp), ("mom2", _fp), ("noise", _fp), ("n", C.c_int64),
                ("var_mode", C.c_int32), ("noise_mode", C.c_int32), ("ratio", C.c_float),
                ("var_floor", C.c_float), ("inv_ratio", C.c_float), ("blocks_per_cu", C.c_int32),
                ("seed", C.c_uint64), ("chain", C.c_uint64),
                ("step", C.c_uint64), ("chain_groups", C.c_uint64), ("unroll", C.c_int32),
                ("pad", C.c_int32)]


EXPORTS = {
    "bdl_version": (C.c_int, []),
    "bdl_last_error": (C.c_char_p, []),
    "bdl_build_runs": (C.c_int, [C.POINTER(Segment), C.c_int32, C.c_int64, C.POINTER(Run),
                                 C.c_int32]),
    "bdl_sgmcmc_step": (C.c_int, [C.POINTER(StepArgs), C.c_void_p]),
    "bdl_moments_update": (C.c_int, [C.POINTER(MomentsArgs), C.c_void_p]),
    "bdl_adam_step": (C.c_int, [C.POINTER(StepArgs), C.POINTER(AdamArgs), C.c_void_p]),
    "bdl_clip_workspace_bytes": (C.c_int64, [C.c_int64]),
    "bdl_sgld_step_clipped": (C.c_int, [C.POINTER(StepArgs), C.c_float, C.c_void_p, C.c_void_p]),
    "bdl_posterior_sample": (C.c_int, [C.POINTER(SampleArgs), C.c_void_p]),
    "bdl_philox_normal": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64,
                                    C.c_void_p]),
    "bdl_set_launch_config": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "bdl_graph_find_step_node": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64,
                                            C.POINTER(C.c_void_p)]),
    "bdl_graph_node_step_args": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "bdl_graph_redirect": (C.c_int, [C.c_void_p, C.c_void_p]),
    # include/bdl_measure.h
    "bdl_stream_mix": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p),
                                 C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "bdl_sgmcmc_step_bare": (C.c_int, [C.POINTER(StepArgs), C.c_void_p]),
    "bdl_stream_mix_schedule": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32,
                                          C.POINTER(C.c_void_p), C.c_int32, C.c_int64,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    # include/bdl_arena.h
    "bdl_arena_reserve": (C.c_int, [C.c_int32, C.c_int64]),
    "bdl_arena_alloc": (C.c_void_p, [C.c_size_t, C.c_int, C.c_void_p]),
    "bdl_arena_free": (None, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "bdl_arena_stats": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.c_int32]),
    "bdl_arena_contains": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64]),
}


class DiagSummary(C.Structure):
    """include/bdl_diag.h bdl_diag_summary (the start of the diagnostic's workspace)."""
    _fields_ = [("n_eval", C.c_int64), ("n_degenerate", C.c_int64), ("n_nonfinite", C.c_int64),
                ("argmax", C.c_int64), ("n_above", C.c_int64 * 3), ("rhat_sum", C.c_double),
                ("rhat_max", C.c_float), ("pad", C.c_float)]


class DiagArgs(C.Structure):
    """include/bdl_diag.h bdl_chain_diag_args."""
    _fields_ = [("mom1", _fp), ("mom2", _fp), ("pooled_mean", _fp), ("pooled_var", _fp),
                ("rhat", _fp), ("workspace", _fp), ("n", C.c_int64), ("chain_groups", C.c_uint64),
                ("chains", C.c_int32), ("var_mode", C.c_int32), ("ratio", C.c_float),
                ("inv_ratio", C.c_float), ("var_floor", C.c_float), ("c1", C.c_float),
                ("thresholds", C.c_float * 3), ("blocks_per_cu", C.c_int32)]


# include/bdl_diag.h: additive to the ABI, bound next to EXPORTS (which stays
# the function list of the three original headers)
DIAG_EXPORTS = {
    "bdl_chain_diag_workspace_bytes": (C.c_int64, [C.c_int64]),
    "bdl_chain_diag": (C.c_int, [C.POINTER(DiagArgs), C.c_void_p]),
}


class ClipSegment(C.Structure):
    """include/bdl_clip.h bdl_clip_segment (a row of the device table: three int64)."""
    _fields_ = [("base", _fp), ("numel", C.c_int64), ("chain_stride", C.c_int64)]


class ClipArgs(C.Structure):
    """include/bdl_clip.h bdl_chain_clip_args."""
    _fields_ = [("segments", _fp), ("nsegments", C.c_int32), ("chains", C.c_int32),
                ("max_norm", C.c_float), ("blocks_per_chain", C.c_int32), ("workspace", _fp)]


CLIP_MAX_SEGMENTS, CLIP_MAX_CHAINS, CLIP_MAX_BLOCKS_PER_CHAIN = 65536, 65535, 1024

# include/bdl_clip.h: additive to the ABI, as DIAG_EXPORTS
CLIP_EXPORTS = {
    "bdl_chain_clip_workspace_bytes": (C.c_int64, [C.c_int32]),
    "bdl_chain_clip": (C.c_int, [C.POINTER(ClipArgs), C.c_void_p]),
}



class ChainScalars(C.Structure):
    """include/bdl_chain_step.h bdl_chain_scalars (a row of the device table: 12 floats)."""
    _fields_ = [("lr", C.c_float * 2), ("noise_scale", C.c_float * 2),
                ("one_minus_alpha", C.c_float), ("prior_sig", C.c_float), ("sigma2", C.c_float),
                ("n_data", C.c_float), ("mu", C.c_float), ("inv_sigma2", C.c_float),
                ("inv_n_data", C.c_float), ("pad", C.c_float)]


class ChainStepArgs(C.Structure):
    """include/bdl_chain_step.h bdl_chain_step_args."""
    _fields_ = [
        ("theta", _fp), ("grad", _fp), ("mom", _fp), ("prior_mean", _fp), ("noise", _fp),
        ("mom1", _fp), ("mom2", _fp), ("nonfinite", _fp), ("runs", _fp), ("grad_base", _fp),
        ("scalars", _fp), ("n1", C.c_int64), ("chain_groups", C.c_uint64),
        ("nruns", C.c_int32), ("chains", C.c_int32), ("method", C.c_int32),
        ("noise_mode", C.c_int32), ("collect", C.c_int32), ("flags", C.c_int32),
        ("blocks_per_chain", C.c_int32), ("unroll", C.c_int32),
        ("nonfinite_per_chain", C.c_int32), ("pad0", C.c_int32),
        ("collect_a", C.c_float), ("collect_b", C.c_float), ("inv_collect_a", C.c_float),
        ("inv_collect_b", C.c_float),
        ("seed", C.c_uint64), ("chain", C.c_uint64), ("step", C.c_uint64),
    ]


# the columns of a scalar row, in bdl_chain_scalars order
CHAIN_SCALAR_COLUMNS = ("lr0", "lr1", "ns0", "ns1", "one_minus_alpha", "prior_sig", "sigma2",
                        "n_data", "mu", "inv_sigma2", "inv_n_data", "pad")
CHAIN_STEP_MAX_CHAINS, CHAIN_STEP_MAX_BLOCKS_PER_CHAIN = 65535, 4096
CHAIN_STEP_MAX_RUNS, CHAIN_STEP_MAX_RUNS_BASES = 4096, 2730

# include/bdl_chain_step.h: additive to the ABI, as DIAG_EXPORTS
CHAIN_STEP_EXPORTS = {
    "bdl_chain_step_unroll_ok": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "bdl_chain_step": (C.c_int, [C.POINTER(ChainStepArgs), C.c_void_p]),
}

class StatsSegment(C.Structure):
    """include/bdl_stats.h bdl_stats_segment (a row of the device table: five int64)."""
    _fields_ = [("grad", _fp), ("numel", C.c_int64), ("grad_stride", C.c_int64),
                ("offset", C.c_int64), ("lr_group", C.c_int64)]


class StatsArgs(C.Structure):
    """include/bdl_stats.h bdl_chain_stats_args."""
    _fields_ = [("theta", _fp), ("mom", _fp), ("prior_mean", _fp), ("segments", _fp),
                ("lr_table", _fp), ("acc", _fp), ("workspace", _fp),
                ("chain_groups", C.c_uint64), ("nsegments", C.c_int32), ("chains", C.c_int32),
                ("lr_row_stride", C.c_int32), ("accumulate", C.c_int32),
                ("blocks_per_chain", C.c_int32), ("pad0", C.c_int32), ("lr", C.c_float * 2)]


STATS_MAX_SEGMENTS, STATS_MAX_CHAINS, STATS_MAX_BLOCKS_PER_CHAIN = 65536, 65535, 256
STATS_MAX_CHAIN_GROUPS = 1 << 40
# the doubles of one (chain, segment) entry of acc, in order
STATS_SUMS = ("G2", "V2", "D2", "DG", "VG", "V2L")

# include/bdl_stats.h: additive to the ABI, as DIAG_EXPORTS
STATS_EXPORTS = {
    "bdl_chain_stats_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "bdl_chain_stats": (C.c_int, [C.POINTER(StatsArgs), C.c_void_p]),
}



class EssFoldArgs(C.Structure):
    """include/bdl_ess.h bdl_ess_fold_args."""
    _fields_ = [("theta", _fp), ("bsum", _fp), ("smean", _fp), ("sM2", _fp), ("bM2", _fp),
                ("n", C.c_int64), ("chain_groups", C.c_uint64), ("sample", C.c_int64),
                ("batch", C.c_int64), ("chains", C.c_int32), ("flags", C.c_int32),
                ("fs", C.c_float), ("fb", C.c_float), ("c", C.c_float),
                ("grid_blocks", C.c_int32)]


class EssSummary(C.Structure):
    """include/bdl_ess.h bdl_ess_summary (the start of the report's workspace)."""
    _fields_ = [("n_eval", C.c_int64), ("n_degenerate", C.c_int64), ("n_nonfinite", C.c_int64),
                ("argmin", C.c_int64), ("n_below", C.c_int64 * 3), ("ess_sum", C.c_double),
                ("ess_min", C.c_float), ("pad", C.c_float)]


class EssArgs(C.Structure):
    """include/bdl_ess.h bdl_chain_ess_args."""
    _fields_ = [("sM2", _fp), ("bM2", _fp), ("ess", _fp), ("mcse", _fp), ("workspace", _fp),
                ("n", C.c_int64), ("chain_groups", C.c_uint64), ("samples", C.c_int64),
                ("batches", C.c_int64), ("chains", C.c_int32), ("grid_blocks", C.c_int32),
                ("thresholds", C.c_float * 3), ("pad0", C.c_int32)]


# bdl_ess_flag
ESS_FIRST_SAMPLE, ESS_FIRST_IN_BATCH, ESS_CLOSE, ESS_FIRST_BATCH = 0x1, 0x2, 0x4, 0x8
ESS_MAX_COUNT, ESS_MAX_CHAINS, ESS_MAX_GRID = 1 << 24, 65535, 2048

# include/bdl_ess.h: additive to the ABI, as DIAG_EXPORTS
ESS_EXPORTS = {
    "bdl_chain_ess_fold": (C.c_int, [C.POINTER(EssFoldArgs), C.c_void_p]),
    "bdl_chain_ess_workspace_bytes": (C.c_int64, [C.c_int64]),
    "bdl_chain_ess": (C.c_int, [C.POINTER(EssArgs), C.c_void_p]),
}



class LowpArgs(C.Structure):
    """include/bdl_lowp.h bdl_lowp_args."""
    _fields_ = [
        ("theta", _fp), ("grad", _fp), ("mom", _fp), ("prior_mean", _fp), ("noise", _fp),
        ("mom1", _fp), ("mom2", _fp), ("shadow", _fp), ("runs", _fp), ("grad_base", _fp),
        ("nonfinite", _fp), ("n", C.c_int64),
        ("nruns", C.c_int32), ("method", C.c_int32), ("noise_mode", C.c_int32),
        ("collect", C.c_int32), ("flags", C.c_int32), ("blocks", C.c_int32),
        ("unroll", C.c_int32), ("pad0", C.c_int32),
        ("lr", C.c_float * 2), ("noise_scale", C.c_float * 2),
        ("one_minus_alpha", C.c_float), ("prior_sig", C.c_float), ("sigma2", C.c_float),
        ("n_data", C.c_float), ("mu", C.c_float), ("collect_a", C.c_float),
        ("collect_b", C.c_float), ("inv_sigma2", C.c_float), ("inv_n_data", C.c_float),
        ("inv_collect_a", C.c_float), ("inv_collect_b", C.c_float), ("pad1", C.c_float),
        ("seed", C.c_uint64), ("chain", C.c_uint64), ("step", C.c_uint64),
        ("philox_offset", C.c_uint64), ("chain_groups", C.c_uint64),
    ]


LOWP_MAX_BLOCKS = 65536
LOWP_UNROLLS = (1, 2, 4)

# include/bdl_lowp.h: additive to the ABI, as DIAG_EXPORTS
LOWP_EXPORTS = {
    "bdl_lowp_step": (C.c_int, [C.POINTER(LowpArgs), C.c_void_p]),
    "bdl_lowp_shadow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                  C.c_void_p]),
}


class LayerSegment(C.Structure):
    """include/bdl_layers.h bdl_layer_segment (a row of the device table: two int64)."""
    _fields_ = [("offset", C.c_int64), ("numel", C.c_int64)]


class DiagLayersArgs(C.Structure):
    """include/bdl_layers.h bdl_diag_layers_args."""
    _fields_ = [("mom1", _fp), ("mom2", _fp), ("segments", _fp), ("table", _fp),
                ("workspace", _fp), ("n", C.c_int64), ("chain_groups", C.c_uint64),
                ("nsegments", C.c_int32), ("chains", C.c_int32), ("var_mode", C.c_int32),
                ("grid_blocks", C.c_int32), ("ratio", C.c_float), ("inv_ratio", C.c_float),
                ("var_floor", C.c_float), ("c1", C.c_float), ("thresholds", C.c_float * 3),
                ("pad0", C.c_int32)]


class EssLayersArgs(C.Structure):
    """include/bdl_layers.h bdl_ess_layers_args."""
    _fields_ = [("sM2", _fp), ("bM2", _fp), ("segments", _fp), ("table", _fp),
                ("workspace", _fp), ("n", C.c_int64), ("chain_groups", C.c_uint64),
                ("samples", C.c_int64), ("batches", C.c_int64), ("nsegments", C.c_int32),
                ("chains", C.c_int32), ("grid_blocks", C.c_int32), ("thresholds", C.c_float * 3)]


LAYERS_MAX_SEGMENTS, LAYERS_MAX_GRID = 65536, 1024

# include/bdl_layers.h: additive to the ABI, as DIAG_EXPORTS
LAYERS_EXPORTS = {
    "bdl_layers_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "bdl_chain_diag_layers": (C.c_int, [C.POINTER(DiagLayersArgs), C.c_void_p]),
    "bdl_chain_ess_layers": (C.c_int, [C.POINTER(EssLayersArgs), C.c_void_p]),
}

PREDICT_MAX_CLASSES, PREDICT_WAVE_CLASSES, PREDICT_MAX_BINS = 8192, 256, 64
PREDICT_MAX_GROUPS, PREDICT_MAX_GRID = 65535, 1024
PREDICT_RESET = 0x1


class PredictTotals(C.Structure):
    """include/bdl_predict.h bdl_predict_totals (one per group, device memory)."""
    _fields_ = [("n", C.c_int64), ("n_labelled", C.c_int64), ("n_nonfinite", C.c_int64),
                ("n_wrong", C.c_int64), ("disagree_sum", C.c_int64), ("nll_sum", C.c_double),
                ("entropy_sum", C.c_double), ("expected_entropy_sum", C.c_double),
                ("mi_sum", C.c_double), ("mi_sum_wrong", C.c_double),
                ("bin_count", C.c_int64 * PREDICT_MAX_BINS),
                ("bin_hits", C.c_int64 * PREDICT_MAX_BINS),
                ("bin_conf", C.c_double * PREDICT_MAX_BINS)]


class PredictArgs(C.Structure):
    """include/bdl_predict.h bdl_predict_args."""
    _fields_ = [("logits", _fp), ("labels", _fp), ("logp", _fp), ("entropy", _fp),
                ("expected_entropy", _fp), ("mutual_info", _fp), ("confidence", _fp),
                ("nll", _fp), ("pred", _fp), ("disagree", _fp), ("totals", _fp),
                ("workspace", _fp), ("batch", C.c_int64), ("members", C.c_int32),
                ("groups", C.c_int32), ("classes", C.c_int32), ("num_bins", C.c_int32),
                ("grid_blocks", C.c_int32), ("flags", C.c_int32),
                ("edges", C.c_float * PREDICT_MAX_BINS)]


# include/bdl_predict.h: additive to the ABI, as DIAG_EXPORTS
PREDICT_EXPORTS = {
    "bdl_predict_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "bdl_predict": (C.c_int, [C.POINTER(PredictArgs), C.c_void_p]),
}


class FnFoldArgs(C.Structure):
    """include/bdl_fn.h bdl_fn_fold_args."""
    _fields_ = [("logits", _fp), ("bsum", _fp), ("smean", _fp), ("sM2", _fp), ("bM2", _fp),
                ("probs", _fp), ("probe", C.c_int64), ("chain_groups", C.c_uint64),
                ("sample", C.c_int64), ("batch", C.c_int64), ("chains", C.c_int32),
                ("classes", C.c_int32), ("flags", C.c_int32), ("fs", C.c_float),
                ("fb", C.c_float), ("c", C.c_float), ("grid_blocks", C.c_int32),
                ("pad0", C.c_int32)]


FN_MAX_CLASSES, FN_WAVE_CLASSES, FN_MAX_GRID = 8192, 256, 2048

# include/bdl_fn.h: additive to the ABI, as DIAG_EXPORTS
FN_EXPORTS = {
    "bdl_fn_fold": (C.c_int, [C.POINTER(FnFoldArgs), C.c_void_p]),
}

TEMPER_MAX_CLASSES, TEMPER_WAVE_CLASSES, TEMPER_MAX_BINS = 8192, 256, 64
TEMPER_MAX_GROUPS, TEMPER_MAX_GRID, TEMPER_MAX_ITER = 65535, 1024, 1024
TEMPER_MAX_T, TEMPER_MIN_T = 100.0, 0.01
TEMPER_RESET = 0x1


class TemperState(C.Structure):
    """include/bdl_temper.h bdl_temper_state (one per group, device memory)."""
    _fields_ = [("nll", C.c_double), ("nll_first", C.c_double), ("d1", C.c_double),
                ("d2", C.c_double), ("n", C.c_int64), ("n_nonfinite", C.c_int64),
                ("n_inf_label", C.c_int64), ("beta", C.c_float), ("iterations", C.c_int32),
                ("sweeps", C.c_int32), ("converged", C.c_int32), ("at_bound", C.c_int32),
                ("degenerate", C.c_int32), ("done", C.c_int32), ("pad0", C.c_int32)]


class TemperFitArgs(C.Structure):
    """include/bdl_temper.h bdl_temper_fit_args."""
    _fields_ = [("logp", _fp), ("labels", _fp), ("state", _fp), ("workspace", _fp),
                ("batch", C.c_int64), ("rtol", C.c_double), ("groups", C.c_int32),
                ("classes", C.c_int32), ("grid_blocks", C.c_int32), ("max_iter", C.c_int32)]


class TemperTotals(C.Structure):
    """include/bdl_temper.h bdl_temper_totals (one per group, device memory)."""
    _fields_ = [("n", C.c_int64), ("n_labelled", C.c_int64), ("n_nonfinite", C.c_int64),
                ("n_wrong", C.c_int64), ("nll_sum", C.c_double), ("entropy_sum", C.c_double),
                ("confidence_sum", C.c_double),
                ("bin_count", C.c_int64 * TEMPER_MAX_BINS),
                ("bin_hits", C.c_int64 * TEMPER_MAX_BINS),
                ("bin_conf", C.c_double * TEMPER_MAX_BINS)]


class TemperReportArgs(C.Structure):
    """include/bdl_temper.h bdl_temper_report_args."""
    _fields_ = [("logp", _fp), ("labels", _fp), ("state", _fp), ("totals", _fp),
                ("workspace", _fp), ("batch", C.c_int64), ("groups", C.c_int32),
                ("classes", C.c_int32), ("num_bins", C.c_int32), ("grid_blocks", C.c_int32),
                ("flags", C.c_int32), ("pad0", C.c_int32),
                ("edges", C.c_float * TEMPER_MAX_BINS)]


# include/bdl_temper.h: additive to the ABI, as DIAG_EXPORTS
TEMPER_EXPORTS = {
    "bdl_temper_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "bdl_temper_fit_sweep": (C.c_int, [C.POINTER(TemperFitArgs), C.c_void_p]),
    "bdl_temper_fit_update": (C.c_int, [C.POINTER(TemperFitArgs), C.c_void_p]),
    "bdl_temper_report": (C.c_int, [C.POINTER(TemperReportArgs), C.c_void_p]),
}

MIXTURE_MAX_CLASSES, MIXTURE_WAVE_CLASSES = 4096, 256
MIXTURE_MAX_PAIRS, MIXTURE_MAX_GRID = 65535, 1024
MIXTURE_MIN_WEIGHT = 1e-10
MIXTURE_RESET = 0x1
MIX_ARITHMETIC, MIX_REFERENCE = 0, 1
MIX_COMBINE = {"arithmetic": MIX_ARITHMETIC, "reference": MIX_REFERENCE}


class MemberScore(C.Structure):
    """include/bdl_mixture.h bdl_member_score_t (one per (member, group), device memory)."""
    _fields_ = [("n", C.c_int64), ("n_nonfinite", C.c_int64), ("n_wrong", C.c_int64),
                ("nll_sum", C.c_double)]


class MemberScoreArgs(C.Structure):
    """include/bdl_mixture.h bdl_member_score_args."""
    _fields_ = [("logits", _fp), ("labels", _fp), ("scores", _fp), ("workspace", _fp),
                ("batch", C.c_int64), ("members", C.c_int32), ("groups", C.c_int32),
                ("classes", C.c_int32), ("grid_blocks", C.c_int32), ("flags", C.c_int32),
                ("pad0", C.c_int32)]


class MixtureTotals(C.Structure):
    """include/bdl_mixture.h bdl_mixture_totals (one per group, device memory)."""
    _fields_ = [("n", C.c_int64), ("n_nonfinite", C.c_int64),
                ("expected_entropy_sum", C.c_double)]


class MixtureArgs(C.Structure):
    """include/bdl_mixture.h bdl_mixture_args."""
    _fields_ = [("logits", _fp), ("weights", _fp), ("labels", _fp), ("logp", _fp),
                ("expected_entropy", _fp), ("totals", _fp), ("workspace", _fp),
                ("batch", C.c_int64), ("components", C.c_int32), ("draws", C.c_int32),
                ("groups", C.c_int32), ("classes", C.c_int32), ("combine", C.c_int32),
                ("grid_blocks", C.c_int32), ("flags", C.c_int32), ("pad0", C.c_int32)]


# include/bdl_mixture.h: additive to the ABI, as DIAG_EXPORTS
MIXTURE_EXPORTS = {
    "bdl_member_score_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "bdl_mixture_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "bdl_member_score": (C.c_int, [C.POINTER(MemberScoreArgs), C.c_void_p]),
    "bdl_mixture": (C.c_int, [C.POINTER(MixtureArgs), C.c_void_p]),
}

RANK_U, RANK_ITILE, RANK_JTILE, RANK_MAX_ROWS = 2, 512, 1024, 65535
RANK_MAX_N = 2 ** 31 - 1


class RankTotals(C.Structure):
    """include/bdl_rank.h bdl_rank_totals (one per row, device memory)."""
    _fields_ = [("n_pos", C.c_int64), ("n_neg", C.c_int64), ("n_excluded", C.c_int64),
                ("u2", C.c_int64), ("fp_at_tpr", C.c_int64), ("ap_sum", C.c_double)]


class RankArgs(C.Structure):
    """include/bdl_rank.h bdl_rank_args."""
    _fields_ = [("scores", _fp), ("marks", _fp), ("ge_pos", _fp), ("ge_neg", _fp),
                ("gt_neg", _fp), ("totals", _fp), ("workspace", _fp), ("n", C.c_int64),
                ("need", C.c_int64), ("rows", C.c_int32), ("scores_per_group", C.c_int32),
                ("mark_rows", C.c_int32), ("tpr_num", C.c_int32), ("tpr_den", C.c_int32),
                ("pad0", C.c_int32)]


# include/bdl_rank.h: additive to the ABI, as DIAG_EXPORTS
RANK_EXPORTS = {
    "bdl_rank_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "bdl_rank": (C.c_int, [C.POINTER(RankArgs), C.c_void_p]),
}

DIVERSITY_MAX_VOTERS, DIVERSITY_MAX_CLASSES, DIVERSITY_WAVE_VOTERS = 64, 8192, 16
DIVERSITY_TILE, DIVERSITY_LDS_STRIDE, DIVERSITY_MAX_GRID = 64, 68, 1024
DIVERSITY_DEFAULT_WORKSPACE = 32 << 20
DIVERSITY_RESET = 0x1
DIVERSITY_INT_MATRICES = ("disagree", "both_wrong", "kl_unbounded")
DIVERSITY_SUM_MATRICES = ("tv_sum", "kl_sum")


def diversity_totals_dtype(voters):
    """include/bdl_diversity.h: the totals of P voters as one NumPy record —
    bdl_diversity_header, then the five [P, P] matrices in the header's order."""
    P = int(voters)
    return np.dtype([(k, np.int64) for k in ("n", "n_labelled", "n_nonfinite", "voters")]
                    + [(k, np.int64, (P, P)) for k in DIVERSITY_INT_MATRICES]
                    + [(k, np.float64, (P, P)) for k in DIVERSITY_SUM_MATRICES])


class DiversityArgs(C.Structure):
    """include/bdl_diversity.h bdl_diversity_args."""
    _fields_ = [("logits", _fp), ("labels", _fp), ("totals", _fp), ("workspace", _fp),
                ("batch", C.c_int64), ("voters", C.c_int32), ("classes", C.c_int32),
                ("grid_blocks", C.c_int32), ("flags", C.c_int32)]


# include/bdl_diversity.h: additive to the ABI, as DIAG_EXPORTS
DIVERSITY_EXPORTS = {
    "bdl_diversity_totals_bytes": (C.c_int64, [C.c_int32]),
    "bdl_diversity_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "bdl_diversity": (C.c_int, [C.POINTER(DiversityArgs), C.c_void_p]),
}

ORDER_SPANS, ORDER_GRID_STRIDE, ORDER_DYNAMIC = 0, 1, 2
CLAIM_GROUPS, CLAIM_SLOTS, CLAIM_SLOTS_PER_STREAM = 2048, 16, 4
DRIFT_EVERY, DRIFT_SAMPLES = 16, 64
DRIFT_WORDS = 4 + 2 * DRIFT_SAMPLES

# include/bdl_order.h: additive to the ABI, as DIAG_EXPORTS
ORDER_EXPORTS = {
    "bdl_order_last": (C.c_int, [C.POINTER(C.c_int32)]),
    "bdl_order_counters": (C.c_int, [C.c_int32, C.POINTER(C.c_uint32)]),
    "bdl_sweep_drift": (C.c_int, [C.POINTER(StepArgs), C.c_int32, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int32), C.c_void_p]),
}

STACK_MAX_VOTERS, STACK_MAX_CLASSES, STACK_MAX_COLS = 64, 8192, 1 << 24
STACK_TILE, STACK_MAX_GRID, STACK_MAX_CHUNK = 1024, 1024, 65536
STACK_RESET, STACK_FIRST, STACK_FINAL = 0x1, 0x2, 0x4
STACK_COUNTERS = ("n_label", "n_nonfinite", "n_impossible")


class StackState(C.Structure):
    """include/bdl_stacking.h bdl_stack_state (one per fit, device memory)."""
    _fields_ = [("w", C.c_double * STACK_MAX_VOTERS), ("objective", C.c_double),
                ("gap", C.c_double), ("objective_uniform", C.c_double), ("n", C.c_int64),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("degenerate", C.c_int32),
                ("pad", C.c_int32)]


class StackGatherArgs(C.Structure):
    """include/bdl_stacking.h bdl_stack_gather_args."""
    _fields_ = [("logp", _fp), ("labels", _fp), ("ell", _fp), ("valid", _fp), ("counters", _fp),
                ("workspace", _fp), ("batch", C.c_int64), ("off", C.c_int64), ("cap", C.c_int64),
                ("voters", C.c_int32), ("classes", C.c_int32), ("grid_blocks", C.c_int32),
                ("flags", C.c_int32)]


class StackFitArgs(C.Structure):
    """include/bdl_stacking.h bdl_stack_fit_args."""
    _fields_ = [("ell", _fp), ("valid", _fp), ("state", _fp), ("workspace", _fp),
                ("n_cols", C.c_int64), ("cap", C.c_int64), ("tol", C.c_double),
                ("voters", C.c_int32), ("iterations", C.c_int32), ("grid_blocks", C.c_int32),
                ("flags", C.c_int32)]


# include/bdl_stacking.h: additive to the ABI, as DIAG_EXPORTS
STACK_EXPORTS = {
    "bdl_stack_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "bdl_stack_gather": (C.c_int, [C.POINTER(StackGatherArgs), C.c_void_p]),
    "bdl_stack_fit": (C.c_int, [C.POINTER(StackFitArgs), C.c_void_p]),
}

EXCHANGE_MAX_CHAINS, EXCHANGE_MAX_VECTORS, EXCHANGE_TILE, EXCHANGE_MAX_GRID = 64, 4, 1024, 65535
EXCHANGE_STEP_BASE = 1 << 63  # Philox step domain of the exchange draws (include/bdl_exchange.h)
EXCHANGE_FIRST, EXCHANGE_ENERGY_ONLY = 0x1, 0x2
EXCHANGE_UP, EXCHANGE_DOWN = 1, 2


class ExchangeState(C.Structure):
    """include/bdl_exchange.h bdl_exchange_state (device memory)."""
    _fields_ = [("q", C.c_double * EXCHANGE_MAX_CHAINS), ("U", C.c_double * EXCHANGE_MAX_CHAINS),
                ("attempts", C.c_uint64 * EXCHANGE_MAX_CHAINS),
                ("accepts", C.c_uint64 * EXCHANGE_MAX_CHAINS),
                ("round_trips", C.c_uint64 * EXCHANGE_MAX_CHAINS), ("refused", C.c_uint64),
                ("partner", C.c_int32 * EXCHANGE_MAX_CHAINS),
                ("replica", C.c_int32 * EXCHANGE_MAX_CHAINS),
                ("direction", C.c_int32 * EXCHANGE_MAX_CHAINS)]


class ExchangeEnergyArgs(C.Structure):
    """include/bdl_exchange.h bdl_exchange_energy_args."""
    _fields_ = [("theta", _fp), ("prior", _fp), ("workspace", _fp), ("n", C.c_int64),
                ("chain_groups", C.c_uint64), ("chains", C.c_int32), ("grid_blocks", C.c_int32)]


class ExchangeDecideArgs(C.Structure):
    """include/bdl_exchange.h bdl_exchange_decide_args."""
    _fields_ = [("state", _fp), ("workspace", _fp), ("loss", _fp), ("beta", _fp),
                ("n", C.c_int64), ("n_data", C.c_double), ("sigma2", C.c_double),
                ("var", C.c_double), ("seed", C.c_uint64), ("chain0", C.c_uint64),
                ("attempt", C.c_uint64), ("chains", C.c_int32), ("flags", C.c_int32)]


class ExchangeSwapArgs(C.Structure):
    """include/bdl_exchange.h bdl_exchange_swap_args."""
    _fields_ = [("state", _fp), ("vectors", _fp * EXCHANGE_MAX_VECTORS),
                ("chain_groups", C.c_uint64), ("nvectors", C.c_int32), ("chains", C.c_int32),
                ("grid_blocks", C.c_int32), ("pad", C.c_int32)]


# include/bdl_exchange.h: additive to the ABI, as DIAG_EXPORTS
EXCHANGE_EXPORTS = {
    "bdl_exchange_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "bdl_exchange_energy": (C.c_int, [C.POINTER(ExchangeEnergyArgs), C.c_void_p]),
    "bdl_exchange_decide": (C.c_int, [C.POINTER(ExchangeDecideArgs), C.c_void_p]),
    "bdl_exchange_swap": (C.c_int, [C.POINTER(ExchangeSwapArgs), C.c_void_p]),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load libbdl_sgmcmc.so once; raise if it is missing (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"bayesdll_amd: HIP library not found at {LIB_PATH}; build it with "
                    "`make -C bayesdll_amd/csrc` (or __graft_entry__.build()). There is no CPU "
                    "fallback for the fused SG-MCMC step.")
            h = C.CDLL(LIB_PATH)
            for name, (res, argt) in (list(EXPORTS.items()) + list(DIAG_EXPORTS.items())
                                      + list(CLIP_EXPORTS.items())
                                      + list(CHAIN_STEP_EXPORTS.items())
                                      + list(STATS_EXPORTS.items())
                                      + list(ESS_EXPORTS.items())
                                      + list(LOWP_EXPORTS.items())
                                      + list(LAYERS_EXPORTS.items())
                                      + list(PREDICT_EXPORTS.items())
                                      + list(FN_EXPORTS.items())
                                      + list(TEMPER_EXPORTS.items())
                                      + list(MIXTURE_EXPORTS.items())
                                      + list(RANK_EXPORTS.items())
                                      + list(DIVERSITY_EXPORTS.items())
                                      + list(ORDER_EXPORTS.items())
                                      + list(STACK_EXPORTS.items())
                                      + list(EXCHANGE_EXPORTS.items())):
                fn = getattr(h, name)
                fn.restype = res
                fn.argtypes = argt
            if h.bdl_version() != ABI_VERSION:
                raise RuntimeError(f"bayesdll_amd: ABI version mismatch ({h.bdl_version()} != "
                                   f"{ABI_VERSION}); rebuild the library")
            _lib = h
    return _lib


def check(rc: int, what: str):
    if rc != BDL_OK:
        msg = lib().bdl_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")
    return rc


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream_handle(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_hip(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"bayesdll_amd: {what} must live on a HIP device (got {t.device}); "
                           "the fused SG-MCMC step has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"bayesdll_amd: {what} must be float32 (got {t.dtype})")
