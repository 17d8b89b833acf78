"""ctypes binding of libgmmvi_hip.so (C ABI: include/gmmvi_hip.h).

The product path has no CPU fallback: if the shared library is missing, or a call fails, this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GMMVI_HIP_LIB", os.path.join(_HERE, "libgmmvi_hip.so"))    # override: experiments only

GAUSS, STUDENT_T = 0, 1
SELF_NORMALIZED, OWN_SAMPLES_ONLY, EXPLICIT_ESTIMATE = 1, 2, 4
MAX_DIM = 64
MORE_REGISTER_MAX_DIM = 21     # gmmvi_more: register-resident ridge system up to here, the tiled route above (D <= 63)
MORE_BLOCKED_MIN_DIM, MORE_BLOCKED_MAX_DIM = 64, 128   # gmmvi_more_blocked: MORE from the blocked component layout
MORE_DIAG_MAX_DIM = 1024       # gmmvi_more_diag: MORE for diagonal-covariance mixtures (F = 2 D + 1 features)
MAX_DIM_BLOCKED = 512          # dense [K, D, D] factors (blocked kernels) exist up to here
CUSTOM_STAGED_MAX_DIM = 120    # gmmvi_target_custom: the staged (LDS) route up to here, the direct route above
CUSTOM_AUTODIFF_TANGENTS = 16  # GMMVI_CUSTOM_AUTODIFF_TANGENTS: tangents per pass of a differentiated user-defined target
CUSTOM_AUTODIFF_MAX_DIM = 512  # gradient calls through a differentiated target stop here (the largest full-covariance D)
CUSTOM_TAPE_RECORD_BYTES = 20       # GMMVI_CUSTOM_TAPE_RECORD_BYTES: scratch per lane and record of a tape-mode gradient call
CUSTOM_TAPE_DEFAULT_CAPACITY = 1024 # GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY: records per lane of a handle's first gradient launch
CUSTOM_TAPE_SCRATCH_BYTES = 1 << 31 # GMMVI_CUSTOM_TAPE_SCRATCH_BYTES: default budget of the tape scratch
MAX_DIM_DIAG = 131072          # diagonal-covariance mixtures: csrc/diag_sweep.hip, csrc/diag.hip
BLOCKED_ABOVE_DEFAULT = 50     # csrc/blocked.h: D > 50 runs the blocked (MFMA) kernels


_blocked_above = None


def _atoi(text):
    """C atoi: optional sign and leading digits, anything else ends the number (no digits: 0)."""
    import re
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


def blocked_above():
    """Dimensions above this take the blocked (MFMA) path.  Mirrors csrc/blocked.h gmmvi_blocked_above(): the environment
    knob GMMVI_BLOCKED_ABOVE is read ONCE per process (the library keeps it in a static), parsed as atoi does, clamped to
    16..64."""
    global _blocked_above
    if _blocked_above is None:
        raw = os.environ.get("GMMVI_BLOCKED_ABOVE")
        t = BLOCKED_ABOVE_DEFAULT if raw is None else _atoi(raw)
        _blocked_above = min(max(t, 16), MAX_DIM)
    return _blocked_above


class GmmviError(RuntimeError):
    pass


_lib = None

_p = C.c_void_p
_i = C.c_int
_f = C.c_float
_sz = C.c_size_t
_u64 = C.c_uint64
_u32 = C.c_uint32

MLP_MAX_LAYERS = 4             # gmmvi_mlp_desc: dense layers of the generic BNN (csrc/bnn_mlp.hip)
MLP_ACTIVATIONS = {"linear": 0, "sigmoid": 1, "relu": 2, "tanh": 3}
MLP_LOSSES = {"mse": 0, "sparse_categorical_crossentropy": 1}


class MlpDesc(C.Structure):
    """gmmvi_mlp_desc (include/gmmvi_hip.h)."""
    _fields_ = [("n_layers", C.c_int32), ("widths", C.c_int32 * (MLP_MAX_LAYERS + 1)),
                ("activations", C.c_int32 * MLP_MAX_LAYERS), ("loss", C.c_int32)]


_i32 = C.c_int32


class TargetSpec(C.Structure):
    """gmmvi_target_spec: what a built-in target's ``_fast_path_target()`` returns; only the members of ``kind`` are set.
    The device arrays behind the pointers belong to the target object, which outlives every plan that copies its spec."""
    _fields_ = [("kind", _i32), ("mix_family", _i32), ("mix_K", _i32), ("mix_nu", _f), ("mix_packed", _p), ("mix_logw", _p),
                ("planar_prior_std", _p), ("planar_goals", _p), ("planar_goals_count", _i32), ("planar_likelihood_std", _f),
                ("logreg_A", _p), ("logreg_M", _i32), ("logreg_prior_mean", _f), ("logreg_prior_std", _f),
                ("talos_model", _p), ("talos_context", _p), ("custom", _p), ("custom_params", _p)]


class StepsizeRule(C.Structure):
    """gmmvi_stepsize_rule."""
    _fields_ = [("mode", _i32), ("min", _f), ("max", _f), ("inc", _f), ("dec", _f)]


def stepsize_rule(src, improvement_based=True):
    """The rule of an adapter object or of its config dict: both name the four numbers alike."""
    if not improvement_based:
        return StepsizeRule(0)
    get = src.__getitem__ if isinstance(src, dict) else lambda name: getattr(src, name)
    return StepsizeRule(1, get("min_stepsize"), get("max_stepsize"), get("stepsize_inc_factor"), get("stepsize_dec_factor"))


class SamtronPlan(C.Structure):
    """gmmvi_samtron_plan."""
    _fields_ = [
        ("K", _i32), ("D", _i32), ("N", _i32), ("target", TargetSpec),
        ("means", _p), ("chols", _p), ("logw", _p), ("packed", _p), ("packed_new", _p),
        ("stepsizes", _p), ("last_eta", _p), ("l2", _p), ("num_updates", _p), ("success_out", _p),
        ("offsets", _p), ("max_per_component", _i32), ("n_old", _i32), ("bg_K", _i32), ("bg_packed", _p), ("bg_logw", _p),
        ("bg_old", _p), ("bg_logw_new", _p), ("bg_log_share_old", _f), ("bg_log_share_new", _f),
        ("seed", _u64), ("first_index", _u64),
        ("db_samples", _p), ("db_tlp", _p), ("db_tgrad", _p), ("db_mapping", _p), ("mapping_base", _i32),
        ("db_means", _p), ("db_chols", _p), ("db_packed", _p),
        ("reward_prev", _p), ("reward_last", _p), ("reward_next", _p), ("weight_slot", _p), ("wstate", _p),
        ("temperature", _f), ("l2_init", _f), ("component_stepsize", StepsizeRule), ("weight_stepsize", StepsizeRule),
        ("weight_update_mode", _i32), ("stein_flags", _i32), ("presample_next", _i32), ("presampled", _i32), ("phase", _i32),
    ]


class ShardedPlan(C.Structure):
    """gmmvi_sharded_plan."""
    _fields_ = [
        ("n_ranks", _i32), ("rank", _i32), ("K", _i32), ("D", _i32), ("N", _i32), ("target", TargetSpec),
        ("means", _p), ("chols", _p), ("packed", _p), ("packed_new", _p),
        ("stepsizes", _p), ("last_eta", _p), ("l2", _p), ("num_updates", _p), ("success_out", _p),
        ("logw_all", _p), ("bg_logw", _p), ("offsets", _p), ("max_per_component", _i32),
        ("seed", _u64), ("first_index", _u64),
        ("e1", _p), ("e2", _p), ("e3", _p),
        ("x_all", _p), ("tlp_all", _p), ("tgrad_all", _p), ("E_all", _p), ("reward_all", _p),
        ("has_pending", _i32), ("reward_col_pending", _p), ("reward_prev", _p), ("reward_last", _p), ("reward_last_all", _p),
        ("wstate", _p), ("temperature", _f), ("l2_init", _f),
        ("component_stepsize", StepsizeRule), ("weight_stepsize", StepsizeRule),
        ("stein_flags", _i32), ("presample_next", _i32), ("presampled", _i32), ("scratch", _p),
    ]


_PROTOS = {
    "gmmvi_device_count": (_i, []),
    "gmmvi_ctx_create": (_i, [C.POINTER(_p), _i]),
    "gmmvi_ctx_destroy": (None, [_p]),
    "gmmvi_last_error": (C.c_char_p, [_p]),
    "gmmvi_sync": (_i, [_p]),
    "gmmvi_num_cus": (_i, [_p]),
    "gmmvi_malloc": (_i, [_p, _sz, C.POINTER(_p)]),
    "gmmvi_free": (_i, [_p, _p]),
    "gmmvi_upload": (_i, [_p, _p, _p, _sz]),
    "gmmvi_download": (_i, [_p, _p, _p, _sz]),
    "gmmvi_copy": (_i, [_p, _p, _p, _sz]),
    "gmmvi_fill_f32": (_i, [_p, _p, _f, _sz]),
    "gmmvi_gather_rows": (_i, [_p, _p, _p, _i, _i, _p]),
    "gmmvi_exp_f32": (_i, [_p, _p, _p, _sz]),
    "gmmvi_logaddexp_f32": (_i, [_p, _p, _p, _f, _p, _f, _sz]),
    "gmmvi_segment_lse_f32": (_i, [_p, _i, _p, _p, _p, _i, _p, _sz, _i]),
    "gmmvi_copy_2d_f32": (_i, [_p, _p, _sz, _p, _sz, _i, _i]),
    "gmmvi_copy_batch": (_i, [_p, _i, C.POINTER(_p), C.POINTER(_p), C.POINTER(_sz)]),
    "gmmvi_normalize_logw": (_i, [_p, _p, _i, _p]),
    "gmmvi_add_heuristic_argmax": (_i, [_p, _p, _p, _i, C.c_double, _p]),
    "gmmvi_unpack_gathered": (_i, [_p, _p, _i, _sz, _i, C.POINTER(_sz), C.POINTER(_p)]),
    "gmmvi_fill_strided_f32": (_i, [_p, _p, _sz, _sz, _f]),
    "gmmvi_remove_column_f32": (_i, [_p, _p, _i, _sz, _i, _i]),
    "gmmvi_add_scalar_i32": (_i, [_p, _p, _p, C.c_int32, _sz]),
    "gmmvi_event_create": (_i, [_p, C.POINTER(_p)]),
    "gmmvi_event_destroy": (_i, [_p, _p]),
    "gmmvi_event_record": (_i, [_p, _p]),
    "gmmvi_event_synchronize": (_i, [_p, _p]),
    "gmmvi_host_alloc": (_i, [_p, _sz, C.POINTER(_p)]),
    "gmmvi_vmm_reserve": (_i, [_p, _sz, C.POINTER(_p), C.POINTER(_sz)]),
    "gmmvi_vmm_grow": (_i, [_p, _p, _sz, _sz, _sz]),
    "gmmvi_vmm_release": (_i, [_p, _p, _sz, _sz, _sz]),
    "gmmvi_host_free": (_i, [_p, _p]),
    "gmmvi_download_async": (_i, [_p, _p, _p, _sz]),
    "gmmvi_event_elapsed_ms": (_i, [_p, _p, _p, C.POINTER(_f)]),
    "gmmvi_profile_enable": (_i, [_p, _i]),
    "gmmvi_profile_report": (_i, [_p, C.c_char_p, _sz]),
    "gmmvi_packed_stride": (_sz, [_i]),
    "gmmvi_pack_components": (_i, [_p, _i, _f, _i, _i, _p, _p, _p, _p]),
    "gmmvi_cholesky": (_i, [_p, _i, _i, _p, _p, _p]),
    "gmmvi_mixture_eval": (_i, [_p, _i, _f, _i, _i, _p, _p, _p, _i, _p, _p, _p]),
    "gmmvi_mixture_eval_dual": (_i, [_p, _i, _f, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "gmmvi_target_planar": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p]),
    "gmmvi_target_logreg": (_i, [_p, _i, _i, _p, _f, _f, _p, _i, _p, _p]),
    "gmmvi_target_logreg_mb": (_i, [_p, _i, _i, _p, _i, _i, _u64, _u32, _f, _f, _p, _i, _p, _p]),
    "gmmvi_target_bnn": (_i, [_p, _i, _i, _i, _i, _p, _p, _u64, _u32, _i, _f, _f, _p, _i, _p, _p]),
    "gmmvi_bnn_predict": (_i, [_p, _i, _i, _i, _p, _i, _p, _i, _p]),
    "gmmvi_target_bnn_classifier": (_i, [_p, _i, _i, _i, _i, _p, _p, _u64, _u32, _i, _f, _f, _p, _i, _p, _p]),
    "gmmvi_bnn_classifier_predict": (_i, [_p, _i, _i, _i, _p, _i, _p, _i, _p]),
    "gmmvi_target_mlp": (_i, [_p, C.POINTER(MlpDesc), _i, _p, _p, _u64, _u32, _i, _f, _f, _p, _i, _p, _p]),
    "gmmvi_mlp_predict": (_i, [_p, C.POINTER(MlpDesc), _p, _i, _p, _i, _p]),
    "gmmvi_target_talos": (_i, [_p, _p, _p, _p, _i, _p, _p]),
    "gmmvi_talos_fk": (_i, [_p, _p, _p, _i, _p, _p]),
    "gmmvi_custom_target_check": (_i, [C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    "gmmvi_custom_target_compile": (_i, [_p, C.c_char_p, C.POINTER(_p)]),
    "gmmvi_custom_target_release": (_i, [_p, _p]),
    "gmmvi_target_custom": (_i, [_p, _p, _i, _p, _p, _i, _p, _p, _i]),
    "gmmvi_custom_target_check_autodiff": (_i, [C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    "gmmvi_custom_target_compile_autodiff": (_i, [_p, C.c_char_p, C.POINTER(_p)]),
    "gmmvi_autodiff_probe": (_i, [_i, _f, _f, _f, _f, C.POINTER(_f), C.POINTER(_f)]),
    "gmmvi_autodiff_probe_special": (_i, [_i, _f, _f, _f, _f, C.POINTER(_f), C.POINTER(_f)]),
    "gmmvi_autodiff_probe_extra": (_i, [_i, _f, _f, C.POINTER(_f), C.POINTER(_f)]),
    "gmmvi_autodiff_probe_vector": (_i, [_i, _p, _i, _i, _i, _p, _f, _i, C.POINTER(_f), _p]),
    "gmmvi_autodiff_probe_nodes": (_i, [_i, _p, _i, _i, _i, _i, _i, _i, C.POINTER(_f), _p]),
    "gmmvi_autodiff_probe_nodes_inputs": (_i, [_i, _p, _i, _i, _i, _i, _i, C.POINTER(_f), _p]),
    "gmmvi_autodiff_probe_affine": (_i, [_p] + [_i] * 14 + [_p, C.POINTER(_f), _p]),
    "gmmvi_custom_target_check_data": (_i, [C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    "gmmvi_custom_target_compile_data": (_i, [_p, C.c_char_p, C.POINTER(_p)]),
    "gmmvi_custom_data_plan": (_i, [_i, C.c_int64, _i, C.POINTER(_i), C.POINTER(_i)]),
    "gmmvi_target_custom_data": (_i, [_p, _p, _i, _p, _p, C.c_int64, _i, _i, C.c_int64, _u64, _u32, _p, _i, _p, _p, _i]),
    "gmmvi_target_custom_data_own_batches": (_i, [_p, _p, _i, _p, _p, C.c_int64, _i, C.c_int64, _u64, _u32, _p, _i, _p, _p, _i]),
    "gmmvi_custom_target_check_tape": (_i, [C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    "gmmvi_custom_target_compile_tape": (_i, [_p, C.c_char_p, C.POINTER(_p)]),
    "gmmvi_custom_tape_plan": (_i, [_i, _i, _sz, C.POINTER(_i), C.POINTER(_i)]),
    "gmmvi_custom_tape_length": (_i, [_p, _p, _i, C.POINTER(_i)]),
    "gmmvi_target_custom_tape": (_i, [_p, _p, _i, _p, _p, _i, _p, _p, _i, _sz]),
    "gmmvi_tape_probe": (_i, [_i, _f, _f, _i, _i, C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "gmmvi_tape_probe_special": (_i, [_i, _f, _f, _i, _i, C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "gmmvi_tape_probe_extra": (_i, [_i, _f, _i, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "gmmvi_tape_probe_vector": (_i, [_i, _p, _i, _i, _i, _p, _f, C.POINTER(_f), _p, C.POINTER(_i)]),
    "gmmvi_tape_probe_nodes": (_i, [_i, _p, _i, _i, _i, _i, _i, C.POINTER(_f), _p, C.POINTER(_i)]),
    "gmmvi_tape_probe_nodes_inputs": (_i, [_i, _p, _i, _i, _i, _i, C.POINTER(_f), _p, C.POINTER(_i)]),
    "gmmvi_tape_probe_affine": (_i, [_p] + [_i] * 13 + [_p, C.POINTER(_f), _p, C.POINTER(_i)]),
    "gmmvi_custom_target_check_data_tape": (_i, [C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    "gmmvi_custom_target_compile_data_tape": (_i, [_p, C.c_char_p, C.POINTER(_p)]),
    "gmmvi_custom_data_tape_plan": (_i, [_i, C.c_int64, _i, _i, _i, _sz, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "gmmvi_target_custom_data_tape": (_i, [_p, _p, _i, _p, _p, C.c_int64, _i, _i, C.c_int64, _u64, _u32, _p, _i, _p, _p, _i, _i, _sz]),
    "gmmvi_target_custom_data_tape_own_batches": (_i, [_p, _p, _i, _p, _p, C.c_int64, _i, C.c_int64, _u64, _u32, _p, _i, _p, _p, _i, _i,
                                                       _sz]),
    "gmmvi_data_tape_probe": (_i, [_i, _p, _p, C.c_int64, _i, _i, C.c_int64, _u64, _u32, _p, _i, _i, _i, _i, _p, _p, C.POINTER(_i)]),
    "gmmvi_custom_data_predictive_plan": (_i, [_i, C.c_int64, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_int64)]),
    "gmmvi_custom_data_predictive": (_i, [_p, _p, _i, _p, _p, C.c_int64, _i, _p, _i, _p, _p, _p, _i]),
    "gmmvi_custom_data_predictive_probe": (_i, [_p, _i, C.c_int64, _i, _p, _p, _p]),
    "gmmvi_sample_components": (_i, [_p, _i, _i, _p, _p, _p, _i, _u64, _u64, _i, _p, _p, _p]),
    "gmmvi_philox_normals": (_i, [_p, _u64, _u64, _i, _i, _i, _p]),
    "gmmvi_philox_uniforms": (_i, [_p, _u64, _u64, _i, _i, _p]),
    "gmmvi_stein": (_i, [_p, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "gmmvi_more": (_i, [_p, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p]),
    "gmmvi_more_blocked": (_i, [_p, _i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p]),
    "gmmvi_more_diag": (_i, [_p, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p]),
    "gmmvi_update_components_kl": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p, _p]),
    "gmmvi_stein_update_kl": (_i, [_p, _i, _i, _p, _p, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p,
                                   C.POINTER(C.c_int32)]),
    "gmmvi_update_components_kl_reference": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p]),
    "gmmvi_update_components_direct": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p]),
    "gmmvi_update_components_iblr": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p]),
    "gmmvi_expected_log_ratios": (_i, [_p, _i, _i, _p, _p, _p, _p, _f, _p, _i, _p, _p, _p]),
    "gmmvi_expected_log_ratios_parts": (_i, [_p, _i, _i, _p, _p, _p, _p, _i, _f, _p, _i, _p, _p, _p]),
    "gmmvi_update_weights_kl": (_i, [_p, _i, _p, _p, _p, _f, _p]),
    "gmmvi_update_weights_direct": (_i, [_p, _i, _p, _p, _p, _f]),
    "gmmvi_component_stepsize_improvement": (_i, [_p, _i, _p, _p, _p, _f, _f, _f, _f]),
    "gmmvi_weight_stepsize_improvement": (_i, [_p, _i, _p, _p, _p, _f, _f, _f, _f]),
    "gmmvi_struct_bytes": (_sz, [_i]),
    "gmmvi_train_iter_samtron": (_i, [_p, C.POINTER(SamtronPlan)]),
    "gmmvi_sharded_scratch_floats": (_sz, [_i, _i, _i]),
    "gmmvi_train_iter_sharded_phase": (_i, [_p, C.POINTER(ShardedPlan), _i]),
    "gmmvi_comm_unique_id": (_i, [C.c_char_p]),
    "gmmvi_comm_init": (_i, [_p, C.c_char_p, _i, _i]),
    "gmmvi_comm_destroy": (_i, [_p]),
    "gmmvi_allgather_f32": (_i, [_p, _p, _p, _sz]),
    "gmmvi_allreduce_f32": (_i, [_p, _p, _sz, _i]),
    "gmmvi_combine_partials": (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    "gmmvi_diag_packed_stride": (_sz, [_i]),
    "gmmvi_diag_pack": (_i, [_p, _i, _i, _p, _p, _p]),
    "gmmvi_diag_mixture_eval": (_i, [_p, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "gmmvi_diag_sample": (_i, [_p, _i, _i, _p, _p, _p, _i, _u64, _u64, _i, _p, _p, _p]),
    "gmmvi_diag_stein": (_i, [_p, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p]),
    "gmmvi_diag_embed": (_i, [_p, _i, _i, _p, _p]),
    "gmmvi_diag_extract": (_i, [_p, _i, _i, _p, _p]),
    "gmmvi_reciprocal_f32": (_i, [_p, _p, _sz, _p]),
    "gmmvi_update_components_diag_kl": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p]),
    "gmmvi_update_components_diag_iblr": (_i, [_p, _i, _i, _p, _p, _p, _p, _p, _f, _p, _p, _p]),
    "gmmvi_mmd_scratch_doubles": (_sz, [_i, _i]),
    "gmmvi_mmd_pair_sum": (_i, [_p, _p, _i, _p, _i, _i, _p, _p, _p]),
}

EXPORTED_SYMBOLS = tuple(_PROTOS.keys())


def _autodiff_ops():
    """The operations of gmmvi_autodiff_probe in index order (csrc/autodiff_probe.hip).  ``_tf`` / ``_ft``: the second / the
    first operand is a float; ``_assign``: the compound form; a trailing ``f``: the f-suffixed spelling of a function."""
    ops = []
    for name in ("add", "sub", "mul", "div"):
        ops += [name, name + "_tf", name + "_ft", name + "_assign", name + "_assign_tf"]
    ops.append("neg")
    for name in ("lt", "le", "gt", "ge", "eq", "ne"):
        ops += [name, name + "_tf", name + "_ft"]
    for name in ("exp", "expm1", "log", "log1p", "sqrt", "rsqrt", "sin", "cos", "tan", "tanh", "atan", "fabs"):
        ops += [name, name + "f"]
    for name in ("fmax", "fmin", "pow"):
        ops += [name, name + "_tf", name + "_ft", name + "f", name + "f_tf", name + "f_ft"]
    ops.append("value")
    return tuple(ops)


AUTODIFF_OPS = _autodiff_ops()

# The operations of gmmvi_autodiff_probe_special and gmmvi_tape_probe_special in index order (csrc/autodiff_probe.hip): the special
# functions of user-defined targets.  A trailing ``f``: the f-suffixed spelling (lgamma has none on a number: lgammaf stays
# ROCm's float function); the library's own functions go by their names
# without ``gmmvi_``; ``_tf`` / ``_ft``: the second / the first operand is a float; ``trigamma`` is a float function only (a
# constant: no tangent, no record).
SPECIAL_OPS = ("lgamma", "erf", "erff", "erfc", "erfcf", "digamma", "sigmoid", "softplus", "log_sigmoid",
               "logaddexp", "logaddexp_tf", "logaddexp_ft", "trigamma")

# The operations of gmmvi_autodiff_probe_extra and gmmvi_tape_probe_extra in index order: the one-operand functions that came
# after SPECIAL_OPS, which stays as it is.  gmmvi_erfcx, gmmvi_ndtr and gmmvi_log_ndtr go by their names without ``gmmvi_``.
EXTRA_OPS = ("erfcx", "ndtr", "log_ndtr", "sinh", "sinhf", "cosh", "coshf", "asin", "asinf", "acos", "acosf")

# The operations of gmmvi_autodiff_probe_vector and gmmvi_tape_probe_vector in index order: the vector primitives on the input
# view (csrc/custom_target_vector.inc), by their names without ``gmmvi_``.  The index is also the kind of the tape's vector record.
VECTOR_OPS = ("dot", "sqdist", "sumsq")
# The operations of gmmvi_autodiff_probe_nodes and gmmvi_tape_probe_nodes in index order: the primitives on arrays of the mode's
# number type (gmmvi_wdot, gmmvi_logsumexp).  The index is also what the header of the tape's node-array record carries.
NODE_OPS = ("wdot", "logsumexp")


def load():
    """Load the shared library (once).  Raises GmmviError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GmmviError(
            f"{LIB_PATH} not found: build it with `make -C gmmvi_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback for the gmmvi hot path.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_count():
    return int(load().gmmvi_device_count())


def check(ctx_handle, rc):
    if rc != 0:
        msg = load().gmmvi_last_error(ctx_handle)
        raise GmmviError(f"libgmmvi_hip error {rc}: {msg.decode() if msg else '?'}")
