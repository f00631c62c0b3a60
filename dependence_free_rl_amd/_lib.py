"""ctypes binding of the C ABI in include/xylo_hip.h (libxylo_hip.so).

The library is the product: there is no CPU fallback.  If the in-tree
``libxylo_hip.so`` is missing, importing this module raises immediately.
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# XH_LIB_PATH: diagnostic builds only (`make diag`, tools/ablate.sh)
LIB_PATH = os.environ.get("XH_LIB_PATH") or os.path.join(HERE, "libxylo_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "xylo_hip.h")

XH_OK, XH_ERR_INVALID, XH_ERR_HIP, XH_ERR_RCCL, XH_ERR_STATE = range(5)
XH_PPO, XH_AC, XH_KLPPO, XH_PG = 0, 1, 2, 3
HEURISTICS = {"random": 0, "firstfit": 1, "bestfit": 2, "minwaste": 3}
XH_POLICY, XH_VALUE = 0, 1
OPTIMIZERS = {"sgd": 0, "momentum": 1, "adam": 2}
(VENV_ACTIONS, VENV_REWARD, VENV_DONE, VENV_BINS, VENV_ITEMS, VENV_RNG,
 VENV_OBS, VENV_MASK, VENV_POLICY, VENV_PCHOICE) = range(10)
# xh_venv_act: what the policy rows hold, how the bin is chosen
ACT_PROBS, ACT_LOGITS = 0, 1
ACT_SAMPLE, ACT_ARGMAX = 0, 1
# the trajectory record's arrays (xh_venv_set_record)
(VREC_ACTION, VREC_PCHOICE, VREC_REWARD, VREC_DONE, VREC_BINS, VREC_ITEMS,
 VREC_COUNT) = range(7)
# xh_venv_record_obs: the state S_t, or the successor row of transition t
VOBS_STATE, VOBS_NEXT = 0, 1
# the statistics of xh_venv_policy_loss (the XH_VLOSS_* enum)
(VLOSS_ROWS, VLOSS_SKIPPED, VLOSS_LOGR_SUM, VLOSS_LOGR_SQSUM, VLOSS_K3_SUM,
 VLOSS_CLIPPED, VLOSS_SURR_SUM, VLOSS_ENTROPY_SUM, VLOSS_VERR_SUM,
 VLOSS_VERR_SQSUM, VLOSS_COUNT) = range(11)
# the exact-KL sums of xh_venv_policy_loss's kl_stats (the XH_VKL_* enum)
VKL_KL_SUM, VKL_ROWS, VKL_KL_SQSUM, VKL_COUNT = range(4)
# the sums of xh_venv_policy_loss_ex's ext_stats (the XH_VEXT_* enum)
(VEXT_ROWS, VEXT_ENTROPY_SUM, VEXT_VCLIP_ROWS, VEXT_VLOSS_SUM,
 VEXT_COUNT) = range(5)
# one row of the VecEnv's episode statistics (the XH_VEP_* enum;
# xh_venv_set_episode_stats) and its per-env state arrays (XH_VEPS_*)
(VEP_ROW, VEP_CALLS, VEP_EPISODES, VEP_LEN_SUM, VEP_LEN_SQSUM, VEP_LEN_MIN,
 VEP_LEN_MAX, VEP_ENVS_FINISHED, VEP_FIRST_LEN_SUM, VEP_FIRST_LEN_SQSUM,
 VEP_RUNNING_SUM, VEP_RUNNING_MAX, VEP_COUNT) = range(13)
VEPS_RUNNING, VEPS_FIRST, VEPS_COUNT = range(3)
COPY_H2D, COPY_D2H, COPY_D2D = 0, 1, 2
# device-resident nets (xh_net_*): the kinds and a net's arrays
NET_POLICY, NET_VALUE, NET_POLICY_LAYERS = 0, 1, 2
NET_PARAMS, NET_GRAD, NET_M, NET_V, NET_COUNT = range(5)
(BUF_BINS, BUF_ITEMS, BUF_ACTION, BUF_POLD, BUF_DONE, BUF_RNG, BUF_V_STATE,
 BUF_V_TERM, BUF_TARGETS, BUF_ADV, BUF_VALUE_GRAD, BUF_POLICY_GRADS,
 BUF_LOGITS, BUF_PROBS, BUF_V_STATE0, BUF_QOLD, BUF_KL, BUF_LEN) = range(18)
# one row of training statistics (the XH_STAT_* enum; xh_trainer_set_stats)
(STAT_ITER, STAT_TRANSITIONS, STAT_EPISODES, STAT_EPLEN_SUM, STAT_EPLEN_SQSUM,
 STAT_REWARD_SUM, STAT_NEGLOGP_SUM, STAT_VERR_SUM, STAT_VERR_SQSUM,
 STAT_TARGET_SUM, STAT_TARGET_SQSUM, STAT_ADV_SUM, STAT_ADV_SQSUM,
 STAT_PGRAD_SQ_FIRST, STAT_PGRAD_SQ_LAST, STAT_VGRAD_SQ, STAT_KL_BETA,
 STAT_KL_MEAN, STAT_PCLIP_STEPS, STAT_PCLIP_SCALE_MIN, STAT_VCLIP_SCALE,
 STAT_COUNT) = range(22)
# one row of PPO update diagnostics (the XH_UPD_* enum;
# xh_trainer_set_update_diag)
(UPD_LEARN, UPD_ROWS, UPD_LOGR_SUM, UPD_LOGR_SQSUM, UPD_K3_SUM, UPD_CLIPPED,
 UPD_SURR_SUM, UPD_ENTROPY_SUM, UPD_KL_SUM, UPD_COUNT) = range(10)
# trainer-state checkpoints (xh_trainer_save_state / load_state): the blob
# version, what a load restores (the XH_STATE_* enum) and the entries of
# xh_trainer_state_digest (the XH_DIG_* enum)
STATE_VERSION = 1
STATE_ALL, STATE_NETS = 0, 1
(DIG_POLICY_PARAMS, DIG_VALUE_PARAMS, DIG_POLICY_OPT_M, DIG_POLICY_OPT_V,
 DIG_VALUE_OPT_M, DIG_VALUE_OPT_V, DIG_ENV_BINS, DIG_ENV_ITEMS, DIG_RNG,
 DIG_KL_BETA, DIG_COUNT) = range(11)
STATE_HEADER_BYTES = 144


class XhError(RuntimeError):
    """A non-zero status from the C ABI (message from xh_last_error())."""


class Config(C.Structure):
    """Mirror of xh_config."""
    _fields_ = [
        ("algo", C.c_int), ("num_envs", C.c_int), ("num_envs_global", C.c_int),
        ("env_offset", C.c_int), ("bins", C.c_int), ("dims", C.c_int),
        ("steps", C.c_int), ("epochs", C.c_int), ("policy_h1", C.c_int),
        ("policy_h2", C.c_int), ("value_h1", C.c_int), ("value_h2", C.c_int),
        ("lr_policy", C.c_float), ("lr_value", C.c_float),
        ("wd_policy", C.c_float), ("wd_value", C.c_float), ("gamma", C.c_float),
        ("lambda_", C.c_float), ("clip_eps", C.c_float),
        ("rng_state", C.c_uint32), ("kl_beta", C.c_float),
        ("kl_target", C.c_float), ("adv_normalize", C.c_int),
        ("lr_scale_rows", C.c_int), ("train_grid_cap", C.c_int),
        ("record_distrib", C.c_int), ("record_last_step", C.c_int)]


class Eval(C.Structure):
    """Mirror of xh_eval."""
    _fields_ = [
        ("n_envs", C.c_int), ("episodes", C.c_int), ("argmax_probs", C.c_int),
        ("rng_state", C.c_uint32), ("init_items", C.c_void_p),
        ("final_items", C.c_void_p), ("rng_out", C.c_void_p),
        ("totals", C.c_void_p), ("steps", C.c_void_p), ("trace", C.c_void_p),
        ("trace_cap", C.c_long), ("elapsed_ms", C.c_double)]


class VenvAdv(C.Structure):
    """Mirror of xh_venv_adv."""
    _fields_ = [
        ("steps", C.c_int), ("values", C.c_void_p), ("v_term", C.c_void_p),
        ("reward", C.c_void_p), ("done", C.c_void_p), ("gamma", C.c_float),
        ("lambda_", C.c_float), ("normalize", C.c_int), ("adv", C.c_void_p),
        ("td_target", C.c_void_p), ("lambda_return", C.c_void_p),
        ("stats", C.c_void_p)]


class VenvLoss(C.Structure):
    """Mirror of xh_venv_loss."""
    _fields_ = [
        ("policy", C.c_void_p), ("kind", C.c_int), ("loss", C.c_int),
        ("rows_dev", C.c_void_p), ("first", C.c_long), ("count", C.c_long),
        ("adv", C.c_void_p), ("action", C.c_void_p), ("p_old", C.c_void_p),
        ("total", C.c_long), ("eps", C.c_float), ("scale", C.c_float),
        ("values_new", C.c_void_p), ("target", C.c_void_p),
        ("value_scale", C.c_float), ("grad", C.c_void_p),
        ("dvalue", C.c_void_p), ("probs_out", C.c_void_p),
        ("stats", C.c_void_p), ("accumulate", C.c_int),
        ("distrib", C.c_void_p), ("beta", C.c_float),
        ("beta_dev", C.c_void_p), ("kl_stats", C.c_void_p)]


class VenvLossExt(C.Structure):
    """Mirror of xh_venv_loss_ext."""
    _fields_ = [
        ("masked", C.c_int), ("legal_dev", C.c_void_p),
        ("ent_coef", C.c_float), ("ent_coef_dev", C.c_void_p),
        ("v_old", C.c_void_p), ("vclip", C.c_float),
        ("ext_stats", C.c_void_p)]


ITEMS_MAX = 16


class ItemSet(C.Structure):
    """Mirror of xh_item_set."""
    _fields_ = [
        ("num_items", C.c_int), ("capacity", C.c_int * 4),
        ("item", (C.c_int * 4) * ITEMS_MAX),
        ("weight", C.c_double * ITEMS_MAX)]


VTAB_MAX_ENTRIES = 16384


class VenvTableInfo(C.Structure):
    """Mirror of struct xh_venv_table_info."""
    _fields_ = [
        ("entries", C.c_int), ("states", C.c_int), ("items", C.c_int),
        ("rows", C.c_int), ("side", C.c_int * 4)]


# calls an A/B library from before them (XH_LIB_PATH) may lack; the wrappers
# that need one raise
_AB_OPTIONAL = ("xh_trainer_table_stats", "xh_trainer_pack_read",
                "xh_item_set_default",
                "xh_item_set_thresholds", "xh_venv_create_ex",
                "xh_venv_set_item_set", "xh_venv_get_item_set",
                "xh_net_create", "xh_net_destroy", "xh_net_num_params",
                "xh_net_get", "xh_net_set", "xh_net_device_ptr",
                "xh_net_get_step", "xh_net_set_step", "xh_net_forward",
                "xh_net_backward", "xh_net_set_optimizer", "xh_net_step",
                "xh_net_set_grid_cap", "xh_net_info",
                "xh_net_forward_record", "xh_net_backward_record",
                "xh_item_set_table_info", "xh_venv_table_info",
                "xh_venv_table_obs", "xh_venv_act_table",
                "xh_venv_table_gather", "xh_venv_table_grad")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libxylo_hip.so not built (%s); run `make lib` or "
            "__graft_entry__.build() -- there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    sig = {
        "xh_last_error": (C.c_char_p, []),
        "xh_version": (C.c_char_p, []),
        "xh_struct_size": (sz, [C.c_char_p]),
        "xh_device_count": (i, [C.POINTER(C.c_int)]),
        "xh_runtime_info": (i, [C.c_char_p, sz]),
        "xh_comm_unique_id": (i, [vp]),
        "xh_ctx_create": (i, [i, i, i, vp, C.POINTER(vp)]),
        "xh_ctx_destroy": (i, [vp]),
        "xh_ctx_synchronize": (i, [vp]),
        "xh_ctx_allreduce_host": (i, [vp, vp, sz]),
        "xh_config_default": (None, [C.POINTER(Config), i, i, i, i, i]),
        "xh_trainer_create": (i, [vp, C.POINTER(Config), C.POINTER(vp)]),
        "xh_trainer_destroy": (i, [vp]),
        "xh_trainer_num_params": (sz, [vp, i]),
        "xh_trainer_set_params": (i, [vp, i, vp, sz]),
        "xh_trainer_get_params": (i, [vp, i, vp, sz]),
        "xh_trainer_set_optimizer": (i, [vp, i, i, C.c_float, C.c_float,
                                         C.c_float, C.c_float]),
        "xh_trainer_set_learning_rate": (i, [vp, i, C.c_float]),
        "xh_trainer_rollout": (i, [vp]),
        "xh_trainer_learn": (i, [vp]),
        "xh_trainer_iterate": (i, [vp, i]),
        "xh_trainer_set_forced_actions": (i, [vp, vp]),
        "xh_trainer_buffer_bytes": (sz, [vp, i]),
        "xh_trainer_get_buffer": (i, [vp, i, vp, sz]),
        "xh_trainer_set_buffer": (i, [vp, i, vp, sz]),
        "xh_trainer_evaluate": (i, [vp, C.POINTER(Eval)]),
        "xh_trainer_seed_streams": (i, [vp, C.c_uint32]),
        "xh_heuristic_evaluate": (i, [vp, i, i, i, C.POINTER(Eval)]),
        "xh_trainer_set_timing": (i, [vp, i]),
        "xh_trainer_kernel_time": (i, [vp, C.c_char_p, C.POINTER(C.c_double),
                                       C.POINTER(C.c_long)]),
        "xh_trainer_reset_timing": (i, [vp]),
        "xh_trainer_kernel_info": (i, [vp, C.c_char_p, sz]),
        "xh_trainer_pack_stats": (i, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long),
                                      C.POINTER(C.c_long)]),
        "xh_trainer_table_stats": (i, [vp, C.POINTER(C.c_int), C.POINTER(C.c_long),
                                       C.POINTER(C.c_long)]),
        "xh_trainer_pack_read": (i, [vp, C.POINTER(C.c_int), vp, sz]),
        "xh_ctx_inject_fault": (i, [vp, i]),
        "xh_trainer_get_env_state": (i, [vp, i, i, vp, vp]),
        "xh_trainer_set_env_state": (i, [vp, i, i, vp, vp]),
        "xh_venv_create": (i, [vp, i, i, i, C.c_uint32, i, i, i,
                               C.POINTER(vp)]),
        "xh_item_set_default": (None, [C.POINTER(ItemSet), i]),
        "xh_item_set_thresholds": (i, [C.POINTER(ItemSet), i,
                                       C.POINTER(C.c_double)]),
        "xh_venv_create_ex": (i, [vp, i, i, i, C.c_uint32, i, i, i,
                                  C.POINTER(ItemSet), C.POINTER(vp)]),
        "xh_venv_set_item_set": (i, [vp, C.POINTER(ItemSet)]),
        "xh_venv_get_item_set": (i, [vp, C.POINTER(ItemSet)]),
        "xh_venv_destroy": (i, [vp]),
        "xh_venv_bytes": (sz, [vp, i]),
        "xh_venv_device_ptr": (vp, [vp, i]),
        "xh_venv_get": (i, [vp, i, vp, sz]),
        "xh_venv_set": (i, [vp, i, vp, sz]),
        "xh_venv_step": (i, [vp, i]),
        "xh_venv_act": (i, [vp, vp, i, i, i]),
        "xh_venv_act_heuristic": (i, [vp, i, i]),
        "xh_item_set_table_info": (i, [C.POINTER(ItemSet), i, i,
                                       C.POINTER(VenvTableInfo)]),
        "xh_venv_table_info": (i, [vp, C.POINTER(VenvTableInfo)]),
        "xh_venv_table_obs": (i, [vp, vp]),
        "xh_venv_act_table": (i, [vp, vp, i, i]),
        "xh_venv_table_gather": (i, [vp, vp, vp, C.c_long, C.c_long, vp]),
        "xh_venv_table_grad": (i, [vp, vp, C.c_long, C.c_long, vp, vp, i]),
        "xh_venv_set_record": (i, [vp, i, i]),
        "xh_venv_record_pos": (i, [vp, C.POINTER(C.c_int)]),
        "xh_venv_record_rewind": (i, [vp]),
        "xh_venv_record_bytes": (sz, [vp, i]),
        "xh_venv_record_ptr": (vp, [vp, i]),
        "xh_venv_get_record": (i, [vp, i, vp, sz]),
        "xh_venv_set_record_distrib": (i, [vp, i]),
        "xh_venv_record_distrib_bytes": (sz, [vp]),
        "xh_venv_record_distrib_ptr": (vp, [vp]),
        "xh_venv_get_record_distrib": (i, [vp, vp, sz]),
        "xh_venv_legal_words": (i, [vp]),
        "xh_venv_set_action_mask": (i, [vp, i]),
        "xh_venv_legal": (i, [vp, vp]),
        "xh_venv_legal_ptr": (vp, [vp]),
        "xh_venv_record_legal_bytes": (sz, [vp]),
        "xh_venv_record_legal_ptr": (vp, [vp]),
        "xh_venv_get_record_legal": (i, [vp, vp, sz]),
        "xh_venv_policy_loss_masked": (i, [vp, C.POINTER(VenvLoss), vp]),
        "xh_venv_policy_loss_ex": (i, [vp, C.POINTER(VenvLoss),
                                       C.POINTER(VenvLossExt)]),
        "xh_venv_kl_beta": (i, [vp, vp, C.c_float, vp, vp]),
        "xh_venv_record_obs": (i, [vp, i, vp, C.c_long, C.c_long, vp]),
        "xh_venv_record_ends": (i, [vp, vp, vp]),
        "xh_venv_advantages": (i, [vp, C.POINTER(VenvAdv)]),
        "xh_venv_policy_loss": (i, [vp, C.POINTER(VenvLoss)]),
        "xh_venv_apply": (i, [vp, i]),
        "xh_venv_reset": (i, [vp, i]),
        "xh_venv_observe": (i, [vp]),
        "xh_venv_synchronize": (i, [vp]),
        "xh_venv_set_timing": (i, [vp, i]),
        "xh_venv_kernel_time": (i, [vp, C.POINTER(C.c_double),
                                    C.POINTER(C.c_long)]),
        "xh_venv_set_episode_stats": (i, [vp, i]),
        "xh_venv_episode_row": (i, [vp]),
        "xh_venv_episode_count": (i, [vp, C.POINTER(C.c_long)]),
        "xh_venv_get_episode_rows": (i, [vp, C.c_long, i, vp]),
        "xh_venv_episode_bytes": (sz, [vp, i]),
        "xh_venv_episode_ptr": (vp, [vp, i]),
        "xh_venv_episode_get": (i, [vp, i, vp, sz]),
        "xh_venv_episode_set": (i, [vp, i, vp, sz]),
        "xh_model_eval": (i, [vp, vp, i, vp, sz, vp, i, i, vp, sz,
                              C.POINTER(C.c_int)]),
        "xh_model_forward": (i, [vp, vp, i, vp, sz, vp, i, i, vp, sz,
                                 C.POINTER(C.c_int)]),
        "xh_model_gradient": (i, [vp, vp, i, vp, sz, vp, i, i, vp, i, vp]),
        "xh_layer_backward": (i, [vp, vp, vp, sz, vp, i, i, vp, i, vp]),
        "xh_layer_gradient": (i, [vp, vp, vp, i, i, vp, i, vp, sz]),
        "xh_action_loss_grad": (i, [vp, i, i, i, vp, vp, vp, vp, C.c_float,
                                    vp]),
        "xh_optimizer_apply": (i, [vp, i, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_float, vp, vp, vp, vp, sz]),
        "xh_trainer_set_grad_clip": (i, [vp, i, C.c_float]),
        "xh_trainer_get_grad_clip_log": (i, [vp, i, vp, i,
                                             C.POINTER(C.c_int)]),
        "xh_clip_grad_norm": (i, [vp, vp, sz, C.c_float,
                                  C.POINTER(C.c_double),
                                  C.POINTER(C.c_float)]),
        "xh_trainer_forget": (i, [vp]),
        "xh_net_create": (i, [vp, i, i, i, i, i, C.POINTER(vp)]),
        "xh_net_destroy": (i, [vp]),
        "xh_net_num_params": (sz, [vp]),
        "xh_net_get": (i, [vp, i, vp, sz]),
        "xh_net_set": (i, [vp, i, vp, sz]),
        "xh_net_device_ptr": (vp, [vp, i]),
        "xh_net_get_step": (i, [vp, C.POINTER(C.c_long)]),
        "xh_net_set_step": (i, [vp, C.c_long]),
        "xh_net_forward": (i, [vp, vp, C.c_long, vp]),
        "xh_net_backward": (i, [vp, vp, C.c_long, vp, i]),
        "xh_net_set_optimizer": (i, [vp, i, C.c_float, C.c_float, C.c_float,
                                     C.c_float]),
        "xh_net_step": (i, [vp, C.c_float, vp]),
        "xh_net_set_grid_cap": (i, [vp, i]),
        "xh_net_info": (i, [vp, C.c_char_p, sz]),
        "xh_net_forward_record": (i, [vp, vp, i, vp, C.c_long, C.c_long, vp]),
        "xh_net_backward_record": (i, [vp, vp, i, vp, C.c_long, C.c_long, vp,
                                       i]),
        "xh_trainer_set_record_last_step": (i, [vp, i]),
        "xh_trainer_set_stats": (i, [vp, i]),
        "xh_trainer_stats_count": (i, [vp, C.POINTER(C.c_long)]),
        "xh_trainer_get_stats": (i, [vp, C.c_long, i, vp]),
        "xh_trainer_set_update_diag": (i, [vp, i, i]),
        "xh_trainer_update_diag_count": (i, [vp, C.POINTER(C.c_long)]),
        "xh_trainer_get_update_diag": (i, [vp, C.c_long, i, vp]),
        "xh_trainer_get_update_diag_rows": (i, [vp, vp, vp, vp, sz]),
        "xh_trainer_update_diag_info": (i, [vp, C.c_char_p, sz]),
        "xh_tensor_reduce": (i, [vp, i, vp, vp, C.c_float, sz, i,
                                 C.POINTER(C.c_double),
                                 C.POINTER(C.c_int64)]),
        "xh_trainer_state_bytes": (sz, [vp]),
        "xh_trainer_save_state": (i, [vp, vp, sz, C.POINTER(sz)]),
        "xh_trainer_load_state": (i, [vp, vp, sz, i]),
        "xh_state_describe": (i, [vp, sz, C.c_char_p, sz]),
        "xh_trainer_state_digest": (i, [vp, C.POINTER(C.c_uint64)]),
        "xh_digest_host": (i, [vp, sz, C.POINTER(C.c_uint64)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name, None)
        if f is None and name in _AB_OPTIONAL and os.environ.get("XH_LIB_PATH"):
            continue  # an A/B library from before the call
        if f is None:
            raise AttributeError("%s: no symbol %s" % (lib._name, name))
        f.restype = res
        f.argtypes = args
    return lib


class Layer(C.Structure):
    """Mirror of xh_layer."""
    _fields_ = [("kind", C.c_int), ("inp", C.c_int), ("out", C.c_int)]


LAYER_FULL, LAYER_CONV1D_1, LAYER_RELU, LAYER_SOFTMAX, LAYER_SOFTMAX_XENT = range(5)
(LOSS_GRADIENT_LOG, LOSS_SOFTMAX_GRADIENT_LOG, LOSS_CLIPPED,
 LOSS_KL_REGULATED) = range(4)

lib = _load()
# device scratch of the VecEnv (venv.py): prototypes of their own, so a caller
# that sets argtypes on lib.xh_tensor_* for its own use does not change them
tensor_alloc = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t,
                           C.POINTER(C.c_void_p))(("xh_tensor_alloc", lib))
tensor_free = C.CFUNCTYPE(C.c_int, C.c_void_p,
                          C.c_void_p)(("xh_tensor_free", lib))
tensor_copy = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_size_t, C.c_int)(("xh_tensor_copy", lib))
for _name, _mirror in (("xh_config", Config), ("xh_eval", Eval),
                       ("xh_layer", Layer), ("xh_venv_adv", VenvAdv),
                       ("xh_venv_loss", VenvLoss),
                       ("xh_venv_loss_ext", VenvLossExt),
                       ("xh_item_set", ItemSet),
                       ("xh_venv_table_info", VenvTableInfo)):
    if _name == "xh_item_set" and not hasattr(lib, "xh_venv_create_ex"):
        continue  # an A/B library from before item sets
    if _name == "xh_venv_table_info" and not hasattr(lib, "xh_venv_act_table"):
        continue  # an A/B library from before logit tables
    if lib.xh_struct_size(_name.encode()) != C.sizeof(_mirror):
        raise ImportError("ctypes mirror of %s is out of date (%d vs %d bytes)"
                          % (_name, C.sizeof(_mirror),
                             lib.xh_struct_size(_name.encode())))
if lib.xh_struct_size(b"xh_stat_row") != STAT_COUNT * 8:
    raise ImportError("STAT_* indices are out of date (%d entries, the library "
                      "has %d)" % (STAT_COUNT,
                                   lib.xh_struct_size(b"xh_stat_row") // 8))
if lib.xh_struct_size(b"xh_upd_row") != UPD_COUNT * 8:
    raise ImportError("UPD_* indices are out of date (%d entries, the library "
                      "has %d)" % (UPD_COUNT,
                                   lib.xh_struct_size(b"xh_upd_row") // 8))
if lib.xh_struct_size(b"xh_vep_row") != VEP_COUNT * 8:
    raise ImportError("VEP_* indices are out of date (%d entries, the library "
                      "has %d)" % (VEP_COUNT,
                                   lib.xh_struct_size(b"xh_vep_row") // 8))
if lib.xh_struct_size(b"xh_state_header") != STATE_HEADER_BYTES:
    raise ImportError("the state blob's header has %d bytes in the library, %d "
                      "here" % (lib.xh_struct_size(b"xh_state_header"),
                                STATE_HEADER_BYTES))


def check(status):
    if status != XH_OK:
        raise XhError("xylo-hip status %d: %s" % (
            status, lib.xh_last_error().decode(errors="replace")))
    return status


def runtime_info():
    """The HIP / RCCL shared objects this process bound (xh_runtime_info)."""
    import json
    buf = C.create_string_buffer(4096)
    check(lib.xh_runtime_info(buf, len(buf)))
    return json.loads(buf.value.decode())


def device_count():
    n = C.c_int()
    check(lib.xh_device_count(C.byref(n)))
    return n.value


def header_symbols():
    """Function names declared by include/xylo_hip.h (for the ABI test)."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(xh_[a-z0-9_]+)\s*\(", text)))
