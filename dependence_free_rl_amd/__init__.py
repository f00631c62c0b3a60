"""dependence_free_rl_amd -- MI355X-native PPO / actor-critic rollout-and-update
path for vectorised bin packing (drop-in for beehover/dependence_free_rl's
xylo::rl / xylo::policy_gradient hot path).  See DESIGN.md."""
from ._lib import (XhError, device_count, lib,  # noqa: F401  (fails loudly
                   runtime_info)                 # if not built)
from ._lib import (STAT_ADV_SQSUM, STAT_ADV_SUM, STAT_COUNT,  # noqa: F401
                   STAT_EPISODES, STAT_EPLEN_SQSUM, STAT_EPLEN_SUM, STAT_ITER,
                   STAT_KL_BETA, STAT_KL_MEAN, STAT_NEGLOGP_SUM,
                   STAT_PCLIP_SCALE_MIN, STAT_PCLIP_STEPS,
                   STAT_PGRAD_SQ_FIRST, STAT_PGRAD_SQ_LAST, STAT_REWARD_SUM,
                   STAT_TARGET_SQSUM, STAT_TARGET_SUM, STAT_TRANSITIONS,
                   STAT_VCLIP_SCALE, STAT_VERR_SQSUM, STAT_VERR_SUM,
                   STAT_VGRAD_SQ)
from ._lib import (UPD_CLIPPED, UPD_COUNT, UPD_ENTROPY_SUM,  # noqa: F401
                   UPD_K3_SUM, UPD_KL_SUM, UPD_LEARN, UPD_LOGR_SQSUM,
                   UPD_LOGR_SUM, UPD_ROWS, UPD_SURR_SUM)
from ._lib import (DIG_COUNT, DIG_ENV_BINS, DIG_ENV_ITEMS,  # noqa: F401
                   DIG_KL_BETA, DIG_POLICY_OPT_M, DIG_POLICY_OPT_V,
                   DIG_POLICY_PARAMS, DIG_RNG, DIG_VALUE_OPT_M,
                   DIG_VALUE_OPT_V, DIG_VALUE_PARAMS, STATE_ALL, STATE_NETS,
                   STATE_VERSION)
from .trainer import (ALGOS, POLICY, VALUE, Context, Trainer,  # noqa: F401
                      clip_grad_norm, describe_state, digest,
                      heuristic_evaluate, init_full_policy,
                      init_policy, init_value,
                      policy_param_count, value_param_count)
from ._lib import (ACT_ARGMAX, ACT_LOGITS, ACT_PROBS, ACT_SAMPLE,  # noqa: F401
                   VENV_PCHOICE, VENV_POLICY, VOBS_NEXT, VOBS_STATE, VREC_ACTION, VREC_BINS,
                   VREC_COUNT, VREC_DONE, VREC_ITEMS, VREC_PCHOICE,
                   VREC_REWARD)
from ._lib import (VLOSS_CLIPPED, VLOSS_COUNT, VLOSS_ENTROPY_SUM,  # noqa: F401
                   VLOSS_K3_SUM, VLOSS_LOGR_SQSUM, VLOSS_LOGR_SUM, VLOSS_ROWS,
                   VLOSS_SKIPPED, VLOSS_SURR_SUM, VLOSS_VERR_SQSUM,
                   VLOSS_VERR_SUM)
from ._lib import (VKL_COUNT, VKL_KL_SQSUM, VKL_KL_SUM,  # noqa: F401
                   VKL_ROWS)
from ._lib import (VEXT_COUNT, VEXT_ENTROPY_SUM, VEXT_ROWS,  # noqa: F401
                   VEXT_VCLIP_ROWS, VEXT_VLOSS_SUM)
from ._lib import (VEP_CALLS, VEP_COUNT, VEP_ENVS_FINISHED,  # noqa: F401
                   VEP_EPISODES, VEP_FIRST_LEN_SQSUM, VEP_FIRST_LEN_SUM,
                   VEP_LEN_MAX, VEP_LEN_MIN, VEP_LEN_SQSUM, VEP_LEN_SUM,
                   VEP_ROW, VEP_RUNNING_MAX, VEP_RUNNING_SUM, VEPS_COUNT,
                   VEPS_FIRST, VEPS_RUNNING)
from ._lib import VTAB_MAX_ENTRIES, VenvTableInfo  # noqa: F401
from .venv import (VecEnv, heuristic_baseline,  # noqa: F401
                   item_set_table_info, item_set_thresholds, legal_words,
                   pack_legal, unpack_legal)
from ._lib import (NET_GRAD, NET_M, NET_PARAMS, NET_POLICY,  # noqa: F401
                   NET_POLICY_LAYERS, NET_V, NET_VALUE)
from .nets import PolicyNet, ValueNet  # noqa: F401

__all__ = ["Context", "Trainer", "POLICY", "VALUE", "init_policy", "init_value",
           "init_full_policy", "clip_grad_norm", "describe_state", "digest",
           "heuristic_evaluate", "XhError", "runtime_info", "device_count", "VecEnv",
           "item_set_thresholds", "heuristic_baseline", "PolicyNet",
           "ValueNet", "item_set_table_info", "VenvTableInfo",
           "VTAB_MAX_ENTRIES"]
