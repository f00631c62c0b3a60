"""Host reference of the VecEnv's invalid-action masking (xh_venv_set_action_
mask, xh_venv_legal, xh_venv_policy_loss_masked).  CPU only, numpy only.

Bin b takes the item iff bins[b][d] >= item[d] for every d < D (bp::
environment::apply leaves the bin non-negative; any other pick is game over).
legal(e) is that set; eff(e) is legal(e) where it is not empty, else all B
bins.  premask replaces the entries of a row outside eff by -inf (logits) or
+0.0f (probs); the masked calls do bit for bit what the unmasked ones do on the
premasked rows.  The packing: W = max(1, B / 32) uint32 words per env, bit b %
32 of word b / 32 is bin b."""
import numpy as np

f32 = np.float32


def words_per_env(B):
    return max(1, B // 32)


def legal_ref(bins, items):
    """bins int [..][B][D], items int [..][>= D] (the first D entries count)
    -> bool [..][B]."""
    bins = np.asarray(bins).astype(np.int32)
    D = bins.shape[-1]
    items = np.asarray(items).astype(np.int32)[..., :D]
    return (bins >= items[..., None, :]).all(axis=-1)


def eff(legal):
    """legal where the row has a legal bin, else every bin."""
    legal = np.asarray(legal, bool)
    return legal | ~legal.any(axis=-1, keepdims=True)


def pack(legal):
    """bool [..][B] -> uint32 [..][W], one bit at a time."""
    legal = np.asarray(legal, bool)
    B = legal.shape[-1]
    out = np.zeros(legal.shape[:-1] + (words_per_env(B),), np.uint32)
    for b in range(B):
        out[..., b // 32] |= legal[..., b].astype(np.uint32) << np.uint32(b % 32)
    return out


def unpack(words, B):
    words = np.asarray(words, np.uint32)
    out = np.zeros(words.shape[:-1] + (B,), bool)
    for b in range(B):
        out[..., b] = (words[..., b // 32] >> np.uint32(b % 32)) & 1
    return out


def premask(rows, eff_set, kind):
    """rows f32 [..][B] with the entries outside eff_set replaced: -inf under
    "logits", +0.0f under "probs"."""
    rows = np.array(rows, f32)
    fill = f32(-np.inf) if kind == "logits" else f32(0.0)
    rows[~np.asarray(eff_set, bool)] = fill
    return rows


# ------------------------------------------------- the episode-count case --
# B = 8, D = 2: items (4,2) / (1,2) at capacity 8, so a bin takes at most 4
# items and an episode of legal picks lasts at most 32 steps: T = 48 contains
# ends under masking too.
EP_B, EP_D, EP_N, EP_T, EP_X0 = 8, 2, 64, 48, 20261


def episode_counts(act_ref_cls, masked):
    """ActRef on uniform rows (premasked where `masked`) for EP_T steps.
    Returns done uint8 [T][N] and legal bool [T][N][B] of the states before
    each step."""
    ref = act_ref_cls(EP_B, EP_D, EP_N, EP_X0)
    uniform = np.full((EP_N, EP_B), 1.0 / EP_B, f32)
    done, legal = [], []
    for _ in range(EP_T):
        lg = legal_ref(ref.bins(), ref.items())
        rows = premask(uniform, eff(lg), "probs") if masked else uniform
        done.append(ref.act(rows)["done"])
        legal.append(lg)
    return np.stack(done), np.stack(legal)
