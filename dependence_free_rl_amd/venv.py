"""Vectorised bin-packing environments for a caller's own policy (xh_venv_*).

    env = VecEnv(ctx, num_envs=32768, bins=64, dims=2, rng_state=7,
                 policy_draws=2)
    obs = env.observe()                 # [N][B][2D] float32
    env.set_actions(actions)            # int32 [N]
    reward, done = env.step()           # agent::step minus react, all envs

or, sampling the caller's policy rows on the device (react + agent::step in
one launch, recording the trajectory):

    env.set_record(steps=T)
    for t in range(T):
        rows = my_policy(env.observe())                 # [N][B] float32
        actions, pchoice, reward, done = env.act(rows)  # or a device pointer
    batch = env.record()                # action / pchoice / reward / done /
                                        # bins / items, [T][N]...

Invalid-action masking is opt-in: env.set_action_mask(True) makes act() mask
each row by the env's legal bins (record()["legal"] keeps the sets),
policy_loss(..., legal=True) masks the minibatch the same way, and env.legal()
returns the current states' sets.  So are PPO's two usual extras:
policy_loss(..., ent_coef=c) adds the entropy bonus's gradient to every row
and policy_loss(..., v_old=..., vclip=...) clips the value loss
(xh_venv_policy_loss_ex).  And episode statistics: after
env.set_episode_stats(rows) the step() / act() / apply() launches count every
env's episode lengths on the device, env.episode_row() appends one row of sums
to a device ring, and env.episode_stats() / episode_curve() /
first_episode_lengths() read them back.

The problem instance is the reference's (two items, capacity 8) unless the
VecEnv is given its own: VecEnv(..., items=[(3, 1), (2, 2), (1, 4)],
weights=[2, 1, 1], capacity=(5, 7)) draws from up to 16 shapes with per-dim
capacities, from the same stream positions, and env.set_item_set(items,
weights) switches the mix during training (a curriculum).

A baseline on the same instance: env.act_heuristic("firstfit") -- or "random",
"bestfit", "minwaste", the reference's heuristic agents -- is an act() whose
pick is the heuristic's, in one launch, and heuristic_baseline(ctx, kind, ...)
plays every env's first episode with it and returns the lengths' statistics.

Mirrors xylo::environment<A,S>::apply / view / reset (rl.h:163-170) with the
id ranging over the batch, bp::environment (bin_packing.h:46-85) and
xylo::agent::step (rl.h:325-349).  State lives in HBM; numpy arrays here are
host copies.  `device_ptr(which)` exposes the device buffers for a policy
kernel of the caller's own on the same device.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ACT_ARGMAX, ACT_LOGITS, ACT_PROBS, ACT_SAMPLE, VENV_ACTIONS,
                   VENV_BINS, VENV_DONE, VENV_ITEMS, VENV_MASK, VENV_OBS,
                   VENV_PCHOICE, VENV_POLICY, VENV_REWARD, VENV_RNG,
                   VOBS_NEXT, VOBS_STATE, VREC_ACTION, VREC_BINS, VREC_DONE,
                   VREC_ITEMS, VREC_PCHOICE, VREC_REWARD, check)

_KINDS = {"probs": ACT_PROBS, "logits": ACT_LOGITS}
_MODES = {"sample": ACT_SAMPLE, "argmax": ACT_ARGMAX}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def legal_words(B):
    """W: uint32 words per env of a packed legal set (xh_venv_legal_words)."""
    return max(1, B // 32)


def pack_legal(legal):
    """bool [..][B] -> uint32 [..][W]: bit b % 32 of word b // 32 is bin b."""
    legal = np.asarray(legal, bool)
    B = legal.shape[-1]
    W = legal_words(B)
    bits = legal.reshape(legal.shape[:-1] + (W, B // W)).astype(np.uint32)
    shifts = np.arange(B // W, dtype=np.uint32)
    return (bits << shifts).sum(-1, dtype=np.uint32)


def unpack_legal(words, B):
    """uint32 [..][W] -> bool [..][B], pack_legal's inverse."""
    words = np.asarray(words, np.uint32)
    W = legal_words(B)
    shifts = np.arange(B // W, dtype=np.uint32)
    bits = (words[..., None] >> shifts) & np.uint32(1)
    return bits.reshape(words.shape[:-1] + (B,)).astype(bool)


def _beta_ptr(beta, name="beta"):
    """The device address in `beta`, or None where it is a value.  An integer
    is an address (as everywhere in this class), so a small one is a mistake:
    beta = 1 is written 1.0.  ent_coef follows the same rule (`name`)."""
    if isinstance(beta, bool) or not isinstance(beta, (int, np.integer)):
        return None
    if int(beta) < 4096:
        raise ValueError("%s: a float, or an integer device pointer to one "
                         "(got the integer %d; write it as a float)"
                         % (name, beta))
    return int(beta)


def _item_set(items, weights, capacity, dims):
    """An _lib.ItemSet of `items` ([K][dims] ints), `weights` ([K], default
    uniform) and `capacity` ([dims] or one int, default 8).  Shapes only are
    checked here; the library checks the values."""
    it = np.asarray(items)
    if it.ndim == 1 and dims == 1:
        it = it.reshape(-1, 1)
    if it.ndim != 2 or it.shape[1] != dims:
        raise ValueError("items: shape %s, expected [K][%d]" % (it.shape, dims))
    K = it.shape[0]
    if not 1 <= K <= _lib.ITEMS_MAX:
        raise ValueError("items: %d items (1..%d)" % (K, _lib.ITEMS_MAX))
    if not np.all(it == np.floor(it)):
        raise ValueError("items: the shapes are integers")
    w = np.ones(K) if weights is None else np.asarray(weights, np.float64)
    if w.shape != (K,):
        raise ValueError("weights: shape %s, expected (%d,)" % (w.shape, K))
    cap = np.broadcast_to(np.asarray(8 if capacity is None else capacity),
                          (dims,))
    s = _lib.ItemSet()
    s.num_items = K
    for d in range(dims):
        s.capacity[d] = int(cap[d])
    for k in range(K):
        for d in range(dims):
            s.item[k][d] = int(it[k, d])
        s.weight[k] = float(w[k])
    return s


def _item_set_dict(s, dims):
    K = s.num_items
    th = (C.c_double * _lib.ITEMS_MAX)()
    check(_lib.lib.xh_item_set_thresholds(C.byref(s), dims, th))
    return {"items": np.array([[s.item[k][d] for d in range(dims)]
                               for k in range(K)], np.int32),
            "weights": np.array([s.weight[k] for k in range(K)], np.float64),
            "capacity": np.array([s.capacity[d] for d in range(dims)],
                                 np.int32),
            "thresholds": np.array(th[:K], np.float64)}


def item_set_thresholds(items, weights=None, capacity=None):
    """The K thresholds c_k of the item draw (xh_item_set_thresholds; host
    only): the item is the first k with u < c_k, u the env's canonical draw.
    float64 [K]; the last one is exactly 1.0."""
    it = np.asarray(items)
    dims = 1 if it.ndim == 1 else it.shape[1]
    return _item_set_dict(_item_set(items, weights, capacity, dims),
                          dims)["thresholds"]


def _table_info_dict(ti, dims):
    return {"entries": ti.entries, "states": ti.states, "items": ti.items,
            "rows": ti.rows,
            "side": np.array(ti.side[:dims], np.int32)}


def item_set_table_info(items, weights=None, capacity=None, bins=64):
    """The logit-table domain of an item set on `bins` bins
    (xh_item_set_table_info; host only): a dict of entries E = K *
    prod(capacity[d] + 1), states, items K, rows R = ceil(E / bins) and side
    int32 [D].  XhError for an invalid set and for E above
    VTAB_MAX_ENTRIES."""
    it = np.asarray(items)
    dims = 1 if it.ndim == 1 else it.shape[1]
    s = _item_set(items, weights, capacity, dims)
    ti = _lib.VenvTableInfo()
    check(_lib.lib.xh_item_set_table_info(C.byref(s), dims, bins,
                                          C.byref(ti)))
    return _table_info_dict(ti, dims)


class VecEnv:
    """xh_venv: N envs of B bins x D dims stepped by one kernel per call."""

    def __init__(self, ctx, num_envs, bins=64, dims=2, rng_state=1,
                 env_offset=0, num_envs_global=None, policy_draws=2, *,
                 items=None, weights=None, capacity=None):
        """items None: the reference's instance (xh_venv_create).  Otherwise
        the venv's own (xh_venv_create_ex): items [K][dims] ints, K <= 16,
        weights [K] (default uniform), capacity [dims] or one int (default
        8)."""
        self.ctx = ctx
        self.N, self.B, self.D = num_envs, bins, dims
        self.h = C.c_void_p()
        self._dev = {}  # device scratch: name -> (address, bytes)
        self._ep_history = 0  # the episode ring's rows (set_episode_stats)
        if items is None:
            if weights is not None or capacity is not None:
                raise ValueError("VecEnv: weights and capacity go with items")
            check(_lib.lib.xh_venv_create(
                ctx.h, num_envs, bins, dims, rng_state, env_offset,
                num_envs_global or num_envs, policy_draws, C.byref(self.h)))
        else:
            s = _item_set(items, weights, capacity, dims)
            check(_lib.lib.xh_venv_create_ex(
                ctx.h, num_envs, bins, dims, rng_state, env_offset,
                num_envs_global or num_envs, policy_draws, C.byref(s),
                C.byref(self.h)))

    # ---- the problem instance ---------------------------------------------
    def set_item_set(self, items, weights=None):
        """Switch the item mix (xh_venv_set_item_set), e.g. the next stage of
        a curriculum: ordered on the stream, in effect from the next draw; the
        items the envs hold stay and no stream position moves.  The capacity
        stays the venv's."""
        cap = self.item_set()["capacity"]
        s = _item_set(items, weights, cap, self.D)
        check(_lib.lib.xh_venv_set_item_set(self.h, C.byref(s)))

    def item_set(self):
        """The set in use (xh_venv_get_item_set) as a dict: items int32
        [K][D], weights float64 [K], capacity int32 [D] and thresholds float64
        [K] (item_set_thresholds)."""
        s = _lib.ItemSet()
        check(_lib.lib.xh_venv_get_item_set(self.h, C.byref(s)))
        return _item_set_dict(s, self.D)

    def _spec(self, which):
        N, B, D = self.N, self.B, self.D
        return {VENV_ACTIONS: (np.int32, (N,)), VENV_REWARD: (np.float32, (N,)),
                VENV_DONE: (np.uint8, (N,)), VENV_BINS: (np.int8, (N, B, D)),
                VENV_ITEMS: (np.int8, (N, 4)), VENV_RNG: (np.uint32, (N,)),
                VENV_OBS: (np.float32, (N, B, 2 * D)),
                VENV_MASK: (np.uint8, (N,)),
                VENV_POLICY: (np.float32, (N, B)),
                VENV_PCHOICE: (np.float32, (N,))}[which]

    def get(self, which):
        dt, shape = self._spec(which)
        out = np.zeros(shape, dt)
        check(_lib.lib.xh_venv_get(self.h, which, _ptr(out), out.nbytes))
        return out

    def set(self, which, arr):
        dt, shape = self._spec(which)
        a = np.ascontiguousarray(arr, dt).reshape(shape)
        check(_lib.lib.xh_venv_set(self.h, which, _ptr(a), a.nbytes))

    def device_ptr(self, which):
        return _lib.lib.xh_venv_device_ptr(self.h, which)

    # ---- environment<A,S> / agent<A,S> ---------------------------------
    def set_actions(self, actions):
        self.set(VENV_ACTIONS, actions)

    def step(self, write_obs=False, fetch=True):
        """agent::step minus react for every env; (reward, done) if fetch."""
        check(_lib.lib.xh_venv_step(self.h, 1 if write_obs else 0))
        if fetch:
            return self.get(VENV_REWARD), self.get(VENV_DONE)
        return None

    def act(self, policy=None, kind="probs", mode="sample", write_obs=False,
            fetch=True):
        """react + agent::step for every env in one launch (xh_venv_act):
        pick a bin from each env's policy row, then step with it.

        policy: a host array [N][B] (uploaded into VENV_POLICY), an integer
        device pointer to N * B floats, or None (VENV_POLICY as it stands).
        kind "probs" | "logits"; mode "sample" (discrete_distribution, two
        draws; needs policy_draws == 2) | "argmax" (first maximum, no draws).
        Returns (actions, pchoice, reward, done) if fetch."""
        ptr = None
        if isinstance(policy, (int, np.integer)):
            ptr = C.c_void_p(int(policy))
        elif policy is not None:
            self.set(VENV_POLICY, policy)
        check(_lib.lib.xh_venv_act(self.h, ptr, _KINDS[kind], _MODES[mode],
                                   1 if write_obs else 0))
        if fetch:
            return (self.get(VENV_ACTIONS), self.get(VENV_PCHOICE),
                    self.get(VENV_REWARD), self.get(VENV_DONE))
        return None

    def act_heuristic(self, kind, write_obs=False, fetch=False):
        """One of the reference's heuristic agents as the act of every env, in
        one launch (xh_venv_act_heuristic): kind "random" | "firstfit" |
        "bestfit" | "minwaste", scored on the venv's own item set and
        capacities; then everything act() does after its pick (the record, the
        mask's words, the episode statistics, OBS if write_obs).  "random"
        needs policy_draws == 2; the others draw nothing.  Returns (actions,
        pchoice, reward, done) if fetch."""
        if kind not in _lib.HEURISTICS:
            raise ValueError("act_heuristic: kind %r (one of %s)"
                             % (kind, ", ".join(sorted(_lib.HEURISTICS))))
        check(_lib.lib.xh_venv_act_heuristic(self.h, _lib.HEURISTICS[kind],
                                             1 if write_obs else 0))
        if fetch:
            return (self.get(VENV_ACTIONS), self.get(VENV_PCHOICE),
                    self.get(VENV_REWARD), self.get(VENV_DONE))
        return None

    # ---- invalid-action masking ------------------------------------------
    def set_action_mask(self, on):
        """Invalid-action masking for act() (xh_venv_set_action_mask): every
        entry of an env's row outside its legal set -- the bins that take the
        item; all bins where none does -- is replaced by -inf (logits) or 0
        (probs) before the pick, and the record keeps the sets ("legal" of
        record(), legal=True of policy_loss()).  Off at creation; with a
        record, turn it on at cursor 0."""
        check(_lib.lib.xh_venv_set_action_mask(self.h, 1 if on else 0))

    def legal(self, packed=False, out=None):
        """The legal set of every env's current state (xh_venv_legal; all
        bins where nothing fits), with the mask on or off: bool [N][B], or the
        uint32 [N][W] words when packed.  out: an integer device pointer that
        receives the words (nothing is returned)."""
        W = legal_words(self.B)
        if out is not None:
            check(_lib.lib.xh_venv_legal(self.h, int(out)))
            return None
        ptr = _lib.lib.xh_venv_legal_ptr(self.h)
        if not ptr:
            check(_lib.XH_ERR_HIP)
        check(_lib.lib.xh_venv_legal(self.h, None))
        words = self._download(ptr, np.uint32, (self.N, W))
        return words if packed else unpack_legal(words, self.B)

    # ---- the trajectory record act() writes -----------------------------
    def set_record(self, steps, states=True, distrib=False):
        """Record the next `steps` act() calls (xh_venv_set_record); 0 turns
        the record off and frees it.  distrib: also record the distribution
        every pick is made from (xh_venv_set_record_distrib), which the "kl"
        loss and want_kl of policy_loss() read."""
        check(_lib.lib.xh_venv_set_record(self.h, int(steps),
                                          1 if states else 0))
        if distrib and steps:
            check(_lib.lib.xh_venv_set_record_distrib(self.h, 1))

    def record_pos(self):
        pos = C.c_int()
        check(_lib.lib.xh_venv_record_pos(self.h, C.byref(pos)))
        return pos.value

    def record(self):
        """The recorded slots [0, cursor) as a dict: action int32 [t][N],
        pchoice / reward float32 [t][N], done uint8 [t][N] and, if recorded,
        the states before each step: bins int8 [t][N][B][D], items int8
        [t][N][4]; and, only while the distribution record is on, distrib
        float32 [t][N][B]; and, only while the action mask is on, legal bool
        [t][N][B], the sets each slot's act() masked with."""
        N, B, D = self.N, self.B, self.D
        spec = {"action": (VREC_ACTION, np.int32, (N,)),
                "pchoice": (VREC_PCHOICE, np.float32, (N,)),
                "reward": (VREC_REWARD, np.float32, (N,)),
                "done": (VREC_DONE, np.uint8, (N,)),
                "bins": (VREC_BINS, np.int8, (N, B, D)),
                "items": (VREC_ITEMS, np.int8, (N, 4))}
        pos, out = self.record_pos(), {}
        for name, (which, dt, shape) in spec.items():
            nbytes = _lib.lib.xh_venv_record_bytes(self.h, which)
            if not nbytes:
                continue
            a = np.zeros(nbytes // np.dtype(dt).itemsize, dt)
            check(_lib.lib.xh_venv_get_record(self.h, which, _ptr(a), nbytes))
            out[name] = a.reshape((-1,) + shape)[:pos]
        nbytes = _lib.lib.xh_venv_record_distrib_bytes(self.h)
        if nbytes:
            a = np.zeros(nbytes // 4, np.float32)
            check(_lib.lib.xh_venv_get_record_distrib(self.h, _ptr(a), nbytes))
            out["distrib"] = a.reshape(-1, N, B)[:pos]
        nbytes = _lib.lib.xh_venv_record_legal_bytes(self.h)
        if nbytes:
            a = np.zeros(nbytes // 4, np.uint32)
            check(_lib.lib.xh_venv_get_record_legal(self.h, _ptr(a), nbytes))
            out["legal"] = unpack_legal(
                a.reshape(-1, N, legal_words(B))[:pos], B)
        return out

    def rewind(self):
        """The next act() writes slot 0 again (xh_venv_record_rewind)."""
        check(_lib.lib.xh_venv_record_rewind(self.h))

    # ---- from the record to the learner's minibatches, on the device ------
    def _scratch(self, name, nbytes):
        """A device block of at least nbytes (xh_tensor_alloc) kept under
        `name` until close(); grown by reallocation."""
        have = self._dev.get(name)
        if have and have[1] >= nbytes:
            return have[0]
        if have:
            check(_lib.tensor_free(self.ctx.h, have[0]))
            del self._dev[name]
        p = C.c_void_p()
        n = (max(nbytes, 16) + 3) // 4
        check(_lib.tensor_alloc(self.ctx.h, n, C.byref(p)))
        self._dev[name] = (p.value, 4 * n)
        return p.value

    def _upload(self, ptr, a):
        raw = np.zeros((a.nbytes + 3) // 4 * 4, np.uint8)
        raw[:a.nbytes] = a.reshape(-1).view(np.uint8)
        check(_lib.tensor_copy(self.ctx.h, ptr, _ptr(raw), raw.size // 4,
                               _lib.COPY_H2D))

    def _download(self, ptr, dtype, shape):
        out = np.zeros(shape, dtype)
        raw = np.zeros((out.nbytes + 3) // 4 * 4, np.uint8)
        if raw.size:
            check(_lib.tensor_copy(self.ctx.h, _ptr(raw), ptr, raw.size // 4,
                                   _lib.COPY_D2H))
        out.reshape(-1).view(np.uint8)[:] = raw[:out.nbytes]
        return out

    def _staged(self, name, arr, dtype, shape):
        """The device address of `arr`: an integer is one already, a host
        array is uploaded into the scratch block `name`."""
        if arr is None:
            return None
        if isinstance(arr, (int, np.integer)):
            return int(arr)
        a = np.ascontiguousarray(arr, dtype)
        if a.shape != shape:
            raise ValueError("%s: shape %s, expected %s" % (name, a.shape,
                                                            shape))
        ptr = self._scratch(name, a.nbytes)
        self._upload(ptr, a)
        return ptr

    def _record_rows(self, who, view, rows, first, count):
        """(view id, device address of the index list or None, count) of the
        view / rows / first / count arguments record_obs documents."""
        view_id = {"state": VOBS_STATE, "next": VOBS_NEXT}[view]
        rows_ptr = None
        if rows is None:
            if count is None:
                P = self.record_pos()
                count = (P + 1 if view_id == VOBS_STATE else P) * self.N - first
        elif isinstance(rows, (int, np.integer)):
            if count is None:
                raise ValueError("%s: count is needed with a device "
                                 "pointer to the rows" % who)
            rows_ptr = int(rows)
        else:
            r = np.ascontiguousarray(rows, np.int32).reshape(-1)
            if count is None:
                count = r.size - first
            if first < 0 or count < 0 or first + count > r.size:
                raise ValueError("%s: rows %d .. %d of a list of %d"
                                 % (who, first, first + count - 1, r.size))
            rows_ptr = self._scratch("rows", r.nbytes)
            self._upload(rows_ptr, r)
        return view_id, rows_ptr, count

    def record_obs(self, view="state", rows=None, first=0, count=None,
                   out=None):
        """observation::to_vector of recorded rows (xh_venv_record_obs), row
        index q = t * N + e.  view "state": S_t of slot t in [0, P], slot P the
        present state; "next": the successor row of transition q -- S_t+1, or
        the terminal view E_t where the row ended.  rows: None (the rows
        first .. first + count - 1), a host int array (uploaded) or an integer
        device pointer to int32 indices, of which first .. first + count - 1
        are taken.  out: an integer device pointer (16-byte aligned; nothing
        is returned), or None for a host array [count][B][2D] float32."""
        B, D = self.B, self.D
        view_id, rows_ptr, count = self._record_rows("record_obs", view, rows,
                                                     first, count)
        dst = out if out is not None else self._scratch(
            "obs", count * B * 2 * D * 4)
        check(_lib.lib.xh_venv_record_obs(self.h, view_id, rows_ptr, first,
                                          count, dst))
        if out is not None:
            return None
        return self._download(dst, np.float32, (count, B, 2 * D))

    # ---- logit tables: act and train on (bin state, item) ------------------
    def table_info(self):
        """The domain of the venv's present item set (xh_venv_table_info): a
        dict of entries E = K * prod(capacity[d] + 1), states S, items K, rows
        R = ceil(E / B) and side int32 [D].  XhError where E is past
        VTAB_MAX_ENTRIES: such a venv keeps the per-row calls."""
        ti = _lib.VenvTableInfo()
        check(_lib.lib.xh_venv_table_info(self.h, C.byref(ti)))
        return _table_info_dict(ti, self.D)

    def table_obs(self, out=None):
        """The table's observations (xh_venv_table_obs): [R][B][2D] float32,
        flat per-bin row e the observation of entry e, zeros from E on.  A
        per-bin network's forward on them, R rows, is the table: [R * B]
        logits.  out: an integer device pointer (16-byte aligned; nothing is
        returned), or None for a host array."""
        R = self.table_info()["rows"]
        dst = out if out is not None else self._scratch(
            "tab_obs", R * self.B * 2 * self.D * 4)
        check(_lib.lib.xh_venv_table_obs(self.h, int(dst)))
        if out is not None:
            return None
        return self._download(dst, np.float32, (R, self.B, 2 * self.D))

    def _table_ptr(self, table):
        if isinstance(table, (int, np.integer)):
            return int(table)
        E = self.table_info()["entries"]
        t = np.ascontiguousarray(table, np.float32).reshape(-1)
        if t.size < E:
            raise ValueError("table: %d floats, the domain has %d entries"
                             % (t.size, E))
        ptr = self._scratch("tab_table", t.nbytes)
        self._upload(ptr, t)
        return ptr

    def _table_rows(self, what, rows, first, count):
        """(rows_ptr, first, count) of the STATE view's rows, as
        record_obs()."""
        if rows is None:
            if count is None:
                count = (self.record_pos() + 1) * self.N - first
            return None, first, count
        if isinstance(rows, (int, np.integer)):
            if count is None:
                raise ValueError("%s: count is needed with a device pointer "
                                 "to the rows" % what)
            return int(rows), first, count
        r = np.ascontiguousarray(rows, np.int32).reshape(-1)
        if count is None:
            count = r.size - first
        if first < 0 or count < 0 or first + count > r.size:
            raise ValueError("%s: rows %d .. %d of a list of %d"
                             % (what, first, first + count - 1, r.size))
        ptr = self._scratch("tab_rows", r.nbytes)
        self._upload(ptr, r)
        return ptr, first, count

    def act_table(self, table, mode="sample", write_obs=False, fetch=False):
        """act(kind="logits") on the rows z[b] = table[entry(bins[b], item)],
        gathered inside the launch (xh_venv_act_table): no policy row is
        formed or read.  table: a host array of at least E floats (uploaded)
        or an integer device pointer, e.g. where pol.forward(table_obs, R,
        out=ptr) wrote.  Everything after the row is act()'s.  Returns
        (actions, pchoice, reward, done) if fetch."""
        check(_lib.lib.xh_venv_act_table(self.h, self._table_ptr(table),
                                         _MODES[mode], 1 if write_obs else 0))
        if fetch:
            return (self.get(VENV_ACTIONS), self.get(VENV_PCHOICE),
                    self.get(VENV_REWARD), self.get(VENV_DONE))
        return None

    def table_logits(self, table, rows=None, first=0, count=None, out=None):
        """The logits of recorded rows from the table (xh_venv_table_gather):
        [count][B] float32, what policy_loss(kind="logits") takes.  rows /
        first / count as record_obs(view="state"); table as act_table().  out:
        an integer device pointer (16-byte aligned; nothing is returned), or
        None for a host array."""
        tptr = self._table_ptr(table)
        rows_ptr, first, count = self._table_rows("table_logits", rows, first,
                                                  count)
        dst = out if out is not None else self._scratch(
            "tab_logits", count * self.B * 4)
        check(_lib.lib.xh_venv_table_gather(self.h, tptr, rows_ptr, first,
                                            count, int(dst)))
        if out is not None:
            return None
        return self._download(dst, np.float32, (count, self.B))

    def table_grad(self, dout, rows=None, first=0, count=None,
                   accumulate=False, out=None):
        """G[e] = the sum of dout[j][b] over the minibatch's (row, bin) pairs
        whose entry is e (xh_venv_table_grad): float32 [R * B], 0 where no row
        touches and from E on; an exact integer sum, the same bits from run to
        run.  dout [count][B]: a host array or an integer device pointer, e.g.
        policy_loss()'s grad.  accumulate adds to what `out` (or, with out
        None, the previous call's block) holds.  net.backward(table_obs, G,
        rows=R) is then the parameter gradient of the whole minibatch.  out:
        an integer device pointer (16-byte aligned; nothing is returned), or
        None for a host array."""
        if not isinstance(dout, (int, np.integer)):
            dout = np.ascontiguousarray(dout, np.float32).reshape(-1, self.B)
            if count is None and rows is None:
                count = dout.shape[0]
        rows_ptr, first, count = self._table_rows("table_grad", rows, first,
                                                  count)
        dptr = self._staged("tab_dout", dout, np.float32, (count, self.B))
        total = self.table_info()["rows"] * self.B
        dst = out if out is not None else self._scratch("tab_g", total * 4)
        check(_lib.lib.xh_venv_table_grad(self.h, rows_ptr, first, count,
                                          dptr, int(dst),
                                          1 if accumulate else 0))
        if out is not None:
            return None
        return self._download(dst, np.float32, (total,))

    def record_ends(self):
        """The ended transitions of the recorded slots (xh_venv_record_ends):
        int32 indices t * N + e, env-major (e ascending, then t)."""
        cap = max(self.record_pos() * self.N, 1)
        p = self._scratch("ends", (cap + 1) * 4)
        check(_lib.lib.xh_venv_record_ends(self.h, p + 4, p))
        got = self._download(p, np.int32, (cap + 1,))
        return got[1:1 + got[0]].copy()

    def advantages(self, values, v_term=None, reward=None, done=None,
                   gamma=0.99, lam=0.95, normalize=False,
                   returns=("adv", "td_target"), steps=None):
        """GAE, TD(0) targets and lambda returns on the device
        (xh_venv_advantages).  Without reward and done the window is the
        record's P slots; with both it is the caller's own, [steps][N].
        values [steps+1][N] and v_term [steps][N] (None: 0) are host arrays or
        integer device pointers, as reward (float32) and done (uint8) are;
        the window's length is `steps`, or the first dimension of the first
        host array among reward, done and values.  normalize covers this
        venv's rows only.  Returns a
        dict of host arrays [steps][N] for the names in `returns` ("adv",
        "td_target", "lambda_return") plus "stats": float64 [4] = sum A, sum
        A^2 (before normalisation), rows, ended rows."""
        N = self.N
        own = reward is not None or done is not None
        if own and (reward is None or done is None):
            raise ValueError("advantages: reward and done go together")
        if own and steps is not None:
            T = int(steps)
        elif own:
            for a in (reward, done, values):
                if not isinstance(a, (int, np.integer)):
                    n = np.asarray(a).shape[0]
                    T = n - 1 if a is values else n
                    break
            else:
                raise ValueError("advantages: with device pointers only, "
                                 "pass steps")
        else:
            T = self.record_pos()
        names = ("adv", "td_target", "lambda_return")
        bad = set(returns) - set(names)
        if bad:
            raise ValueError("advantages: returns %s" % sorted(bad))
        a = _lib.VenvAdv()
        a.steps = T if own else 0
        a.values = self._staged("values", values, np.float32, (T + 1, N))
        a.v_term = self._staged("v_term", v_term, np.float32, (T, N))
        a.reward = self._staged("reward", reward, np.float32, (T, N))
        a.done = self._staged("done", done, np.uint8, (T, N))
        a.gamma, a.lambda_, a.normalize = gamma, lam, 1 if normalize else 0
        # one block: [adv | td_target | lambda_return | stats], 16-byte parts
        part = (T * N * 4 + 15) // 16 * 16
        base = self._scratch("adv", 3 * part + 32)
        a.adv = base
        a.td_target = base + part if "td_target" in returns else None
        a.lambda_return = base + 2 * part if "lambda_return" in returns else None
        a.stats = base + 3 * part
        check(_lib.lib.xh_venv_advantages(self.h, C.byref(a)))
        out = {n: self._download(base + k * part, np.float32, (T, N))
               for k, n in enumerate(names) if n in returns}
        out["stats"] = self._download(base + 3 * part, np.float64, (4,))
        return out

    def policy_loss(self, policy, adv, kind="logits", loss="clipped",
                    rows=None, first=0, count=None, eps=0.2, scale=1.0,
                    action=None, p_old=None, values=None, target=None,
                    value_scale=1.0, want_probs=False, want_stats=False,
                    accumulate=False, beta=0.0, distrib=None, want_kl=False,
                    legal=None, ent_coef=0.0, v_old=None, vclip=None,
                    want_ext=False):
        """The loss head of the caller's network on a minibatch of the
        recorded window (xh_venv_policy_loss): from the network's output rows
        policy [count][B] ("logits": xh_venv_act's softmax first, or "probs")
        to dL/d(output) under loss "clipped" (PPO, eps), "log" (policy_loss /
        actor-critic) or "kl" (KL-PPO: "log" + beta * (p - q), q the rows'
        sampling distributions), times scale.  beta is a float or an integer
        device pointer to one float (what kl_beta() maintains); distrib
        [total][B] is a host array, an integer device pointer, or None for the
        record's (set_record(distrib=True)).  want_kl adds "kl_stats" float64
        [VKL_COUNT] -- the exact KL(q || p) sum, the rows and the sum of
        squares -- under any loss; it needs the distributions too.  Output row j has the index q = rows[first
        + j] (rows: a host int array or an integer device pointer) or first +
        j into adv, action, p_old and target, all [total]; action / p_old None
        are the record's, with total = P * N.  values [count] with target
        turns the value head on: dvalue = (values - target[q]) * value_scale.
        Every array is a host array or an integer device pointer; count is
        needed where neither policy nor rows is a host array.  Returns a dict
        of host arrays: "grad" [count][B], and where asked "dvalue" [count],
        "probs" [count][B] and "stats" float64 [VLOSS_COUNT]; accumulate adds
        this call's statistics to the previous call's (the epoch's first
        minibatch passes False).

        legal: None, today's call; otherwise the rows are premasked by their
        legal sets first (xh_venv_policy_loss_masked): True takes the record's
        (set_action_mask with a record; action / p_old must be the record's
        too), or the caller's [total] sets indexed by q -- a host bool
        [total][B] or uint32 [total][W] array, or an integer device pointer to
        the words.  A set with no bin leaves its row unmasked.

        ent_coef, v_old, vclip, want_ext: all at their defaults, today's
        call; otherwise xh_venv_policy_loss_ex.  ent_coef > 0 -- a float, or
        an integer device pointer to one float, as beta is -- adds the
        gradient of the entropy bonus -ent_coef * H(p) to every row before
        scale (for "probs" the unconstrained partial: the caller's softmax
        sits behind it).  v_old [total] (with values, target and vclip > 0)
        makes the value head PPO2's clipped one: dvalue is 0 where the
        clipped error is the larger.  want_ext adds "ext_stats" float64
        [VEXT_COUNT]: the rows, the f32 entropies' sum, the rows whose dvalue
        the clip zeroed and the sum of the larger squared errors; accumulate
        applies to it as to "stats"."""
        B = self.B
        losses = {"clipped": _lib.LOSS_CLIPPED,
                  "log": _lib.LOSS_SOFTMAX_GRADIENT_LOG,
                  "kl": _lib.LOSS_KL_REGULATED}
        host = lambda x: x is not None and not isinstance(  # noqa: E731
            x, (int, np.integer))
        rows_ptr = None
        if host(rows):
            r = np.ascontiguousarray(rows, np.int32).reshape(-1)
            if count is None:
                count = r.size - first
            if first < 0 or count < 0 or first + count > r.size:
                raise ValueError("policy_loss: rows %d .. %d of a list of %d"
                                 % (first, first + count - 1, r.size))
            rows_ptr = self._staged("vl_rows", r, np.int32, r.shape)
        elif rows is not None:
            rows_ptr = int(rows)
        if count is None:
            if not host(policy):
                raise ValueError("policy_loss: count is needed with device "
                                 "pointers only")
            count = np.asarray(policy).reshape(-1, B).shape[0]
        total = 0
        for x in (adv, action, p_old, target, v_old):
            if host(x):
                total = np.asarray(x).size
                break
        else:
            if host(distrib):
                total = np.asarray(distrib).size // B
            elif action is not None or p_old is not None:
                total = self.record_pos() * self.N
        a = _lib.VenvLoss()
        if host(policy):
            policy = np.asarray(policy, np.float32).reshape(-1, B)
        a.policy = self._staged("vl_policy", policy, np.float32, (count, B))
        a.kind, a.loss = _KINDS[kind], losses[loss]
        a.rows_dev, a.first, a.count, a.total = rows_ptr, first, count, total

        def flat(name, x, dtype, n):
            if host(x):
                x = np.asarray(x, dtype).reshape(-1)
            return self._staged(name, x, dtype, (n,))
        a.adv = flat("vl_adv", adv, np.float32, total)
        a.action = flat("vl_action", action, np.int32, total)
        a.p_old = flat("vl_pold", p_old, np.float32, total)
        a.eps, a.scale, a.value_scale = eps, scale, value_scale
        a.values_new = flat("vl_values", values, np.float32, count)
        a.target = flat("vl_target", target, np.float32, total)
        n = max(count, 1)
        a.grad = self._scratch("vl_grad", n * B * 4)
        if values is not None:
            a.dvalue = self._scratch("vl_dvalue", n * 4)
        if want_probs:
            a.probs_out = self._scratch("vl_probs", n * B * 4)
        if want_stats:
            a.stats = self._scratch("vl_stats", _lib.VLOSS_COUNT * 8)
        if want_stats or want_kl or want_ext:
            a.accumulate = 1 if accumulate else 0
        if host(distrib):
            distrib = np.asarray(distrib, np.float32).reshape(-1, B)
        a.distrib = self._staged("vl_distrib", distrib, np.float32, (total, B))
        if _beta_ptr(beta) is not None:
            a.beta_dev = _beta_ptr(beta)
        else:
            a.beta = float(beta)
        if want_kl:
            a.kl_stats = self._scratch("vl_kl", _lib.VKL_COUNT * 8)
        ent_ptr = _beta_ptr(ent_coef, "ent_coef")
        ext = (ent_ptr is not None or float(ent_coef) != 0.0 or
               v_old is not None or vclip is not None or want_ext)
        lptr = None
        if legal is not None:
            if isinstance(legal, (int, np.integer)) and not isinstance(
                    legal, (bool, np.bool_)):
                lptr = int(legal)
            elif not isinstance(legal, (bool, np.bool_)):
                w = np.asarray(legal)
                if w.dtype == np.bool_:
                    w = pack_legal(w.reshape(-1, B))
                w = np.ascontiguousarray(w, np.uint32).reshape(
                    -1, legal_words(B))
                lptr = self._staged("vl_legal", w, np.uint32,
                                    (total, legal_words(B)))
            elif not legal:
                raise ValueError("policy_loss: legal is None, True, an array "
                                 "or a device pointer")
        if ext:
            x = _lib.VenvLossExt()
            x.masked, x.legal_dev = 0 if legal is None else 1, lptr
            if ent_ptr is not None:
                x.ent_coef_dev = ent_ptr
            else:
                x.ent_coef = float(ent_coef)
            x.v_old = flat("vl_vold", v_old, np.float32, total)
            if vclip is not None:
                x.vclip = float(vclip)
            if want_ext:
                x.ext_stats = self._scratch("vl_ext", _lib.VEXT_COUNT * 8)
            check(_lib.lib.xh_venv_policy_loss_ex(self.h, C.byref(a),
                                                  C.byref(x)))
        elif legal is None:
            check(_lib.lib.xh_venv_policy_loss(self.h, C.byref(a)))
        else:
            check(_lib.lib.xh_venv_policy_loss_masked(self.h, C.byref(a),
                                                      lptr))
        out = {"grad": self._download(a.grad, np.float32, (count, B))}
        if values is not None:
            out["dvalue"] = self._download(a.dvalue, np.float32, (count,))
        if want_probs:
            out["probs"] = self._download(a.probs_out, np.float32, (count, B))
        if want_stats:
            out["stats"] = self._download(a.stats, np.float64,
                                          (_lib.VLOSS_COUNT,))
        if want_kl:
            out["kl_stats"] = self._download(a.kl_stats, np.float64,
                                             (_lib.VKL_COUNT,))
        if want_ext:
            out["ext_stats"] = self._download(x.ext_stats, np.float64,
                                              (_lib.VEXT_COUNT,))
        return out

    def kl_beta(self, kl_stats, d_targ, beta):
        """kl_ppo_learner's beta rule on the device (xh_venv_kl_beta): from an
        epoch's accumulated kl_stats -- a host float64 [VKL_COUNT] array or an
        integer device pointer, e.g. the block policy_loss(want_kl=True) wrote
        -- beta halves / doubles around d_targ and is clamped to [1e-25, 0.1].
        beta: an integer device pointer to the float updated in place, or a
        float (staged, updated and read back).  Returns (beta_after,
        mean_kl)."""
        stats = self._staged("kb_stats", kl_stats, np.float64,
                             (_lib.VKL_COUNT,))
        bptr = _beta_ptr(beta)
        if bptr is None:
            bptr = self._staged("kb_beta", np.array([beta], np.float32),
                                np.float32, (1,))
        log = self._scratch("kb_log", 16)
        check(_lib.lib.xh_venv_kl_beta(self.h, stats, float(d_targ), bptr,
                                       log))
        got = self._download(log, np.float32, (3,))
        return float(got[2]), float(got[1])

    # ---- episode statistics, counted on the device ------------------------
    def set_episode_stats(self, rows):
        """Episode statistics (xh_venv_set_episode_stats): from now on every
        step() / act() / apply() launch counts each env's steps and, where the
        step ends the episode, the finished length; episode_row() reduces the
        counts into one row of a device ring of `rows` rows.  Calling it again
        restarts everything; 0 turns the statistics off and frees them.  An
        episode in flight is counted from this call on: switch on after
        creation or a reset."""
        check(_lib.lib.xh_venv_set_episode_stats(self.h, int(rows)))
        self._ep_history = int(rows)

    def episode_row(self):
        """Append one row to the ring (xh_venv_episode_row; asynchronous) and
        clear the window's accumulators."""
        check(_lib.lib.xh_venv_episode_row(self.h))

    def episode_count(self):
        """Rows taken since set_episode_stats (xh_venv_episode_count)."""
        n = C.c_long()
        check(_lib.lib.xh_venv_episode_count(self.h, C.byref(n)))
        return n.value

    def episode_stats(self, first=None, count=None):
        """Rows [first, first + count) as float64 [rows][VEP_COUNT]
        (xh_venv_get_episode_rows; synchronises).  Default: every row still in
        the ring."""
        total = self.episode_count()
        if first is None:
            held = min(total, self._ep_history)
            first = total - (held if count is None else min(count, held))
        if count is None:
            count = total - first
        out = np.zeros((count, _lib.VEP_COUNT), np.float64)
        check(_lib.lib.xh_venv_get_episode_rows(self.h, first, count,
                                                _ptr(out)))
        return out

    def episode_curve(self):
        """Per-row series derived from episode_stats(): a dict of float64
        arrays, one entry per row in the ring -- "row", "calls", "episodes",
        "len_mean", "len_std" (population), "return_mean" (an episode's
        return is its length - 1), "len_min", "len_max", "return_min",
        "return_max", "envs_finished", "first_len_mean", "first_len_std",
        "first_return_mean".  NaN where a row has no episode (or, for the
        first-episode entries, no env has finished one)."""
        r = self.episode_stats()
        L = _lib
        with np.errstate(invalid="ignore", divide="ignore"):
            n = r[:, L.VEP_EPISODES]
            mean = r[:, L.VEP_LEN_SUM] / n
            var = r[:, L.VEP_LEN_SQSUM] / n - mean * mean
            k = r[:, L.VEP_ENVS_FINISHED]
            fmean = r[:, L.VEP_FIRST_LEN_SUM] / k
            fvar = r[:, L.VEP_FIRST_LEN_SQSUM] / k - fmean * fmean
        return {"row": r[:, L.VEP_ROW], "calls": r[:, L.VEP_CALLS],
                "episodes": n, "len_mean": mean,
                "len_std": np.sqrt(np.maximum(var, 0.0)),
                "return_mean": mean - 1.0,
                "len_min": r[:, L.VEP_LEN_MIN], "len_max": r[:, L.VEP_LEN_MAX],
                "return_min": r[:, L.VEP_LEN_MIN] - 1.0,
                "return_max": r[:, L.VEP_LEN_MAX] - 1.0,
                "envs_finished": k, "first_len_mean": fmean,
                "first_len_std": np.sqrt(np.maximum(fvar, 0.0)),
                "first_return_mean": fmean - 1.0}

    def episode_state(self):
        """(running, first): int32 [N] each -- the steps of every env's
        episode in flight and every env's first finished length, -1 where it
        has none yet (xh_venv_episode_get)."""
        out = []
        for which in (_lib.VEPS_RUNNING, _lib.VEPS_FIRST):
            a = np.zeros(self.N, np.int32)
            check(_lib.lib.xh_venv_episode_get(self.h, which, _ptr(a),
                                               a.nbytes))
            out.append(a)
        return tuple(out)

    def set_episode_state(self, running, first):
        """Continue another run's counts (xh_venv_episode_set): after
        set(VENV_BINS / ITEMS / RNG) of a saved state -- set(VENV_BINS) zeroes
        the running lengths, so this call comes last.  Take a row before
        saving: the window's accumulators are not part of the state."""
        for which, arr in ((_lib.VEPS_RUNNING, running),
                           (_lib.VEPS_FIRST, first)):
            a = np.ascontiguousarray(arr, np.int32).reshape(self.N)
            check(_lib.lib.xh_venv_episode_set(self.h, which, _ptr(a),
                                               a.nbytes))

    def first_episode_lengths(self):
        """The lengths of the envs' first finished episodes, int32 [k], k =
        the envs that have finished one: one episode per env, the unbiased
        sample of a vector env's evaluation."""
        first = self.episode_state()[1]
        return first[first >= 0]

    def apply(self, mask=None):
        """environment::apply(actions[e], e) for the masked envs (no reset);
        returns game_over per env ([N] uint8; 0 for the envs not applied)."""
        if mask is not None:
            self.set(VENV_MASK, np.asarray(mask, np.uint8))
        check(_lib.lib.xh_venv_apply(self.h, 0 if mask is None else 1))
        return self.get(VENV_DONE)

    def reset(self, mask=None):
        """environment::reset(e) for the masked envs (all if mask is None)."""
        if mask is not None:
            self.set(VENV_MASK, np.asarray(mask, np.uint8))
        check(_lib.lib.xh_venv_reset(self.h, 0 if mask is None else 1))

    def observe(self):
        """observation::to_vector of every env: [N][B][2D] float32."""
        check(_lib.lib.xh_venv_observe(self.h))
        return self.get(VENV_OBS)

    def view(self):
        """(bins [N][B][D] int8, items [N][D] int8): environment::view."""
        return self.get(VENV_BINS), self.get(VENV_ITEMS)[:, :self.D]

    def synchronize(self):
        check(_lib.lib.xh_venv_synchronize(self.h))

    def set_timing(self, on):
        """HIP events around every later launch (xh_venv_set_timing); drops
        the events recorded so far."""
        check(_lib.lib.xh_venv_set_timing(self.h, 1 if on else 0))

    def kernel_time(self):
        """(milliseconds, launches) of the timed launches."""
        ms, n = C.c_double(), C.c_long()
        check(_lib.lib.xh_venv_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self.h:
            check(_lib.lib.xh_venv_destroy(self.h))
            self.h = C.c_void_p()
            for ptr, _ in self._dev.values():
                check(_lib.tensor_free(self.ctx.h, ptr))
            self._dev = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def heuristic_baseline(ctx, kind, bins, dims, num_envs, items=None,
                       weights=None, capacity=None, rng_state=1,
                       max_steps=100000, row_every=64):
    """What a heuristic agent scores on an instance: a fresh VecEnv on it
    (policy_draws 2 for "random", 0 otherwise) with episode statistics on,
    driven by act_heuristic(kind) until every env has finished its first
    episode or max_steps steps were taken.  One episode_row() and one
    synchronising read every row_every steps; no per-step host traffic.

    Returns a dict over the envs' first episodes (one per env, the unbiased
    sample): "episodes" (the envs that finished one), "len_mean", "len_min",
    "len_max", "return_mean" / "return_min" / "return_max" (an episode's
    return is its length - 1; all NaN while episodes == 0),
    "steps" (launches made) and "finished" (episodes == num_envs)."""
    if row_every < 1 or max_steps < 1:
        raise ValueError("heuristic_baseline: row_every and max_steps >= 1")
    env = VecEnv(ctx, num_envs, bins=bins, dims=dims, rng_state=rng_state,
                 policy_draws=2 if kind == "random" else 0, items=items,
                 weights=weights, capacity=capacity)
    try:
        env.set_episode_stats(2)
        steps, done = 0, False
        while steps < max_steps and not done:
            for _ in range(min(row_every, max_steps - steps)):
                env.act_heuristic(kind)
                steps += 1
            env.episode_row()
            row = env.episode_stats(count=1)[0]
            done = int(row[_lib.VEP_ENVS_FINISHED]) == num_envs
        first = env.first_episode_lengths().astype(np.int64)
    finally:
        env.close()
    k = int(first.size)
    nan = float("nan")
    mean = float(first.sum()) / k if k else nan
    lo, hi = (int(first.min()), int(first.max())) if k else (nan, nan)
    return {"kind": kind, "episodes": k, "len_mean": mean, "len_min": lo,
            "len_max": hi, "return_mean": mean - 1.0, "return_min": lo - 1,
            "return_max": hi - 1, "steps": steps, "finished": k == num_envs}
