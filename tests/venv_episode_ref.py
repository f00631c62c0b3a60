"""Host restatement of the VecEnv's episode statistics (xh_venv_set_episode_
stats / xh_venv_episode_row).  CPU only, numpy integer arithmetic only.

The input is a history of calls: for each step / act / apply launch, live bool
[N] (the envs the call applied: not masked out, action not refused, row not
refused) and done bool [N] (the call's verdicts, XH_VENV_DONE).  A live step
adds 1 to the env's running length; where it is done the finished length (the
overflowing step included) goes into the window's accumulators and into the
env's first length if it has none, and the count restarts.  A row reduces the
window and clears it; the running and the first lengths stay.

The helpers below produce such histories from ActRef (tests/venv_act_ref.py):
every pick, apply and reset is the oracle's."""
import numpy as np

(ROW, CALLS, EPISODES, LEN_SUM, LEN_SQSUM, LEN_MIN, LEN_MAX, ENVS_FINISHED,
 FIRST_LEN_SUM, FIRST_LEN_SQSUM, RUNNING_SUM, RUNNING_MAX, COUNT) = range(13)


class EpisodeRef:
    """The counts of one venv of N envs since statistics were switched on."""

    def __init__(self, N):
        self.N = N
        self.running = np.zeros(N, np.int32)
        self.first = np.full(N, -1, np.int32)
        self.rows_taken = 0
        self.calls = 0
        self.window = []       # the lengths finished since the last row
        self.lengths = [[] for _ in range(N)]  # every finished length, per env

    def call(self, live, done):
        """One step / act / apply launch."""
        live = np.asarray(live, bool).reshape(self.N)
        done = np.asarray(done, bool).reshape(self.N)
        assert not (done & ~live).any(), "an env not applied reports no end"
        self.calls += 1
        for e in range(self.N):
            if not live[e]:
                continue
            self.running[e] += 1
            if done[e]:
                n = int(self.running[e])
                self.window.append(n)
                self.lengths[e].append(n)
                if self.first[e] < 0:
                    self.first[e] = n
                self.running[e] = 0

    def restart(self, mask=None):
        """xh_venv_reset(mask) / xh_venv_set(XH_VENV_BINS): the running length
        of the selected envs (all if None) back to 0, nothing counted."""
        if mask is None:
            self.running[:] = 0
        else:
            self.running[np.asarray(mask, bool).reshape(self.N)] = 0

    def set_state(self, running, first):
        """xh_venv_episode_set of both arrays."""
        self.running = np.array(running, np.int32).reshape(self.N)
        self.first = np.array(first, np.int32).reshape(self.N)

    def row(self):
        """xh_venv_episode_row: float64 [COUNT]."""
        w = np.array(self.window, np.int64)
        fin = self.first[self.first >= 0].astype(np.int64)
        run = self.running.astype(np.int64)
        r = np.zeros(COUNT, np.float64)
        r[ROW] = self.rows_taken
        r[CALLS] = self.calls
        r[EPISODES] = len(w)
        r[LEN_SUM] = int(w.sum())
        r[LEN_SQSUM] = int((w * w).sum())
        r[LEN_MIN] = int(w.min()) if len(w) else np.nan
        r[LEN_MAX] = int(w.max()) if len(w) else np.nan
        r[ENVS_FINISHED] = len(fin)
        r[FIRST_LEN_SUM] = int(fin.sum())
        r[FIRST_LEN_SQSUM] = int((fin * fin).sum())
        r[RUNNING_SUM] = int(run.sum())
        r[RUNNING_MAX] = int(run.max())
        self.rows_taken += 1
        self.calls = 0
        self.window = []
        return r


def rows_of_history(done, live, row_points, ref=None):
    """done / live bool [S][N]; row_points: the numbers of calls after which a
    row is taken (ascending, repeats allowed, at most S).  Returns (rows
    float64 [R][COUNT], running int32 [N], first int32 [N], the EpisodeRef)."""
    done, live = np.asarray(done, bool), np.asarray(live, bool)
    S, N = done.shape
    ref = ref or EpisodeRef(N)
    pts = list(row_points)
    assert pts == sorted(pts) and (not pts or pts[-1] <= S)
    rows = []
    for s in range(S + 1):
        while pts and pts[0] == s:
            rows.append(ref.row())
            pts.pop(0)
        if s < S:
            ref.call(live[s], done[s])
    return (np.array(rows, np.float64).reshape(-1, COUNT), ref.running.copy(),
            ref.first.copy(), ref)


def lengths_from_done(done, live):
    """The finished lengths per env, from the flags alone: a list of lists."""
    return rows_of_history(done, live, [])[3].lengths


# ------------------------------------------------------- ActRef histories --
def act_history(ref, rows, mode="sample", masked=False, refuse=None):
    """ActRef.act over rows [S][N][B] (probabilities).  masked: each row is
    premasked by the env's legal set first (venv_mask_ref), what xh_venv_act
    does with the action mask on.  refuse: {step: set of envs} left untouched.
    Returns done, live bool [S][N]."""
    import venv_mask_ref as mr
    refuse = refuse or {}
    done, live = [], []
    for s, r in enumerate(rows):
        if masked:
            r = mr.premask(r, mr.eff(mr.legal_ref(ref.bins(), ref.items())),
                           "probs")
        out = ref.act(r, mode, refuse=refuse.get(s, ()))
        lv = np.ones(ref.N, bool)
        lv[list(refuse.get(s, ()))] = False
        done.append(out["done"].astype(bool))
        live.append(lv)
    return np.stack(done), np.stack(live)


def step_history(ref, actions):
    """ActRef.step over actions int [S][N] (all in range).  Returns done, live
    bool [S][N]."""
    done = [ref.step(a)["done"].astype(bool) for a in actions]
    return np.stack(done), np.ones((len(actions), ref.N), bool)


def count_between_resets(ref):
    """Instruments ActRef's envs: every apply counts a step, every reset (the
    oracle env's own, after a game over) closes an episode.  Returns the list
    of lists the closed lengths are appended to, per env."""
    closed = [[] for _ in ref.envs]
    for e, env in enumerate(ref.envs):
        steps = [0]
        apply0, reset0 = env.apply, env.reset

        def apply(choice, steps=steps, apply0=apply0):
            steps[0] += 1
            return apply0(choice)

        def reset(steps=steps, reset0=reset0, out=closed[e]):
            out.append(steps[0])
            steps[0] = 0
            return reset0()
        env.apply, env.reset = apply, reset
    return closed
