"""What the packed train epoch rests on ("duplicate rows";
dependence_free_rl_amd/csrc/spec8_pack_layout.h): a bin starts at (8, 8),
only ever loses whole items (4, 2) or (1, 2), and every bin is reset on game
over, so an env-step's 64 bins hold few distinct states -- ten are reachable.
Checked on the CPU oracle's own rollout, long enough to see resets."""
import numpy as np

B, D, WIDTHS = 64, 2, (128, 128)
REACHABLE = {(8, 8), (4, 6), (7, 6), (0, 4), (3, 4), (6, 4), (2, 2), (5, 2), (1, 0), (4, 0)}


def test_an_env_step_holds_at_most_ten_distinct_bin_states():
    from dependence_free_rl_amd import init_policy, init_value
    from oracle import pyoracle as po
    N, T = 2, 384
    pp, vp = init_policy(D, *WIDTHS, seed=61), init_value(B, D, seed=62)
    orc = po.Trainer(po.OR_PPO, B, D, N, T,
                     po.perbin_model(2 * D, list(WIDTHS), po.OR_SOFTMAX), pp,
                     po.full_model(B * 2 * D, [64, 32], 1), vp, x0=4711)
    orc.rollout()
    bins = np.asarray(orc.buf(po.BUF_STEP_BINS)).reshape(N * T, B, D)
    done = np.asarray(orc.buf(po.BUF_STEP_DONE)).reshape(N, T)
    assert done.sum() >= 2, "the window must see resets"
    # a reset follows every game over but the window's last step
    after = bins.reshape(N, T, B, D)[:, 1:][done[:, :-1] != 0]
    assert len(after) and (after == 8).all()
    most = 0
    for step in bins:
        states = {tuple(int(v) for v in s) for s in step}
        assert states <= REACHABLE, states - REACHABLE
        most = max(most, len(states))
    assert most <= 10
    print("distinct bin states per env-step: at most %d over %d env-steps, %d resets" % (
        most, N * T, int(done.sum())))
