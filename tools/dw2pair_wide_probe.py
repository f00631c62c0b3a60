"""Per-block gradient error (W1, b1, W2, b2, w3, b3; units of u sum|terms|
against the oracle) of tests/test_gpu_spec8_dw2pair.py's wide-g case for
several w3 scales, with and without h1_units, under the library XH_LIB_PATH
names (diagnostic; not part of the suite):

    [XH_LIB_PATH=build/<name>/libxylo_hip.so] python tools/dw2pair_wide_probe.py 1 8 16 32
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_gpu_spec8_dw2pair as t  # noqa: E402
from conftest import grad_units  # noqa: E402
from dependence_free_rl_amd import Context  # noqa: E402

ctx = Context(device=0)
H, F0 = t.H, t.F0
blocks = [("W1", 0, t.OB1), ("b1", t.OB1, t.OW2), ("W2", t.OW2, t.OB2),
          ("b2", t.OB2, t.OW3), ("w3", t.OW3, t.OW3 + H), ("b3", t.OW3 + H, t.OW3 + H + 1)]
for scale in [float(s) for s in sys.argv[1:]]:
    for h1s in (False, True):
        t.W3_PEAK = scale
        pp = t._params(True, h1s)
        dev, ref, mag, orc = t._device_and_oracle(ctx, "ppo", pp)
        om, orow = t._g_range(orc, "ppo", pp)
        u, idx, _ = grad_units(dev[0], ref[0], mag[0])
        out = ["w3x%g h1s=%d G/med=2^%.1f G/rowmax=2^%.1f all med %.3f p99 %.1f" % (
            scale, h1s, np.log2(om), np.log2(orow), np.median(u), np.percentile(u, 99))]
        for name, a, b in blocks:
            m = (idx >= a) & (idx < b)
            if m.any():
                out.append("%s med %.3f p99 %.1f max %.1f" % (
                    name, np.median(u[m]), np.percentile(u[m], 99), u[m].max()))
        print(os.environ.get("XH_LIB_PATH", "product"), " | ".join(out), flush=True)
ctx.close()
