"""Child process of test_hip_more_blocked.py (not a test module): one seeded gmmvi_more_blocked call (K = 3, D = 64) under
whatever GMMVI_MORE_WS_GB the parent put into the environment.

    python more_blocked_group_child.py OUT.npz

OUT receives h [K,D,D] and g [K,D]."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gmmvi_amd import hip_ops  # noqa: E402
from gmmvi_amd.device import get_context  # noqa: E402
from test_hip_more_blocked import _stein_inputs, _device_inputs  # noqa: E402


def main(dst):
    ctx = get_context()
    k, d, n = 3, 64, 6500
    m, x, mapping, tlp, bg = _stein_inputs(np.random.default_rng(77), k, d, n)
    packed, chols, xd, ld, lp = _device_inputs(ctx, m, x, d)
    h, g = hip_ops.more_blocked(ctx, packed, chols, xd, ld, lp, ctx.asarray(bg), ctx.asarray(tlp),
                                ctx.asarray(np.full(k, 1e-6)), d)
    np.savez(dst, h=h.numpy(), g=g.numpy())


if __name__ == "__main__":
    main(sys.argv[1])
