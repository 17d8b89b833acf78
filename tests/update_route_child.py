"""Child process of test_hip_update.py (not a test module): the library reads GMMVI_BLOCKED_ABOVE once per
process, so the register-resident update kernels at D = 51 ... 64 (the generic four-wave instance of update_kl_fast_kernel and
update_plain_kernel, both beyond 64 KB of dynamic LDS from D = 55 / 57) run here, in a fresh interpreter with the knob in its
environment.

    python update_route_child.py OUT.npz CASE_ID ...

The cases are rebuilt from update_cases.py by their ids; OUT receives c{c}_r{round}_{name} for every output of update_device.run_round.  The
parent computes the references."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import update_cases as cases  # noqa: E402
from update_device import run_round  # noqa: E402


def main(dst, ids):
    from gmmvi_amd.device import get_context
    ctx = get_context()
    res = {}
    for c, case_id in enumerate(ids):
        case = cases.make_case(cases.spec_by_id(case_id))
        for rnd in range(len(case["rounds"])):
            for name, v in run_round(ctx, case, rnd).items():
                res[f"c{c}_r{rnd}_{name}"] = v
    np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
