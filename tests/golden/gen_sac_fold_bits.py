#!/usr/bin/env python3
"""Record tests/golden/sac_fold_bits.npz: the bits SAC's weighted, clipped and scoring paths and the staged bf16 update leave behind from a fixed
start (tests/_sac_fold_bits.py).

Run ON AN MI355X with the library of the commit whose behaviour is to be pinned (the parent of the change that folded these paths into the shared
code: build that commit, or point HX_LIBRARY at its library, then run this file); test_weighted_paths_give_the_parents_bits (tests/test_per_gpu.py),
test_clipped_paths_give_the_parents_bits (tests/test_sac_clip_gpu.py), test_scoring_gives_the_parents_bits (tests/test_per_score_gpu.py) and
test_staged_bf16_update_gives_the_parents_bits (tests/test_sac_bf16_gpu.py) replay it.

max_norm is taken from the norms that library reports (grad_norms_host) for the weighted update under a clip that never binds: a bound just above
the policy's largest norm of the four calls, so that the clip binds for the critics and not for the policy; the coefficients of the weighted,
clipped run are checked for exactly that, and max_norm is stored in the file.

    python tests/golden/gen_sac_fold_bits.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hirl4ucav_amd.agents import sac_engine as SE  # noqa: E402
from tests import _sac_fold_bits as F  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sac_fold_bits.npz")
    params = sac_params()
    norms = F.probe_norms(SE, params)
    print("norms under a clip that never binds (Q1, Q2, policy per call):\n", norms)
    lo = norms[:, 2].max()

    def coefficients(r, case):
        coef = r[f"{case}/clip_ws"][2:].astype(np.int32).view(np.float32)  # (all CALLS * 6 words are among the sampled ones)
        assert coef.size == F.CALLS * 6
        return coef.reshape(F.CALLS, 6)[:, 3:]

    # a binding clip changes the later calls' norms (critics that step less keep larger TD errors), so the pattern is looked for in the weighted, clipped
    # run itself: the first bound just above the policy's largest unclipped norm under which both critics are clipped in every call and the policy never
    best = None
    for f in (1.01, 1.03, 1.06, 1.1, 1.2):
        max_norm = float(np.float32(lo * f))
        coef = coefficients(F.record(SE, params, max_norm, cases=("weighted_clipped",)), "weighted_clipped")
        print("max_norm", max_norm, "coefficients per call (Q1, Q2, policy):\n", coef)
        if (coef[:, :2] < 1.0).all() and (coef[:, 2] == 1.0).all():
            break
        if (coef[:, 2] == 1.0).all() and (coef[:, :2] < 1.0).any(0).all():  # second best: never the policy, each critic in some call
            n = int((coef[:, :2] < 1.0).sum())
            best = max(best or (0, 0.0), (n, max_norm))
    else:
        if best is None:
            raise SystemExit("no max_norm above the policy's norms clips the critics and never the policy")
        max_norm = best[1]
        print(f"NOTE: no bound clips both critics in EVERY call; taking {max_norm}: {best[0]} of {2 * F.CALLS} critic steps clipped, the policy never")
    rec = F.record(SE, params, max_norm)
    again = F.record(SE, params, max_norm)
    for k in rec:  # a recording is worth keeping only if the same library repeats it
        if not k.endswith("/td_losses"):
            assert np.array_equal(rec[k], again[k]), f"{k} differs between two runs of the same library"
    for case in ("clipped", "clipped_fixed_alpha"):
        print(case, "coefficients per call (Q1, Q2, policy):\n", coefficients(rec, case))
    rec["max_norm"] = np.asarray([max_norm], np.float32)
    np.savez_compressed(out, **rec)
    print("max_norm", max_norm, "recorded", len(rec), "vectors ->", out, os.path.getsize(out), "bytes")
