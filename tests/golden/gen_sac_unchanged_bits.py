#!/usr/bin/env python3
"""Record tests/golden/sac_unchanged_bits.npz: the bits hx_sac_learn and the staged sequence (hx_sac_adam) leave behind from a fixed start.

Run ON AN MI355X with the library of the commit whose behaviour is to be pinned (the parent of the prioritized-replay change: build that
commit, then run this file from its tree); tests/test_per_gpu.py::test_unchanged_paths_give_the_parents_bits replays it.

    python tests/golden/gen_sac_unchanged_bits.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hirl4ucav_amd.agents import sac_engine as SE  # noqa: E402
from tests import _sac_bits  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sac_unchanged_bits.npz")
    rec = _sac_bits.record(SE, sac_params())
    np.savez_compressed(out, **rec)
    print("recorded", len(rec), "vectors ->", out)
