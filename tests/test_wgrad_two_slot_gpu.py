"""The two-slot partition of the weight-gradient launch (wgrad2_kernel: one job, two slots, rows0 + rows1 <= 256, fp32 — HIRL's actor step and SAC's
imitative policy step on 224 workgroups) against the one-partition-for-all kernel it replaces there (HX_WGRAD_TWO_SLOT=0): BIT FOR BIT.

The library reads the knob once per process, so tests/_wgrad_two_slot_child.py runs every case once in a process with HX_WGRAD_TWO_SLOT=0 and once in a
process with the default (two processes for the whole module), each leaving its arrays in a temporary directory.

Compared by their bits: the actor's gradient after every call, actor / moments / target after six learn() calls (three actor calls, the third with the
Polyak step; BC weight estimated, stored, given), the acting images (fp32 and the three exact-split parts), the stored BC weight and losses[5] (the
weight the launch's thread 0 logs).  losses[0], [2], [3], [4] are float atomicAdd sums over the workgroups of the BACKWARD launches, which are the same
launches in both processes and differ in the last bit between any two runs (tests/test_sac_gpu.py, tests/test_hirl_gpu.py compare them at rtol 1e-6, and
so does this test); losses[1] is formed from them by the launch under test and must have equal bits whenever its two inputs do.

B = 144 does not fit the rule (288 rows): both processes run the same kernel there, and the case only checks that the fall-back is taken without harm
(the library has no launch-count query)."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIRL_BITS = ("actor", "m_actor", "v_actor", "target_actor", "w2_f32i", "w2_x9")
SAC_BITS = ("policy", "m_policy", "v_policy", "alpha_state", "w2_f32i")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = []
    for knob in ("0", None):
        d = tmp_path_factory.mktemp("two_slot_" + (knob or "default"))
        env = {k: v for k, v in os.environ.items() if k != "HX_WGRAD_TWO_SLOT"}
        if knob is not None:
            env["HX_WGRAD_TWO_SLOT"] = knob
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_wgrad_two_slot_child.py"), str(d)], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0 and "two-slot child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
        out.append(d)
    return out


def load(runs, case):
    return [np.load(os.path.join(str(d), case + ".npz")) for d in runs]


def same_bits(a, b, name):
    assert a[name].dtype == b[name].dtype and a[name].dtype.kind == "i" and a[name].shape == b[name].shape, name
    bad = np.flatnonzero(a[name] != b[name])
    assert bad.size == 0, f"{name}: {bad.size} of {a[name].size} words differ, first at {bad[:8]}"


@pytest.mark.parametrize("case", ["b16", "b48", "b128", "b144", "staged128", "slope128"])
def test_hirl_actor_step_two_slot_partition_is_bit_identical(runs, case):
    """b16: fewer rows than row groups — most threads of both stages own no row (clamped loads, zeros handed over).  b48: a ragged last MFMA group per
    half.  b128: the workload's shape, rows0 + rows1 exactly 256.  b144: beyond the rule.  staged128: hx_hirl_actor_wgrad without Adam, then hx_adam.
    slope128: the RELU = false instantiation (slope 0.01)."""
    old, new = load(runs, case)
    for k in range(6):
        same_bits(old, new, f"grad_actor{k}")
        same_bits(old, new, f"wstate{k}")
        lo, ln = old[f"losses{k}"], new[f"losses{k}"]
        print(case, "call", k, "losses", lo.tolist(), ln.tolist())
        assert lo[5].view(np.int32) == ln[5].view(np.int32), (k, lo[5], ln[5])
        np.testing.assert_allclose(lo, ln, rtol=1e-6, atol=0, err_msg=f"call {k}")
        if (lo[2:4].view(np.int32) == ln[2:4].view(np.int32)).all():
            assert lo[1].view(np.int32) == ln[1].view(np.int32), (k, lo[1], ln[1])
    for name in HIRL_BITS:
        same_bits(old, new, name)
    assert np.abs(old["grad_actor4"].view(np.float32)).max() > 0 and np.isfinite(old["actor"].view(np.float32)).all()


def test_sac_imitative_policy_step_two_slot_partition_is_bit_identical(runs):
    """hx_sac_learn_imitative at B = 128: policy(s) weighted 1 - w, policy(s_e) weighted w, the log-alpha step by the launch's thread 0."""
    old, new = load(runs, "sac128")
    for k in range(4):
        same_bits(old, new, f"grad_policy{k}")
        lo, ln = old[f"losses{k}"], new[f"losses{k}"]
        assert (lo[3:8].view(np.int32) == ln[3:8].view(np.int32)).all(), (k, lo, ln)
        np.testing.assert_allclose(lo[:3], ln[:3], rtol=1e-6, atol=0, err_msg=f"call {k}")
    for name in SAC_BITS:
        same_bits(old, new, name)
    assert np.abs(old["grad_policy3"].view(np.float32)).max() > 0
