"""The head riders of the critics' weight-gradient launch (hx_wgrad.hip head_rider_wg: the head of actor(s) — and of bc_actor(s) on a soft-estimate
call — evaluated once per row on workgroups of launch D, launch G reading the finished action rows: act_mode 2) against the form they replace
(HX_HEAD_RIDER=0: every column workgroup of launch G evaluates the heads for its 16 rows): BIT FOR BIT.

The library reads the knob once per process, so tests/_head_rider_child.py runs every case once in a process with HX_HEAD_RIDER=0 and once in a process
with HX_HEAD_RIDER=1 (two processes for the whole module), each leaving its arrays in a temporary directory.

A case is six consecutive learn() calls (three actor calls, the third with the Polyak step) of one engine: batch 16 (one row tile), 48 (three tiles, no
multiple of the 8 XCDs), 128, 256 (16 rider workgroups per head job) x HIRL-soft with the weight estimated in the first call (two head jobs), HIRL-fixed,
TD3 (use_bc = 0, slope 0.01: the non-ReLU instantiations), layerNorm = False x the fp32 / the bf16 update path x reference order (learn) / front loop
(step_learn, 64 envs) x one-call / the staged sequence (hx_hirl_critic_grads[_back] carrying the riders, hx_hirl_actor_backward with fwd_done = 2).

Compared by their bits after every call: grad_actor, grad_critic, the stored BC weight, losses[5], the action rows and LayerNorm statistics of the slots
the riders write (outv[:, 0:4] / st2 of actor(s), of bc_actor(s) on the soft call); after the six calls: all five networks, the Adam moments, every W2
image (fp32 acting image, exact-split parts, the bf16 update path's ten).  losses[0], [2], [3], [4] are float atomicAdd sums over the workgroups of the
BACKWARD launches: the same launches on the same inputs in both processes, and they differ in the last bit between any two runs of ONE build
(tests/test_wgrad_two_slot_gpu.py, tests/test_front_gpu.py and tests/test_hirl_gpu.py compare them at rtol 1e-6, and so does this test); losses[1] is
formed from them and must have equal bits whenever its inputs do.  Every such word is printed before it is asserted.

Guard: with a sentinel around what the riders may write (hx_hirl_critic_grads(actor_fwd = 1) alone, B = 48), the sentinel is still there afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from tests._head_rider_child import BATCHES, DTYPES, MODES, ORDERS, SENTINEL, SEQS  # noqa: E402


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = []
    for knob in ("0", "1"):
        d = tmp_path_factory.mktemp("head_rider_" + knob)
        env = dict(os.environ)
        env["HX_HEAD_RIDER"] = knob
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_head_rider_child.py"), str(d)], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0 and "head-rider child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
        out.append(d)
    return out


def load(runs, case):
    return [np.load(os.path.join(str(d), case + ".npz")) for d in runs]


def same_bits(a, b, name):
    assert a[name].dtype == b[name].dtype and a[name].dtype.kind in "iu" and a[name].shape == b[name].shape, name
    bad = np.flatnonzero(a[name] != b[name])
    assert bad.size == 0, f"{name}: {bad.size} of {a[name].size} words differ, first at {bad[:8]}"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_head_riders_are_bit_identical_to_launch_g_evaluating_its_heads(runs, dtype, order, seq, mode, B):
    case = "-".join((dtype, order, seq, mode, f"b{B}"))
    old, new = load(runs, case)
    assert set(old.files) == set(new.files)
    for k in range(6):
        lo, ln = old[f"losses{k}"], new[f"losses{k}"]
        print(case, "call", k, "losses", lo.tolist(), ln.tolist())
        for name in ("grad_actor", "grad_critic", "wstate"):
            same_bits(old, new, f"{name}{k}")
        assert lo[5].view(np.int32) == ln[5].view(np.int32), (k, lo[5], ln[5])
        np.testing.assert_allclose(lo, ln, rtol=1e-6, atol=0, err_msg=f"call {k}")
        if (lo[2:4].view(np.int32) == ln[2:4].view(np.int32)).all():
            assert lo[1].view(np.int32) == ln[1].view(np.int32), (k, lo[1], ln[1])
    for name in old.files:
        if not name.startswith("losses"):
            same_bits(old, new, name)
    # the slots hold what a head leaves: actions inside tanh's range, a positive reciprocal standard deviation
    for k in (0, 2, 4):
        a = new[f"outv_api{k}"].view(np.float32)
        assert a.shape == (B, 4) and np.isfinite(a).all() and np.abs(a).max() <= 1.0 and np.abs(a).max() > 0.0
        assert (new[f"st2_api{k}"].view(np.float32)[:, 1] > 0).all()
    assert ("outv_bcs0" in new.files) == (mode in ("soft", "noln"))
    assert np.isfinite(new["losses5"]).all()


def test_head_riders_write_their_rows_and_nothing_else(runs):
    """B = 48: three row tiles in sixteen spare workgroup slots, one head job.  Around outv[0:48][0:4] and st2[0:48] of actor(s)'s slot everything keeps its
    sentinel: columns 4..7 of the action rows (where st2 rows beyond the batch would land), the words behind the action rows (outv rows beyond the batch),
    and the whole slot of bc_actor(s) (a second head job that is not there)."""
    old, new = load(runs, "guard")
    for r in (old, new):
        assert (r["outv"][:, 4:] == SENTINEL).all()
        assert (r["behind"] == SENTINEL).all()
        assert (r["bcs"] == SENTINEL).all()
    assert (old["outv"][:, :4] == SENTINEL).all() and (old["st2"] == SENTINEL).all()  # knob off: this call has no launch that evaluates the head
    a = new["outv"][:, :4]
    assert np.isfinite(a).all() and np.abs(a).max() <= 1.0 and (a != SENTINEL).all()
    assert (new["st2"] != SENTINEL).all() and (new["st2"][:, 1] > 0).all()
