"""Replay-ring slots in row-tile order (include/hirl4ucav.h HX_LAYOUT_ORDERED_SLOTS), as bench.py's loop fills its ring: each step's rows land in env
order, two runs with the same arguments hold the same ring, draw the same minibatches and end with the same networks bit for bit, and the ring holds
exactly the rows that one atomic per workgroup would have stored."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")


def make(argv, ordered=True):
    import bench

    return bench.Loop(bench.parse(argv + ["--ordered-slots"]), 0, 1, torch.device("cuda", 0), ordered_slots=ordered)


@needs_gpu
@pytest.mark.parametrize("argv", [["--no-front"], ["--agent", "sac", "--scenario", "serpentine"]])
def test_each_step_stores_its_rows_in_env_order(argv):
    """The per-tile acting launch (HIRL's 32-row, SAC's 16-row workgroups at 4,096 envs): step t's n rows are slots [T0, T0 + n) in env order."""
    loop = make(argv)
    assert not loop.front and loop.replay.slot_header is not None
    n = loop.env.n
    for _ in range(3):
        prev = loop.env.obs.clone()
        t0 = int(loop.replay.total.item())
        loop.step()
        torch.cuda.synchronize()
        assert int(loop.replay.total.item()) == t0 + n  # no episode reaches its time limit in three steps: every env stores
        assert torch.equal(loop.replay.ring[t0:t0 + n, 0:13], prev)
    assert loop.replay.slot_status() == 0
    loop.close()


@needs_gpu
@pytest.mark.parametrize("argv", [[], ["--no-front"]])
def test_same_arguments_fill_the_ring_and_draw_the_same_minibatches(argv):
    """bench.py's default front loop and the reference-order loop: 40 steps, twice — ring, last minibatch, networks and actions bit for bit."""
    runs = []
    for _ in range(2):
        loop = make(argv)
        for _ in range(40):
            loop.step()
        torch.cuda.synchronize()
        n = int(loop.replay.total.item())
        runs.append([loop.replay.ring[:n].clone(), loop.eng.rows.clone(), loop.eng.actor.clone(), loop.eng.critic.clone(), loop.actions.clone(),
                     loop.replay.slot_status(), loop.front])
        loop.close()
        del loop
    a, b = runs
    assert a[0].shape[0] == 40 * 4096 and a[6] == (argv == [])
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    assert a[5] == b[5] == 0


@needs_gpu
def test_ordered_ring_holds_the_rows_an_atomic_ring_holds():
    """After one step the two rings hold the same rows, in some order for the atomic one: no slot was lost or written twice."""
    rows = []
    for ordered in (True, False):
        loop = make(["--no-front"], ordered)
        assert (loop.replay.slot_header is not None) == ordered
        loop.step()
        torch.cuda.synchronize()
        r = loop.replay.ring[:int(loop.replay.total.item())].cpu().numpy()
        rows.append(r[np.lexsort(r.T[::-1])])
        loop.close()
        del loop
    assert rows[0].shape == rows[1].shape == (4096, 32)
    np.testing.assert_array_equal(rows[0], rows[1])
