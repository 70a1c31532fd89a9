"""The episode record without a GPU: the numpy model of hx_trace_push against a loop written the way the reference's validate() collects its
lists (train_all.py:22-66), the coverage of the seeded stream both test files use, the reference's file set, the flags, and the host-only
helpers of utils/trace.py on arrays."""
import csv
import os

import numpy as np
import pytest

from hirl4ucav_amd import _lib
from hirl4ucav_amd.utils import trace as TR
from tests import _trace_model as M

K, STEPS = 130, 24


@pytest.fixture(scope="module")
def s():
    return M.stream()


@pytest.fixture(scope="module")
def model(s):
    return M.run(M.TraceModel(K, STEPS), s)


def reference_loop(s, i, steps):
    """one episode of env i as validate() runs it: step while not done, append before looking at done, read the env's flags when done is SEEN"""
    total, done = 0.0, False
    out = {"self_pos": [], "oppo_pos": [], "distance": [], "fire": [], "lock": [], "missile": [], "launches": 0, "hits": 0, "kill": False,
           "fire_success": False, "end_step": -1}
    flags = 0
    for step in range(steps):
        if not done:
            st = s["state"][step]
            reward, done, success = float(s["reward"][step, i]), bool(s["done"][step, i]), int(s["success"][step, i])
            flags = int(st[M.W_FLAGS, i])
            total += reward
            with np.errstate(invalid="ignore"):
                a = st[0:3, i].copy().view(np.float32).astype(np.float64)
                o = st[13:16, i].copy().view(np.float32).astype(np.float64)
            d = a - o
            out["distance"].append(float(np.sqrt((d * d).sum())))
            if flags & _lib.F_FIRED:
                out["fire"].append(step)
            if flags & _lib.F_LOCKED_PREV:
                out["lock"].append(step)
            if flags & _lib.F_SLOT_PREV:
                out["missile"].append(step)
            out["self_pos"].append(a)
            out["oppo_pos"].append(o)
            out["launches"] += success != 0
            out["hits"] += success == 1
            if done:
                out["end_step"] = step
            if step == steps - 1:
                break
        else:
            break
    if done:  # the env has not been stepped since: its flags are those of the step that raised done
        out["kill"], out["fire_success"] = bool(flags & _lib.F_EPISODE_SUCCESS), bool(flags & _lib.F_FIRE_SUCCESS)
    out["total"] = total
    return out


def same(a, b):
    """equal as bits where both are float arrays (NaN positions compare equal to themselves)"""
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_model_is_the_references_loop(s, model):
    kill, fire_success = TR.summary_masks(model.end_flags)
    for j in range(K):
        ref = reference_loop(s, j, STEPS)
        T = int(model.nrec[j])
        ep = TR.decode_episode(model.log[:, :T, j])
        assert T == len(ref["distance"])
        assert same(ep["self_pos"], np.array(ref["self_pos"]).reshape(T, 3)) and same(ep["oppo_pos"], np.array(ref["oppo_pos"]).reshape(T, 3))
        assert same(ep["distance"], ref["distance"])
        assert (ep["fire"], ep["lock"], ep["missile"]) == (ref["fire"], ref["lock"], ref["missile"])
        assert float(model.total[j]) == ref["total"]  # integer-valued rewards: the fp32 sum and the float64 loop agree exactly
        assert float(ep["reward"].astype(np.float64).sum()) == ref["total"]
        assert int(model.end_step[j]) == ref["end_step"]
        assert (int(model.launches[j]), int(model.hits[j])) == (ref["launches"], ref["hits"])
        assert (bool(kill[j]), bool(fire_success[j])) == (ref["kill"], ref["fire_success"])
        assert ep["success"].tolist() == s["success"][:T, j].tolist()
    assert model.alive == int((model.end_step < 0).sum())


def test_stream_covers_the_edges(s, model):
    done, succ, end = s["done"][:, :K] != 0, s["success"][:, :K], model.end_step
    assert (end == 0).sum() >= 1
    assert (end == STEPS - 1).sum() >= 1
    assert (end < 0).sum() >= 10
    after = np.arange(STEPS)[:, None] > np.where(end < 0, STEPS, end)[None, :]  # [t, j]: t lies behind env j's end
    assert (done & after).any(0).sum() >= 10
    running = ~after
    for v in (-1, 0, 1):
        assert ((succ == v) & running).any() and ((succ == v) & after).any()
    assert np.isnan(s["state"][:, 0:3, :K].copy().view(np.float32)).any()  # NaN payloads travel through the log as bits
    assert (s["done"] > 1).any() and (s["state"][:, M.W_FLAGS] >> 16).any()


def test_reset_and_replay_and_gather(s, model):
    again = M.run(model.__class__(K, STEPS), s)
    M.run(again, s)
    assert np.array_equal(again.log, model.log) and all(np.array_equal(a, b) for a, b in zip(again.summaries().values(), model.summaries().values()))
    ids = np.random.default_rng(1).permutation(300)[:65]
    g, full = M.run(M.TraceModel(65, STEPS, ids), s), M.run(M.TraceModel(300, STEPS), s)
    assert np.array_equal(g.total, full.total[ids]) and np.array_equal(g.end_step, full.end_step[ids])
    for jj, i in enumerate(ids):
        T = full.nrec[i]
        assert np.array_equal(g.log[:, :T, jj], full.log[:, :T, i])


def test_files_read_back_row_for_row(tmp_path, s, model):
    j = int(np.argmax(model.nrec == STEPS))
    # (positions folded into the finite range: the CSV round trip is about rows and columns)
    ep = TR.decode_episode(np.concatenate([model.log[:6, :STEPS, j] % np.uint32(0x4B000000), model.log[6:, :STEPS, j]]))
    TR.write_episode_files(ep, str(tmp_path), 7)
    rows = (lambda name: list(csv.reader(open(os.path.join(tmp_path, "csv", f"{name}7.csv"), newline=""))))
    assert sorted(os.listdir(tmp_path / "csv")) == ["distance7.csv", "fire7.csv", "lock7.csv", "oppo_pos7.csv", "self_pos7.csv"]
    for name in ("self_pos", "oppo_pos"):
        got = rows(name)
        assert len(got) == STEPS and all(len(r) == 3 for r in got)
        assert np.array_equal(np.array(got, np.float64), ep[name])
    got = rows("distance")
    assert all(len(r) == 1 for r in got) and np.array_equal(np.array(got, np.float64)[:, 0], ep["distance"])
    assert [[str(i)] for i in ep["fire"]] == rows("fire") and [[str(i)] for i in ep["lock"]] == rows("lock")
    assert ep["fire"] and ep["lock"]


def test_figures_exist(tmp_path, model):
    pytest.importorskip("matplotlib")
    j = int(np.argmax(model.nrec == STEPS))
    ep = TR.decode_episode(np.concatenate([model.log[:6, :STEPS, j] % np.uint32(0x4B000000), model.log[6:, :STEPS, j]]))
    TR.write_episode_files(ep, str(tmp_path), "round1")
    for f in ("trajectories_round1.png", "distance_round1.png"):
        assert os.path.getsize(tmp_path / f) > 0


def test_plot_flags_parse():
    from hirl4ucav_amd import train_all, validate_all

    assert train_all.parser().parse_args(["--plot"]).plot is True and train_all.parser().parse_args([]).plot is False
    base = ["--model_name", "x", "--model_dir", "/a/model"]
    a = validate_all.parser().parse_args(base + ["--plot", "--plot_dir", "/p"])
    assert (a.plot, a.plot_dir) == (True, "/p")
    a = validate_all.parser().parse_args(base)
    assert (a.plot, a.plot_dir) == (False, None)
    assert validate_all.plot_dir_of(a) == os.path.normpath("/a/plot")


def test_plot_helpers_live_in_the_product_package():
    import hirl.utils.plot as alias
    from hirl4ucav_amd.utils import plot

    for name in ("plot_3d_trajectories", "plot_distance", "plot_2d_trajectories"):
        assert getattr(alias, name) is getattr(plot, name)


def test_env_id_checks():
    assert TR.check_env_ids(None, 5) is None
    ids = TR.check_env_ids([4, 0, 2], 5)
    assert ids.dtype == np.int32 and ids.tolist() == [4, 0, 2]
    assert TR.check_env_ids(np.array([3], np.int64), 5).tolist() == [3]
    for bad in ([0, 5], [-1], [1, 1], [], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            TR.check_env_ids(bad, 5)


def test_workspace_layout_and_flag_decoding():
    off, words = TR.workspace_layout(130, 24)
    assert words == 130 * (8 * 24 + 6) + 1 and off["log"] == 0 and off["total"] == 8 * 24 * 130 and off["alive"] == words - 1
    assert [off[n] - off["total"] for n in TR.SUMMARY_NAMES] == [130 * i for i in range(6)]
    sm = TR.split_summary(np.arange(12, dtype=np.uint32) + np.uint32(0xFFFFFFFA), 2)
    assert sm["end_step"].tolist() == [-2, -1] and sm["end_flags"].tolist() == [0, 1] and sm["total"].dtype == np.float32
    kill, fired = TR.summary_masks(np.array([0, _lib.F_EPISODE_SUCCESS, _lib.F_FIRE_SUCCESS | _lib.F_DONE, 0xFFFF0000], np.uint32))
    assert kill.tolist() == [False, True, False, False] and fired.tolist() == [False, False, True, False]
    log = np.zeros((8, 3), np.uint32)
    log[0:3, 1] = np.array([3.0, 0.0, 4.0], np.float32).view(np.uint32)
    log[7] = [_lib.F_FIRED | (0xFF << 16), _lib.F_LOCKED_PREV | _lib.F_SLOT_PREV | (1 << 16), _lib.F_LOCKED | _lib.F_SLOT]
    ep = TR.decode_episode(log)
    assert (ep["fire"], ep["lock"], ep["missile"]) == ([0], [1], [1]) and ep["success"].tolist() == [-1, 1, 0]
    assert ep["distance"].tolist() == [0.0, 5.0, 0.0] and ep["self_pos"].shape == (3, 3) and ep["self_pos"].dtype == np.float64
