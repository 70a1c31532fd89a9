"""CPU tests of success upsampling: the integer model (tests/_upsample_model.py) against a brute-force cumulative sum over explicit per-slot weights, its
exactness on a tiny ring, the edge words, train_all's flags and refusals, the façade's host rule for expert_upsample, the Philox model against a known
vector, and the coverage of the seeded inputs that tests/test_upsample_gpu.py feeds to hx_ups_*."""
import types

import numpy as np
import pytest

from tests import _upsample_model as M

CAP = 3000  # three blocks of 1,024 with a ragged last one (the GPU tests' ring)
LIVES = (1, 63, 64, 65, 1023, 1024, 1025, 3000)


@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_model_equals_brute_force(pattern):
    for live in LIVES:
        lab = M.make_labels(pattern, CAP, live, seed=live)
        cnt = M.counts(lab, live, CAP)
        words = M.make_words(lab, live, CAP, 10, 64, seed=live)
        np.testing.assert_array_equal(M.draw_slots(lab, cnt, live, CAP, 10, words), M.brute_slots(lab, live, CAP, 10, words))
        assert M.weight_total(cnt, live, CAP, 10) == int(M.slot_weights(lab, live, CAP, 10).sum())
    # a wrapped ring: total beyond cap, every slot live
    lab = M.make_labels(pattern, CAP, CAP, seed=7)
    words = M.make_words(lab, 5 * CAP + 17, CAP, 3, 64, seed=1)
    np.testing.assert_array_equal(M.draw_slots(lab, M.counts(lab, 5 * CAP + 17, CAP), 5 * CAP + 17, CAP, 3, words), M.brute_slots(lab, 5 * CAP + 17, CAP, 3, words))


def test_every_target_hits_its_slot_exactly_weight_times():
    """a tiny ring: enumerating every t in [0, W) hits slot i exactly w_i times, and never a slot beyond the live length"""
    cap, live, boost = 40, 29, 10
    lab = np.zeros(cap, np.int8)
    lab[[0, 5, 6, 28]] = 1
    lab[[3, 9]] = -1
    lab[30:] = 1  # stale labels beyond the live length weigh nothing
    w = M.slot_weights(lab, live, cap, boost)
    W = int(w.sum())
    assert W == live + 9 * 4
    words = [M.word_for_target(t, W) for t in range(W)]
    idx = M.draw_slots(lab, M.counts(lab, live, cap), live, cap, boost, words)
    np.testing.assert_array_equal(np.bincount(idx, minlength=cap), w)
    assert idx.max() < live


def test_edge_words():
    lab = M.make_labels("mixed", CAP, 2000, seed=3)
    W = M.weight_total(M.counts(lab, 2000, CAP), 2000, CAP, 10)
    assert M.target(0, W) == 0 and M.target(M.MASK64, W) == W - 1
    first, last = M.draw_slots(lab, M.counts(lab, 2000, CAP), 2000, CAP, 10, [0, M.MASK64])
    assert first == 0 and last == 1999
    assert M.fire_replacement(0, 0, 7, 128) == (0, 0) and M.fire_replacement(M.MASK64, M.MASK64, 7, 128) == (6, 127)
    assert M.fire_replacement(M.MASK64, 1 << 63, 1, 128) == (0, 64)


def test_no_success_row_is_the_uniform_draw():
    """without a success row the target IS the uniform index (word n) >> 64"""
    lab = M.make_labels("none", CAP, 1025, seed=1)
    words = M.make_words(lab, 1025, CAP, 10, 200, seed=2)
    np.testing.assert_array_equal(M.draw_slots(lab, M.counts(lab, 1025, CAP), 1025, CAP, 10, words), [(x * 1025) >> 64 for x in words])


def test_mark_new_model_covers_only_touched_blocks():
    lab = M.make_labels("mixed", CAP, CAP, seed=5)
    cnt0 = np.zeros(3, np.uint32)
    cnt, marked = M.mark_new(cnt0, 0, lab, 1500, CAP, 100)  # 1,500 rows arrived, the bound says 100: block 0 only, marked = 100
    assert marked == 100 and cnt[0] == M.counts(lab, 1500, CAP)[0] and cnt[1] == 0
    assert M.touched_blocks(2990, 3020, CAP, 64) == ([0, 2], 3020)  # a wrapped range
    assert M.touched_blocks(0, 9000, CAP, 1 << 20) == ([0, 1, 2], 9000)  # more than cap new rows: the whole ring
    assert M.touched_blocks(5, 5, CAP, 64) == ([], 5)


def test_philox_model_known_vector():
    """Philox4x32-10 of the Random123 known-answer tests: counter and key all ones"""
    assert M.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert M.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    w = M.philox_words(7, 3, 4, fire=True)
    assert len(w) == 6 and len(set(w)) == 6 and M.philox_words(7, 3, 4) == w[:4] and M.philox_words(7, 4, 4) != w[:4]


def test_seeded_inputs_cover_the_edges():
    """what tests/test_upsample_gpu.py relies on"""
    for live in LIVES:
        for pattern in M.PATTERNS:
            lab = M.make_labels(pattern, CAP, live, seed=live)
            n1 = int((lab[:live] == 1).sum())
            if pattern == "none":
                assert n1 == 0
            if pattern == "all":
                assert n1 == live
            if pattern == "last_live":
                assert n1 == 1 and lab[live - 1] == 1
            if pattern == "beyond_live":
                assert n1 == 0 and (live == CAP or (lab[live:] == 1).all())
            if pattern == "boundaries" and live > 1025:
                assert lab[1023] == 1 and lab[1024] == 1 and lab[2047] == 1 and lab[2048] == 1
            if pattern == "mixed" and live >= 63:
                assert {-1, 0, 1} <= set(lab[:live].tolist())
            words = M.make_words(lab, live, CAP, 10, 16, seed=1)
            assert words[0] == 0 and words[1] == M.MASK64 and len(words) == 16
    # every slot of a small ring: the first and the last target of each interval
    lab = M.make_labels("mixed", 70, 65, seed=2)
    words = M.make_words(lab, 65, 70, 10, 0, every_slot=True)
    assert len(words) == 2 + 2 * 65
    idx = M.draw_slots(lab, M.counts(lab, 65, 70), 65, 70, 10, words[2:])
    np.testing.assert_array_equal(idx, np.repeat(np.arange(65), 2))
    W = int(M.slot_weights(lab, 65, 70, 10).sum())
    for s in (0, 17, 64):
        lo, hi = M.slot_interval(lab, 65, 70, 10, s)
        assert M.target(words[2 + 2 * s], W) == lo and M.target(words[3 + 2 * s], W) == hi


def test_parse_args_accepts_and_refuses(capsys):
    from hirl4ucav_amd import train_all as T

    cfg = T.parse_args(["--agent", "HIRL", "--type", "soft", "--buffer_upsample", "--expert_upsample"])
    assert cfg.buffer_upsample and cfg.expert_upsample and cfg.upsample_boost == 10
    for argv in (["--agent", "HIRL", "--type", "linear", "--buffer_upsample", "--upsample_boost", "2"], ["--agent", "HIRL", "--type", "fixed", "--expert_upsample"],
                 ["--agent", "TD3", "--buffer_upsample", "--upsample_boost", "255"], ["--agent", "BC", "--expert_upsample"],
                 ["--agent", "HIRL", "--buffer_upsample", "--dtype", "bf16"], ["--agent", "HIRL", "--buffer_upsample", "--gpus", "1"]):
        T.parse_args(argv)
    plain = T.parse_args(["--agent", "HIRL"])
    assert not plain.buffer_upsample and not plain.expert_upsample and T.upsample_refusal(plain) is None
    for argv, word in ((["--agent", "SAC", "--type", "SAC", "--buffer_upsample"], "not --agent SAC"),
                       (["--agent", "SAC", "--type", "SAC", "--expert_upsample"], "not --agent SAC"),
                       (["--agent", "BC", "--buffer_upsample"], "no replay ring"),
                       (["--agent", "TD3", "--expert_upsample"], "no expert table"),
                       (["--agent", "HIRL", "--buffer_upsample", "--gpus", "2"], "one GPU"),
                       (["--agent", "HIRL", "--buffer_upsample", "--upsample_boost", "1"], "2..255"),
                       (["--agent", "HIRL", "--buffer_upsample", "--upsample_boost", "256"], "2..255")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        err = capsys.readouterr().err
        assert "upsample" in err and word in err, (argv, err)
    cfg = types.SimpleNamespace(agent="HIRL", type="soft", buffer_upsample=False, expert_upsample=True, gpus=None, upsample_boost=10)
    assert T.upsample_refusal(cfg) is None and T.upsample_refusal(cfg, n_fire=3) is None
    assert "one GPU" in T.upsample_refusal(cfg, world=2) and "no row whose fire action is 1" in T.upsample_refusal(cfg, n_fire=0)


def test_uniform_memory_keeps_refusing_and_names_the_new_class():
    pytest.importorskip("torch")
    from hirl4ucav_amd.utils.buffer import UniformMemory

    with pytest.raises(NotImplementedError, match="SuccessUpsampler"):
        UniformMemory(100, upsample=True)


def test_facade_expert_upsample_host_rule():
    """Agent.learn with expert_upsample: idx_bc[np.random.randint(B)] <- np.random.choice(target_indices), drawn AFTER the np.random.choice(...,
    replace=False) of HIRL.py:249 and in the reference's order (the fire row, then the row it replaces); off: the plain draw"""
    torch = pytest.importorskip("torch")
    from hirl4ucav_amd.agents.HIRL import Agent

    B, N = 16, 200
    rng = np.random.default_rng(0)
    actions = rng.uniform(-1, 1, (N, 4)).astype(np.float32)
    actions[[7, 90, 150], 3] = 1.0
    seen = {}

    class Eng:
        actor_trainable = True

        def assemble(self, ring, idx, expert_ring=None, n_main=None, bc_table=None, idx_bc=None):
            seen["idx_bc"] = idx_bc.cpu().numpy().copy()

        def learn(self, **kw):
            pass

        def losses_host(self):
            return (0.0,) * 6

    buf = types.SimpleNamespace(sample_indices=lambda k: list(range(k)), ring=None)
    ag = object.__new__(Agent)
    ag.__dict__.update(batchSize=B, expert_warm_up=False, buffer=buf, expert_buffer=buf, expert_states=np.zeros((N, 13), np.float32), expert_actions=actions,
                       actionDim=4, TD3LearningNoise=0.2, eng=Eng(), _bc_table=None, _last=(0.0,) * 6, bc_weight=0.0,
                       target_indices=np.where(actions[:, 3] == 1)[0], expert_upsample=False, buffer_upsample=False)
    np.testing.assert_array_equal(ag.target_indices, [7, 90, 150])
    np.random.seed(5)
    ag.learn(0.0, 0)
    plain = seen["idx_bc"]
    np.random.seed(5)
    want = np.random.choice(N, B, replace=False)
    np.testing.assert_array_equal(plain, want)
    selected = np.random.choice(ag.target_indices)
    want[np.random.randint(B)] = selected
    ag.expert_upsample = True
    np.random.seed(5)
    ag.learn(0.0, 0)
    np.testing.assert_array_equal(seen["idx_bc"], want)
    assert (seen["idx_bc"] != plain).sum() <= 1 and selected in (7, 90, 150)
    assert torch is not None
