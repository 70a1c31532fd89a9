"""CPU tests of self-imitation (include/hirl4ucav.h "Self-imitation"): the numpy model of the rule (tests/_selfimit_model.py) held to the invariants the
header states, on seeded streams that provably contain every case; the host-only helpers of utils/selfimit.py, SelfExpert's ring / table / snapshot
record, train_all's flags and every refusal by name.  The kernels are held to the model, bit for bit, by tests/test_selfimit_gpu.py."""
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _selfimit_model as M  # noqa: E402


def run_stream(n, L, m, e0, calls=60, seed=0, bc_e0=None, cursor=0, check=None):
    off, lab = M.make_offline(e0)
    ring0, succ0 = M.initial_ring(off, lab, m)
    bc = None
    if bc_e0 is not None:
        bc = M.initial_ring(M.make_offline(bc_e0, seed=12)[0], np.zeros(bc_e0, np.int8), m)[0]
    obs0, ctr0, stream = M.make_stream(n, L, calls, seed)
    model = M.SelfModel(ring0, succ0, e0, m, n, L, obs0, ctr0, bc=bc, bc_e0=bc_e0 or 0, cursor=cursor)
    for c, args in enumerate(stream):
        before = (model.ring.copy(), model.success.copy(), model.cursor, list(model.counters))
        accepted = model.push(*args)
        if check is not None:
            check(model, before, accepted, args, c)
    return model, (off, lab)


def test_model_invariants_on_a_seeded_stream():
    """offline rows untouched; every slot a complete row after every call; the written rows of one episode contiguous mod M and oldest first; accepted
    episodes a leading run in env order; the cursor the sum of accepted rows"""
    n, L, m, e0 = 130, 5, 12, 3
    off, lab = M.make_offline(e0)
    total = [0]

    def check(model, before, accepted, args, c):
        ring0, succ0, cursor0, counters0 = before
        obs_new, act, rew, done, succ, ctr = args
        assert np.array_equal(model.ring[:e0], M.u32(off)) and np.array_equal(model.success[:e0], lab)
        kills = [e for e in range(n) if done[e] and rew[e] > 0]
        envs = [e for e, _ in accepted]
        assert envs == kills[:len(envs)], "a leading run of the kill envs, in env order"
        k, seen = 0, set()
        for e, slots in accepted:
            assert 1 <= len(slots) <= L
            for j, slot in enumerate(slots):
                assert slot == e0 + (cursor0 + k) % m and slot not in seen  # contiguous mod M from the cursor on, no slot twice
                seen.add(slot)
                k += 1
                row = model.ring[slot]
                if M.finite_bits(row).all() and not np.array_equal(row, ring0[slot]):
                    assert row[31] == np.float32(1.0 if j == len(slots) - 1 else 0.0).view(np.uint32)
                    if j + 1 < len(slots) and M.finite_bits(model.ring[slots[j + 1]]).all() and not np.array_equal(model.ring[slots[j + 1]], ring0[slots[j + 1]]):
                        assert np.array_equal(row[17:30], model.ring[slots[j + 1]][0:13]), "s' of row j is s of row j + 1: oldest first"
                    if j == len(slots) - 1:
                        assert np.array_equal(row[17:30], M.u32(obs_new[e])) and row[30] == M.u32(rew[e:e + 1])[0]
        assert k <= m and model.cursor == cursor0 + k
        total[0] += k
        untouched = np.ones(e0 + m, bool)
        untouched[list(seen)] = False
        assert np.array_equal(model.ring[untouched], ring0[untouched]) and np.array_equal(model.success[untouched], succ0[untouched])
        assert M.finite_bits(model.ring).all(), "every slot holds a complete (finite) row: a non-finite row is never written"
        assert model.counters[M.KILLS] - counters0[M.KILLS] == len(kills)
        assert model.counters[M.DROPPED] - counters0[M.DROPPED] == len(kills) - len(envs)

    model, _ = run_stream(n, L, m, e0, check=check)
    assert model.cursor == total[0] > 5 * m and model.counters[M.EPISODES] > 20
    assert model.counters[M.ROWS] + model.events["nonfinite_rows"] == total[0]


def test_the_seeded_stream_covers_every_case():
    """60 calls, 130 envs, L = 5, M = 12: kills of episodes shorter than, as long as and longer than L, a kill on an episode's first step, a done without a
    kill, the time limit, two kills of one call inside one 64-env group and in different groups, a call whose kill rows exceed M (a drop), the cursor
    crossing M, a non-finite row — each counted; and the same at L = 1"""
    model, _ = run_stream(130, 5, 12, 3)
    ev = model.events
    print(ev, model.counters)
    for key in ("kill_short", "kill_full", "kill_long", "kill_first", "done_no_kill", "trunc", "same_group", "other_group", "drop_calls", "wraps", "nonfinite_rows"):
        assert ev[key] >= 1, key
    assert ev["calls"] == 60 and ev["drop_calls"] >= 2 and model.counters[M.DROPPED] >= 100
    one, _ = run_stream(130, 1, 5, 3)
    assert one.events["kill_full"] + one.events["kill_long"] == one.counters[M.KILLS] > 0 and one.events["kill_short"] == 0
    assert one.events["drop_calls"] >= 1 and one.events["wraps"] >= 1 and one.counters[M.EPISODES] == one.counters[M.ROWS] + one.events["nonfinite_rows"]
    small, _ = run_stream(1, 2, 5, 3)  # one env: never a drop (L <= M)
    assert small.counters[M.DROPPED] == 0 and small.counters[M.EPISODES] == small.counters[M.KILLS] > 0


@pytest.mark.parametrize("cursor0", [2 ** 32 - 2, 2 ** 40, 2 ** 64 - 3])
def test_the_cursor_is_a_64_bit_word(cursor0):
    """slots follow (cursor + k) mod M in exact arithmetic; the cursor itself is stored mod 2^64"""
    seen = []
    model, _ = run_stream(65, 2, 12, 3, calls=30, cursor=cursor0, check=lambda mo, before, acc, args, c: seen.append((before[2], acc)))
    for cur, acc in seen:
        k = 0
        for _, slots in acc:
            for slot in slots:
                assert slot == 3 + (cur + k) % 12
                k += 1
    total = sum(len(s) for _, acc in seen for _, s in acc)
    assert total > 12 and model.cursor == (cursor0 + total) % 2 ** 64


def test_the_bc_table_takes_the_same_rows():
    """after every call: the slot of every accepted row that was written to the ring (a finite row) holds that row's (s, a) and 15 zero words in the table,
    at the same online index; every other table row is what it was; the offline table rows stand"""
    e0, b0, m = 3, 7, 12
    table0 = M.u32(M.initial_ring(M.make_offline(b0, seed=12)[0], np.zeros(b0, np.int8), m)[0])
    state = {"bc": table0.copy(), "rewritten": 0, "skipped": 0}

    def check(model, before, accepted, args, c):
        ring0, want = before[0], state["bc"].copy()
        for _, slots in accepted:
            for slot in slots:
                if np.array_equal(model.ring[slot], ring0[slot]):  # not written: a non-finite row (a written row carries this call's fresh words)
                    state["skipped"] += 1
                    continue
                want[b0 + slot - e0, :17], want[b0 + slot - e0, 17:] = model.ring[slot, :17], 0
                state["rewritten"] += 1
        assert np.array_equal(model.bc, want), c
        state["bc"] = model.bc.copy()

    model, _ = run_stream(65, 5, 12, e0, bc_e0=b0, check=check)
    assert state["rewritten"] == model.counters[M.ROWS] > 3 * m and state["skipped"] == model.events["nonfinite_rows"] >= 1
    assert np.array_equal(model.bc[:b0], table0[:b0]) and not np.array_equal(model.bc[b0:], table0[b0:]) and (model.bc[b0:, 17:] == 0).all()


# ---- host helpers -------------------------------------------------------------------------------------------------------------------------------
def test_host_helpers():
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils import selfimit as S

    assert S.tape_bytes(4096, 256) == 76 * 256 * 4096 == 79_691_776 and S.tape_bytes(1, 1) == 76
    assert (S.SELF_FIELDS, S.SELF_MAX_STEPS, S.SELF_COUNTERS) == (19, 65535, 4)
    for args, word in (((8, 5, 0, 1), "online_rows 0"), ((8, 0, 4, 1), "offline table is empty"), ((0, 5, 4, 1), "n_envs 0"), ((2 ** 31, 5, 4, 1), "n_envs"),
                       ((8, 5, 4, 0), "steps 0"), ((8, 5, 70000, 65536), "steps 65536"), ((8, 5, 4, 5), "steps 5 > online_rows 4"),
                       ((8, 2 ** 31 - 4, 4, 1), "fewer than 2\\^31")):
        assert re.search(word, S.self_args_refusal(*args)), args
    assert S.self_args_refusal(8, 5, 4, 4) is None and S.self_args_refusal(2 ** 31 - 1, 1, 65535, 65535) is None
    lay = S.workspace_layout(130, 5)
    assert lay["tape"] == (0, 19 * 5 * 130) and lay["obs_prev"] == (12350, 13 * 130) and lay["len"][0] == 12350 + 1690 and lay["groups"] == 3
    assert lay["wcount"] == (12350 + 1690 + 390, 4) and lay["wkills"][1] == 4 and lay["cursor"][0] % 2 == 0 and lay["cursor"][1] == 4
    assert lay["counters"] == (lay["cursor"][0] + 4, 24) and lay["words"] == lay["counters"][0] + 24
    odd = S.workspace_layout(1, 1)  # 19 + 13 + 3 + 2 + 2 = 39 words: one pad word in front of the 64-bit part
    assert odd["cursor"][0] == 40 and odd["words"] == 40 + 4 + 8
    L = _lib.load()
    for n, steps in ((1, 1), (63, 2), (64, 5), (65, 5), (130, 5), (4096, 256), (131072, 7)):
        assert int(L.hx_self_workspace_words(n, steps)) == S.workspace_layout(n, steps)["words"], (n, steps)
    assert [int(L.hx_self_workspace_words(*a)) for a in ((0, 1), (-1, 1), (2 ** 31, 1), (8, 0), (8, 65536))] == [0] * 5
    assert "HxSelf" not in _lib.STRUCTS  # (one workspace pointer crosses the boundary, no struct)
    assert S.counter_sums(torch.arange(12, dtype=torch.int64)) == (3, 12, 21, 30)
    hdr = open(_lib._abi.INCLUDE_DIR + "/hirl4ucav.h").read()
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 133 and "133: self-imitation" in hdr and "dist < 5.7e6 m" in hdr


def cpu_expert(n=8, m=12, steps=5, e0=5, bc=None):
    from hirl4ucav_amd.utils import selfimit as S

    env = types.SimpleNamespace(n=n, device=torch.device("cpu"))
    off, lab = M.make_offline(e0)
    table = None if bc is None else torch.from_numpy(M.make_offline(bc, seed=12)[0])
    return S.SelfExpert(env, torch.from_numpy(off), torch.from_numpy(lab), m, steps, bc_table_offline=table), off, lab


def test_self_expert_builds_branch_experts_ring_and_round_trips():
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils import pilot as P
    from hirl4ucav_amd.utils import selfimit as S

    se, off, lab = cpu_expert(bc=7)
    env = types.SimpleNamespace(n=8, device=torch.device("cpu"))
    be = P.BranchExpert(env, torch.from_numpy(off), torch.from_numpy(lab), 12, 4)
    assert torch.equal(se.ring.ring.view(torch.int32), be.ring.ring.view(torch.int32)) and torch.equal(se.ring.success, be.ring.success)
    assert se.ring.capacity == 5 + 12 + P.BRANCH_SLACK and se.ring.fixed_len == 17
    oe = P.OnlineExpert(env, torch.from_numpy(M.make_offline(7, seed=12)[0]), 12, 4)
    assert torch.equal(se.table, oe.table) and se.bc_offline_rows == 7
    assert se.work.numel() == S.workspace_layout(8, 5)["words"] and not bool(se.work.any())
    for fn, args in ((se.push, (torch.zeros(8, 4),)), (se.reset, ())):
        with pytest.raises(_lib.HxError, match="runs on the GPU only"):
            fn(*args)
    # a state with content, written by hand (the kernels need the GPU)
    se.ring.ring[5:17] = torch.arange(12 * 32, dtype=torch.float32).reshape(12, 32)
    se.ring.success[5:17] = 1
    se.table[7:] = 3.0
    se.call = 7
    se.set_cursor(2 ** 64 - 3)
    se._part("counters").view(torch.int64)[:] = torch.tensor([4, 3, 9, 1])
    se._part("len")[:] = 2  # tape-side state: not in the record
    st = se.state_dict()
    assert set(st) == {"online", "success", "call", "online_rows", "steps", "offline_rows", "bc", "cursor", "counters", "bc_online", "bc_offline_rows"}
    assert st["cursor"] == 2 ** 64 - 3 and st["call"] == 7 and st["bc"] is True and sum(v.numel() * v.element_size() for v in st.values() if torch.is_tensor(v)) < 4096
    other, _, _ = cpu_expert(bc=7)
    other.load_state_dict(st)
    assert other.call == 7 and other.cursor() == 2 ** 64 - 3 and other.counters() == (4, 3, 9, 1) == se.counters()
    assert torch.equal(other.ring.ring, se.ring.ring) and torch.equal(other.ring.success, se.ring.success) and torch.equal(other.table, se.table)
    assert not bool(other._part("len").any()), "the tape's side of the workspace is not restored: every len starts at 0"
    for kw, word in ((dict(m=13), "--expert_self 12 --expert_self_steps 5 --expert_self_bc, this run has --expert_self 13"), (dict(steps=4), "this run has --expert_self 12 --expert_self_steps 4"),
                     (dict(bc=None), "--expert_self_bc, this run has --expert_self 12 --expert_self_steps 5$"), (dict(e0=6), "behind 5 offline expert rows"),
                     (dict(bc=8), "behind 7 offline rows"), (dict(n=65), "cover 1 groups")):
        args = dict(bc=7)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            cpu_expert(**args)[0].load_state_dict(st)
    for kw, word in ((dict(steps=13), "SelfExpert: steps 13 > online_rows 12"), (dict(steps=0), "SelfExpert: steps 0"), (dict(m=0), "SelfExpert: online_rows 0")):
        with pytest.raises(ValueError, match=word):
            cpu_expert(**kw)
    with pytest.raises(ValueError, match="SelfExpert: the offline rows are fp32"):
        S.SelfExpert(env, torch.zeros(5, 31), torch.zeros(5, dtype=torch.int8), 12, 5)


# ---- train_all ----------------------------------------------------------------------------------------------------------------------------------
HIRL = ["--agent", "HIRL", "--type", "soft", "--num_envs", "64"]
SELF = ["--expert_self", "64", "--expert_self_steps", "8"]


def test_parser_defaults_and_each_refusal_by_name(capsys):
    from hirl4ucav_amd import train_all as T

    d = T.parse_args(HIRL)
    assert (d.expert_self, d.expert_self_steps, d.expert_self_bc) == (0, 256, False) and T.expert_self_refusal(d) is None
    ok = T.parse_args(HIRL + SELF + ["--expert_self_bc", "--expert_floor", "32", "--hirl_multi_step", "3", "--env", "mixed"])
    assert (ok.expert_self, ok.expert_self_steps, ok.expert_self_bc) == (64, 8, True)
    for kind in (["--agent", "HIRL", "--type", "linear"], ["--agent", "HIRL", "--type", "fixed"], ["--agent", "SAC", "--type", "ESAC"], ["--agent", "HIRL", "--type", "soft", "--dtype", "bf16"],
                 ["--agent", "HIRL", "--type", "soft", "--loop", "reference"], ["--agent", "HIRL", "--type", "soft", "--expert_online", "64"]):
        assert T.parse_args(kind + SELF).expert_self == 64
    for argv, word in ((HIRL + SELF + ["--expert_branch", "64"], "--expert_self does not go with --expert_branch"),
                       (HIRL + SELF + ["--expert_self_bc", "--expert_online", "64"], "--expert_self_bc does not go with --expert_online"),
                       (["--agent", "SAC", "--type", "ESAC", "--per"] + SELF, "--expert_self does not go with --per"),
                       (HIRL + SELF + ["--gpus", "2"], "--expert_self runs on one GPU"),
                       (["--agent", "TD3"] + SELF, "TD3 reads no expert ring"),
                       (["--agent", "BC"] + SELF, "--agent BC reads no expert ring"),
                       (["--agent", "SAC", "--type", "SAC"] + SELF, "--agent SAC --type SAC reads no expert ring"),
                       (["--agent", "SAC", "--type", "ESAC", "--expert_self_bc"] + SELF, "--expert_self_bc goes with --agent HIRL"),
                       (HIRL + ["--expert_self", "64", "--expert_self_steps", "65"], "--expert_self_steps 65 > --expert_self 64"),
                       (HIRL + ["--expert_self", "64", "--expert_self_steps", "0"], "--expert_self_steps 0"),
                       (HIRL + ["--expert_self", "70000", "--expert_self_steps", "65536"], "--expert_self_steps 65536"),
                       (HIRL + ["--expert_self", "-1"], "--expert_self -1"),
                       (HIRL + ["--expert_self_bc"], "--expert_self_bc goes with --expert_self ROWS > 0")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        err = capsys.readouterr().err
        assert ("--per with --type ESAC" if "--per" in argv else word) in err, argv  # (--per's own rule speaks first at the parser; the rule below names it too)
        assert word in T.expert_self_refusal(T.parser().parse_args(argv))
    assert "one GPU" in T.expert_self_refusal(T.parser().parse_args(HIRL + SELF), world=2)


def test_resume_refusals_by_name():
    from hirl4ucav_amd import train_all as T

    se, _, _ = cpu_expert(n=64, m=64, steps=8)
    driver = {"expert_self": se.state_dict()}
    cfg = lambda *extra: T.parser().parse_args(HIRL + list(extra))  # noqa: E731
    assert T.expert_self_resume_refusal(cfg(*SELF), None) is None and T.expert_self_resume_refusal(cfg(*SELF), driver) is None
    assert T.expert_self_resume_refusal(cfg(), {}) is None
    for args, word in ((("--expert_self", "32", "--expert_self_steps", "8"), "was run with --expert_self 64, --expert_self 32 given"),
                       ((), "was run with --expert_self 64, --expert_self 0 given"),
                       (("--expert_self", "64", "--expert_self_steps", "9"), "was run with --expert_self_steps 8, --expert_self_steps 9 given"),
                       (tuple(SELF) + ("--expert_self_bc",), "was run without --expert_self_bc, this run is with it")):
        assert T.expert_self_resume_refusal(cfg(*args), driver) == word
    assert T.expert_self_resume_refusal(cfg(*SELF), {}) == "was run with --expert_self 0, --expert_self 64 given"
