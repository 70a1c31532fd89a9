"""GPU tests of self-imitation (hx_self_push / hx_self_reset, hx_selfimit.hip; utils.selfimit.SelfExpert; train_all --expert_self) against the CPU
model of the rule, tests/_selfimit_model.py.  Rows are copies, so every comparison is bit equality: ring, success bytes, BC table, cursor and the
counters after EVERY call.  Shapes: 1 env, 63, 64, 65 and 130 (a ragged last wave; one, two and three workgroups), L = 1, 2, 5, M = 5 and 12 with
L <= M, 3 offline rows; the streams are tests/test_selfimit_cpu.py's, which asserts that they contain every case."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _selfimit_model as M  # noqa: E402

POISON, E0, BC0 = 0x7FC0DEAD, 3, 7


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import selfimit

    return selfimit


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class RawSelf:
    """hx_self_push over a ring, success bytes, a BC table and a workspace with guards behind each, fed from arrays (no env), beside the model"""

    def __init__(self, S, n, L, m, stream_seed=0, calls=60, bc=True, cursor=0):
        from hirl4ucav_amd import _lib

        self.n, self.L, self.m, self.call = n, L, m, 0
        off, lab = M.make_offline(E0)
        ring0, succ0 = M.initial_ring(off, lab, m)
        bc0 = M.initial_ring(M.make_offline(BC0, seed=12)[0], np.zeros(BC0, np.int8), m)[0] if bc else None
        self.obs0, self.ctr0, self.stream = M.make_stream(n, L, calls, stream_seed)
        self.model = M.SelfModel(ring0, succ0, E0, m, n, L, self.obs0, self.ctr0, bc=bc0, bc_e0=BC0, cursor=cursor)
        full = np.full((E0 + m + 2, 32), POISON, np.int32)
        full[:E0 + m] = ring0.view(np.int32)
        sfull = np.full(E0 + m + 64, 0x5A, np.int8)
        sfull[:E0 + m] = succ0
        self.ring, self.success, self.table = dev(full), dev(sfull), None
        if bc:
            bfull = np.full((BC0 + m + 2, 32), POISON, np.int32)
            bfull[:BC0 + m] = bc0.view(np.int32)
            self.table = dev(bfull)
        self.lay = S.workspace_layout(n, L)
        self.work = torch.zeros(self.lay["words"] + 64, dtype=torch.int32, device="cuda")
        self.work[self.lay["words"]:] = POISON
        self.work[:self.lay["cursor"][0]] = 0x5A5A5A5A  # tape, obs_prev, len, last_ctr, klen, wcount, wkills: hx_self_reset sets every word it owns
        if cursor:
            v = cursor - 2 ** 64 if cursor >= 2 ** 63 else cursor
            self.part("cursor").view(torch.int64)[0] = v
        o, c = dev(self.obs0), dev(self.ctr0)  # (held until the launch has run)
        _lib.call("hx_self_reset", self.work.data_ptr(), self.lay["words"], n, L, o.data_ptr(), c.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()

    def part(self, name):
        at, words = self.lay[name]
        return self.work[at:at + words]

    def args(self, c):
        obs, act, rew, done, succ, ctr = (dev(a) for a in self.stream[c])
        return (self.work.data_ptr(), self.lay["words"], self.n, self.L, obs.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(), succ.data_ptr(), ctr.data_ptr(), self.ring.data_ptr(),
                self.success.data_ptr(), E0, self.m, None if self.table is None else self.table.data_ptr(), BC0, self.call), (obs, act, rew, done, succ, ctr)

    def push(self, c):
        from hirl4ucav_amd import _lib

        a, keep = self.args(c)
        _lib.call("hx_self_push", *a, _lib.stream_ptr())
        torch.cuda.synchronize()
        self.call += 1
        return self.model.push(*self.stream[c])

    def check(self, what):
        m, end = self.m, E0 + self.m
        t, b = self.ring.cpu().numpy(), self.success.cpu().numpy()
        assert (t[end:] == POISON).all() and (b[end:] == 0x5A).all() and bool((self.work[self.lay["words"]:] == POISON).all()), what + ": guards"
        rows = np.nonzero((t[:end].view(np.uint32) != self.model.ring).any(1))[0]
        assert rows.size == 0, what + f": ring rows {rows.tolist()} differ (E0 = {E0}), words {np.nonzero(t[rows[0]].view(np.uint32) != self.model.ring[rows[0]])[0].tolist()} of the first"
        assert np.array_equal(b[:end], self.model.success), what + ": success bytes"
        if self.table is not None:
            bt = self.table.cpu().numpy()
            assert (bt[BC0 + m:] == POISON).all() and np.array_equal(bt[:BC0 + m].view(np.uint32), self.model.bc), what + ": BC table"
        cur = self.part("cursor").cpu().view(torch.int64).numpy().view(np.uint64)
        assert int(cur[self.call & 1]) == self.model.cursor, what + f": cursor {int(cur[self.call & 1])}, the model's {self.model.cursor}"
        cnt = self.part("counters").cpu().view(torch.int64).reshape(4, -1).sum(1).tolist()
        assert cnt == self.model.counters, what + f": counters {cnt}, the model's {self.model.counters}"


CASES = [(n, L, m) for n in (1, 63, 64, 65, 130) for L in (1, 2, 5) for m in (5, 12) if L <= m]


@pytest.mark.parametrize("n,L,m", CASES)
def test_push_equals_the_model(S, n, L, m):
    """60 calls of the seeded stream; after EVERY call ring, success bytes, BC table (given where n + L is odd), cursor and counters bit for bit, every
    guard intact.  From 63 envs on the kill rows of a call exceed M (drops); the cursor crosses M everywhere but at one env with M = 12"""
    raw = RawSelf(S, n, L, m, bc=(n + L) % 2 == 1)
    raw.check("start")
    for c in range(60):
        raw.push(c)
        raw.check(f"call {c}")
    ev = raw.model.events
    assert (ev["wraps"] >= 1 or (n == 1 and m == 12)) and raw.model.counters[M.EPISODES] >= 2 and ev["trunc"] >= 1 and ev["done_no_kill"] >= 1
    if n >= 63:
        assert ev["drop_calls"] >= 1 and ev["same_group"] >= 1 and ev["nonfinite_rows"] >= 1 and ev["kill_long"] >= 1
    if n >= 65:
        assert ev["other_group"] >= 1


def test_the_same_inputs_give_the_same_bits(S):
    """130 envs (three workgroups in both launches) twice in fresh workspaces: the whole workspace — tape included —, ring, bytes and table are identical"""
    runs = []
    for _ in range(2):
        raw = RawSelf(S, 130, 5, 12)
        for c in range(60):
            raw.push(c)
        raw.check("end")
        runs.append((raw.work.clone(), raw.ring.clone(), raw.success.clone(), raw.table.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cursor0", [2 ** 32 - 2, 2 ** 40, 2 ** 64 - 3])
@pytest.mark.parametrize("n,L,m", [(65, 2, 12), (130, 5, 12)])
def test_the_cursor_is_64_bit(S, n, L, m, cursor0):
    """the cursor preset: carried across 2^32, at 2^40, and through the wrap of the 64-bit word itself — the model's slots after every call"""
    raw = RawSelf(S, n, L, m, calls=30, cursor=cursor0)
    raw.check("start")
    total = 0
    for c in range(30):
        total += sum(len(s) for _, s in raw.push(c))
        raw.check(f"cursor {cursor0}, call {c}")
    assert total > m and raw.model.cursor == (cursor0 + total) % 2 ** 64 and (cursor0 < 2 ** 63 or raw.model.cursor < 2 ** 32)


def test_refusals_leave_every_buffer_untouched(S):
    from hirl4ucav_amd import _lib

    raw = RawSelf(S, 65, 5, 12)
    for c in range(3):
        raw.push(c)
    before = [t.clone() for t in (raw.work, raw.ring, raw.success, raw.table)]
    good, keep = raw.args(3)
    good = good + (_lib.stream_ptr(),)

    def swap(i, v):
        return good[:i] + (v,) + good[i + 1:]

    ring, table, obs, act = raw.ring.data_ptr(), raw.table.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr()
    work = raw.work.data_ptr()
    words = raw.lay["words"]
    bad = [swap(0, None), swap(0, work + 4), swap(0, work + 8), swap(1, 0), swap(1, words - 1), swap(1, words + 1), swap(1, words + 64),  # (the allocation's own length)
           swap(2, 0), swap(2, -1), swap(2, 1 << 31), swap(2, 64), swap(2, 66), swap(3, 0), swap(3, -1), swap(3, 65536), swap(3, 4), swap(3, 6), swap(3, 13),
           good[:1] + (S.workspace_layout(65, 13)["words"], 65, 13) + good[4:],  # a consistent triple, but L > online_rows
           swap(4, None), swap(4, obs + 4), swap(5, None), swap(5, act + 8), swap(6, None), swap(7, None), swap(8, None), swap(9, None),
           swap(10, None), swap(10, ring + 64), swap(10, ring + 4), swap(11, None), swap(12, -1), swap(12, (1 << 31) - 12), swap(13, 0), swap(13, 4), swap(13, 1 << 31),
           swap(14, table + 64), swap(15, -1), swap(15, (1 << 31) - 12)]
    for a in bad:
        with pytest.raises(_lib.HxError, match=r"hx_self_push failed \(-1\)"):
            _lib.call("hx_self_push", *a)
    o, c = dev(raw.obs0), dev(raw.ctr0)
    tail = (o.data_ptr(), c.data_ptr(), _lib.stream_ptr())
    for a in ((None, words, 65, 5) + tail, (work, words, 65, 5, None) + tail[1:], (work, words, 65, 5, o.data_ptr(), None, tail[2]), (work, words, 65, 0) + tail,
              (work, words, 0, 5) + tail, (work + 8, words, 65, 5) + tail, (work, words - 1, 65, 5) + tail, (work, words, 65, 6) + tail, (work, words, 130, 5) + tail):
        with pytest.raises(_lib.HxError, match=r"hx_self_reset failed \(-1\)"):
            _lib.call("hx_self_reset", *a)
    torch.cuda.synchronize()
    for t0, t in zip(before, (raw.work, raw.ring, raw.success, raw.table)):
        assert torch.equal(t0, t), "a refused call wrote something"
    raw.push(3)  # ... and the next good call goes on where the last one stopped
    raw.check("after the refusals")


def fly(S, steps, bc):
    """64 real straight_line envs (seed 7, random reset, auto-reset, no time limit) flown by hx_pilot_act + hx_env_step, SelfExpert.push() behind each
    step; the per-step buffers go to the host and into the model"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.pilot import device_pilot_actions

    n, L, m = 64, 8, 64
    env = BatchedHarfangEnv(n, scenario="straight_line", seed=7, auto_reset=True, random_reset=True)
    env.reset()
    off, lab = M.make_offline(E0)
    table = torch.from_numpy(M.make_offline(BC0, seed=12)[0]).cuda() if bc else None
    se = S.SelfExpert(env, dev(off), dev(lab), m, L, bc_table_offline=table)
    se.reset()
    ring0, succ0 = M.initial_ring(off, lab, m)
    bc0 = M.initial_ring(M.make_offline(BC0, seed=12)[0], np.zeros(BC0, np.int8), m)[0] if bc else None
    model = M.SelfModel(ring0, succ0, E0, m, n, L, env.obs.cpu().numpy(), env.episode_ctr.cpu().numpy().view(np.uint32), bc=bc0, bc_e0=BC0)
    act = torch.zeros((n, 4), device="cuda")
    taken = []
    for _ in range(steps):
        device_pilot_actions(env, out=act)
        env.step(act)
        se.push(act)
        taken.append(torch.cat([env.obs.view(torch.int32), act.view(torch.int32), env.reward.view(torch.int32)[:, None], env.done.int()[:, None],
                                env.success.int()[:, None], env.episode_ctr.view(torch.int32)[:, None]], 1))
    host = torch.stack(taken).cpu().numpy()
    for h in host:
        model.push(h[:, 0:13].view(np.float32), h[:, 13:17].view(np.float32), h[:, 17].view(np.float32), h[:, 18].astype(np.uint8), h[:, 19].astype(np.int8),
                   h[:, 20].view(np.uint32))
    return env, se, model, (off, lab)


def test_real_envs_end_to_end(S):
    """1,100 steps of the pursuit pilot over 64 real envs: the CPU oracle's env under tests/_pilot_model.py's actions measured 19 kills in these 1,100
    calls (the first at call 1,048, envs 4 and 22 both at call 1,085; every episode longer than L = 8, so 19 * 8 = 152 rows over M = 64 slots).  The final
    ring, success bytes, BC table, cursor and counters equal the model's fed with the device's own per-step buffers, and at least one episode was written"""
    env, se, model, (off, lab) = fly(S, 1100, bc=True)
    end = E0 + 64
    assert np.array_equal(se.ring.ring[:end].cpu().numpy().view(np.uint32), model.ring) and np.array_equal(se.ring.success[:end].cpu().numpy(), model.success)
    assert np.array_equal(se.table.cpu().numpy().view(np.uint32), model.bc)
    assert se.cursor() == model.cursor and list(se.counters()) == model.counters and se.call == 1100
    print(f"1,100 calls: counters {se.counters()}, events {model.events}")
    assert model.counters[M.EPISODES] >= 1 and model.counters[M.ROWS] >= 8
    on = se.ring.ring[E0:end]
    written = ~(on.view(torch.int32)[:, None, :] == dev(off).view(torch.int32)[None]).all(2).any(1)
    assert int(written.sum()) >= 8 and bool((on[written][:, 30] > 0).any()) and bool(((on[written][:, 31] == 0) | (on[written][:, 31] == 1)).all())
    # the state round trip on the device: another object over the same offline rows takes the record; the tape stays behind
    other = S.SelfExpert(env, dev(off), dev(lab), 64, 8, bc_table_offline=torch.from_numpy(M.make_offline(BC0, seed=12)[0]).cuda())
    other.load_state_dict(se.state_dict())
    other.reset()
    assert other.call == se.call and other.cursor() == se.cursor() and other.counters() == se.counters()
    assert torch.equal(other.ring.ring.view(torch.int32), se.ring.ring.view(torch.int32)) and torch.equal(other.ring.success, se.ring.success)
    assert torch.equal(other.table.view(torch.int32), se.table.view(torch.int32))
    assert not bool(other._part("len").any()) and not bool(other._part("tape").any()) and bool(se._part("tape").any())
    assert torch.equal(other._part("obs_prev").view(13, 64).t().contiguous().view(torch.int32), env.obs.view(torch.int32))


# ---- train_all -------------------------------------------------------------------------------------------------------------------------------
def test_train_all_expert_self(S, tmp_path, monkeypatch, capsys):
    """HIRL-soft at 64 envs, 2 driver episodes of 12 steps with --expert_self 64 --expert_self_steps 8: one hx_self_push behind every acting launch,
    exploration included, one hx_self_reset; the four scalars are written per driver episode from the device counters; the offline rows stand; the
    snapshot carries the record without the tape and resumes; the refusals fire"""
    from hirl4ucav_amd import train_all as T
    from tests import test_branch_gpu as G

    names, runs, writers = G.spy(monkeypatch)
    self_args = ["--expert_self", "64", "--expert_self_steps", "8"]
    out_dir = T.main(T.parse_args(G.HIRL + self_args + ["--expert_self_bc", "--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    run, start, start_succ = runs[0]
    e0 = run.selfx.offline_rows
    assert names.count("hx_self_push") == G.EXPLORE + 2 * 12 == run.selfx.call and names.count("hx_self_reset") == 1 and "hx_pilot_branch" not in names
    assert run.expert is run.selfx.ring and run.bc_table is run.selfx.table and run.selfx.steps == 8 and run.selfx.online_rows == 64
    assert torch.equal(run.expert.ring[:e0], start[:e0]) and torch.equal(run.expert.success[:e0], start_succ[:e0]) and bool(torch.isfinite(run.expert.ring).all())
    kills, eps, rows_w, dropped = run.selfx.counters()
    assert kills == eps + dropped and rows_w <= 8 * eps and run.selfx.cursor() >= rows_w
    tags = ["Expert/Self Kills", "Expert/Self Episodes Written", "Expert/Self Rows Written", "Expert/Self Episodes Dropped"]
    rows = writers[0].rows
    assert [(t, s) for t, v, s in rows if t.startswith("Expert/Self")] == [(t, s) for s in (0, 1) for t in tags]
    assert [v for t, v, s in rows if t.startswith("Expert/Self")][4:] == [float(v) for v in (kills, eps, rows_w, dropped)]
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]["expert_self"]
    assert snap["call"] == run.selfx.call and snap["steps"] == 8 and snap["bc"] is True and snap["cursor"] == run.selfx.cursor() and "work" not in snap
    assert torch.equal(snap["online"].view(torch.int32), run.expert.ring[e0:e0 + 64].cpu().view(torch.int32))
    assert sum(v.numel() * v.element_size() for v in snap.values() if torch.is_tensor(v)) < 64 * 2 * 128 + 1024
    del names[:]
    T.main(T.parse_args(G.HIRL + self_args + ["--expert_self_bc", "--episodes", "3", "--result_dir", str(tmp_path / "b"), "--resume", out_dir]))
    resumed = runs[1][0]
    assert names.count("hx_self_reset") == 1 and names.count("hx_self_push") == 12 and resumed.selfx.call == G.EXPLORE + 36
    assert all(a >= b for a, b in zip(resumed.selfx.counters(), (kills, eps, rows_w, dropped)))
    for other, word in ((["--expert_self", "32", "--expert_self_steps", "8", "--expert_self_bc"], "was run with --expert_self 64, --expert_self 32 given"),
                        (["--expert_self", "64", "--expert_self_steps", "4", "--expert_self_bc"], "was run with --expert_self_steps 8, --expert_self_steps 4 given"),
                        (self_args, "was run with --expert_self_bc, this run is without it"), ([], "was run with --expert_self 64, --expert_self 0 given")):
        with pytest.raises(SystemExit, match=word):
            T.main(T.parse_args(G.HIRL + other + ["--episodes", "3", "--result_dir", str(tmp_path / "c"), "--resume", out_dir]))
    for argv, word in ((G.HIRL + self_args + G.BRANCH, "--expert_self does not go with --expert_branch"),
                       (["--agent", "TD3"] + G.COMMON + self_args, "TD3 reads no expert ring")):
        ns = T.parser().parse_args(argv + ["--result_dir", str(tmp_path / "d")])
        with pytest.raises(SystemExit, match=word):
            T.main(ns)


@pytest.mark.parametrize("kind", ["reference", "ESAC", "ISAC"])
def test_train_all_expert_self_other_forms(S, tmp_path, monkeypatch, kind):
    """the reference's order, E-SAC and ISAC: one push behind every acting launch, the ring the engine reads is SelfExpert's"""
    from hirl4ucav_amd import train_all as T
    from tests import test_branch_gpu as G

    names, runs, writers = G.spy(monkeypatch)
    T.main(T.parse_args(G.agent_args(kind, tmp_path) + ["--expert_self", "64", "--expert_self_steps", "8", "--episodes", "1", "--result_dir", str(tmp_path / "a")]))
    run = runs[0][0]
    assert names.count("hx_self_push") == G.EXPLORE + 12 == run.selfx.call and run.expert is run.selfx.ring and run.selfx.table is None
    assert bool(torch.isfinite(run.expert.ring).all()) and len([1 for t, _, _ in writers[0].rows if t.startswith("Expert/Self")]) == 4
