"""CPU tests of n-step returns for HIRL and TD3: the numpy model of the expert table's relabelling (tests/_nstep_label_model.py) against float64 and
against the push model of the rule (tests/_nstep_model.py) fed step by step, the classes of the seeded table the GPU test compares on, the `last`
builder, train_all's flag with its refusals, the loop line, the snapshot's refusals and the header."""
import os
import re
import types

import numpy as np
import pytest

from tests import _nstep_label_model as LM
from tests import _nstep_model as M

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.99
NS = (1, 2, 3, 8)
U = 2.0 ** -24  # the unit roundoff of fp32


@pytest.mark.parametrize("n", NS)
def test_model_against_float64(n):
    """r against sum_k gamma^k r_k and (1 - d') gamma against gamma^m in float64, gamma being the fp32 number the kernel multiplies by.
    Bound of r: term k carries at most k roundings in its weight (w_k = fl(w_{k-1} gamma), w_0 = 1 and w_1 = gamma exact), one in its product
    and at most m in the m additions behind it (0 + t_0 is exact) — k + 1 + m <= 2 m roundings, so |r - sum| <= g(2 m) sum_k gamma^k |r_k| with
    g(j) = j u / (1 - j u), u = 2^-24 (Higham's gamma_j).  Bound of the done column: boot = w_{m-1} carries at most m - 1 roundings and 1 - boot one
    more, both on numbers <= 1, and the product with gamma in float64 none: |(1 - d') gamma - gamma^m| <= g(m) .  A terminal row holds d' = 1."""
    rows, last, _ = LM.make_table(n)
    out = LM.relabel(rows, last, n, GAMMA)
    g = float(np.float32(GAMMA))
    m = LM.steps_of(last, n)
    for j in range(rows.shape[0]):
        k = np.arange(m[j])
        r = rows[j:j + m[j], 30].astype(np.float64)
        exact, mass = float((g ** k * r).sum()), float((g ** k * np.abs(r)).sum())
        mm = int(m[j])
        assert abs(float(out[j, 30]) - exact) <= (2 * mm * U / (1 - 2 * mm * U)) * mass, (j, mm)
        e = j + mm - 1
        if rows[e, 31] != 0:
            assert out[j, 31] == 1.0
        else:
            assert abs((1.0 - float(out[j, 31])) * g - g ** mm) <= mm * U / (1 - mm * U), (j, mm)
        np.testing.assert_array_equal(out[j, 0:17], rows[j, 0:17])
        np.testing.assert_array_equal(out[j, 17:30], rows[e, 17:30])


def test_n1_is_the_input_in_value():
    rows, last, _ = LM.make_table(1)
    rows[5, 30] = -0.0
    out = LM.relabel(rows, last, 1, GAMMA)
    assert (out == rows).all() and not np.signbit(out[5, 30])  # (0 + -0 = +0: equal in value, not in bits)


def push_model_rows(rows, last, n):
    """every segment step by step through the push model of the rule for one env: reset at the segment's first state, one push per row with the
    recorded s' as obs_new, and — behind a segment that ends without done — the time-limit call (the episode counter moves, nothing is stored)"""
    out = []
    end = LM.segment_ends(last)
    j, ctr = 0, 0
    zero4 = np.zeros((1, 4), np.float32)
    while j < rows.shape[0]:
        e = int(end[j])
        m = M.NStepModel(1, n, GAMMA)
        m.reset(rows[j:j + 1, 0:13], [ctr])
        for t in range(j, e + 1):
            done = rows[t, 31] != 0
            ctr += int(done)
            got, _, _ = m.push(rows[t:t + 1, 17:30], rows[t:t + 1, 13:17], rows[t:t + 1, 30], [done], [0], [ctr])
            out.append(got)
        if rows[e, 31] == 0:
            ctr += 1
            got, _, _ = m.push(rows[e:e + 1, 17:30], zero4, [0.0], [False], [0], [ctr])
            out.append(got)
        assert m.pending() == 0
        j = e + 1
    return np.concatenate(out)


@pytest.mark.parametrize("n", NS)
def test_model_against_the_push_model(n):
    """the independent check of the rule: the rows hx_nstep_push's model emits for a segment, in the order it emits them (oldest head first = row
    order), are the relabelled rows bit for bit"""
    rows, last, _ = LM.make_table(n)
    want = push_model_rows(rows, last, n)
    got = LM.relabel(rows, last, n, GAMMA)
    assert want.shape == got.shape
    np.testing.assert_array_equal(want.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("n", NS)
def test_seeded_table_hides_no_case(n):
    """what the GPU comparison leans on: segments of 1, 2, n - 1, n, n + 1 and 70 rows, one that ends exactly at row 63 and one exactly at row 64, a
    final segment without done, segments with and without done, a +600 terminal, finite rewards; and rows of every length 1 .. n"""
    rows, last, segs = LM.make_table(n)
    lens = {k for _, k, _ in segs}
    assert {1, 2, n, n + 1, 70} <= lens and (n == 1 or n - 1 in lens)
    ends = {j + k - 1 for j, k, _ in segs}
    assert 63 in ends and 64 in ends and segs[-1][0] + segs[-1][1] == rows.shape[0] == 300 and not segs[-1][2] and rows[-1, 31] == 0
    assert any(t for _, _, t in segs) and any(not t for _, _, t in segs[:-1])
    assert np.isfinite(rows).all() and (rows[:, 30] > 590).any() and all(rows[j, 31] == 1 for j in np.nonzero(rows[:, 30] > 590)[0])
    assert set(np.unique(rows[:, 31])) == {0.0, 1.0} and (last[rows[:, 31] == 1] == 1).all() and last[-1] == 1
    for j, k, _ in segs:  # within a segment row j + 1 starts where row j ended
        np.testing.assert_array_equal(rows[j + 1:j + k, 0:13], rows[j:j + k - 1, 17:30])
    assert set(LM.steps_of(last, n)) == set(range(1, n + 1))
    for E in (1, 2, 63, 64, 65, 130):  # the cut tables of the GPU test end a segment at their last row
        r, l, s = LM.make_table(n, E)
        assert r.shape == (E, 32) and l[-1] == 1 and r[-1, 31] == 0 and sum(k for _, k, _ in s) == E


def test_last_builder():
    """segment_last against expert_pair_indices: a segment ends at a terminal pair (the reference skips the pair behind it: a gap), and at the file's
    last row; two files: each ends a segment"""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.buffer import segment_last

    rng = np.random.default_rng(4)
    for trial in range(20):
        done = rng.random(40) < 0.15
        done[-1] = trial % 2 == 0
        keep = T.expert_pair_indices(done)
        last = segment_last(done[keep].astype(np.float32), keep)
        assert last.dtype == np.uint8 and last.shape == keep.shape and last[-1] == 1
        for j in range(len(keep) - 1):
            assert bool(last[j]) == bool(done[keep[j]]) == (keep[j + 1] != keep[j] + 1), (trial, j)
        np.testing.assert_array_equal(segment_last(torch.from_numpy(done[keep].astype(np.float32)), torch.from_numpy(keep)), last)
    a, b = np.zeros(5, np.float32), np.array([0, 1, 0], np.float32)
    two = np.concatenate([segment_last(a, np.arange(5)), segment_last(b, np.array([0, 1, 3]))])
    np.testing.assert_array_equal(two, [0, 0, 0, 0, 1, 0, 1, 1])
    np.testing.assert_array_equal(segment_last(a), [0, 0, 0, 0, 1])
    np.testing.assert_array_equal(segment_last(np.zeros(4), np.array([0, 1, 5, 6])), [0, 1, 0, 1])  # any gap ends a segment
    with pytest.raises(ValueError, match="pair indices"):
        segment_last(a, np.arange(4))


HIRL = ["--agent", "HIRL", "--type", "soft", "--synthetic_expert"]


def test_flag_defaults_and_what_it_goes_with():
    from hirl4ucav_amd import train_all as T

    assert T.parse_args(HIRL).hirl_multi_step == 1 and T.parse_args(["--agent", "TD3"]).hirl_multi_step == 1
    assert T.parse_args(HIRL + ["--hirl_multi_step", "1"]).hirl_multi_step == 1
    for argv in (HIRL, ["--agent", "HIRL", "--type", "linear", "--synthetic_expert"], ["--agent", "HIRL", "--type", "fixed", "--synthetic_expert"],
                 ["--agent", "TD3"]):
        hirl = argv[1] == "HIRL"
        for more in ([[], ["--dtype", "bf16"], ["--dtype", "f32x9"], ["--dtype", "bf16_policy"], ["--separate_launches"], ["--loop", "reference"],
                      ["--hirl_grad_clip", "1.0"], ["--hirl_per"], ["--buffer_upsample"], ["--env", "mixed"], ["--gpus", "1"]] +
                     ([["--expert_upsample"], ["--expert_floor", "32"], ["--expert_online", "128"], ["--expert_branch", "96"],
                       ["--expert_branch", "96", "--expert_branch_steps", "4"], ["--expert_floor", "32", "--expert_branch", "96"]] if hirl else [])):
            for n in (2, 3, 8):
                cfg = T.parse_args(argv + more + ["--hirl_multi_step", str(n)])
                assert cfg.hirl_multi_step == n and cfg.multi_step == 1 and T.hirl_multi_step_refusal(cfg) is None and T.nstep_refusal(cfg) is None, (argv, more)
    assert "--hirl_multi_step" in T.parser().format_help()


def test_refusals_word_for_word(capsys):
    from hirl4ucav_amd import train_all as T

    for argv, words in ((["--agent", "SAC", "--type", "SAC", "--hirl_multi_step", "3"],
                         "--hirl_multi_step goes with --agent HIRL or TD3, not --agent SAC: SAC has --multi_step (SacAgent(multi_step=N))"),
                        (["--agent", "SAC", "--type", "ESAC", "--synthetic_expert", "--hirl_multi_step", "3"], "SAC has --multi_step"),
                        (["--agent", "BC", "--synthetic_expert", "--hirl_multi_step", "2"],
                         "--hirl_multi_step goes with --agent HIRL or TD3, not --agent BC (behaviour cloning has no replay ring and no TD target)"),
                        (HIRL + ["--hirl_multi_step", "3", "--gpus", "2"],
                         "--hirl_multi_step runs on one GPU (the per-env windows are rank-local and untested on sharded ranks): use --gpus 1"),
                        (["--agent", "TD3", "--hirl_multi_step", "3", "--gpus", "8"], "--hirl_multi_step runs on one GPU"),
                        (HIRL + ["--hirl_multi_step", "0"], "--hirl_multi_step 0: the number of steps is 1 (off) or 2..8"),
                        (HIRL + ["--hirl_multi_step", "9"], "--hirl_multi_step 9: the number of steps is 1 (off) or 2..8"),
                        (["--agent", "TD3", "--hirl_multi_step", "-2"], "--hirl_multi_step -2: the number of steps is 1 (off) or 2..8"),
                        (HIRL + ["--hirl_multi_step", "3", "--num_envs", "64", "--buffer_size", "191"],
                         "--hirl_multi_step 3 with --buffer_size 191: one step can store N * --num_envs = 192 rows: use a larger --buffer_size"),
                        (HIRL + ["--multi_step", "3"], "--multi_step goes with --agent SAC"),  # SacAgent's keyword stays SAC's
                        (HIRL + ["--multi_step", "3", "--hirl_multi_step", "3"], "--multi_step goes with --agent SAC")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert words in " ".join(capsys.readouterr().err.split()), argv
    assert T.parse_args(HIRL + ["--hirl_multi_step", "3", "--num_envs", "64", "--buffer_size", "192"]).hirl_multi_step == 3
    ns = types.SimpleNamespace
    assert T.hirl_multi_step_refusal(ns(agent="HIRL", hirl_multi_step=3, gpus=1, buffer_size=1000, num_envs=8), world=2) == (
        "--hirl_multi_step runs on one GPU (the per-env windows are rank-local and untested on sharded ranks): use --gpus 1")
    assert T.hirl_multi_step_refusal(ns(agent="SAC", hirl_multi_step=1, gpus=8)) is None  # (without the flag nothing is its business)
    assert T.hirl_multi_step_refusal(ns(agent="HIRL", gpus=8)) is None


def test_nstep_refusal_keeps_its_results():
    """--multi_step's own results are what they were; for HIRL and TD3 the message goes on to name the new flag"""
    from hirl4ucav_amd import train_all as T

    ns = types.SimpleNamespace
    old = "--multi_step goes with --agent SAC (n-step returns are SacAgent's: SAC/agent.py:121-124), not --agent "
    for agent in ("HIRL", "TD3"):
        got = T.nstep_refusal(ns(agent=agent, type="soft", multi_step=3, per_new="max", gpus=None))
        assert got == old + agent + ": HIRL and TD3 have --hirl_multi_step N"
    assert T.nstep_refusal(ns(agent="BC", type="soft", multi_step=3, per_new="max", gpus=None)) == old + "BC"
    sac = dict(agent="SAC", type="SAC", per_new="max", gpus=None)
    assert T.nstep_refusal(ns(multi_step=3, **sac)) is None and T.nstep_refusal(ns(multi_step=1, **sac)) is None
    assert T.nstep_refusal(ns(multi_step=3, hirl_multi_step=1, **sac)) is None
    assert T.nstep_refusal(ns(multi_step=9, **sac)) == "--multi_step 9: the number of steps is 1 (off) or 2..8"
    assert T.nstep_refusal(ns(multi_step=3, **sac), world=2) == "--multi_step runs on one GPU (the per-env windows are not built for sharded ranks): use --gpus 1"
    assert T.nstep_refusal(ns(multi_step=3, agent="SAC", type="ISAC", per_new="max", gpus=None)) == (
        "--multi_step with --type ISAC: n-step returns with the imitative branch are not built: use --type SAC or ESAC")
    assert T.nstep_refusal(ns(multi_step=3, agent="SAC", type="SAC", per_new="td", gpus=None)) == (
        "--multi_step with --per_new td: scoring n-step rows at insert is not built: use --per_new max")
    assert T.nstep_refusal(ns(agent="HIRL", type="soft", multi_step=1, hirl_multi_step=3, per_new="max", gpus=None)) is None


def test_resume_refuses_another_n_by_the_flags_name():
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils import checkpoint as CK

    ns = types.SimpleNamespace
    three, one = {"engine": {"multi_step": {"n": 3}}}, {"engine": {}}
    assert T.hirl_multi_step_resume_refusal(ns(agent="HIRL", hirl_multi_step=3), None) is None
    assert T.hirl_multi_step_resume_refusal(ns(agent="HIRL", hirl_multi_step=3), three) is None
    assert T.hirl_multi_step_resume_refusal(ns(agent="TD3", hirl_multi_step=1), one) is None and T.hirl_multi_step_resume_refusal(ns(agent="TD3"), one) is None
    assert T.hirl_multi_step_resume_refusal(ns(agent="HIRL", hirl_multi_step=2), three) == (
        "was run with --hirl_multi_step 3, --hirl_multi_step 2 given: resume with the flag the run was started with")
    assert T.hirl_multi_step_resume_refusal(ns(agent="TD3", hirl_multi_step=1), three) == (
        "was run with --hirl_multi_step 3, --hirl_multi_step 1 given: resume with the flag the run was started with")
    assert T.hirl_multi_step_resume_refusal(ns(agent="HIRL", hirl_multi_step=3), one) == (
        "was run with --hirl_multi_step 1, --hirl_multi_step 3 given: resume with the flag the run was started with")
    assert T.hirl_multi_step_resume_refusal(ns(agent="SAC", hirl_multi_step=1), three) is None  # (SAC's --multi_step: utils/checkpoint.py's own check)

    class Ins:
        def __init__(self, n):
            self.n, self.loaded = n, None

        def state(self):
            return {"n": self.n, "num_envs": 8, "gamma": 0.99, "ws": torch.zeros(4)}

        def load_state(self, st):
            self.loaded = st

    def fake(n, flag="--hirl_multi_step"):
        e = ns(arena=torch.arange(8, dtype=torch.float32), critic_step=4, actor_step=2, update_count=2, actor_trainable=True, sample_calls=4, act_calls=9,
               grad_clip=None, prioritized=None, multi_step=Ins(n) if n > 1 else None)
        if flag:
            e.multi_step_flag = flag
        return e

    plain, st = CK.engine_state(fake(1)), CK.engine_state(fake(3))
    assert "multi_step" not in plain and st["multi_step"]["n"] == 3  # a snapshot of a run without the flag stays what it was
    e = fake(3)
    CK.load_engine_state(e, st)
    assert e.multi_step.loaded["n"] == 3
    for eng, snap, words in ((fake(2), st, "snapshot was written under --hirl_multi_step 3, this engine runs under --hirl_multi_step 2"),
                             (fake(1), st, "snapshot was written under --hirl_multi_step 3, this engine runs under --hirl_multi_step 1"),
                             (fake(3), plain, "snapshot was written under --hirl_multi_step 1, this engine runs under --hirl_multi_step 3"),
                             (fake(2, flag=None), st, "snapshot was written under --multi_step 3, this engine runs under --multi_step 2")):  # SacEngine keeps its flag
        with pytest.raises(ValueError, match=re.escape(words)):
            CK.load_engine_state(eng, snap)


def _run(agent, n_step, n=64, loop="front", separate=False, grad_clip=None, hirl_per=False):
    cfg = types.SimpleNamespace(loop=loop, separate_launches=separate, updates_per_step=1, dtype="f32", log_rewards=False, status_check_every=0,
                                resume=None, on_front_trip="exit", snapshot_every=0)
    return types.SimpleNamespace(config=cfg, world=1, rank=0, sac=agent == "SAC", n=n, device=torch.device("cpu"), batch=128, per=hirl_per, hirl_per=hirl_per,
                                 grad_clip=grad_clip, inserter=object() if n_step > 1 else None, multi_step=n_step, hirl_multi_step=n_step if agent != "SAC" else 1,
                                 buffer_upsample=False, expert_upsample=False, episode0=0)


def test_loop_line(capsys, monkeypatch):
    """the front loop stays up to 8,192 envs and says how the n-step rows get into the ring; beyond, and under --separate_launches / --loop reference /
    --hirl_per, the reference's order, with the reason; without the flag the line is the parent's; SAC's --multi_step keeps its words"""
    from hirl4ucav_amd import train_all as T

    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    front = "vector loop: front launch (env step + first launches of learn() in one launch; draw before the insert)"
    for agent in ("HIRL", "TD3"):
        for n in (64, 8192):
            run = _run(agent, 3, n=n)
            T.choose_loop(run)
            assert run.front and capsys.readouterr().out.strip() == front + (
                " (--hirl_multi_step 3: the n-step rows are written by a launch of their own behind the front launch's call; the minibatch is drawn before the "
                "previous step's rows)")
        run = _run(agent, 3, n=8193)
        T.choose_loop(run)
        assert not run.front and capsys.readouterr().out.strip() == (
            "vector loop: reference order (--hirl_multi_step 3: the n-step rows are written by a launch of their own behind the acting launch; more than 8,192 "
            "envs: the front launch's persistent and streaming acting roles need a ring in the env)")
        for kw in ({"loop": "reference"}, {"separate": True}):
            run = _run(agent, 2, **kw)
            T.choose_loop(run)
            assert not run.front and capsys.readouterr().out.strip() == (
                "vector loop: reference order (--hirl_multi_step 2: the n-step rows are written by a launch of their own behind the acting launch)")
    run = _run("HIRL", 3, hirl_per=True)
    T.choose_loop(run)
    line = capsys.readouterr().out
    assert not run.front and "(--hirl_per: " in line and "(--hirl_multi_step 3: the n-step rows are written by a launch of their own behind the acting launch)" in line
    run = _run("HIRL", 3, grad_clip=0.5)
    T.choose_loop(run)
    line = capsys.readouterr().out
    assert run.front and "behind the front launch's call" in line and "--hirl_grad_clip 0.5: the clipped update runs as stages behind the front launch" in line
    run = _run("HIRL", 1)
    T.choose_loop(run)
    assert run.front and capsys.readouterr().out.strip() == front
    run = _run("SAC", 3)
    T.choose_loop(run)
    assert not run.front_sac and capsys.readouterr().out.strip() == (
        "vector loop: reference order (--multi_step 3: the n-step rows are written by a launch of their own behind the acting launch)")


def test_one_push_per_env_step_in_every_step_form(monkeypatch):
    """HIRL's / TD3's front form leaves the push to HirlEngine.step_learn and tells after_env_step so; the reference-order step — an episode's last step
    in the front loop included — pushes in after_env_step; both mark_new bounds are the inserter's"""
    from hirl4ucav_amd import train_all as T

    class Ins:
        max_rows, pushes = 192, 0

        def push(self, env, actions):
            self.pushes += 1

    class Marks:
        def __init__(self):
            self.bounds = []

        def mark_new(self, k=None):
            self.bounds.append(k)

    class Eng:
        def __init__(self, ins):
            self.ins, self.calls = ins, []

        def step_learn(self, env, *a, **kw):  # (HirlEngine.step_learn with an inserter set pushes once, behind its launches)
            self.calls.append("step_learn")
            self.ins.push(env, None)

        def act_step(self, env, **kw):
            self.calls.append("act_step")

        def sample(self, *a, **kw):
            self.calls.append("sample")

        def learn(self, **kw):
            self.calls.append("learn")

    def run_of(front):
        ins, ups, rep = Ins(), Marks(), Marks()
        cfg = types.SimpleNamespace(separate_launches=False, updates_per_step=1)
        run = types.SimpleNamespace(config=cfg, inserter=ins, front=front, sac=False, esac=False, isac=False, env=None, actions=None, estats=None, per=True,
                                    per_new="max", replay=rep, n=64, upsampler=ups, ret=None, eng=Eng(ins), expert=None, bc_table=None, batch=128, expert_num=0,
                                    warm_up_rate=10, seed=0, rank=0, max_step=12, writer=None, log_rate=300, episode=0)
        return run, ins, ups, rep

    run, ins, ups, rep = run_of(True)
    T.step_front_hirl(run, 0, 0.0, 0.0)
    assert ins.pushes == 1 and run.eng.calls == ["step_learn"] and ups.bounds == [192] and rep.bounds == [192]
    T.step_reference(run, 11, 0.0, 0.0)  # the episode's last step only acts: the engine has not pushed
    assert ins.pushes == 2 and run.eng.calls == ["step_learn", "act_step"] and ups.bounds == [192, 192]
    run, ins, ups, rep = run_of(False)
    T.step_reference(run, 0, 0.0, 0.0)
    assert ins.pushes == 1 and run.eng.calls == ["act_step", "sample", "learn"] and rep.bounds == [192]
    ups = Marks()
    T.after_env_step(types.SimpleNamespace(inserter=None, estats=None, per=False, n=64, upsampler=ups, ret=None), 0)
    assert ups.bounds == [64]


def test_header_declares_the_entry_point_and_the_binding_reads_it():
    import ctypes

    from hirl4ucav_amd import _abi

    hdr = open(os.path.join(ROOT, "include", "hirl4ucav.h")).read()
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 132 and "132: n-step returns for HIRL and TD3" in hdr
    assert "n-step returns for a labelled expert table" in hdr and "Row j stays row j" in hdr
    f = _abi.abi().functions
    assert "hx_nstep_label" in f
    restype, argtypes = f["hx_nstep_label"][:2]
    assert restype is ctypes.c_int and len(argtypes) == 7 and argtypes[2] is ctypes.c_int64 and argtypes[3] is ctypes.c_int32 and argtypes[4] is ctypes.c_float
    mk = open(os.path.join(ROOT, "hirl4ucav_amd", "csrc", "Makefile")).read()
    assert re.search(r"^hx_nstep_label\.o:.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(ENVFLAGS\)", mk, re.M), "built without contraction, like hx_nstep.hip"
