"""The replay ring's 64-bit counter beyond 2^32 in every kernel that turns DeviceReplay.total into a ring slot: the SHIFTED TWIN.

State A is built the ordinary way at a small total with the ring full (T_small = cap + h, head h); B is a copy of every device buffer of A with
D = T_big - T_small, a multiple of cap, added to its counters only (total, PER's marked, word 0 of the ordered-slot header), T_big from
tests/_ring_model.EDGE_TOTALS.  The same call runs on both with the same seeds, call words and actions.  Afterwards
  (i)   B's counters equal A's plus exactly D, as Python integers;
  (ii)  every other buffer is equal in bits wherever the path fixes the slot order (one inserting workgroup, or ordered slots); where several
        workgroups race for the atomic, the rows written are equal as sorted rows with their step_success byte, and the set of slots written is
        equal (both rings are refilled with the same NaN-free table before the call: a written slot is one that differs from the table);
  (iii) the slots B wrote are slots(T_big, rows_written, cap) of the model, in Python integers.
Every assertion is an equality of integers or of bits, except the loss sums of the two front launches, which keep their files' own tolerance for
atomically summed losses (rtol 1e-6, atol 1e-7).

The consumers of `total`, by file and line (a search for `total` under hirl4ucav_amd/csrc finds no other):
  csrc/hx_env_block.h:116          env step with fused insert: 64-bit atomicAdd, ring_slot        test_env_step_insert
  csrc/hx_env_dev.h:557            ring_slot: fp64 quotient estimate, one correction step         every insert test; test_ring_slot_correction_branch
  csrc/hx_act_body.h:505-572       per-tile acting launches with fused insert                     test_hirl_act_step, test_sac_act_step
  csrc/hx_actp_body.h:62           persistent acting kernel (the same tail)                       test_persistent_act_step
  csrc/hx_env_dev.h:532-553        ordered slots: header word 0, t0 + before (+ nstore)           test_ordered_slots
  csrc/hx_nstep.hip:96-105         n-step window: atomicAdd result through two 32-bit shuffles    test_nstep_push
  csrc/hx_update.h:357-384, :400   draw_map / slot_of_draw, draw_fused                            test_draw (fused, deferred), both front tests
  csrc/hx_sampler.hip:55           the draw as a launch of its own                                test_draw (own launch), both front tests
  csrc/hx_per.hip:19-49            PER mark_new: [marked, total), mk % cap, marked <- mk + len    test_per_mark_new
  csrc/hx_per.hip:182              PER sample: the live length min(total, cap)                    test_per_sample
  csrc/hx_score.hip:33-69, :152    PER score-new: score_plan, (start + i) % cap, marked           test_per_score_new
  utils/buffer.py:31-45            int(total.item()), store_rows                                  len() in every test; tests/test_ring_counter_cpu.py
  utils/checkpoint.py:86-105       replay_state / load_replay_state: total.fill_(python int)      test_checkpoint_*

Capacities: 512 and 1,024 divide 2^32, so a counter cut to 32 bits still finds the right slot there (total mod cap survives the cut).  Every path
that runs at one of them (n-step, PER, the two front launches) therefore also runs at a capacity that does not: 1,000, 700 or 2,500.

ring_slot's two correction branches: at the capacities used here (512, 700, 1000, 1024, 2500, 20000) neither can run for total < 2^52 — the estimate
is exact there (tests/test_ring_counter_cpu.py), so those cases cover the documented domain and cannot reach the branches.  The "high" branch does run
at other capacities (1006: most multiples of cap whose quotient is high in its binade); test_ring_slot_correction_branch runs the env step from such
totals.  No total below 2^52 that reaches the "low" branch is known."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402
from tests import _nstep_model as M  # noqa: E402
from tests import _ring_model as R  # noqa: E402

SUCCESS_FILL = 77
LOSS_TOL = dict(rtol=1e-6, atol=1e-7)  # tests/test_front_gpu.py, tests/test_sac_front_small_gpu.py: loss sums are accumulated with atomics


@pytest.fixture(scope="module")
def hx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import types

    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents import engine, sac_engine
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils import buffer, checkpoint

    _lib.load()
    return types.SimpleNamespace(lib=_lib, E=engine, SE=sac_engine, Env=BatchedHarfangEnv, B=buffer, C=checkpoint)


@functools.lru_cache(maxsize=None)
def table(cap):
    """the rows both rings hold before a call: the seeded replay table (plausible, NaN-free: the front launches learn from them), repeated"""
    return torch.from_numpy(np.resize(D.make_data(D.DATA_SEED)["replay"], (cap, 32)).copy()).cuda()


def refill(*reps):
    for rep in reps:
        rep.ring.copy_(table(rep.capacity))
        rep.success.fill_(SUCCESS_FILL)


def make_twin(hx, cap, t_big, ordered=False):
    """-> (replay A at T_small = cap + h, replay B at t_big, D)"""
    t_small, d = R.twin_offset(t_big, cap)
    a, b = hx.B.DeviceReplay(cap, ordered_slots=ordered), hx.B.DeviceReplay(cap, ordered_slots=ordered)
    refill(a, b)
    a.total.fill_(t_small)
    b.total.copy_(a.total)
    b.total.add_(d)
    assert int(b.total.item()) == t_big and int(a.total.item()) == t_small and len(a) == len(b) == cap
    return a, b, d


def written(rep):
    return (rep.ring != table(rep.capacity)).any(1).nonzero().flatten()


def check_call(ra, rb, ta0, tb0, d, exact, what):
    """(i), (ii), (iii) after one inserting call on both sides, for the rings and their counters -> (A's total, B's total, rows written)"""
    cap = ra.capacity
    ta1, tb1 = int(ra.total.item()), int(rb.total.item())
    k = ta1 - ta0
    assert tb1 == ta1 + d and tb1 - tb0 == k and 0 <= k <= cap, (what, ta0, ta1, tb0, tb1, d)
    assert len(ra) == len(rb) == cap, what
    wa, wb = written(ra), written(rb)
    want = sorted(R.slots(tb0, k, cap))
    assert wb.tolist() == want, (what, "slots B wrote", tb0, k, wb.tolist()[:8], want[:8])
    assert wa.tolist() == want == sorted(R.slots(ta0, k, cap)), (what, "slots A wrote")
    keep = torch.ones(cap, dtype=torch.bool, device="cuda")
    keep[wb] = False
    assert bool((rb.success[keep] == SUCCESS_FILL).all()) and bool((ra.success[keep] == SUCCESS_FILL).all()), (what, "step_success outside the written slots")
    if exact:
        assert torch.equal(ra.ring.view(torch.int32), rb.ring.view(torch.int32)) and torch.equal(ra.success, rb.success), (what, "ring bits")
    else:
        sa = M.sort_rows(ra.ring[wa].cpu().numpy(), ra.success[wa].cpu().numpy())
        sb = M.sort_rows(rb.ring[wb].cpu().numpy(), rb.success[wb].cpu().numpy())
        assert np.array_equal(sa, sb), (what, "rows written, sorted")
    return ta1, tb1, k


ENV_FIELDS = ("obs", "reward", "done", "success", "episode_ctr")


def make_envs(hx, n, reps, max_step, layout=0):
    """one env per side, the same seed; the episode step counters staggered (env i starts at step i % max_step) so that every step leaves some rows
    unstored (time limit) and the workgroups ask for different numbers of slots"""
    envs = []
    for rep in reps:
        env = hx.Env(n, scenario=(np.arange(n) % 3).astype(np.int32), seed=5, max_step=max_step, auto_reset=True, random_reset=True,
                     replay=rep, layout=layout)
        env.reset()
        w = env.state.view(torch.int32)[36]
        w.copy_((w & -65536) | (torch.arange(n, device="cuda", dtype=torch.int32) % max_step))
        envs.append(env)
    assert torch.equal(envs[0]._state_store, envs[1]._state_store) and torch.equal(envs[0].obs, envs[1].obs)
    return envs


def assert_envs_equal(ea, eb, what):
    assert torch.equal(ea._state_store.view(torch.int32), eb._state_store.view(torch.int32)), (what, "env state")
    for f in ENV_FIELDS:
        assert torch.equal(getattr(ea, f), getattr(eb, f)), (what, f)


def run_twin(hx, n, cap, t_big, steps, step_fn, exact, what, max_step=7, layout=0, ordered=False):
    """`steps` inserting calls step_fn(env, k) on both sides; all three properties after every call.  (From the top of the domain, 2^52 - 2 cap - 3, only
    as many calls as stay below 2^52.)"""
    steps = min(steps, (R.TOTAL_BOUND - t_big) // n)
    ra, rb, d = make_twin(hx, cap, t_big, ordered)
    ea, eb = make_envs(hx, n, (ra, rb), max_step, layout)
    ta, tb = int(ra.total.item()), int(rb.total.item())
    ks = []
    for k in range(steps):
        refill(ra, rb)
        oa = [t.clone() for t in step_fn(ea, k)]
        ob = step_fn(eb, k)
        for x, y in zip(oa, ob):
            assert torch.equal(x, y), (what, k, "outputs")
        assert_envs_equal(ea, eb, (what, k))
        ta, tb, rows = check_call(ra, rb, ta, tb, d, exact, (what, t_big, k))
        ks.append(rows)
    assert 0 < min(ks) < n and max(ks) <= n and sum(ks) > 0, (what, ks)  # time-limit rows were left out in every step
    return ra, rb, ea, eb


def actions_for(n, k):
    return torch.from_numpy(np.random.default_rng(1000 + k).uniform(-1, 1, (n, 4)).astype(np.float32)).cuda()


LAYOUTS = [(0, 0), (1, 32), (1, 64), (1, 128), (1, 256), (1, 512), (0, 64), (0, 128), (0, 256)]  # tests/test_env_gpu.py


@pytest.mark.parametrize("n,pair,epb", [(64, p, e) for p, e in LAYOUTS] + [(300, 0, 0)])
def test_env_step_insert(hx, n, pair, epb):
    """BatchedHarfangEnv.step with replay= (csrc/hx_env_block.h:116: 64-bit atomicAdd, then ring_slot, csrc/hx_env_dev.h:557), cap = 1000, max_step = 7,
    12 steps from every total of EDGE_TOTALS: 64 envs in every launch layout of tests/test_env_gpu.py (one workgroup wherever the layout holds 64
    envs: ring bits; (1, 32) has two) and 300 envs (ragged, five workgroups racing for the atomic).  At cap = 1000 ring_slot's correction branches
    cannot run below 2^52 (tests/test_ring_counter_cpu.py): these cases cover the documented domain without them."""
    from tests.test_env_gpu import LAYOUTS as THEIRS

    assert THEIRS == LAYOUTS
    exact = (n <= 256) if epb == 0 else (epb >= n)
    for t_big in R.EDGE_TOTALS(1000, n):
        run_twin(hx, n, 1000, t_big, 12, lambda env, k: env.step(actions_for(n, k)), exact, f"env step {n} envs layout {(pair, epb)}",
                 layout=hx.lib.layout(pair, epb) if epb else 0)


def test_ring_slot_correction_branch(hx):
    """ring_slot's "high" correction (csrc/hx_env_dev.h:561) on the device: capacity 1006, 64 envs in one workgroup, so the atomicAdd returns the
    total itself — a multiple of 1006 whose fp64 quotient estimate is one too small (tests/_ring_model.CORRECTION_TOTALS; the CPU file proves that
    the branch runs there).  The rows must start at slot 0; the twin A sits at total = 1006, where the estimate is exact."""
    cap = R.CORRECTION_CAP
    for t_big in R.CORRECTION_TOTALS():
        taken = []
        assert R.ring_slot_estimate(t_big, cap, taken) == 0 and taken == ["high"] and t_big % cap == 0
        run_twin(hx, 64, cap, t_big, 3, lambda env, k: env.step(actions_for(64, k)), True, "env step at a corrected multiple")


def hirl_engine(hx, fmt):
    p = D.make_params(31)
    e = hx.E.HirlEngine(batch=128)
    e.load_params(p["actor"], p["critic"], p["bc_actor"])
    if fmt == "f32":
        e.x9_rows = None  # fp32 MFMA at every size
    else:
        e.set_act_dtype({"x9": "f32x9", "bf16": "bf16"}[fmt])
    return e


def engine_step(e, **kw):
    """act_step of ONE engine on either side: the call word (it keys the Philox noise) is pinned to the step"""
    def fn(env, k):
        e.act_calls = 10 + k
        return e.act_step(env, **kw)
    return fn


@pytest.mark.parametrize("fmt", ["f32", "x9", "bf16"])
def test_hirl_act_step(hx, fmt):
    """HirlEngine.act_step, the per-tile kernel (csrc/hx_act_body.h:505-572: atomicAdd per workgroup, the base re-assembled from two readfirstlane
    halves, ring_slot), acting formats f32, x9 and bf16: 83 envs (six workgroups, a ragged last one), cap = 1000, 9 steps over a time limit of 7."""
    e = hirl_engine(hx, fmt)
    for t_big in R.EDGE_TOTALS(1000, 83):
        run_twin(hx, 83, 1000, t_big, 9, engine_step(e, sigma=0.1, seed=3), False, f"HIRL act_step {fmt}")


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
def test_persistent_act_step(hx, fmt):
    """HirlEngine.act_step beyond 8,192 envs: the persistent kernel (csrc/hx_actp.hip, hx_actp_body.h:62 hands `total` to the same tail), 8,192 + 40
    envs, cap = 20,000, 3 steps, bf16 and f32."""
    e = hirl_engine(hx, fmt)
    n = 8192 + 40
    for t_big in R.EDGE_TOTALS(20000, n):
        run_twin(hx, n, 20000, t_big, 3, engine_step(e, sigma=0.1, seed=3), False, f"persistent act_step {fmt}", max_step=3)


def sac_engine(hx, batch=128):
    from tests.test_oracle_sac import sac_params

    p = sac_params()
    e = hx.SE.SacEngine(batch=batch)
    e.load_params(p["policy"], p["q1"], p["q2"])
    return e


def test_sac_act_step(hx):
    """SacEngine.act_step (hx_sac_act_step from the fp32 image: the per-tile body of csrc/hx_act_body.h with SAC's 16-row workgroups): 300 envs, cap = 1000"""
    e = sac_engine(hx)
    for t_big in R.EDGE_TOTALS(1000, 300):
        run_twin(hx, 300, 1000, t_big, 9, engine_step(e, seed=3), False, "SAC act_step")


def test_ordered_slots(hx):
    """DeviceReplay(ordered_slots=True) under the per-tile acting launch (csrc/hx_env_dev.h:532-553: header word 0 read relaxed, t0 + before, the last
    tile writes t0 + before + nstore): 300 envs, cap = 1000, 6 steps.  The slot order is fixed: rings in bits; header word 0 shifted by D, words 1
    (launch sequence) and 2 (status) equal, slot_status 0."""
    e = hirl_engine(hx, "f32")
    for t_big in R.EDGE_TOTALS(1000, 300):
        ra, rb, _, _ = run_twin(hx, 300, 1000, t_big, 6, engine_step(e, sigma=0.1, seed=3), True, "ordered slots", ordered=True)
        ha, hb = ra.slot_header.cpu().tolist(), rb.slot_header.cpu().tolist()
        assert hb[0] - ha[0] == R.twin_offset(t_big, 1000)[1] and hb[0] > t_big
        assert ha[1] == hb[1] == 6 and ha[2] == hb[2] == 0 and ra.slot_status() == rb.slot_status() == 0
        assert ha[3:] == hb[3:]  # the tiles' published words: (sequence << 32) | rows


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("cap", [1024, 1000])
@pytest.mark.parametrize("n_envs", [64, 300])
def test_nstep_push(hx, n_envs, cap):
    """NStepInserter.push (csrc/hx_nstep.hip:96-105: the atomicAdd's result broadcast over the wave as two 32-bit halves through __shfl, then
    ring_slot), n = 3, cap = 1,024 and 1,000 (1,024 divides 2^32: a counter cut to 32 bits still finds the right slot there, so the power of two alone
    would not notice a lost high half), the seeded inputs of tests/_nstep_model.make_inputs, 20 calls: 64 envs (one workgroup: slot order in bits) and 300
    envs (five).  B's inserter is a copy of A's workspace; the numpy model's total runs at T_big too, and B's rows are read back from the slots the
    model names (tests/test_nstep_gpu.check_call)."""
    from tests.test_nstep_gpu import GAMMA, check_call as model_check

    n = 3
    obs0, steps = M.make_inputs(n_envs, n, 20)
    ctr0 = np.zeros(n_envs, np.int32)
    for t_big in R.EDGE_TOTALS(cap, n * n_envs):
        ra, rb, d = make_twin(hx, cap, t_big)
        ia, ib = hx.B.NStepInserter(ra, n_envs, n, GAMMA), hx.B.NStepInserter(rb, n_envs, n, GAMMA)
        ia.reset_arrays(dev(obs0), dev(ctr0))
        ib.ws.copy_(ia.ws)
        model = M.NStepModel(n_envs, n, GAMMA)
        model.reset(obs0, ctr0)
        model.total = t_big
        ta, tb = int(ra.total.item()), t_big
        for c, st in enumerate(steps):
            obs, act, rew, done, suc, ctr = st
            if tb + n * n_envs >= R.TOTAL_BOUND:  # (from the top of the domain: only the calls that stay below 2^52)
                assert c >= 2
                break
            refill(ra, rb)
            for ins in (ia, ib):
                ins.push_arrays(dev(obs), dev(act), dev(rew), dev(done), dev(suc), dev(ctr.astype(np.int32)))
            what = f"n-step {n_envs} envs from {t_big}, call {c}"
            assert model_check(ib, model, rb, tb, model.push(*st), n_envs <= 64, what) == model.total
            assert isinstance(model.total, int) and torch.equal(ia.ws.view(torch.int32), ib.ws.view(torch.int32)), what
            ta, tb, _ = check_call(ra, rb, ta, tb, d, n_envs <= 64, what)
        assert tb > t_big + (cap if n_envs > 64 and c == len(steps) - 1 else 0), "the ring wrapped"


DRAW_CAP, DRAW_B = 700, 128


def draw_totals(h):
    """totals with head h: T_small = cap + h, and h behind the first multiple of cap beyond 2^32, beyond 2^40, and the last one with room below 2^52;
    plus, whatever their heads, EDGE_TOTALS are drawn from in test_draw_at_the_edge_totals"""
    cap = DRAW_CAP
    return cap + h, [((1 << 32) // cap + 1) * cap + h, ((1 << 40) // cap + 1) * cap + h, (R.TOTAL_BOUND - 2 * cap - 3) // cap * cap - cap + h]


def draws(hx, e, rep, tot, guard, fused):
    """idx [20, 128] and the gathered rows of 20 draws at total = tot, call words 1..20"""
    lib = hx.lib
    rep.total.fill_(tot)
    assert int(rep.total.item()) == tot
    idx, rows = [], []
    for call in range(1, 21):
        if fused:  # the deferred draw inside learn()'s first launch (csrc/hx_update.h:397 draw_fused)
            e.sample_calls = call - 1
            e.sample(rep, n_main=DRAW_B, seed=7, defer=True)
            e._pending[0].guard = guard
            e.learn()
        else:      # a launch of its own (csrc/hx_sampler.hip:55)
            lib.call("hx_sample_batch_guarded", rep.total.data_ptr(), DRAW_CAP, rep.ring.data_ptr(), None, 0, None, 0, DRAW_B, DRAW_B, 1, 7, call, 0.2,
                     e._idx.data_ptr(), None, e._noise.data_ptr(), e.rows.data_ptr(), None, guard, lib.stream_ptr())
        idx.append(e._idx.clone())
        rows.append(e.rows.clone())
    return torch.stack(idx), torch.stack(rows)


def check_draws(hx, e, rep, small, bigs, guard, fused):
    ia, rows_a = draws(hx, e, rep, small, guard, fused)
    ok = R.allowed_slots(small, DRAW_CAP, guard)
    assert len(ok) == DRAW_CAP - guard and np.isin(ia.cpu().numpy(), ok).all()
    for t_big in bigs:
        ib, rows_b = draws(hx, e, rep, t_big, guard, fused)
        what = (t_big, t_big % DRAW_CAP, guard, "fused" if fused else "own launch")
        assert torch.equal(ia, ib), what
        assert torch.equal(rows_a.view(torch.int32), rows_b.view(torch.int32)), what
        i = ib.cpu().numpy()
        assert np.isin(i, R.allowed_slots(t_big, DRAW_CAP, guard)).all() and all(len(set(r.tolist())) == DRAW_B for r in i), what
        assert np.array_equal(R.allowed_slots(t_big, DRAW_CAP, guard), ok), what


@pytest.fixture(scope="module")
def draw_world(hx):
    p = D.make_params(31)
    e = hx.E.HirlEngine(batch=DRAW_B, use_bc=False)
    e.load_params(p["actor"], p["critic"], None)
    rep = hx.B.DeviceReplay(DRAW_CAP)
    refill(rep)
    return e, rep


@pytest.mark.parametrize("fused", [False, True], ids=["own-launch", "fused"])
@pytest.mark.parametrize("guard", [0, 150])
@pytest.mark.parametrize("h", [10, 620, 0, 699])
def test_draw(hx, draw_world, h, guard, fused):
    """The uniform draw (csrc/hx_update.h:357-384 draw_map: tot % cap, (uint32_t)tot under tot < cap, the guard window behind the head; slot_of_draw),
    as a launch of its own (csrc/hx_sampler.hip:55) and fused into learn()'s first launch (draw_fused, hx_update.h:397-401): cap = 700, batch 128,
    guard 0 and 150, heads 10, 620 (the window wraps), 0 and 699.  20 calls: idx and the gathered rows identical to the twin's, every index in
    allowed_slots(T_big, cap, guard), no index twice in a minibatch."""
    e, rep = draw_world
    small, bigs = draw_totals(h)
    check_draws(hx, e, rep, small, bigs, guard, fused)


@pytest.mark.parametrize("fused", [False, True], ids=["own-launch", "fused"])
def test_draw_at_the_edge_totals(hx, draw_world, fused):
    """the same from every total of EDGE_TOTALS(700, 1), each against the twin with its head, guard 150"""
    e, rep = draw_world
    for t_big in R.EDGE_TOTALS(DRAW_CAP, 1):
        check_draws(hx, e, rep, R.twin_offset(t_big, DRAW_CAP)[0], [t_big], 150, fused)


def sync_sides(hx, dst, src, d):
    """side `dst` <- a copy of every device buffer and host counter of `src`; its total alone is shifted by d"""
    (e1, env1, rep1), (e0, env0, rep0) = dst, src
    e1.arena.copy_(e0.arena)
    for k in ("critic_step", "actor_step", "update_count", "actor_trainable", "sample_calls", "act_calls", "learning_steps"):
        if hasattr(e0, k):
            setattr(e1, k, getattr(e0, k))
    env1._state_store.copy_(env0._state_store)
    for k in ENV_FIELDS:
        getattr(env1, k).copy_(getattr(env0, k))
    if env0.stats is not None:
        env1.stats.copy_(env0.stats)
    rep1.ring.copy_(rep0.ring)
    rep1.success.copy_(rep0.success)
    rep1.total.copy_(rep0.total)
    rep1.total.add_(d)


@pytest.mark.parametrize("cap", [1024, 1000])
def test_hirl_front_launch(hx, cap):
    """HirlEngine.step_learn (hx_hirl_front: the per-tile acting workgroups insert — csrc/hx_act_body.h:505-572 —, the draw of this call as a launch of its
    own — csrc/hx_sampler.hip:55, guard = n —, the next call's draw fused into the learn() part — csrc/hx_update.h:397): make_pair of
    tests/test_front_gpu.py at 64 envs and cap = 1,024 (the configuration of its refusal test; and cap = 1,000, which does not divide 2^32), 4 steps.  Before every step side B is made a copy of
    side A with its total shifted (two 32-row acting workgroups race for the atomic, so a free-running ring would differ in its order), and both draw
    afresh.  idx, the row tiles, the smoothing noise, the next call's idx, actions, env state, networks and Adam moments in bits (what
    test_front_launch_equals_act_step_then_guarded_learn asserts in bits), loss sums at its tolerance, rings as sorted rows."""
    from tests.test_front_gpu import NETS, make_pair

    n = 64
    for t_big in R.EDGE_TOTALS(cap, n):
        t_small, d = R.twin_offset(t_big, cap)
        side, exp, bc = make_pair(hx.E, n, cap, True, 0.0, seed=1)
        (a, env_a, rep_a), (b, env_b, rep_b) = side
        rep_a.total.fill_(t_small)
        ta, tb = t_small, t_big
        for k in range(4):
            refill(rep_a)
            sync_sides(hx, side[1], side[0], d)
            assert int(rep_b.total.item()) == tb
            outs = []
            for e, env in ((a, env_a), (b, env_b)):
                e.front_reset()
                outs.append([t.clone() for t in e.step_learn(env, exp, bc, n_main=96, act_sigma=0.1, act_seed=3, sample_seed=11,
                                                             bc_weight_now=100 if k % 2 == 0 else None, bc_warm_up_weight=0.05)])
                e.front_check()
            what = ("HIRL front launch", t_big, k)
            for x, y in zip(*outs):
                assert torch.equal(x, y), what
            assert_envs_equal(env_a, env_b, what)
            for name in ("_idx", "_noise", "rows", "_idx_bc", "bc_rows"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
            assert torch.equal(a._front_tiles[0][2], b._front_tiles[0][2]), (what, "the next call's idx")
            i = b._idx.cpu().numpy()
            assert len(set(i[:96])) == 96 and np.isin(i[:96], R.allowed_slots(tb, cap, n)).all(), what
            j = b._front_tiles[0][2].cpu().numpy()
            np.testing.assert_allclose(a.losses_host(), b.losses_host(), err_msg=str(what), **LOSS_TOL)
            for name in NETS:
                assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
            ta, tb, rows = check_call(rep_a, rep_b, ta, tb, d, False, what)
            assert len(set(j[:96])) == 96 and np.isin(j[:96], R.allowed_slots(tb, cap, n)).all(), (what, "the next call's idx")
            assert 0 < rows <= n


@pytest.mark.parametrize("cap", [512, 700])
def test_sac_small_front_launch(hx, cap):
    """SacEngine.step_learn, the per-tile acting role (hx_sac_front): the smallest case of tests/test_sac_front_small_gpu.py's list (200 envs, cap = 512,
    fp32, batch 128; and cap = 700, which does not divide 2^32), 4 steps, as test_hirl_front_launch: B a copy of A before every step, total shifted, the draw a launch of its own with guard = n."""
    from tests.test_sac_front_small_gpu import STATE, make_side

    n = 200
    for t_big in R.EDGE_TOTALS(cap, n):
        t_small, d = R.twin_offset(t_big, cap)
        side = [make_side(hx.SE, n, cap, "f32"), make_side(hx.SE, n, cap, "f32")]
        (a, env_a, rep_a), (b, env_b, rep_b) = side
        rep_a.total.fill_(t_small)
        ta, tb = t_small, t_big
        for k in range(4):
            refill(rep_a)
            sync_sides(hx, side[1], side[0], d)
            outs = []
            for e, env in ((a, env_a), (b, env_b)):
                e._front_drawn = None  # no tile in waiting: this call draws with a launch of its own
                outs.append([t.clone() for t in e.step_learn(env, None, act_seed=3, sample_seed=11)])
            what = ("SAC front launch", t_big, k)
            for x, y in zip(*outs):
                assert torch.equal(x, y), what
            assert_envs_equal(env_a, env_b, what)
            assert torch.equal(a._idx, b._idx) and torch.equal(a.rows.view(torch.int32), b.rows.view(torch.int32)), what
            assert torch.equal(a._front_tiles[0][1], b._front_tiles[0][1]), (what, "the next call's idx")
            i = b._idx.cpu().numpy()
            assert len(set(i)) == 128 and np.isin(i, R.allowed_slots(tb, cap, n)).all(), what
            np.testing.assert_allclose(a.losses_host(), b.losses_host(), err_msg=str(what), **LOSS_TOL)
            for name in STATE:
                assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
            ta, tb, rows = check_call(rep_a, rep_b, ta, tb, d, False, what)
            j = b._front_tiles[0][1].cpu().numpy()
            assert len(set(j)) == 128 and np.isin(j, R.allowed_slots(tb, cap, n)).all(), (what, "the next call's idx")


# PER capacities: 1,024 (one block of sums; it divides 2^32, so a counter cut to 32 bits would still find the right slot), 1,000 (no divisor of 2^32, a
# padded block) and 2,500 (three blocks: the block a workgroup owns follows from marked % cap too)
PER_CAPS = (1024, 1000, 2500)


def pending_counts(cap):
    return (0, 1, 300, cap, cap + 5)


def per_totals(cap):
    """EDGE_TOTALS, and 2^32 + 150 so that [marked, total) straddles 2^32 for the pending counts 300, cap and cap + 5"""
    return R.EDGE_TOTALS(cap, 300) + [(1 << 32) + 150]


def per_twin(hx, t_big, pending, fill=None, PER_CAP=1024):
    """two prioritized replays, T_small = 2 cap + h (room for cap + 5 pending rows), marked = total - pending; prio seeded (or `fill`), bsum its sums"""
    h = t_big % PER_CAP
    t_small = 2 * PER_CAP + h
    d = t_big - t_small
    assert d % PER_CAP == 0
    rng = np.random.default_rng(5)
    prio = torch.from_numpy(rng.uniform(0.05, 2.0, PER_CAP).astype(np.float32)).cuda()
    reps = []
    for shift in (0, d):
        rep = hx.B.PrioritizedReplay(PER_CAP)
        rep.ring.copy_(table(PER_CAP))
        rep.prio.copy_(prio) if fill is None else rep.prio.fill_(fill)
        rep.pmax_t.fill_(2.5)
        rep.total.fill_(t_small)
        rep.marked_t.fill_(t_small - pending)
        rep.total.add_(shift)
        rep.marked_t.add_(shift)
        rep.resum()
        reps.append(rep)
    assert int(reps[1].total.item()) == t_big and reps[1].marked == t_big - pending and reps[0].marked == t_small - pending
    return reps[0], reps[1], d


@pytest.mark.parametrize("PER_CAP", PER_CAPS)
@pytest.mark.parametrize("max_new", [None, 64])
def test_per_mark_new(hx, max_new, PER_CAP):
    """PER mark_new (csrc/hx_per.hip:19-49: [marked, total) as unsigned differences, mk % cap, marked <- mk + len), cap = 1,024 (and 1,000 and 2,500: PER_CAPS), pending rows 0, 1, 300, cap
    and cap + 5 behind every edge total and 2^32 + 150: prio and bsum in bits, marked shifted by D, and the slots that took pmax are
    slots(marked, len, cap) of the model; with max_new = 64 only the first 64 pending rows are marked."""
    for t_big in per_totals(PER_CAP):
        for pending in pending_counts(PER_CAP):
            a, b, d = per_twin(hx, t_big, pending, PER_CAP=PER_CAP)
            before = b.prio.clone()
            for rep in (a, b):
                rep.mark_new(max_new)
            what = ("mark_new", t_big, pending, max_new)
            k = min(pending, max_new or PER_CAP, PER_CAP)
            whole = min(pending, max_new or PER_CAP) >= PER_CAP
            want_marked = t_big if whole else t_big - pending + k
            assert b.marked == want_marked and b.marked - a.marked == d, (what, b.marked, a.marked)
            assert int(b.total.item()) == t_big and len(b) == PER_CAP, what
            assert torch.equal(a._prio.view(torch.int32), b._prio.view(torch.int32)) and torch.equal(a.bsum.view(torch.int32), b.bsum.view(torch.int32)), what
            assert a.pmax == b.pmax == 2.5
            want = before.clone()
            if k:
                want[R.slots(t_big - pending, k, PER_CAP)] = 2.5
            assert torch.equal(b.prio, want), (what, "the slots that took pmax")
            sums = b.bsum.clone()
            b.resum()
            assert torch.equal(sums.view(torch.int32), b.bsum.view(torch.int32)), (what, "block sums")


@pytest.mark.parametrize("PER_CAP", PER_CAPS)
def test_per_sample(hx, PER_CAP):
    """PER sample (csrc/hx_per.hip:182: the live length min(total, cap) enters the importance weights): idx, weights and the gathered rows in bits"""
    u = torch.from_numpy(np.random.default_rng(9).random(128).astype(np.float32)).cuda()
    for t_big in per_totals(PER_CAP):
        a, b, _ = per_twin(hx, t_big, 0, PER_CAP=PER_CAP)
        for kw in (dict(u=u, beta=0.4), dict(seed=3, call=5, beta=0.7)):  # injected uniforms; Philox
            out = []
            for rep in (a, b):
                idx, w, rows = torch.zeros(128, dtype=torch.int32, device="cuda"), torch.zeros(128, device="cuda"), torch.zeros(128 * 32, device="cuda")
                rep.sample_into(128, idx, w, rows, **kw)
                out.append((idx, w, rows))
            for x, y in zip(*out):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (t_big, sorted(kw))
            assert bool((out[1][1] > 0).all()) and bool(torch.isfinite(out[1][1]).all()) and 0 <= int(out[1][0].min()) and int(out[1][0].max()) < PER_CAP


@pytest.mark.parametrize("PER_CAP", PER_CAPS[:2])
def test_per_score_new(hx, PER_CAP):
    """PER score-new (csrc/hx_score.hip:33-69 score_plan, (start + i) % cap; :152 marked), the smallest chunk of tests/test_per_score_gpu.py (32 rows),
    cap = 1,024 and 1,000, the pending counts of test_per_mark_new: the call's workspace (the chunk's idx, its gathered tile), errors, prio and bsum in bits, marked
    shifted by D, and the slots that got a score are slots(marked, len, cap) — or every slot once the pending rows cover the ring."""
    e = sac_engine(hx, batch=16)
    eps = torch.from_numpy(np.random.default_rng(4).normal(size=(1024 + 16, 4)).astype(np.float32)).cuda()
    for t_big in per_totals(PER_CAP):
        for pending in pending_counts(PER_CAP):
            a, b, d = per_twin(hx, t_big, pending, fill=0.125, PER_CAP=PER_CAP)
            bound = max(pending, 16)
            for rep in (a, b):
                rep.score_chunk = 32
                e.score_new(rep, bound, eps=eps[:bound])
            what = ("score_new", t_big, pending)
            k = min(pending, PER_CAP)
            assert b.marked == t_big and b.marked - a.marked == d and int(b.total.item()) == t_big, (what, a.marked, b.marked)
            assert torch.equal(a._score_ws.view(torch.int32), b._score_ws.view(torch.int32)), (what, "workspace: idx and tile")
            assert torch.equal(a.errors[:bound].view(torch.int32), b.errors[:bound].view(torch.int32)), (what, "errors")
            assert torch.equal(a._prio.view(torch.int32), b._prio.view(torch.int32)) and torch.equal(a.bsum.view(torch.int32), b.bsum.view(torch.int32)), what
            assert a.pmax == b.pmax
            scored = (b.prio != 0.125).nonzero().flatten().tolist()
            assert scored == sorted(R.slots(t_big - pending if pending < PER_CAP else t_big, k, PER_CAP)), (what, "slots scored")
            assert bool(torch.isfinite(b.errors[:k]).all())


def test_checkpoint_after_an_env_step(hx, tmp_path):
    """utils/checkpoint.py:86-105 (replay_state: int(total.item()); load_replay_state: total.fill_(python int)) and env_state at every T_big: B is
    saved after two steps, loaded into a fresh replay and env, and one more step on both leaves rings (one workgroup: bits), counters and env state
    equal to the unsaved twin's."""
    n, cap = 64, 1000
    for t_big in R.EDGE_TOTALS(cap, n):
        ra, rb, ea, eb = run_twin(hx, n, cap, t_big, 2, lambda env, k: env.step(actions_for(n, k)), True, "before the snapshot")
        path = str(tmp_path / f"replay_{t_big}.pt")
        torch.save({"replay": hx.C.replay_state(rb), "env": hx.C.env_state(eb)}, path)
        snap = torch.load(path, map_location="cpu", weights_only=False)
        assert snap["replay"]["total"] == int(rb.total.item()) and type(snap["replay"]["total"]) is int and snap["replay"]["total"] > t_big
        rc = hx.B.DeviceReplay(cap)
        ec = hx.Env(n, scenario=(np.arange(n) % 3).astype(np.int32), seed=5, max_step=7, auto_reset=True, random_reset=True, replay=rc)
        ec.reset()
        hx.C.load_replay_state(rc, snap["replay"])
        hx.C.load_env_state(ec, snap["env"])
        assert int(rc.total.item()) == int(rb.total.item()) and len(rc) == cap
        tb = int(rb.total.item())
        refill(rb, rc)
        for env in (eb, ec):
            env.step(actions_for(n, 2))
        assert_envs_equal(eb, ec, ("after the snapshot", t_big))
        check_call(rb, rc, tb, tb, 0, True, ("after the snapshot", t_big))


def test_checkpoint_of_an_nstep_inserter(hx):
    """NStepInserter.state / load_state with its replay's snapshot at every T_big: ten calls, snapshot, a fresh replay and inserter, ten more calls on
    both — rings, windows and counters equal to the unsaved twin's (64 envs: slot order in bits)."""
    from tests.test_nstep_gpu import GAMMA

    n_envs, n = 64, 3
    obs0, steps = M.make_inputs(n_envs, n, 20)
    for cap, t_big in [(cap, t) for cap in (1024, 1000) for t in R.EDGE_TOTALS(cap, n * n_envs)]:
        rb = hx.B.DeviceReplay(cap)
        refill(rb)
        rb.total.fill_(t_big)
        ib = hx.B.NStepInserter(rb, n_envs, n, GAMMA)
        ib.reset_arrays(dev(obs0), dev(np.zeros(n_envs, np.int32)))
        push = lambda ins, st: ins.push_arrays(dev(st[0]), dev(st[1]), dev(st[2]), dev(st[3]), dev(st[4]), dev(st[5].astype(np.int32)))  # noqa: E731
        for st in steps[:10]:
            push(ib, st)
        rs, ws = hx.C.replay_state(rb), ib.state()
        rc = hx.B.DeviceReplay(cap)
        ic = hx.B.NStepInserter(rc, n_envs, n, GAMMA)
        hx.C.load_replay_state(rc, rs)
        ic.load_state(ws)
        tb = int(rb.total.item())
        assert int(rc.total.item()) == tb == rs["total"] and tb > t_big
        for st in steps[10:]:
            refill(rb, rc)
            for ins in (ib, ic):
                push(ins, st)
            assert torch.equal(ib.ws.view(torch.int32), ic.ws.view(torch.int32))
            tb = check_call(rb, rc, tb, tb, 0, True, ("n-step after the snapshot", t_big))[1]


def test_checkpoint_round_trip_of_a_prioritized_replay(hx):
    """replay_state / load_replay_state of a PrioritizedReplay with `marked` (checkpoint.py:89-93, 106-114) at total = 2^40 + 5 and at every edge total,
    3 rows pending: total and marked come back as the same Python integers, prio / pmax in bits, the block sums as resum forms them, and mark_new on
    both marks the same three slots."""
    for PER_CAP, t_big in [(cap, t) for cap in PER_CAPS[:2] for t in [(1 << 40) + 5] + per_totals(cap)]:
        _, b, _ = per_twin(hx, t_big, 3, PER_CAP=PER_CAP)
        st = hx.C.replay_state(b)
        assert st["total"] == t_big and st["per"]["marked"] == t_big - 3 and type(st["total"]) is int and type(st["per"]["marked"]) is int
        c = hx.B.PrioritizedReplay(PER_CAP)
        hx.C.load_replay_state(c, st)
        assert int(c.total.item()) == t_big and c.marked == t_big - 3 and len(c) == PER_CAP and c.pmax == b.pmax
        for rep in (b, c):
            rep.mark_new()
        assert c.marked == b.marked == t_big
        assert torch.equal(b._prio.view(torch.int32), c._prio.view(torch.int32)) and torch.equal(b.bsum.view(torch.int32), c.bsum.view(torch.int32))
        assert torch.equal(b.ring, c.ring)
        assert (c.prio == 2.5).nonzero().flatten().tolist() == sorted(R.slots(t_big - 3, 3, PER_CAP))
