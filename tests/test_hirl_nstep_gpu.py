"""GPU tests of n-step returns for HIRL and TD3: hx_nstep_label (the expert table's relabelling) against its numpy model bit for bit, HirlEngine.set_multi_step
in the reference order and in the front form, learn() on n-step rows against the oracle, and train_all --hirl_multi_step.  Logged loss sums (float
atomics) are compared at rtol 1e-6 / atol 1e-7, everything else as bits.  Smallest shapes that can still go wrong: one workgroup and two, a ragged tail,
segments that end on and behind a workgroup's last row."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _nstep_label_model as LM  # noqa: E402
from tests import _nstep_model as M  # noqa: E402
from tests import _sharded_lockstep as LS  # noqa: E402

GAMMA = 0.99
GUARD = 64  # words behind rows_out


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- (a) the kernel ----------------------------------------------------------------------------------------------------------------------------------
def label_call(rows_in, last, E_, n, gamma, out):
    from hirl4ucav_amd import _lib

    _lib.call("hx_nstep_label", rows_in.data_ptr(), last.data_ptr(), E_, n, gamma, out.data_ptr(), _lib.stream_ptr())


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 130, 300])
def test_label_equals_the_model(E, rows, n):
    """the seeded table of tests/test_hirl_nstep_cpu.py::test_seeded_table_hides_no_case cut at `rows`: rows_out equals the model's bit for bit, the
    guard words behind it and rows_in are untouched; once more with the final `last` byte cleared (the table's end ends a segment whatever it says:
    nothing is read past E), and through utils.buffer.nstep_relabel"""
    from hirl4ucav_amd.utils.buffer import nstep_relabel

    table, last, _ = LM.make_table(n, rows)
    want = LM.relabel(table, last, n, GAMMA)
    for clear_final in (False, True):
        lb = last.copy()
        if clear_final:
            lb[-1] = 0
        rin, lst = dev(table), dev(lb)
        out = torch.full((rows * 32 + GUARD,), float("nan"), device="cuda")
        out[rows * 32:] = 12345.0
        label_call(rin, lst, rows, n, GAMMA, out)
        got = out.cpu().numpy()
        assert np.array_equal(bits(got[:rows * 32]).reshape(rows, 32), bits(want)), (rows, n, clear_final)
        assert (got[rows * 32:] == 12345.0).all(), "guard words"
        assert np.array_equal(bits(rin.cpu().numpy()), bits(table)), "rows_in"
    got = nstep_relabel(dev(table), last, n, GAMMA)
    assert got.shape == (rows, 32) and np.array_equal(bits(got.cpu().numpy()), bits(want))
    if n == 1:
        assert np.array_equal(got.cpu().numpy(), table)  # equal in value


def test_label_argument_errors(E):
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils.buffer import nstep_relabel

    buf = torch.zeros(64 * 32 * 3 + 8, device="cuda")
    rin, out = buf[:64 * 32], buf[64 * 32 * 2:64 * 32 * 3]
    last = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()
    ok = (rin.data_ptr(), last.data_ptr(), 64, 3, GAMMA, out.data_ptr(), st)

    def call(**kw):
        a = dict(zip(("rows_in", "last", "E", "n", "gamma", "rows_out", "stream"), ok))
        a.update(kw)
        _lib.call("hx_nstep_label", *a.values())

    call()
    for kw, words in (({"n": 0}, "hx_nstep_label: n is 1..8, got 0"), ({"n": 9}, "hx_nstep_label: n is 1..8, got 9"), ({"n": -1}, "n is 1..8"),
                      ({"E": 0}, "hx_nstep_label: 0 < E < 2^31 rows, got 0"), ({"E": -5}, "0 < E < 2^31 rows, got -5"), ({"E": 1 << 31}, "0 < E < 2^31"),
                      ({"gamma": 1.5}, "gamma in [0, 1]"), ({"gamma": -0.1}, "gamma in [0, 1]"),
                      ({"rows_in": None}, "rows_in [E][32], last [E] and rows_out [E][32]"), ({"last": None}, "rows_in [E][32], last [E] and rows_out"),
                      ({"rows_out": None}, "rows_in [E][32], last [E] and rows_out"),
                      ({"rows_in": rin.data_ptr() + 4}, "16-byte aligned"), ({"rows_out": out.data_ptr() + 8}, "16-byte aligned"),
                      ({"rows_out": rin.data_ptr()}, "rows_out must not overlap rows_in"),
                      ({"rows_out": rin.data_ptr() + 64 * 128 - 16}, "rows_out must not overlap rows_in"),
                      ({"rows_in": out.data_ptr() + 128}, "rows_out must not overlap rows_in")):
        with pytest.raises(_lib.HxError) as err:
            call(**kw)
        assert words in str(err.value), (kw, str(err.value))
    call(rows_out=rin.data_ptr() + 64 * 128)  # back to back is no overlap
    with pytest.raises(ValueError, match="fp32 \\[E, 32\\]"):
        nstep_relabel(torch.zeros(4, 31, device="cuda"), last[:4], 3, GAMMA)
    with pytest.raises(ValueError, match="last bytes"):
        nstep_relabel(torch.zeros(4, 32, device="cuda"), last[:3], 3, GAMMA)
    torch.cuda.synchronize()


# ---- (b) the engine in the reference order ---------------------------------------------------------------------------------------------------------------
def test_act_step_then_push_through_a_real_env(E):
    """BatchedHarfangEnv(64, max_step=7, replay=None), HirlEngine.act_step and the inserter's push for 30 steps, n = 3: the model fed with the recorded
    outputs gives the same total, rows (in slot order: one workgroup), step_success and windows after every step"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay, NStepInserter
    from tests.test_nstep_gpu import check_call

    e = LS.make_engine(E, 128, D.make_params(31))
    env = BatchedHarfangEnv(64, scenario="serpentine", seed=3, max_step=7, replay=None)
    rep = DeviceReplay(1024)
    ins = NStepInserter(rep, 64, 3, GAMMA)
    e.set_multi_step(ins)
    obs0 = env.reset().cpu().numpy().copy()
    ins.reset(env)
    model = M.NStepModel(64, 3, GAMMA)
    model.reset(obs0, env.episode_ctr.cpu().numpy())
    t, kinds = 0, set()
    for step in range(30):
        act, obs, rew, done, suc = e.act_step(env, sigma=0.1, seed=5)
        ins.push(env, act)
        want = model.push(obs.cpu().numpy(), act.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), suc.cpu().numpy(), env.episode_ctr.cpu().numpy())
        kinds |= {k[3] for k in want[2]}
        t = check_call(ins, model, rep, t, want, True, f"step {step}")
    assert {"trunc", "full"} <= kinds and t > 64 * 20


_ring = {}


def nstep_ring():
    """the outlier table of tests/_bf16_ragged.py (+600 rows) relabelled by the model at n = 3, a segment ending at every done row and every seventh
    row: full rows with d' = 1 - gamma^2, shorter ones, terminal ones.  Made once, left unchanged."""
    if not _ring:
        from tests import _bf16_ragged as R

        rows = R.data()["replay"]
        last = ((rows[:, 31] != 0) | (np.arange(rows.shape[0]) % 7 == 6)).astype(np.uint8)
        _ring["host"] = LM.relabel(rows, last, 3, GAMMA)
        _ring["dev"] = dev(_ring["host"])
        assert len(np.unique(_ring["host"][:, 31])) == 4  # 0, 1 - gamma, 1 - gamma^2, 1
    return _ring["host"], _ring["dev"]


@pytest.mark.parametrize("B", [16, 48])
@pytest.mark.parametrize("kind", ["hirl", "td3"])
def test_learn_on_nstep_rows_matches_the_oracle(E, kind, B):
    """two learn() calls (an actor call, a critic-only call) on minibatches of n-step rows against HirlOracle.learn on the same rows with the one-step
    gamma, from synchronised states: losses, every gradient entry and the stepped parameters under the bars of tests/test_hirl_gpu.py — the done column
    is read arithmetically, so a row's discount rides in it"""
    from tests import _bf16_ragged as R
    from tests.test_hirl_gpu import assert_losses, check_params, device_tables, oracle_learn_checked, sync_oracle

    host, ring = nstep_ring()
    p, data = R.params(), R.data()
    _, _, bc = device_tables(data)
    use_bc = kind == "hirl"
    e = LS.make_engine(E, B, p, use_bc=use_bc, slope=0.0 if use_bc else 0.01)
    o = H.HirlOracle(p["actor"], p["critic"], p["bc_actor"] if use_bc else None, slope=0.0 if use_bc else 0.01, use_bc=use_bc)
    for k, (idx, ibc, noise) in enumerate(R.calls("soft" if use_bc else "td3", B)[:2]):
        rows = host[idx]
        assert len(np.unique(rows[:, 31])) >= 3, "terminal, full and short rows in every minibatch"
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        if use_bc:
            e.assemble(ring, dev(idx), bc_table=bc, idx_bc=dev(ibc))
            e.learn(noise=dev(noise), bc_weight_now=100, bc_warm_up_weight=0.1)
            args = ((rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]), R.bc_batch_of(ibc), noise, 100, 0.1)
        else:
            e.assemble(ring, dev(idx))
            e.learn(noise=dev(noise))
            args = ((rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]), None, noise)
        what = f"{kind} B={B} call {k}"
        ref = oracle_learn_checked(E, e, o, args, was_actor_call, what + " gradients")
        n = 6 if use_bc else 2
        print(f"\n[hirl n-step] {what}: losses {np.asarray(e.losses_host()[:n])} oracle {np.asarray(ref[:n])}")
        assert_losses(e.losses_host()[:n], ref[:n], what)
        check_params(e, o, E, what + " params", was_actor_call)


@pytest.mark.parametrize("B", [16, 48])
@pytest.mark.parametrize("kind", ["hirl", "td3"])
def test_bf16_learn_on_nstep_rows_matches_the_rounded_operand_oracle(E, kind, B):
    """the same in bf16 against the rounded-operand oracle, with the bars and the method of tests/test_bf16_ragged_gpu.py"""
    from tests import _bf16_ragged as R
    from tests import test_bf16_update_gpu as U
    from tests.test_hirl_gpu import device_tables, sync_oracle

    host, ring = nstep_ring()
    p, data = R.params(), R.data()
    _, _, bc = device_tables(data)
    use_bc = kind == "hirl"
    e = LS.make_engine(E, B, p, use_bc=use_bc, slope=0.0 if use_bc else 0.01)
    e.set_update_dtype("bf16")
    o = R.new_oracle("soft" if use_bc else "td3")
    for k, (idx, ibc, noise) in enumerate(R.calls("soft" if use_bc else "td3", B)[:2]):
        rows = host[idx]
        batch = (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31])
        was_actor = e.actor_trainable
        sync_oracle(o, e, E)
        pre = (e.actor.clone(), e.critic.clone())
        if use_bc:
            e.assemble(ring, dev(idx), bc_table=bc, idx_bc=dev(ibc))
            e.learn(noise=dev(noise), bc_weight_now=R.SOFT, bc_warm_up_weight=R.WARM)
        else:
            e.assemble(ring, dev(idx))
            e.learn(noise=dev(noise))
        got = e.losses_host()
        what = f"bf16 {kind} B={B} call {k}"
        with H.Bf16Layer2(), U.KernelKinks(U.learn_masks(e, E, pre, was_actor, soft=use_bc, use_bc=use_bc, B=B)):
            ref = o.learn(batch, R.bc_batch_of(ibc) if use_bc else None, noise, *((R.SOFT, R.WARM) if use_bc else ()))
        n = 6 if use_bc else 2
        print(f"\n[hirl n-step] {what}: losses {np.asarray(got[:n])} oracle {np.asarray(ref[:n])}; critic gradient "
              f"{U.grad_stats(e.grad_critic, o.last_grads['critic'], E.CRITIC_LAYOUT)}")
        np.testing.assert_allclose(got[:n], ref[:n], rtol=U.LOSS_RTOL, atol=U.LOSS_ATOL, err_msg=what + " losses vs the rounded-operand oracle")
        U.check_grads(e.grad_critic, o.last_grads["critic"], E.CRITIC_LAYOUT, what + " critic gradient")
        if was_actor:
            U.check_grads(e.grad_actor, o.last_grads["actor"], E.ACTOR_LAYOUT, what + " actor gradient")
        U.check_params(e, o, E, what + " parameters", was_actor)
        U.assert_images_current(e, E, what)


def test_a_planted_reward_reaches_the_target_through_three_steps(E):
    """a hand-built segment of three rows, 1,000 planted in the LAST one's reward, relabelled on the device at n = 3: row 0's TD error, read through
    set_prioritized's _errors, is |Q1(s_0, a_0) - (r0 + gamma r1 + gamma^2 r2 + gamma^3 min Q'(s'_2, pi'(s'_2)))| with the heads of the oracle's networks
    (float64 from there on), to the bar tests/test_hirl_per_gpu.py holds errors to; without the plant the error is a far smaller one"""
    from hirl4ucav_amd.utils.buffer import nstep_relabel
    from tests.test_hirl_per_gpu import ERR_ATOL, ERR_RTOL, replay_of

    B = 16
    p, data = D.make_params(11), D.make_data(12)
    table = data["replay"][:B].copy()
    table[:, 31] = 0.0
    table[1, 0:13], table[2, 0:13] = table[0, 17:30], table[1, 17:30]
    last = np.ones(B, np.uint8)
    last[0:2] = 0
    noise = np.array([0.05, -0.1, 0.02, 0.0], np.float32)
    g = float(np.float32(GAMMA))
    errs = []
    for plant in (1000.0, 0.0):
        t = table.copy()
        t[2, 30] += np.float32(plant)
        ring = nstep_relabel(dev(t), last, 3, GAMMA)
        want_row = LM.relabel(t, last, 3, GAMMA)
        assert np.array_equal(bits(ring.cpu().numpy()), bits(want_row)) and want_row[0, 31] == np.float32(1) - np.float32(np.float32(GAMMA) * np.float32(GAMMA))
        e = LS.make_engine(E, B, p, use_bc=False, slope=0.01)
        e.set_prioritized(replay_of(ring))
        o = H.HirlOracle(p["actor"], p["critic"], None, slope=0.01, use_bc=False)
        idx = np.arange(B, dtype=np.int32)
        e.assemble(ring, dev(idx))
        e.set_weights(np.ones(B, np.float32), B, idx=idx)
        e.learn(noise=dev(noise))
        with torch.no_grad():
            s0, a0, s3 = (torch.from_numpy(t[0:1, 0:13]), torch.from_numpy(t[0:1, 13:17]), torch.from_numpy(t[2:3, 17:30]))
            na = (H.actor_forward(o.target_actor, s3, o.slope) + torch.from_numpy(noise).clamp(-o.noise_clamp, o.noise_clamp)).clamp(-1, 1)
            tq1, tq2 = H.critic_forward(o.target_critic, s3, na, o.slope)
            q1, _ = H.critic_forward(o.critic, s0, a0, o.slope)
        r = t[0:3, 30].astype(np.float64)
        y = r[0] + g * r[1] + g * g * r[2] + g ** 3 * float(torch.min(tq1, tq2))
        want = abs(float(q1) - y)
        got = float(e._errors[0])
        print(f"\n[hirl n-step] planted {plant}: |Q1 - y| {got} expected {want}")
        np.testing.assert_allclose(got, want, rtol=ERR_RTOL, atol=ERR_ATOL)
        errs.append(got)
    assert abs(errs[0] - errs[1]) > 900.0, errs  # (the plant moves the target by gamma^2 1,000)


# ---- (c) the front form ------------------------------------------------------------------------------------------------------------------------------
def make_pair(E, n, cap, use_bc, slope, act, n_step=3):
    """two engines with an env WITHOUT a ring, a replay and an n-step inserter each (tests/test_front_gpu.make_pair otherwise)"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay, NStepInserter

    params = D.make_params(31)
    rng = np.random.default_rng(n)
    exp = DeviceReplay(64)
    exp.store_rows(torch.from_numpy(rng.normal(size=(40, 32)).astype(np.float32)))
    bc = torch.from_numpy(rng.normal(size=(150, 32)).astype(np.float32)).cuda() if use_bc else None
    scen = (np.arange(n) % 3).astype(np.int32)
    side = []
    for _ in range(2):
        e = E.HirlEngine(batch=128, use_bc=use_bc, slope=slope)
        e.x9_rows, e.front_x9 = None, False  # "f32" = fp32 MFMA in the front launch too: act_step below x9_rows is its reference
        e.load_params(params["actor"], params["critic"], params["bc_actor"] if use_bc else None)
        if act == "bf16":
            e.set_update_dtype("bf16")
        if act != "f32":
            e.set_act_dtype(act)
        rep = DeviceReplay(cap)
        env = BatchedHarfangEnv(n, scenario=scen, seed=5, max_step=6, auto_reset=True, random_reset=True, replay=None)
        env.reset()
        ins = NStepInserter(rep, n, n_step, GAMMA)
        ins.reset(env)
        e.set_multi_step(ins)
        side.append((e, env, rep, ins))
    return side, exp, bc


def sync(dst, src):
    from tests.test_front_gpu import sync as sync3

    sync3(dst[:3], src[:3])
    dst[3].ws.copy_(src[3].ws)


def recording(names):
    """context: every library call's name goes into `names`"""
    from hirl4ucav_amd import _lib

    class Ctx:
        def __enter__(self):
            self.real = _lib.call
            _lib.call = lambda name, *a: names.append(name) or self.real(name, *a)

        def __exit__(self, *exc):
            _lib.call = self.real

    return Ctx()


@pytest.mark.parametrize("use_bc,slope,act,clip", [(True, 0.0, "f32", None), (False, 0.01, "f32", None), (True, 0.0, "f32x9", None), (True, 0.0, "bf16", None),
                                                   (True, 0.0, "f32", 0.05), (False, 0.01, "bf16", 0.05)],
                         ids=["hirl-f32", "td3-f32", "hirl-x9", "hirl-bf16", "hirl-f32-clip", "td3-bf16-clip"])
def test_front_form_equals_guarded_draw_act_step_learn_push(E, use_bc, slope, act, clip):
    """step_learn with an inserter against the same step as separate launches, from synchronised states, 64 envs = one env workgroup and one pushing
    workgroup, a ring of 512 that wraps: act_step on the env without a ring, learn() on a minibatch drawn (deferred, guard = 64) from the ring as it
    stood BEFORE THE PREVIOUS STEP'S PUSH — that is when the front form drew it: inside the previous call, in front of that call's push — launch B in the
    front launch's tiling, then the push.  Bit for bit in everything both leave behind; exactly one push per step on either side."""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils.buffer import DeviceReplay
    from tests.test_front_gpu import NETS, sorted_rows

    L = _lib.load()
    n, cap = 64, 512
    side, exp, bc = make_pair(E, n, cap, use_bc, slope, act)
    (a, env_a, rep_a, ins_a), (b, env_b, rep_b, ins_b) = side
    for e in (a, b):
        e.set_grad_clip(clip)
    for _ in range(5):  # enough rows in the ring for the first draw of 96 behind a guard of 64
        out = a.act_step(env_a, sigma=0.1, seed=3)
        ins_a.push(env_a, out[0])
    assert int(rep_a.total.item()) >= 96 + n
    before = DeviceReplay(cap)  # the ring as it stood before the previous step's push (before the first step: as it stands)
    before.ring.copy_(rep_a.ring)
    before.total.copy_(rep_a.total)
    names_a, names_b, steps = [], [], 10
    real_push = ins_a.push

    def push_a(env, actions):  # (what the front form's NEXT minibatch was drawn from, a moment ago)
        push_a.ring, push_a.total = rep_a.ring.clone(), rep_a.total.clone()
        real_push(env, actions)

    ins_a.push = push_a
    for k in range(steps):
        sync(side[1], side[0])
        w = ((100 if k % 4 == 0 else (None if k % 4 < 3 else 0.3)) if use_bc else 0.0)
        with recording(names_a):
            out_a = a.step_learn(env_a, exp, bc, n_main=96, act_sigma=0.1, act_seed=3, sample_seed=11, bc_weight_now=w, bc_warm_up_weight=0.05)
        with recording(names_b):
            out_b = b.act_step(env_b, sigma=0.1, seed=3)
            b.sample(before, exp, bc, n_main=96, seed=11, defer=True)
            b._pending[0].guard = n
            L.hx_debug_set_fwd_nt(64, 1, 1)  # launch B in the front launch's tiling (tests/test_front_gpu.py)
            try:
                b.learn(bc_weight_now=w, bc_warm_up_weight=0.05)
            finally:
                L.hx_debug_set_fwd_nt(0, 0, 0)
            ins_b.push(env_b, out_b[0])
        a.front_check()
        before.ring.copy_(push_a.ring)
        before.total.copy_(push_a.total)
        for x, y, name in zip(out_a, out_b, ("actions", "obs", "reward", "done", "success")):
            assert torch.equal(x, y), (k, name)
        assert torch.equal(env_a._state_store, env_b._state_store) and torch.equal(env_a.episode_ctr, env_b.episode_ctr), k
        assert torch.equal(rep_a.total, rep_b.total) and LS.bits_equal(ins_a.ws, ins_b.ws), k
        np.testing.assert_array_equal(bits(rep_a.ring.cpu().numpy()), bits(rep_b.ring.cpu().numpy()), err_msg=f"step {k}: replay rows")
        assert torch.equal(rep_a.success, rep_b.success), k
        for name in ("_idx", "_noise", "rows") + (("_idx_bc", "bc_rows") if use_bc else ()):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        np.testing.assert_allclose(a.losses_host(), b.losses_host(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
        for name in NETS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        if clip is not None:
            assert LS.bits_equal(a.clip_ws, b.clip_ws), k
        assert a._front_drawn[:3] == (env_a, env_a.steps_issued, rep_a) and a._front_drawn[8] == a.sample_calls + 1
    assert names_a.count("hx_nstep_push") == names_b.count("hx_nstep_push") == steps, "one push per env step"
    assert names_a.count("hx_hirl_front") == steps and names_a.count("hx_sample_batch_guarded") == 1 and "hx_actor_act_step" not in names_a
    assert ("hx_hirl_learn_back" in names_a) == (clip is None) and ("hx_hirl_critic_grads_back" in names_a) == (clip is not None)
    assert int(rep_a.total.item()) > cap, "the ring was meant to wrap"
    d = sorted_rows(rep_a)[:, 31]
    assert ((d > 0) & (d < 1)).any(), "n-step rows in the ring"


def test_switched_off_the_parents_paths_call_for_call(E):
    """set_multi_step(None): step_learn and the reference order issue the parent's library calls, name for name, and leave the same state (16 envs: one
    workgroup in the acting launch and in the front launch, so the ring's slot order — and with it every draw — is the same in both runs)"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay, NStepInserter

    params = D.make_params(31)
    seqs, engines = [], []
    for back in (False, True):
        e = LS.make_engine(E, 128, params, use_bc=False, slope=0.01)
        rep = DeviceReplay(512)
        env = BatchedHarfangEnv(16, scenario="straight_line", seed=5, max_step=50, replay=rep)
        env.reset()
        if back:
            e.set_multi_step(NStepInserter(DeviceReplay(512), 16, 3, GAMMA))
            e.set_multi_step(None)
        assert e.multi_step is None
        names = []
        with recording(names):
            for _ in range(10):  # 160 rows: a draw of 128 behind a guard of 16
                e.act_step(env, sigma=0.1, seed=3)
            for _ in range(3):
                e.step_learn(env, None, None, act_sigma=0.1, act_seed=3, sample_seed=11)
            e.act_step(env, sigma=0.1, seed=3)
            e.sample(rep, seed=11, defer=True)
            e.learn()
        seqs.append(names)
        engines.append(e)
    assert seqs[0] == seqs[1] and "hx_nstep_push" not in seqs[0] and "hx_hirl_front" in seqs[0]
    LS.assert_same_state(engines[0], engines[1], "n-step returns switched off again")


def test_engine_refusals(E):
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay, NStepInserter, PrioritizedReplay

    e = LS.make_engine(E, 128, D.make_params(31))
    with pytest.raises(TypeError, match="NStepInserter"):
        e.set_multi_step(DeviceReplay(64))
    with pytest.raises(ValueError, match="gamma = 0.9"):
        e.set_multi_step(NStepInserter(DeviceReplay(1024), 64, 3, 0.9))
    rep = DeviceReplay(1024)
    ins = NStepInserter(rep, 64, 3, GAMMA)
    e.set_multi_step(ins)
    assert e.multi_step is ins and E.HirlEngine.multi_step_flag == "--hirl_multi_step"
    names = []
    with recording(names), pytest.raises(_lib.HxError, match="build it with replay=None"):  # env.replay together with an inserter
        e.step_learn(BatchedHarfangEnv(64, replay=rep))
    with recording(names), pytest.raises(ValueError, match="built for 64 envs"):
        e.step_learn(BatchedHarfangEnv(128, replay=None))
    # beyond 8,192 envs the refusal is read off the arguments: nothing is launched
    big = BatchedHarfangEnv(8192 + 64, replay=None)
    e.set_multi_step(NStepInserter(DeviceReplay(3 * (8192 + 64)), 8192 + 64, 3, GAMMA))
    with recording(names), pytest.raises(_lib.HxError, match="at most 8,192 envs \\(8256 given\\)"):
        e.step_learn(big)
    assert not names and not e.needs_reload
    per = PrioritizedReplay(1024)
    e2 = LS.make_engine(E, 128, D.make_params(31))
    e2.set_prioritized(per)
    with pytest.raises(_lib.HxError, match="another replay"):
        e2.set_multi_step(ins)
    e2.set_multi_step(NStepInserter(per, 64, 3, GAMMA))
    with pytest.raises(_lib.HxError, match="set_prioritized\\(\\) goes with sample\\(\\) \\+ learn\\(\\)"):  # the reference order only
        e2.step_learn(BatchedHarfangEnv(64, replay=None))
    e3 = LS.make_engine(E, 128, D.make_params(31))
    e3.world = 2
    with pytest.raises(_lib.HxError, match="one GPU"):
        e3.set_multi_step(ins)


# ---- (d) the driver ------------------------------------------------------------------------------------------------------------------------------------
NSTEP = ["--hirl_multi_step", "3"]
EXPLORE = 4  # ceil(20 * 12 / 64) exploration steps


def spy(monkeypatch):
    """-> (names of every library call, the runs with a copy of the expert ring as load_expert_tables left it (None: TD3), the writers)"""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import Recorder

    names, runs, writers, real_call, real_load = [], [], [], _lib.call, T.load_expert_tables

    def load(run):
        real_load(run)
        runs.append((run, run.expert.ring.clone() if run.expert is not None else None))

    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real_call(name, *a))
    monkeypatch.setattr(T, "load_expert_tables", load)
    monkeypatch.setattr(T, "make_writer", lambda d: writers.append(Recorder()) or writers[-1])
    return names, runs, writers


def expected_expert_rows(T, cfg, n):
    """the model's relabelling of the one-step rows label_expert gives for this command line"""
    from hirl4ucav_amd.utils.buffer import segment_last

    out = []
    for es, ea in T.load_expert_files(cfg):
        rows, _, keep = T.label_expert_pairs(es, ea, torch.device("cuda"))
        rows = rows.cpu().numpy()
        out.append((rows, segment_last(rows[:, 31], keep)))
    rows, last = np.concatenate([r for r, _ in out]), np.concatenate([l for _, l in out])
    return rows, LM.relabel(rows, last, n, GAMMA)


@pytest.mark.parametrize("kind", ["front", "reference", "td3"])
def test_train_all_hirl_multi_step(E, tmp_path, monkeypatch, capsys, kind):
    """2 driver episodes of 12 steps at 64 envs, HIRL in both loop forms and TD3: the loop line, one push per env step (the exploration steps
    included) whoever issues it, the env without a ring, n-step rows in the replay, the offline expert ring equal to the model's relabelling bit for bit,
    the snapshot's windows; without the flag no new call is made"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import COMMON, HIRL

    args = ["--agent", "TD3"] + COMMON if kind == "td3" else HIRL + ["--loop", kind]
    names, runs, writers = spy(monkeypatch)
    cfg = T.parse_args(args + NSTEP + ["--episodes", "2", "--result_dir", str(tmp_path / "a")])
    out_dir = T.main(cfg)
    out = capsys.readouterr().out
    front = kind != "reference"
    if front:
        assert ("vector loop: front launch (env step + first launches of learn() in one launch; draw before the insert) (--hirl_multi_step 3: the n-step rows "
                "are written by a launch of their own behind the front launch's call") in out
        assert names.count("hx_hirl_front") == 2 * 11 and names.count("hx_actor_act_step") == 2  # (an episode's last step only acts)
    else:
        assert "vector loop: reference order (--hirl_multi_step 3: the n-step rows are written by a launch of their own behind the acting launch)" in out
        assert names.count("hx_actor_act_step") == 2 * 12 and "hx_hirl_front" not in names
    steps = names.count("hx_hirl_front") + names.count("hx_actor_act_step")
    assert names.count("hx_nstep_push") == steps + EXPLORE and names.count("hx_nstep_reset") == 1, "one push per env step"
    assert names.count("hx_nstep_label") == (0 if kind == "td3" else 1)
    run = runs[0][0]
    assert run.env.replay is None and run.eng.multi_step is run.inserter and run.inserter.n == 3
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert snap["engine"]["multi_step"]["n"] == 3 and torch.isfinite(snap["engine"]["arena"]).all()
    live = snap["replay"]["ring"][:min(snap["replay"]["total"], 4096)]
    d = live[:, 31]
    assert snap["replay"]["total"] > 64 * 12 and ((d > 0) & (d < 1)).sum() > len(d) // 2 and torch.isfinite(live).all()
    if kind != "td3":
        one_step, want = expected_expert_rows(T, cfg, 3)
        got = runs[0][1][:want.shape[0]].cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), "the expert ring is the model's relabelling"
        assert not np.array_equal(got[:, 30], one_step[:, 30]) and np.array_equal(bits(got[:, 0:17]), bits(one_step[:, 0:17]))
    del names[:]
    T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    assert names and not {"hx_nstep_push", "hx_nstep_reset", "hx_nstep_label"} & set(names)


def test_train_all_hirl_multi_step_resume(E, tmp_path):
    """--separate_launches (one env workgroup, one pushing workgroup: the run is reproducible): 1 episode + --resume to 2 equals the uninterrupted run bit
    for bit — the arena but its logged loss slots (rtol 1e-6 / atol 1e-7), the replay ring and the inserter's windows; --resume under another N is
    refused by the flag's name, both ways"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import HIRL

    args = HIRL + NSTEP + ["--separate_launches"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a, b = (torch.load(os.path.join(d, "state_rank0.pt"), map_location="cpu", weights_only=False) for d in (whole, rest))
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and a["engine"]["counters"] == b["engine"]["counters"]
    e = E.HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-6, atol=1e-7)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] and torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32))
    ma, mb = a["engine"]["multi_step"], b["engine"]["multi_step"]
    assert ma["n"] == mb["n"] == 3 and torch.equal(ma["ws"].view(torch.int32), mb["ws"].view(torch.int32))
    for other, words in ((["--hirl_multi_step", "2"], "was run with --hirl_multi_step 3, --hirl_multi_step 2 given"),
                         ([], "was run with --hirl_multi_step 3, --hirl_multi_step 1 given")):
        with pytest.raises(SystemExit, match=words):
            T.main(T.parse_args(HIRL + other + ["--separate_launches", "--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))
    plain = T.main(T.parse_args(HIRL + ["--separate_launches", "--episodes", "1", "--result_dir", str(tmp_path / "e")]))
    with pytest.raises(SystemExit, match="was run with --hirl_multi_step 1, --hirl_multi_step 3 given"):
        T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "f"), "--resume", plain]))


@pytest.mark.parametrize("more", [["--hirl_per", "--per_beta_annealing", "0.01"], ["--expert_floor", "32", "--expert_branch", "96", "--expert_branch_per_step", "40"],
                                  ["--buffer_upsample"]], ids=["per", "floor-branch", "upsample"])
def test_train_all_hirl_multi_step_with(E, tmp_path, monkeypatch, capsys, more):
    """one episode of 12 steps together with --hirl_per (every stored row holds a priority: mark_new's bound is n * num_envs), with --expert_floor 32
    --expert_branch (the offline region is the model's relabelling, branch rows stay one-step rows) and with --buffer_upsample (the counts cover every
    stored row)"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import HIRL

    names, runs, writers = spy(monkeypatch)
    cfg = T.parse_args(HIRL + NSTEP + more + ["--episodes", "1", "--result_dir", str(tmp_path / "a")])
    out_dir = T.main(cfg)
    steps = names.count("hx_hirl_front") + names.count("hx_actor_act_step")
    assert steps == 12 and names.count("hx_nstep_push") == steps + EXPLORE
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert snap["engine"]["multi_step"]["n"] == 3 and torch.isfinite(snap["engine"]["arena"]).all()
    run = runs[0][0]
    if "--hirl_per" in more:
        per = snap["replay"]["per"]
        n_live = min(snap["replay"]["total"], 4096)
        assert snap["engine"]["prioritized"] is True and per["marked"] == snap["replay"]["total"] and (per["prio"][:n_live] > 0).all()
        assert "hx_hirl_front" not in names and names.count("hx_per_mark_new") == 12 + 1
    elif "--buffer_upsample" in more:
        assert "hx_hirl_front" not in names and run.upsampler.marked == int(run.replay.total.item())
        assert int(run.upsampler.cnt.sum().item()) == int((run.replay.success[:min(int(run.replay.total.item()), 4096)] == 1).sum().item())
    else:
        one_step, want = expected_expert_rows(T, cfg, 3)
        e0 = want.shape[0]
        assert np.array_equal(bits(runs[0][1][:e0].cpu().numpy()), bits(want)), "the offline region is the model's relabelling"
        assert "hx_pilot_branch" in names and "hx_hirl_front" in names
        ring = run.expert.ring[:e0 + 96].cpu().numpy()
        assert np.array_equal(bits(ring[:e0]), bits(want)), "the branches leave the offline region alone"
        d = ring[e0:, 31]
        assert ((d == 0) | (d == 1) | np.isin(bits(d), bits(want[:, 31]))).all()  # branch rows are one-step rows (the rest: the cyclic copy it started as)
