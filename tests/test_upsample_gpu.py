"""GPU tests of success upsampling (hx_ups_* through SuccessUpsampler, HirlEngine.set_upsample and train_all --buffer_upsample / --expert_upsample)
against the integer model tests/_upsample_model.py — counts, `marked`, idx and rows bit for bit after every call: the rule has no float arithmetic.
Smallest shapes that can still go wrong: a ring of 3,000 slots = three blocks of 1,024 with a ragged last one (the label array ends inside a 16-byte
load), live lengths around the wave (64) and the block (1,024), batches 1, 16, 17, 128, 256."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402
from tests import _upsample_model as M  # noqa: E402

CAP = 3000
LIVES = (1, 63, 64, 65, 1023, 1024, 1025, 3000)
GUARD = -7


@pytest.fixture(scope="module")
def B_():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import buffer

    return buffer


def new_replay(B_, cap, total, labels):
    rep = B_.DeviceReplay(cap)
    rng = np.random.default_rng(cap)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(cap, 32)).astype(np.float32)))
    rep.success.copy_(torch.from_numpy(np.asarray(labels, np.int8)))
    rep.total.fill_(total)
    return rep


def check_state(ups, labels, total, cnt_model=None, marked=None):
    torch.cuda.synchronize()
    want = M.counts(labels, total, ups.replay.capacity) if cnt_model is None else cnt_model
    np.testing.assert_array_equal(ups.cnt.cpu().numpy().astype(np.uint32), want)
    assert ups.marked == (total if marked is None else marked)
    assert ups.weight_total() == M.weight_total(want, total, ups.replay.capacity, ups.boost)
    return want


def draw(ups, batch, n_main, words, seed=0, call=0):
    """-> idx[:n_main]; checks the gathered rows, the rows beyond n_main and the guard words behind both arrays"""
    idx = torch.full((batch + 8,), GUARD, dtype=torch.int32, device="cuda")
    rows = torch.full((batch + 2, 32), float(GUARD), device="cuda")
    x = None if words is None else torch.from_numpy(M.words_tensor(words)).cuda()
    ups.draw_into(batch, n_main, idx, rows, x=x, seed=seed, call=call)
    torch.cuda.synchronize()
    got = idx[:n_main].cpu().numpy()
    assert (idx[n_main:] == GUARD).all() and (rows[n_main:] == GUARD).all(), "rows beyond n_main / guard words were written"
    assert torch.equal(rows[:n_main], ups.replay.ring[idx[:n_main].long()]), "the gathered tile is not the drawn rows"
    return got


@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_counts_and_draws_at_every_live_length(B_, pattern):
    """recount and an injected draw of 128 rows at live lengths 1 .. 3,000 of a ring of 3,000; then the ring wrapped by 700 further rows that flip
    the labels of the slots they overwrite, covered by mark_new"""
    for live in LIVES:
        lab = M.make_labels(pattern, CAP, live, seed=live)
        rep = new_replay(B_, CAP, live, lab)
        ups = B_.SuccessUpsampler(rep, 10)
        ups.recount()
        cnt = check_state(ups, lab, live)
        words = M.make_words(lab, live, CAP, 10, 128, seed=live)
        got = draw(ups, 128, 128, words)
        np.testing.assert_array_equal(got, M.draw_slots(lab, cnt, live, CAP, 10, words), err_msg=f"{pattern} live {live}")
        assert got.max() < live
        if pattern == "none":  # no success row: the plain uniform draw
            np.testing.assert_array_equal(got, [(w * live) >> 64 for w in words])
        if pattern == "beyond_live":
            assert M.weight_total(cnt, live, CAP, 10) == live
    # wrapped: total = 3,000 + 700; the overwritten slots 0..699 change their labels (1 <-> not 1), the counts follow through mark_new
    lab = M.make_labels(pattern, CAP, CAP, seed=9)
    rep = new_replay(B_, CAP, CAP, lab)
    ups = B_.SuccessUpsampler(rep, 10)
    ups.recount()
    cnt = check_state(ups, lab, CAP)
    lab2 = lab.copy()
    lab2[:700] = np.where(lab[:700] == 1, 0, np.where(np.arange(700) % 3 == 0, 1, -1))
    rep.success.copy_(torch.from_numpy(lab2))
    rep.total.fill_(CAP + 700)
    ups.mark_new(700)
    cnt2, marked = M.mark_new(cnt, CAP, lab2, CAP + 700, CAP, 700)
    check_state(ups, lab2, CAP + 700, cnt2, marked)
    np.testing.assert_array_equal(cnt2, M.counts(lab2, CAP + 700, CAP))
    words = M.make_words(lab2, CAP + 700, CAP, 10, 128, seed=3)
    np.testing.assert_array_equal(draw(ups, 128, 128, words), M.draw_slots(lab2, cnt2, CAP + 700, CAP, 10, words))


def test_every_slot_of_a_small_ring(B_):
    """words 0 and 2^64 - 1, and for every live slot the two words whose targets are the first and the last integer of the slot's interval"""
    for boost in (2, 10, 255):
        lab = M.make_labels("mixed", 70, 65, seed=2)
        rep = new_replay(B_, 70, 65, lab)
        ups = B_.SuccessUpsampler(rep, boost)
        ups.recount()
        cnt = check_state(ups, lab, 65)
        words = M.make_words(lab, 65, 70, boost, 0, every_slot=True)
        got = draw(ups, len(words), len(words), words)
        np.testing.assert_array_equal(got, M.draw_slots(lab, cnt, 65, 70, boost, words))
        np.testing.assert_array_equal(got[2:], np.repeat(np.arange(65), 2))
        assert got[0] == 0 and got[1] == 64


@pytest.mark.parametrize("batch", [1, 16, 17, 128, 256])
def test_batch_sizes_and_untouched_rows(B_, batch):
    lab = M.make_labels("boundaries", CAP, 2100, seed=1)
    rep = new_replay(B_, CAP, 2100, lab)
    ups = B_.SuccessUpsampler(rep, 10)
    ups.recount()
    cnt = check_state(ups, lab, 2100)
    for n_main in sorted({batch, max(batch - batch // 4, 1), 1}):
        words = M.make_words(lab, 2100, CAP, 10, n_main, seed=batch + n_main)
        np.testing.assert_array_equal(draw(ups, batch, n_main, words), M.draw_slots(lab, cnt, 2100, CAP, 10, words))


def test_stale_counts_never_leave_the_live_length(B_):
    """rows stored since the last mark_new (the counts say less than the labels, or more): the model's rule, and no index beyond the live length"""
    lab = M.make_labels("mixed", CAP, 1500, seed=4)
    rep = new_replay(B_, CAP, 1500, lab)
    ups = B_.SuccessUpsampler(rep, 10)
    ups.recount()
    cnt = check_state(ups, lab, 1500)
    lab2 = lab.copy()
    lab2[:1500] = np.where(lab[:1500] == 1, 0, lab[:1500])  # every success row overwritten by a plain one: the counts are too large now
    rep.success.copy_(torch.from_numpy(lab2))
    words = M.make_words(lab, 1500, CAP, 10, 128, seed=5)
    got = draw(ups, 128, 128, words)
    np.testing.assert_array_equal(got, M.draw_slots(lab2, cnt, 1500, CAP, 10, words))
    assert got.max() < 1500


@pytest.mark.parametrize("n_envs", [64, 65, 300])
def test_mark_new_through_a_real_env(B_, n_envs):
    """an env inserts into a ring of 1,500 slots until it has wrapped; mark_new(n) behind every step: the counts equal a recount of replay.success on
    the host, marked == total.  Then a bound smaller than the rows that arrived advances marked by that bound only and recounts only the blocks those
    rows fell into."""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    cap = 1500
    rep = B_.DeviceReplay(cap)
    ups = B_.SuccessUpsampler(rep, 10)
    env = BatchedHarfangEnv(n_envs, scenario="straight_line", seed=2, max_step=9, auto_reset=True, random_reset=True, replay=rep)
    env.reset()
    gen = torch.Generator(device="cuda").manual_seed(n_envs)
    steps = cap // n_envs + 6
    for _ in range(steps):
        a = torch.rand((n_envs, 4), device="cuda", generator=gen) * 2 - 1
        a[:, 3] = torch.where(torch.rand(n_envs, device="cuda", generator=gen) < 0.5, 1.0, -1.0)
        env.step(a)
        ups.mark_new(n_envs)
        total = int(rep.total.item())
        check_state(ups, rep.success.cpu().numpy(), total)
    assert total > cap
    # labels written directly (as if the next rows carried them), n_envs rows arrive, the bound says 40
    cnt = ups.cnt.cpu().numpy().astype(np.uint32)
    lab = M.make_labels("mixed", cap, cap, seed=n_envs)
    rep.success.copy_(torch.from_numpy(lab))
    rep.total += n_envs
    ups.mark_new(40)
    cnt2, marked = M.mark_new(cnt, total, lab, total + n_envs, cap, 40)
    assert marked == total + 40
    check_state(ups, lab, total + n_envs, cnt2, marked)
    ups.mark_new(n_envs)  # the rest
    cnt3, marked = M.mark_new(cnt2, marked, lab, total + n_envs, cap, n_envs)
    check_state(ups, lab, total + n_envs, cnt3, marked)
    assert marked == total + n_envs
    ups.mark_new(n_envs)  # nothing new: nothing moves
    check_state(ups, lab, total + n_envs, cnt3, marked)


def test_philox_draw(B_):
    """x = NULL: the words are Philox4x32-10(seed; row, call): the same (seed, call) gives the same indices, another call others, all as the model
    forms them; over 32 calls x 128 rows on a live length of 2,000 with 100 success rows (boost 10, W = 2,900) the drawn success rows lie within 5
    binomial standard deviations of 4,096 x 1,000 / 2,900 (the uniform sampler gives about 205); no index reaches the live length"""
    live = 2000
    lab = np.zeros(CAP, np.int8)
    lab[np.random.default_rng(0).choice(live, 100, replace=False)] = 1
    lab[live:] = 1
    rep = new_replay(B_, CAP, live, lab)
    ups = B_.SuccessUpsampler(rep, 10)
    ups.recount()
    cnt = check_state(ups, lab, live)
    W = M.weight_total(cnt, live, CAP, 10)
    assert W == 2900
    a = draw(ups, 128, 128, None, seed=11, call=1)
    np.testing.assert_array_equal(a, draw(ups, 128, 128, None, seed=11, call=1))
    assert (a != draw(ups, 128, 128, None, seed=11, call=2)).any() and (a != draw(ups, 128, 128, None, seed=12, call=1)).any()
    hits, n = 0, 0
    for call in range(32):
        got = draw(ups, 128, 128, None, seed=(5 << 32) | 77, call=call)
        np.testing.assert_array_equal(got, M.draw_slots(lab, cnt, live, CAP, 10, M.philox_words((5 << 32) | 77, call, 128)))
        assert got.max() < live
        hits += int((lab[got] == 1).sum())
        n += 128
    p = 10 * 100 / W
    mean, sd = n * p, (n * p * (1 - p)) ** 0.5
    print(f"drawn success rows {hits} of {n}: window {mean - 5 * sd:.0f} .. {mean + 5 * sd:.0f}")
    assert mean - 5 * sd <= hits <= mean + 5 * sd


def _bc_tiles(batch, n_table, seed):
    rng = np.random.default_rng(seed)
    table = torch.from_numpy(rng.normal(size=(n_table, 32)).astype(np.float32)).cuda()
    plain = torch.from_numpy(rng.choice(np.arange(100, n_table), batch, replace=False).astype(np.int32)).cuda()  # (no fire row among them)
    return table, plain


@pytest.mark.parametrize("n_fire", [1, 5])
def test_bc_replacement(B_, n_fire):
    """exactly one row of idx_bc / bc_rows differs from the plain draw, it is a fire row, and it is the model's (injected words and Philox); without an
    upsampler (n_main = 0) and together with the main draw"""
    batch = 128
    table, plain = _bc_tiles(batch, 400, n_fire)
    fire = torch.tensor([3, 17, 42, 56, 99][:n_fire], dtype=torch.int32, device="cuda")
    lab = M.make_labels("mixed", CAP, 2000, seed=1)
    rep = new_replay(B_, CAP, 2000, lab)
    ups = B_.SuccessUpsampler(rep, 10)
    ups.recount()
    cnt = check_state(ups, lab, 2000)
    cases = [([0, 0], None), ([M.MASK64, M.MASK64], None), ([0x123456789ABCDEF0, 0xFEDCBA9876543210], None), (None, (9, 4))]
    for with_main in (False, True):
        for words, key in cases:
            idx_bc, bc_rows = plain.clone(), table[plain.long()].clone()
            n_main = 96 if with_main else 0
            idx = torch.full((batch,), GUARD, dtype=torch.int32, device="cuda")
            rows = torch.full((batch, 32), float(GUARD), device="cuda")
            if words is None:
                allw = M.philox_words(key[0], key[1], n_main, fire=True)
                x = None
            else:
                allw = M.make_words(lab, 2000, CAP, 10, n_main, seed=2)[:n_main] + words
                x = torch.from_numpy(M.words_tensor(allw)).cuda()
            B_.draw_call(ups if with_main else None, rep.ring, batch, n_main, idx, rows, x, key[0] if key else 0, key[1] if key else 0, fire, table, idx_bc,
                         bc_rows)
            torch.cuda.synchronize()
            j, k = M.fire_replacement(allw[n_main], allw[n_main + 1], n_fire, batch)
            changed = torch.nonzero(idx_bc != plain).reshape(-1).tolist()
            assert changed == [k] and int(idx_bc[k]) == int(fire[j])
            assert torch.equal(bc_rows, table[idx_bc.long()]) and not torch.equal(bc_rows[k], table[plain[k].long()])
            if with_main:
                np.testing.assert_array_equal(idx[:n_main].cpu().numpy(), M.draw_slots(lab, cnt, 2000, CAP, 10, allw[:n_main]))
                assert (idx[n_main:] == GUARD).all() and (rows[n_main:] == GUARD).all()
            else:
                assert (idx == GUARD).all() and (rows == GUARD).all()


def test_refusals(B_):
    from hirl4ucav_amd import _lib

    rep = new_replay(B_, CAP, 100, np.zeros(CAP, np.int8))
    for boost in (1, 256, 0):
        with pytest.raises(ValueError, match="2..255"):
            B_.SuccessUpsampler(rep, boost)
    ups = B_.SuccessUpsampler(rep, 10)
    idx, rows = torch.zeros(128, dtype=torch.int32, device="cuda"), torch.zeros((128, 32), device="cuda")
    for batch, n_main in ((0, 0), (1025, 1), (16, 17), (16, -1)):
        with pytest.raises(_lib.HxError, match="batch"):
            ups.draw_into(batch, n_main, idx, rows)
    with pytest.raises(_lib.HxError, match="nothing to do"):
        ups.draw_into(16, 0, idx, rows)
    with pytest.raises(_lib.HxError, match="needs ups"):
        B_.draw_call(None, rep.ring, 16, 4, idx, rows)
    fire = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.HxError, match="bc_table"):
        ups.draw_into(16, 4, idx, rows, fire=fire)
    with pytest.raises(ValueError, match="int32"):
        ups.draw_into(16, 4, idx, rows, fire=fire.long(), bc_table=rows, idx_bc=idx, bc_rows=rows)
    with pytest.raises(_lib.HxError, match="max_new"):
        _lib.call("hx_ups_mark_new", __import__("ctypes").byref(ups.ups), 0, None)
    with pytest.raises(ValueError, match="upsample_boost"):
        ups.load_state({"boost": 3, "marked": 0})
    assert ups.state() == {"boost": 10, "marked": 0}


NETS = ("actor", "target_actor", "bc_actor", "critic", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic", "wstate", "soft_count")


def _engine(params):
    from hirl4ucav_amd.agents import engine as E

    eng = E.HirlEngine(batch=128)
    eng.load_params(params["actor"], params["critic"], params["bc_actor"])
    return eng


def test_engine_sample_and_learn(B_):
    """sample() with an upsampler and the fire rows: rows [n_main, B), the noise and the untouched BC rows are the plain sample()'s of the same seed
    and call, rows [0, n_main) the model's Philox draw; learn() behind it is bit-identical to assemble() with the same indices followed by learn():
    networks, moments, soft weight and soft count bit for bit; the logged losses, sums of float atomics, at the bar identical launches are held to
    elsewhere in the suite (measured here: up to 2 ulp apart).  step_learn refuses."""
    from hirl4ucav_amd import _lib

    params, data = D.make_params(1), D.make_data(2)
    lab = M.make_labels("mixed", D.N_REPLAY, D.N_REPLAY, seed=3)
    rep = B_.DeviceReplay(D.N_REPLAY)
    rep.store_rows(torch.from_numpy(data["replay"]), torch.from_numpy(lab))
    expert = B_.DeviceReplay(D.N_EXPERT_ROWS + 10)
    expert.store_rows(torch.from_numpy(data["expert_rows"]))
    bc = np.zeros((D.N_EXPERT, 32), np.float32)
    bc[:, 0:13], bc[:, 13:17] = data["expert_s"], data["expert_a"]
    bc_table = torch.from_numpy(bc).cuda()
    fire = B_.fire_rows(bc_table)
    np.testing.assert_array_equal(fire.cpu().numpy(), np.where(data["expert_a"][:, 3] == 1)[0])
    assert fire.numel() > 1
    ups = B_.SuccessUpsampler(rep, 10)
    ups.mark_new()
    cnt = check_state(ups, lab, D.N_REPLAY)
    plain, up, ref = _engine(params), _engine(params), _engine(params)
    up.set_upsample(ups, fire)
    n_main = 100
    for call in (1, 2, 3):
        pi, pb, pn = (t.clone() for t in plain.sample(rep, expert, bc_table, n_main=n_main, seed=21))
        ui, ub, un = (t.clone() for t in up.sample(rep, expert, bc_table, n_main=n_main, seed=21, defer=(call == 2)))  # (defer is ignored)
        torch.cuda.synchronize()
        assert up._pending is None and up.upsample_calls == call == up.sample_calls
        assert torch.equal(ui[n_main:], pi[n_main:]) and torch.equal(un, pn) and torch.equal(up.rows.view(-1, 32)[n_main:], plain.rows.view(-1, 32)[n_main:])
        words = M.philox_words(21, call, n_main, fire=True)
        np.testing.assert_array_equal(ui[:n_main].cpu().numpy(), M.draw_slots(lab, cnt, D.N_REPLAY, D.N_REPLAY, 10, words[:n_main]))
        assert torch.equal(up.rows.view(-1, 32)[:n_main], rep.ring[ui[:n_main].long()])
        j, k = M.fire_replacement(words[n_main], words[n_main + 1], fire.numel(), 128)
        want_b = pb.clone()
        want_b[k] = fire[j]
        assert torch.equal(ub, want_b) and torch.equal(up.bc_rows.view(-1, 32), bc_table[ub.long()])
        up.learn(bc_weight_now=100 if call == 1 else None)
        ref.assemble(rep.ring, ui, expert_ring=expert.ring, n_main=n_main, bc_table=bc_table, idx_bc=ub)
        ref.learn(noise=un, bc_weight_now=100 if call == 1 else None)
        torch.cuda.synchronize()
        for name in NETS:
            assert torch.equal(getattr(up, name).view(torch.int32), getattr(ref, name).view(torch.int32)), (call, name)
        # the logged losses are sums of float atomics: two identical runs already differ in their last bit (tests/test_bf16_update_gpu.py,
        # tests/test_facade_gpu.py), so they are held to the bar those tests hold identical launches to; everything that feeds the next step is exact
        la, lb = np.asarray(up.losses_host(), np.float32), np.asarray(ref.losses_host(), np.float32)
        print(f"call {call}: losses bit-equal {np.array_equal(la.view(np.uint32), lb.view(np.uint32))}, max |diff| {np.abs(la - lb).max():.3g}")
        np.testing.assert_allclose(la, lb, rtol=1e-6, atol=1e-7)
        plain.learn(bc_weight_now=100 if call == 1 else None)  # (keeps the plain engine's call counters in step)
    env = types.SimpleNamespace(replay=rep, n=64)
    with pytest.raises(_lib.HxError, match="set_upsample"):
        up.step_learn(env, expert, bc_table, n_main=n_main)
    up.set_upsample(None, None)  # off again: the deferred draw is back
    up.sample(rep, expert, bc_table, n_main=n_main, seed=21, defer=True)
    assert up._pending is not None
    other = B_.SuccessUpsampler(expert, 10)
    up.set_upsample(other, None)
    with pytest.raises(_lib.HxError, match="another replay ring"):
        up.sample(rep, expert, bc_table, n_main=n_main, seed=21)


ARGS = ["--env", "straight_line", "--random", "--seed", "3", "--num_envs", "64", "--buffer_size", "4096", "--max_step", "12", "--checkpoint_rate", "1000",
        "--snapshot_every", "1", "--synthetic_expert", "--separate_launches"]  # (one env workgroup: the insert order, and with it the run, is reproducible)


def test_train_all_hirl_upsample_and_resume(B_, tmp_path, capsys):
    """train_all --agent HIRL --type soft --buffer_upsample --expert_upsample at 64 envs, 2 episodes of 12 steps, against 1 episode + --resume to 2:
    the same networks, moments, ring, labels and counters; the snapshot carries the flags and the upsampler's state with marked == total.  --resume
    under other flags is refused by name."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.agents.engine import HirlEngine

    args = ["--agent", "HIRL", "--type", "soft"] + ARGS + ["--buffer_upsample", "--expert_upsample"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert "vector loop: reference order" in out and "--buffer_upsample --expert_upsample: the upsampled draw is a launch of its own" in out
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a = torch.load(os.path.join(whole, "state_rank0.pt"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(rest, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and a["engine"]["counters"] == b["engine"]["counters"]
    assert a["engine"]["upsample"] == b["engine"]["upsample"]
    u = a["engine"]["upsample"]
    assert u["expert"] is True and u["buffer"] == {"boost": 10, "marked": a["replay"]["total"]} and u["calls"] == a["engine"]["counters"]["sample_calls"] > 0
    e = HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-4, atol=1e-6)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] > 64 * 20
    assert torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32)) and torch.equal(a["replay"]["success"], b["replay"]["success"])
    for other, word in ((["--expert_upsample"], "--buffer_upsample"), (["--buffer_upsample"], "--expert_upsample"), ([], "upsample"),
                        (["--buffer_upsample", "--expert_upsample", "--upsample_boost", "4"], "--upsample_boost")):
        with pytest.raises(ValueError, match=word):
            T.main(T.parse_args(["--agent", "HIRL", "--type", "soft"] + ARGS + other + ["--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))


def test_train_all_td3_and_bc(B_, tmp_path, capsys):
    """--agent TD3 --buffer_upsample (the extension: the same engine draws for both) and --agent BC --expert_upsample run; an expert table without a
    fire row is refused"""
    from hirl4ucav_amd import train_all as T

    run = T.main(T.parse_args(["--agent", "TD3"] + ARGS + ["--buffer_upsample", "--upsample_boost", "3", "--episodes", "1", "--result_dir", str(tmp_path / "t")]))
    snap = torch.load(os.path.join(run, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert snap["engine"]["upsample"]["buffer"] == {"boost": 3, "marked": snap["replay"]["total"]} and snap["engine"]["upsample"]["expert"] is False
    d = T.main(T.parse_args(["--agent", "BC", "--env", "straight_line", "--seed", "1", "--episodes", "2", "--max_step", "20", "--synthetic_expert",
                             "--expert_upsample", "--checkpoint_rate", "1000", "--result_dir", str(tmp_path / "bc")]))
    log = capsys.readouterr().out
    assert log.count("bc_loss") == 2 and os.path.isdir(os.path.join(d, "model"))
    csv = tmp_path / "nofire.csv"
    T_cfg = T.parse_args(["--agent", "BC", "--episodes", "1", "--max_step", "2", "--expert_upsample", "--expert_csv", str(csv), "--result_dir", str(tmp_path / "n")])
    real = T.load_expert_files
    T.load_expert_files = lambda config: [(np.zeros((300, 13), np.float32), -np.ones((300, 4), np.float32))]
    try:
        with pytest.raises(SystemExit, match="no row whose fire action is 1"):
            T.main(T_cfg)
    finally:
        T.load_expert_files = real


def test_facade_expert_upsample(B_):
    """the façade Agent with expert_upsample = True under a seeded np.random: learn() runs, and the BC minibatch it assembled holds the row the
    reference's call order picks"""
    from hirl4ucav_amd.agents.HIRL import Agent

    data = D.make_data(2)
    np.random.seed(4)
    torch.manual_seed(4)
    ag = Agent(1e-3, 1e-3, 13, 4, 256, 512, 0.005, 0.99, 4096, 16, True, "t", expert_states=data["expert_s"], expert_actions=data["expert_a"], bc_weight=0.5)
    assert ag.buffer_upsample is False and ag.expert_upsample is False
    np.testing.assert_array_equal(ag.target_indices, np.where(data["expert_a"][:, 3] == 1)[0])
    for r in data["replay"][:64]:
        ag.buffer.store(r[0:13], r[13:17], r[17:30], r[30], r[31], 0)
    ag.expert_upsample = True
    import random

    random.seed(1)
    np.random.seed(8)
    out = ag.learn(0.5, 0)
    np.random.seed(8)
    want = np.random.choice(D.N_EXPERT, 16, replace=False)
    selected = np.random.choice(ag.target_indices)
    want[np.random.randint(16)] = selected
    torch.cuda.synchronize()
    assert torch.equal(ag.eng.bc_rows.view(-1, 32)[:16], ag._bc_table[torch.from_numpy(want).cuda().long()])
    assert len(out) == 6 and all(np.isfinite(float(v)) for v in out) and data["expert_a"][selected, 3] == 1
