"""--hirl_per for HIRL and TD3 (train_all's name for HirlEngine.set_prioritized; --per stays SacAgent's keyword and stays refused for them), the parts
that need no GPU: the weighted restatement of tests/_hirl_per against a float64 evaluation of the same formula, the restatement without weights against
the reference's golden, the priority step rule on tests/_per_check.PerModel, train_all's flag, refusals, resume rule and loop line, the snapshot record,
the header's entry point.

Bars: those tests/test_oracle_hirl.py holds HirlOracle to its golden — returned losses rtol 1e-5 / atol 1e-6, parameter probes after the Adam step rtol 1e-5 /
atol 2e-6, their |x| sums rtol 1e-6."""
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _hirl_per as W  # noqa: E402
from tests import _per_check as P  # noqa: E402

torch.set_num_threads(1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(B, seed, data):
    rng = np.random.default_rng(seed)
    idx, ibc = rng.integers(0, D.N_REPLAY, B), rng.integers(0, D.N_EXPERT, B)
    rows = data["replay"][idx]
    batch = (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31])
    return batch, (data["expert_s"][ibc], data["expert_a"][ibc]), rng.normal(0, 0.2, 4).astype(np.float32), rng.uniform(0.05, 1.0, B).astype(np.float32)


@pytest.mark.parametrize("use_bc,layer_norm", [(True, True), (False, True), (True, False)], ids=["hirl", "td3", "noln"])
@pytest.mark.parametrize("B,n_main", [(16, 16), (48, 43), (144, 1)])
def test_weighted_restatement_against_float64(use_bc, layer_norm, B, n_main):
    """critic loss, |Q1 - y| of every row and the critic after its Adam step (the weighted gradient, through 128 probes and the |x| sum as the golden
    test reads them) against float64 autograd of mean(w (Q1 - y)^2) + mean(w (Q2 - y)^2) with w = weights[:n_main] ++ ones, from the same state;
    the actor half is the oracle's own: same actor as the unweighted oracle given the same critic"""
    params = D.make_params(5) if layer_norm else D.plain_layernorm(D.make_params(5))
    data = D.make_data(6)
    kw = dict(slope=0.0 if use_bc else 0.01, use_bc=use_bc, layer_norm=layer_norm)
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"] if use_bc else None, **kw)
    batch, bc, noise, weights = _inputs(B, [B, n_main], data)
    w = W.row_weights(B, weights, n_main)
    assert (w[n_main:] == 1.0).all() and np.array_equal(w[:n_main], weights[:n_main]) and w[:n_main].min() < 1.0
    loss64, g64, err64, _ = W.critic_grads64(o, batch, noise, w)
    c64 = {k: v.detach().to(torch.float64).clone() for k, v in o.critic.items()}
    H.Adam(c64, 1e-3).step(c64, g64)
    out, err = W.weighted_learn(o, batch, bc if use_bc else None, noise, *((100, 0.05) if use_bc else ()), weights=weights, n_main=n_main)
    np.testing.assert_allclose(out[0], loss64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(err, err64, rtol=1e-5, atol=1e-6)
    s, a, v = D.net_probe(H.flatten(o.critic, H.CRITIC_KEYS))
    s64, a64, v64 = D.net_probe(np.concatenate([c64[k].numpy().ravel() for k in H.CRITIC_KEYS]))
    np.testing.assert_allclose(v, v64, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(a, a64, rtol=1e-6)
    # the gradient itself, entry by entry, at what fp32 autograd of a mean over B rows resolves: 1e-4 |g| + 2e-5 max|g| (tests/test_hirl_gpu.py's bar)
    for k in H.CRITIC_KEYS:
        g, r = o.last_grads["critic"][k].numpy().astype(np.float64), g64[k].numpy()
        assert (np.abs(g - r) <= 1e-4 * np.abs(r) + 2e-5 * max(np.abs(r).max(), 1e-30)).all(), k
    # the weights matter: the unweighted loss is another number
    plain = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"] if use_bc else None, **kw)
    ref = plain.learn(batch, bc if use_bc else None, noise, *((100, 0.05) if use_bc else ()))
    assert abs(ref[0] - out[0]) > 1e-3 * abs(ref[0])
    assert out[0] < ref[0]  # (every weight <= 1)


def test_unit_weights_and_no_weights_are_the_oracle():
    """weights of exactly 1 give the oracle's bits (x * 1.0 is exact, the mean is the same reduction); without weights nothing is substituted"""
    params, data = D.make_params(5), D.make_data(6, outliers=True)
    a, b, c = (H.HirlOracle(params["actor"], params["critic"], params["bc_actor"]) for _ in range(3))
    for k in range(2):
        batch, bc, noise, _ = _inputs(32, k, data)
        ra = a.learn(batch, bc, noise, 100, 0.05)
        rb, eb = W.weighted_learn(b, batch, bc, noise, 100, 0.05, weights=np.ones(32, np.float32))
        rc, ec = W.weighted_learn(c, batch, bc, noise, 100, 0.05)
        assert ec is None and rc == ra and eb.shape == (32,)
        np.testing.assert_allclose(rb, ra, rtol=1e-6, atol=1e-7)
        for key in a.critic:
            assert torch.equal(a.critic[key], c.critic[key])
            torch.testing.assert_close(a.critic[key], b.critic[key], rtol=1e-5, atol=2e-6)
    assert H.F is torch.nn.functional  # the substitution is scoped


@pytest.mark.parametrize("mode", ["soft_e0", "fixed_e32"])
def test_restatement_without_weights_reproduces_the_golden(mode, golden_dir):
    from tests.test_oracle_hirl import batches_for_call, check_probes

    g = np.load(os.path.join(golden_dir, f"hirl_learn_{mode}.npz"))
    params, data = D.make_params(D.PARAM_SEED), D.make_data(D.DATA_SEED)
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"])
    for k in range(g["out"].shape[0]):
        batch, bc = batches_for_call(g, data, k)
        w_in = g["bc_w_in"][k]
        ret, err = W.weighted_learn(o, batch, bc, g["noise"][k], 100 if w_in == 100 else float(w_in), float(g["warm_in"][k]))
        assert err is None
        np.testing.assert_allclose(ret, g["out"][k], rtol=1e-5, atol=1e-6, err_msg=f"{mode} call {k}")
        check_probes(g, k, [(o.actor, H.ACTOR_KEYS), (o.critic, H.CRITIC_KEYS), (o.target_actor, H.ACTOR_KEYS), (o.target_critic, H.CRITIC_KEYS)])


def test_step_rule_on_the_model():
    """mark_new -> draw -> update(idx[:n_main], errors[:n_main]): the drawn slots hold (err + 1e-4)^alpha, a repeated slot the maximum, no other slot
    changes — expert indices (rows [n_main, B)) never reach the store"""
    cap, B, n_main, alpha = 300, 16, 11, 0.6
    m = P.PerModel(cap, alpha=alpha)
    m.mark_new(200)
    m.update(np.arange(0, 200, 7), np.linspace(0.0, 30.0, 29))  # uneven priorities
    before = m.prio.copy()
    u = (np.arange(n_main) + 0.5) / n_main
    u[3] = u[2] + 1e-9  # two targets inside one slot's interval: a repeat
    idx_main = m.draw(u)
    assert len(set(idx_main.tolist())) < n_main and idx_main[2] == idx_main[3]
    assert (before[idx_main] > 0).all() and idx_main.max() < 200
    idx = np.concatenate([idx_main, np.arange(B - n_main) + 1])  # expert indices that WOULD be valid main slots
    errors = np.linspace(0.5, 8.0, B)
    errors[2], errors[3] = 4.0, 0.25
    w = m.weights(idx_main, 0.4, 200)
    assert w.max() == 1.0 and w.min() > 0.0
    m.update(idx[:n_main], errors[:n_main])
    want = before.copy()
    p_new = (errors[:n_main] + P.EPS) ** alpha  # (one vectorised power, as the model forms it)
    for s in set(idx_main.tolist()):
        want[s] = max(p_new[r] for r in range(n_main) if idx_main[r] == s)
    np.testing.assert_array_equal(m.prio, want)
    assert m.prio[idx_main[2]] == p_new[2] > p_new[3]  # the maximum, not the last
    touched = np.zeros(cap, bool)
    touched[idx_main] = True
    assert np.array_equal(m.prio[~touched], before[~touched])
    expert_only = [s for s in idx[n_main:] if not touched[s]]  # live main slots the expert indices name and the draw did not
    assert expert_only and all(before[s] > 0 and m.prio[s] == before[s] for s in expert_only)


HIRL = ["--agent", "HIRL", "--type", "soft", "--synthetic_expert"]


def test_train_all_flag_defaults_and_what_it_goes_with():
    from hirl4ucav_amd import train_all as T

    assert not T.parse_args(HIRL).hirl_per and not T.parse_args(["--agent", "TD3"]).hirl_per
    cfg = T.parse_args(HIRL + ["--hirl_per"])
    assert cfg.hirl_per and not cfg.per and (cfg.per_alpha, cfg.per_beta, cfg.per_beta_annealing) == (0.6, 0.4, 0.0001)
    cfg = T.parse_args(["--agent", "TD3", "--hirl_per", "--per_alpha", "0.7", "--per_beta", "0.5", "--per_beta_annealing", "0.001"])
    assert (cfg.per_alpha, cfg.per_beta, cfg.per_beta_annealing) == (0.7, 0.5, 0.001)
    for argv in (HIRL, ["--agent", "HIRL", "--type", "linear", "--synthetic_expert"], ["--agent", "HIRL", "--type", "fixed", "--synthetic_expert"],
                 ["--agent", "TD3"]):
        hirl = argv[1] == "HIRL"
        for more in [[], ["--dtype", "bf16"], ["--hirl_grad_clip", "1.0"], ["--env", "mixed"], ["--separate_launches"], ["--loop", "reference"],
                     ["--buffer_size", str(1 << 24)]] + ([["--expert_floor", "8"], ["--expert_branch", "96"], ["--expert_online", "128"]] if hirl else []):
            cfg = T.parse_args(argv + more + ["--hirl_per"])
            assert cfg.hirl_per and T.hirl_per_refusal(cfg) is None and T.per_refusal(cfg) is None, (argv, more)
    assert "--hirl_per" in T.parser().format_help()


def test_train_all_refusals(capsys):
    from hirl4ucav_amd import train_all as T

    for argv, word in ((["--agent", "SAC", "--type", "SAC", "--hirl_per"], "has --per"),
                       (["--agent", "SAC", "--type", "ESAC", "--synthetic_expert", "--hirl_per"], "has --per"),
                       (["--agent", "BC", "--synthetic_expert", "--hirl_per"], "not --agent BC"),
                       (HIRL + ["--hirl_per", "--gpus", "2"], "--hirl_per runs on one GPU"),
                       (["--agent", "TD3", "--hirl_per", "--gpus", "8"], "--hirl_per runs on one GPU"),
                       (HIRL + ["--hirl_per", "--buffer_upsample"], "--hirl_per does not go with --buffer_upsample"),
                       (HIRL + ["--hirl_per", "--expert_upsample"], "--hirl_per does not go with --expert_upsample"),
                       (["--agent", "TD3", "--hirl_per", "--buffer_upsample"], "both redraw the same rows"),
                       (HIRL + ["--hirl_per", "--buffer_size", str((1 << 24) + 1)], "at most 2^24"),
                       (HIRL + ["--hirl_per", "--per_new", "td"], "--per_new td goes with --per"),
                       (HIRL + ["--per"], "goes with --agent SAC"),                  # SacAgent's keyword stays SAC's, in its old words
                       (["--agent", "TD3", "--per"], "--per goes with --agent SAC --type SAC (prioritized replay is SacAgent's: SAC/agent.py:112-118), not --agent TD3"),
                       (HIRL + ["--per", "--hirl_per"], "goes with --agent SAC")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert word in " ".join(capsys.readouterr().err.split()), argv
    ns = types.SimpleNamespace
    assert T.hirl_per_refusal(ns(agent="HIRL", hirl_per=True, gpus=1, buffer_size=100), world=2) == (
        "--hirl_per runs on one GPU (priorities and block sums are not exchanged between ranks): use --gpus 1")
    assert T.hirl_per_refusal(ns(agent="HIRL", hirl_per=False, gpus=8, buffer_size=1 << 30)) is None  # (without the flag nothing is its business)
    assert T.hirl_per_refusal(ns(agent="SAC", gpus=1)) is None
    # --per's own results are what they were
    assert T.per_refusal(ns(agent="HIRL", per=True, type="soft", gpus=1)) == (
        "--per goes with --agent SAC --type SAC (prioritized replay is SacAgent's: SAC/agent.py:112-118), not --agent HIRL")
    assert T.per_refusal(ns(agent="HIRL", per=False, hirl_per=True, type="soft", gpus=1)) is None


def test_resume_refuses_the_other_setting_by_name():
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils import checkpoint as CK

    ns = types.SimpleNamespace
    with_, without = {"engine": {"prioritized": True}}, {"engine": {}}
    assert T.hirl_per_resume_refusal(ns(agent="HIRL", hirl_per=True), None) is None
    assert T.hirl_per_resume_refusal(ns(agent="HIRL", hirl_per=True), with_) is None and T.hirl_per_resume_refusal(ns(agent="TD3", hirl_per=False), without) is None
    assert "was run without --hirl_per" in T.hirl_per_resume_refusal(ns(agent="HIRL", hirl_per=True), without)
    assert "was run with --hirl_per" in T.hirl_per_resume_refusal(ns(agent="TD3", hirl_per=False), with_)
    assert T.hirl_per_resume_refusal(ns(agent="SAC", hirl_per=False), with_) is None  # (SAC's --per: utils/checkpoint.py's own check)

    def fake(prioritized):
        return ns(per_flag="--hirl_per", arena=torch.arange(8, dtype=torch.float32), critic_step=4, actor_step=2, update_count=2, actor_trainable=True,
                  sample_calls=4, act_calls=9, grad_clip=None, prioritized=object() if prioritized else None, per_calls=7 if prioritized else 0)

    plain = CK.engine_state(fake(False))
    assert "prioritized" not in plain and "per_calls" not in plain  # a snapshot of a run without the flag stays what it was
    st = CK.engine_state(fake(True))
    assert st["prioritized"] is True and st["per_calls"] == 7
    e = fake(True)
    e.per_calls = 0
    CK.load_engine_state(e, st)
    assert e.per_calls == 7 and e.critic_step == 4
    for eng, snap in ((fake(False), st), (fake(True), plain)):
        with pytest.raises(ValueError, match="--hirl_per"):
            CK.load_engine_state(eng, snap)
    sac_like = ns(arena=torch.arange(8, dtype=torch.float32), prioritized=None, grad_clip=None)
    with pytest.raises(ValueError, match=r"\(--per\)"):  # SacEngine's message keeps its flag
        CK.load_engine_state(sac_like, {"arena": torch.arange(8, dtype=torch.float32), "prioritized": True, "counters": {}})


def _run(agent, hirl_per, loop="front", separate=False, grad_clip=None):
    cfg = types.SimpleNamespace(loop=loop, separate_launches=separate, updates_per_step=1, dtype="f32", log_rewards=False, status_check_every=0,
                                resume=None, on_front_trip="exit", snapshot_every=0)
    return types.SimpleNamespace(config=cfg, world=1, rank=0, sac=agent == "SAC", n=8, device=torch.device("cpu"), batch=128, per=hirl_per or agent == "SAC",
                                 hirl_per=hirl_per, grad_clip=grad_clip, inserter=None, buffer_upsample=False, expert_upsample=False, episode0=0)


def test_loop_line(capsys, monkeypatch):
    """under --hirl_per the loop takes the reference's order whatever --loop says and names the reason; without the flag the line is the parent's"""
    from hirl4ucav_amd import train_all as T

    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    reason = "(--hirl_per: the front launch draws before the step's insert, so the priorities of the drawn rows could be written into overwritten slots)"
    for agent in ("HIRL", "TD3"):
        for kw in ({}, {"loop": "reference"}, {"separate": True}):
            run = _run(agent, True, **kw)
            T.choose_loop(run)
            line = capsys.readouterr().out
            assert not run.front and not run.front_sac and line.strip() == "vector loop: reference order " + reason, line
    run = _run("HIRL", True, grad_clip=0.5)
    T.choose_loop(run)
    line = capsys.readouterr().out
    assert not run.front and reason in line and "--hirl_grad_clip 0.5: the clipped update runs as stages, a norm launch" in line and "behind the front" not in line
    run = _run("HIRL", False)
    T.choose_loop(run)
    assert run.front and capsys.readouterr().out.strip() == "vector loop: front launch (env step + first launches of learn() in one launch; draw before the insert)"
    run = _run("SAC", False)  # SAC's --per keeps its words
    T.choose_loop(run)
    assert "(--per: the front launch draws before the step's insert" in capsys.readouterr().out and not run.front_sac


def test_header_declares_the_entry_point_and_the_binding_reads_it():
    import ctypes

    from hirl4ucav_amd import _abi

    hdr = open(os.path.join(ROOT, "include", "hirl4ucav.h")).read()
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 131 and "131: prioritized replay for HIRL and TD3" in hdr
    assert "Prioritized replay for HIRL / TD3" in hdr and "the actor half" in hdr
    f = _abi.abi().functions
    nets, batch, hyper = (ctypes.POINTER(_abi.abi().structs[k]) for k in ("HxNets", "HxBatch", "HxHyper"))
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert f["hx_hirl_critic_grads_weighted"] == (ctypes.c_int, [nets, batch, hyper, vp, i32, vp, i32, vp])
    mk = open(os.path.join(ROOT, "hirl4ucav_amd", "csrc", "Makefile")).read()
    assert "hx_hirl_per.o" in mk and "hx_hirl_per" not in re.sub(r"^OBJS.*$", "", mk, flags=re.M)  # built by the generic rule: hx_sac.hip's flags
    assert os.path.exists(os.path.join(ROOT, "tools", "asan_hirl_per_host.cpp"))
