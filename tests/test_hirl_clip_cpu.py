"""--hirl_grad_clip for HIRL and TD3 (train_all's name for HirlEngine.set_grad_clip; --grad_clip stays SacAgent's keyword and stays refused for them), the parts that need no GPU: the clip rule of tests/_hirl_clip against torch.nn.utils.clip_grad_norm_ itself on modules
of HIRL's shapes (LayerNorm included), the oracle's two optimisers behind it, train_all's flags, refusals and loop line, the snapshot rule, the façade's
keyword, the header's entry points."""
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_clip as C  # noqa: E402
from tests import _hirl_data as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Block(torch.nn.Module):
    """one MLP block of HIRL.py's shapes: Linear, LayerNorm, Linear, LayerNorm, Linear"""

    def __init__(self, i, o):
        super().__init__()
        self.full1, self.layernorm1 = torch.nn.Linear(i, 256), torch.nn.LayerNorm(256)
        self.full2, self.layernorm2 = torch.nn.Linear(256, 512), torch.nn.LayerNorm(512)
        self.final = torch.nn.Linear(512, o)


class Critic(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q1, self.q2 = Block(17, 1), Block(17, 1)


@pytest.mark.parametrize("net", ["actor", "critic"])
@pytest.mark.parametrize("scale,max_norm", [(1e-3, 1.0), (1.0, 1.0), (30.0, 0.5), (1.0, 1e30)])
def test_clip_once_is_clip_grad_norm_over_the_optimizers_parameters(net, scale, max_norm):
    """clip_once over every tensor of a gradient dict == torch.nn.utils.clip_grad_norm_(module.parameters(), max_norm): the total norm it returns and the
    gradients it leaves, bit for bit — both Q heads and every LayerNorm parameter under ONE norm for the critic"""
    torch.manual_seed(3)
    m = Block(13, 4) if net == "actor" else Critic()
    g = {}
    for name, p in m.named_parameters():
        p.grad = torch.randn_like(p) * scale * (10.0 if "layernorm" in name else 1.0)
        g[name] = p.grad.clone()
    assert sum(1 for k in g if "layernorm" in k) == (4 if net == "actor" else 8)
    total = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)
    norm, coef = C.clip_once(g, max_norm)
    assert norm == total.item() and (coef < 1.0) == (norm + 1e-6 > max_norm)
    for name, p in m.named_parameters():
        assert torch.equal(p.grad, g[name]), name
    without = {k: v for k, v in g.items() if "layernorm" not in k}
    assert C.total_norm(without).item() < C.total_norm(g).item()  # the LayerNorm parameters count


def _oracle(use_bc=True):
    params = D.make_params(5)
    return H.HirlOracle(params["actor"], params["critic"], params["bc_actor"] if use_bc else None, slope=0.0 if use_bc else 0.01, use_bc=use_bc)


def _call(o, data, rng, B, use_bc=True):
    idx, ibc = rng.integers(0, D.N_REPLAY, B), rng.integers(0, D.N_EXPERT, B)
    rows = data["replay"][idx]
    ob = (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31])
    return o.learn(ob, (data["expert_s"][ibc], data["expert_a"][ibc]) if use_bc else None, rng.normal(0, 0.2, 4).astype(np.float32), *((100, 0.05) if use_bc else ()))


@pytest.mark.parametrize("use_bc", [True, False], ids=["hirl", "td3"])
def test_oracle_behind_the_clip(use_bc):
    """HirlOracle.opt_critic / opt_actor behind ClippedAdam: a clip that never binds leaves the unclipped oracle's bits; one that binds scales the
    gradient Adam sees (first step from zero moments: m = (1 - b1) coef g exactly) and records norm and coefficient of each optimizer; last_grads
    stays unclipped; copy.deepcopy (tests/test_hirl_gpu.oracle_checked) carries the clip along"""
    import copy

    data = D.make_data(6, outliers=True)
    plain, loose, tight = _oracle(use_bc), C.install_clip(_oracle(use_bc), 1e30), C.install_clip(_oracle(use_bc), 1e-3)
    outs = [_call(o, data, np.random.default_rng(1), 16, use_bc) for o in (plain, loose, tight)]
    assert outs[0] == outs[1]
    for k in plain.critic:
        assert torch.equal(plain.critic[k], loose.critic[k]) and torch.equal(plain.opt_critic.m[k], loose.opt_critic.m[k])
    for k in plain.actor:
        assert torch.equal(plain.actor[k], loose.actor[k])
    assert loose.last_coefs == {"critic": 1.0, "actor": 1.0}
    for name, opt in (("critic", tight.opt_critic), ("actor", tight.opt_actor)):
        g = tight.last_grads[name]
        norm = C.total_norm(g).item()
        assert tight.last_norms[name] == norm and norm > 1e-3 and tight.last_coefs[name] == pytest.approx(1e-3 / (norm + 1e-6), rel=1e-6)
        for k in g:
            torch.testing.assert_close(opt.m[k], g[k] * tight.last_coefs[name] * 0.1, rtol=1e-5, atol=0)
        assert any("layernorm" in k for k in g)
    twin = copy.deepcopy(tight)
    twin.clip["max_norm"] = 7.0
    assert tight.clip["max_norm"] == 1e-3 and twin.opt_critic.cfg is twin.clip and twin.opt_actor.log["norms"] is twin.last_norms


HIRL = ["--agent", "HIRL", "--type", "soft", "--synthetic_expert"]


def test_train_all_flags_and_refusals(capsys):
    from hirl4ucav_amd import train_all as T

    assert T.parse_args(HIRL).hirl_grad_clip is None and T.parse_args(["--agent", "TD3"]).hirl_grad_clip is None  # the default: no clip
    for argv in (HIRL, ["--agent", "HIRL", "--type", "linear", "--synthetic_expert"], ["--agent", "HIRL", "--type", "fixed", "--synthetic_expert"],
                 ["--agent", "TD3"]):
        for more in ([], ["--loop", "reference"], ["--separate_launches"], ["--dtype", "bf16"], ["--dtype", "f32x9"], ["--gpus", "8"],
                     ["--env", "mixed"], ["--buffer_upsample"]):
            cfg = T.parse_args(argv + more + ["--hirl_grad_clip", "2.5"])
            assert cfg.hirl_grad_clip == 2.5 and cfg.grad_clip is None and T.hirl_clip_refusal(cfg) is None and T.hirl_clip_refusal(cfg, world=8) is None, (argv, more)
    for argv, word in ((["--agent", "BC", "--hirl_grad_clip", "1.0"], "not --agent BC"), (["--agent", "BC", "--hirl_grad_clip", "1.0"], "ONE fused call"),
                       (HIRL + ["--hirl_grad_clip", "0"], "positive"), (HIRL + ["--hirl_grad_clip", "-1"], "positive"),
                       (HIRL + ["--hirl_grad_clip", "nan"], "positive"), (["--agent", "TD3", "--hirl_grad_clip", "inf"], "positive"),
                       (["--agent", "SAC", "--type", "SAC", "--hirl_grad_clip", "1.0"], "SAC clips with --grad_clip C"),
                       (HIRL + ["--grad_clip", "1.0"], "--grad_clip goes with --agent SAC"),  # SacAgent's keyword stays SAC's; the refusal names the other flag
                       (HIRL + ["--grad_clip", "1.0"], "HIRL and TD3 clip with --hirl_grad_clip C"),
                       (["--agent", "TD3", "--grad_clip", "1.0"], "--hirl_grad_clip C"),
                       (HIRL + ["--fixed_alpha", "0.2"], "--fixed_alpha goes with --agent SAC")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert word in " ".join(capsys.readouterr().err.split()), argv
    assert "--hirl_grad_clip C" in T.parser().format_help() and "HIRL / TD3" in " ".join(T.parser().format_help().split())


def test_sac_refusals_word_for_word(capsys):
    """SAC's own rules and words are what they were: one GPU, positive, and the two flags' refusal for agents they do not go with"""
    from hirl4ucav_amd import train_all as T

    sac = ["--agent", "SAC", "--type", "SAC"]
    cfg = T.parse_args(sac + ["--grad_clip", "1.0"])
    assert T.clip_refusal(cfg) is None
    assert T.clip_refusal(cfg, world=2) == "--grad_clip runs on one GPU (the norm is taken over one rank's gradient, before any exchange): use --gpus 1"
    ns = types.SimpleNamespace
    assert T.clip_refusal(ns(agent="SAC", grad_clip=0.0, fixed_alpha=None, gpus=1)) == "--grad_clip 0.0: the maximum gradient norm is a positive number"
    assert T.clip_refusal(ns(agent="SAC", grad_clip=None, fixed_alpha=-0.1, gpus=1)) == "--fixed_alpha -0.1: the entropy coefficient is a number >= 0"
    assert T.clip_refusal(ns(agent="SAC", grad_clip=1.0, fixed_alpha=None, gpus=2)) == T.clip_refusal(cfg, world=2)
    assert T.clip_refusal(ns(agent="TD3", grad_clip=None, fixed_alpha=0.2, gpus=1)) == (
        "--fixed_alpha goes with --agent SAC (gradient clipping and the fixed entropy coefficient are SacAgent's: SAC/agent.py:108-110, 310-320), "
        "not --agent TD3")
    assert T.clip_refusal(ns(agent="BC", grad_clip=1.0, fixed_alpha=None, gpus=1)) == (
        "--grad_clip goes with --agent SAC (gradient clipping and the fixed entropy coefficient are SacAgent's: SAC/agent.py:108-110, 310-320), "
        "not --agent BC")
    assert T.clip_refusal(ns(agent="HIRL", grad_clip=None, fixed_alpha=None, gpus=8)) is None
    assert T.clip_refusal(ns(agent="HIRL", grad_clip=None, fixed_alpha=None, hirl_grad_clip=1.0, gpus=8)) is None  # (the other flag is not its business)
    assert T.hirl_clip_refusal(cfg) is None and T.hirl_clip_refusal(ns(agent="HIRL", gpus=8)) is None


def _run(agent, grad_clip, loop="front", separate=False, world=1, batch=128, dtype="f32"):
    cfg = types.SimpleNamespace(loop=loop, separate_launches=separate, updates_per_step=1, dtype=dtype, log_rewards=False, status_check_every=0,
                                resume=None, on_front_trip="exit", snapshot_every=0)
    return types.SimpleNamespace(config=cfg, world=world, rank=0, sac=agent == "SAC", n=8, device=torch.device("cpu"), batch=batch, per=False,
                                 grad_clip=grad_clip, inserter=None, buffer_upsample=False, expert_upsample=False, episode0=0)


def test_loop_line(capsys, monkeypatch):
    """a clipped HIRL / TD3 run keeps the front loop and says that the clipped update runs as stages behind it; unclipped, the line is the parent's"""
    from hirl4ucav_amd import train_all as T

    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)  # (one process on one GPU: what choose_loop asks before it takes the front loop)

    run = _run("HIRL", 1.5)
    T.choose_loop(run)
    line = capsys.readouterr().out
    assert run.front and "vector loop: front launch" in line and "--hirl_grad_clip 1.5: the clipped update runs as stages behind the front launch" in line
    run = _run("TD3", 0.25, loop="reference")
    T.choose_loop(run)
    line = capsys.readouterr().out
    assert not run.front and "vector loop: reference order (--hirl_grad_clip 0.25: the clipped update runs as stages, a norm launch" in line
    run = _run("HIRL", 1.0, separate=True)
    T.choose_loop(run)
    assert not run.front and "reference order (--hirl_grad_clip 1" in capsys.readouterr().out
    run = _run("HIRL", None)
    T.choose_loop(run)
    line = capsys.readouterr().out
    assert run.front and line.strip() == "vector loop: front launch (env step + first launches of learn() in one launch; draw before the insert)"
    run = _run("SAC", 1.0)
    T.choose_loop(run)
    assert "(--grad_clip: the clipped update runs as stages, which have no front form)" in capsys.readouterr().out and not run.front_sac


def _fake_engine(grad_clip=None):
    return types.SimpleNamespace(grad_clip_flag="--hirl_grad_clip", arena=torch.arange(8, dtype=torch.float32), critic_step=4, actor_step=2, update_count=2, actor_trainable=True, sample_calls=4,
                                 act_calls=9, grad_clip=grad_clip)


def test_snapshot_carries_the_clip_and_resume_refuses_another():
    from hirl4ucav_amd.utils import checkpoint as CK

    plain = CK.engine_state(_fake_engine())
    assert "grad_clip" not in plain  # an unclipped snapshot stays what it was
    st = CK.engine_state(_fake_engine(grad_clip=1.5))
    assert st["grad_clip"] == 1.5
    e = _fake_engine(grad_clip=1.5)
    e.arena.zero_()
    e.critic_step = 0
    CK.load_engine_state(e, st)
    assert torch.equal(e.arena, torch.arange(8, dtype=torch.float32)) and e.critic_step == 4
    for eng, snap in ((_fake_engine(grad_clip=2.0), st), (_fake_engine(), st), (_fake_engine(grad_clip=1.5), plain)):
        with pytest.raises(ValueError, match="--hirl_grad_clip"):
            CK.load_engine_state(eng, snap)


def test_header_declares_the_entry_points_and_the_binding_reads_them():
    import ctypes

    from hirl4ucav_amd import _abi

    hdr = open(os.path.join(ROOT, "include", "hirl4ucav.h")).read()
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 130 and "130: gradient-norm clipping for HIRL and TD3" in hdr
    f = _abi.abi().functions
    nets, hyper = (ctypes.POINTER(_abi.abi().structs[k]) for k in ("HxNets", "HxHyper"))
    i32, f32, vp = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
    assert f["hx_hirl_clip_floats"] == (ctypes.c_int64, []) and f["hx_hirl_clip_shape"] == (ctypes.c_int, [vp])
    assert f["hx_hirl_grad_norm"] == (ctypes.c_int, [nets, hyper, i32, i32, f32, f32, i32, vp, vp, vp])
    assert f["hx_adam_clipped"] == (ctypes.c_int, [nets, hyper, i32, i32, f32, i32, f32, f32, i32, vp, f32, vp, vp])
    mk = open(os.path.join(ROOT, "hirl4ucav_amd", "csrc", "Makefile")).read()
    assert "hx_hirl_clip.o" in mk and "hx_hirl_clip" not in re.sub(r"^OBJS.*$", "", mk, flags=re.M)  # built by the generic rule: hx_clip.hip's flags


def test_facade_keyword_is_trailing_and_optional():
    import inspect

    from hirl4ucav_amd.agents import HIRL, TD3

    for mod in (HIRL, TD3):
        p = list(inspect.signature(mod.Agent.__init__).parameters.values())[-1]
        assert p.name == "grad_clip" and p.default is None
