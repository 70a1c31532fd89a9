"""CPU tests of gradient-norm clipping and the fixed entropy coefficient for SAC: tests/_sac_clip.py (the restated clip and fixed alpha over the SAC
oracle) PINNED against golden vectors recorded from the reference's own SacAgent(grad_clip=c).learn and SacAgent(entropy_tuning=False).learn
(tests/golden/sac_clip_learn.npz, tests/golden/gen_sac_clip_golden.py); train_all's flags and refusals; the snapshot's two new fields."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import sac_oracle as S
from tests import _hirl_data as D
from tests import _sac_clip as C
from tests.test_oracle_sac import sac_params

torch.set_num_threads(1)


def _replay(o, g, data, pre="", learn=None):
    """the golden's six calls on the oracle `o`, held to the bars tests/test_oracle_sac.py uses for sac_learn.npz"""
    for k in range(g[pre + "out"].shape[0]):
        rows = data["replay"][g[pre + "idx"][k]]
        out = (learn or o.learn)((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), g[pre + "eps"][k, 0], g[pre + "eps"][k, 1])
        np.testing.assert_allclose(out, g[pre + "out"][k], rtol=1e-5, atol=1e-6, err_msg=f"{pre}call {k}")
        for j, net in enumerate((o.policy, o.q1, o.q2, o.q1_t, o.q2_t)):
            s, a, v = D.net_probe(S.flatten(net))
            np.testing.assert_allclose(v, g[pre + "probe_val"][k][j], rtol=1e-5, atol=2e-6, err_msg=f"{pre}call {k} net {j}")
            np.testing.assert_allclose(a, g[pre + "probe_abs"][k][j], rtol=1e-6)
        yield k


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "sac_clip_learn.npz"))
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"]) and D.checksum(data) == str(g["data_checksum"])
    return g, params, data


@pytest.mark.parametrize("reference_passes", [False, True], ids=["single_clip", "reference_passes"])
def test_clipped_oracle_matches_reference(golden_dir, reference_passes):
    """The single whole-network clip this project builds, and the reference's repeated passes (update_params loops over network.modules()), both replay the
    reference's recorded run inside the unclipped golden's bars; the norms before clipping are the ones the reference's first pass found."""
    g, params, data = _golden(golden_dir)
    c = float(g["grad_clip"])
    assert ((g["norms"] > c).sum(0) >= 4).all()  # the golden is worth something: every network clips on at least four of the six calls
    o = C.install_clip(S.SacOracle(params["policy"], params["q1"], params["q2"]), c, reference_passes=reference_passes)
    for k in _replay(o, g, data):
        got = [o.last_norms[n] for n in ("q1", "q2", "policy")]
        np.testing.assert_allclose(got, g["norms"][k], rtol=2e-5, err_msg=f"call {k} norms")
        for n, norm in zip(("q1", "q2", "policy"), got):
            assert abs(o.last_coefs[n] - min(1.0, c / (norm + 1e-6))) < 1e-6 and (o.last_coefs[n] == 1.0) == (norm + 1e-6 <= c)


def test_single_clip_departure_from_the_reference_is_measured(golden_dir):
    """DESIGN.md 5's figure: the reference clips the whole network, then the inner Sequential (the same parameters again), then every Linear.  After the
    first clip the norm is max_norm norm / (norm + 1e-6), so the second pass scales by a factor within 1e-6 / max_norm of 1 and the per-Linear passes
    (whose norms are below the network's) by exactly 1.  Both orders run the golden's six calls; the parameters they end with differ by less than the
    bar the golden itself is replayed with (atol 2e-6) — printed, and asserted at a tenth of it."""
    g, params, data = _golden(golden_dir)
    c = float(g["grad_clip"])
    a = C.install_clip(S.SacOracle(params["policy"], params["q1"], params["q2"]), c)
    b = C.install_clip(S.SacOracle(params["policy"], params["q1"], params["q2"]), c, reference_passes=True)
    worst_factor = 0.0
    for k in range(g["out"].shape[0]):
        rows = data["replay"][g["idx"][k]]
        batch = (rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31])
        a.learn(batch, g["eps"][k, 0], g["eps"][k, 1])
        b.learn(batch, g["eps"][k, 0], g["eps"][k, 1])
        for n in ("q1", "q2", "policy"):  # the second pass's factor on the reference's side, from the golden's own norm
            norm = g["norms"][k][{"q1": 0, "q2": 1, "policy": 2}[n]]
            after = min(norm, c * norm / (norm + 1e-6))
            worst_factor = max(worst_factor, 1.0 - min(1.0, c / (after + 1e-6)))
    d = max(float(np.abs(S.flatten(x) - S.flatten(y)).max()) for x, y in ((a.policy, b.policy), (a.q1, b.q1), (a.q2, b.q2)))
    print(f"single clip vs the reference's passes after 6 calls: max |dparam| {d:.3e}; the second pass's factor is within {worst_factor:.3e} of 1 "
          f"(1e-6 / max_norm = {1e-6 / c:.3e})")
    assert worst_factor <= 1e-6 / c * 1.0001
    assert d <= 2e-7


def test_fixed_alpha_oracle_matches_reference(golden_dir):
    g, params, data = _golden(golden_dir)
    x = float(g["ent_coef"])
    o = C.install_fixed_alpha(S.SacOracle(params["policy"], params["q1"], params["q2"]), x)
    for k in _replay(o, g, data, pre="fixed_", learn=lambda *a: C.fixed_learn(o, *a)):
        assert o.log_alpha.item() == 0.0 and o.opt_alpha.t == 0  # the log-alpha state is never touched
    assert np.all(g["fixed_out"][:, 3] == 0.0) and np.all(g["fixed_out"][:, 5] == np.float32(x))


def test_train_all_flags_and_refusals(capsys):
    from hirl4ucav_amd import train_all as T

    cfg = T.parse_args(["--agent", "SAC", "--type", "SAC", "--grad_clip", "1.0"])
    assert cfg.grad_clip == 1.0 and cfg.fixed_alpha is None and T.clip_refusal(cfg) is None
    cfg = T.parse_args(["--agent", "SAC", "--type", "ESAC", "--fixed_alpha", "0.2", "--synthetic_expert"])
    assert cfg.fixed_alpha == 0.2 and cfg.grad_clip is None and T.clip_refusal(cfg) is None
    plain = T.parse_args(["--agent", "SAC", "--type", "SAC"])
    assert plain.grad_clip is None and plain.fixed_alpha is None and T.clip_refusal(plain) is None
    assert T.clip_refusal(T.parse_args(["--agent", "SAC", "--type", "SAC", "--fixed_alpha", "0.2", "--gpus", "2"])) is None  # fixed alpha shards
    for argv, word in ((["--agent", "HIRL", "--grad_clip", "1.0"], "--agent SAC"), (["--agent", "TD3", "--fixed_alpha", "0.2"], "--agent SAC"),
                       (["--agent", "SAC", "--type", "SAC", "--grad_clip", "0"], "positive"),
                       (["--agent", "SAC", "--type", "SAC", "--grad_clip", "nan"], "positive"),
                       (["--agent", "SAC", "--type", "SAC", "--fixed_alpha", "-0.1"], ">= 0"),
                       (["--agent", "SAC", "--type", "SAC", "--grad_clip", "1.0", "--gpus", "2"], "--gpus 1")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    cfg = T.parse_args(["--agent", "SAC", "--type", "SAC", "--grad_clip", "1.0"])
    assert "--gpus 1" in T.clip_refusal(cfg, world=2)  # a launcher's world size counts as --gpus does


def _fake_engine(grad_clip=None, ent_coef=None):
    return types.SimpleNamespace(arena=torch.arange(8, dtype=torch.float32), learning_steps=3, grad_clip=grad_clip, entropy_tuning=ent_coef is None,
                                 ent_coef=ent_coef)


def test_snapshot_carries_clip_and_entropy_mode_and_refuses_another():
    from hirl4ucav_amd.utils import checkpoint as CK

    plain = CK.engine_state(_fake_engine())
    assert "grad_clip" not in plain and "fixed_alpha" not in plain  # a plain snapshot stays what it was
    st = CK.engine_state(_fake_engine(grad_clip=1.5, ent_coef=0.2))
    assert st["grad_clip"] == 1.5 and st["fixed_alpha"] == 0.2
    e = _fake_engine(grad_clip=1.5, ent_coef=0.2)
    e.arena.zero_()
    e.learning_steps = 0
    CK.load_engine_state(e, st)  # round trip
    assert torch.equal(e.arena, torch.arange(8, dtype=torch.float32)) and e.learning_steps == 3
    for other, word in ((_fake_engine(grad_clip=2.0, ent_coef=0.2), "--grad_clip"), (_fake_engine(ent_coef=0.2), "--grad_clip"),
                        (_fake_engine(grad_clip=1.5), "--fixed_alpha"), (_fake_engine(grad_clip=1.5, ent_coef=0.3), "--fixed_alpha")):
        with pytest.raises(ValueError, match=word):
            CK.load_engine_state(other, st)
    with pytest.raises(ValueError, match="--grad_clip"):
        CK.load_engine_state(_fake_engine(grad_clip=1.0), plain)
    with pytest.raises(ValueError, match="--fixed_alpha"):
        CK.load_engine_state(_fake_engine(ent_coef=0.2), plain)
