"""CPU tests of prioritized replay for SAC: the weighted-learn checker (tests/_per_check.py) PINNED against golden vectors recorded from the
reference's SacAgent(per=True).learn (tests/golden/gen_sac_per_golden.py), the numpy model of the priority store against itself, and the driver's
refusals.  The bars are those of tests/test_oracle_sac.py for the plain update; the errors handed to update_priority are held to the same bar."""
import os

import numpy as np
import pytest
import torch

from oracle import sac_oracle as S
from tests import _hirl_data as D
from tests import _per_check as P
from tests.test_oracle_sac import sac_params

torch.set_num_threads(1)


def test_weighted_learn_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "sac_per_learn.npz"))
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"]) and D.checksum(data) == str(g["data_checksum"])
    assert g["out"].shape == (6, 6) and g["weights"].shape == (6, 128) and g["errors"].shape == (6, 128)
    assert np.all(g["weights"] > 0) and np.all(g["weights"] <= 1) and np.all(g["weights"].max(1) == 1.0)
    o = P.WeightedSacOracle(params["policy"], params["q1"], params["q2"])
    for k in range(6):
        rows = data["replay"][g["idx"][k]]
        out, err = o.learn((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), g["eps"][k, 0], g["eps"][k, 1], g["weights"][k])
        np.testing.assert_allclose(out, g["out"][k], rtol=1e-5, atol=1e-6, err_msg=f"per call {k}")
        np.testing.assert_allclose(err, g["errors"][k], rtol=1e-5, atol=1e-6, err_msg=f"per call {k} errors")
        for j, net in enumerate((o.policy, o.q1, o.q2, o.q1_t, o.q2_t)):
            s, a, v = D.net_probe(S.flatten(net))
            np.testing.assert_allclose(v, g["probe_val"][k][j], rtol=1e-5, atol=2e-6, err_msg=f"call {k} net {j}")
            np.testing.assert_allclose(a, g["probe_abs"][k][j], rtol=1e-6)
    assert o.learning_steps == 6  # targets moved at calls 3 and 6 (before the update)


def test_unit_weights_are_the_plain_update():
    """weights == 1 in the checker is SacOracle.learn, bit for bit (same formulas: x * 1 == x)"""
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    a, b = S.SacOracle(params["policy"], params["q1"], params["q2"]), P.WeightedSacOracle(params["policy"], params["q1"], params["q2"])
    rng = np.random.default_rng(2)
    for k in range(3):
        rows = data["replay"][rng.choice(D.N_REPLAY, 48, replace=False)]
        e1, e2 = rng.normal(size=(2, 48, 4)).astype(np.float32)
        batch = (rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31])
        ref = a.learn(batch, e1, e2)
        got, err = b.learn(batch, e1, e2, np.ones(48, np.float32))
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7)
        assert err.shape == (48,) and np.all(err >= 0)
    for key in S.MLP_KEYS:
        np.testing.assert_allclose(b.policy[key].detach().numpy(), a.policy[key].detach().numpy(), rtol=1e-6, atol=1e-8)


def test_store_model_draw_weights_and_duplicates():
    m = P.PerModel(2500, alpha=0.6)
    pr = np.zeros(2500)
    pr[:1000], pr[1000:1024], pr[2048:2300] = 2.0, 0.0, 1.0  # a run of zeros, a whole empty block in the middle, zeros at the tail
    m.set(np.arange(2500), pr)
    S_ = pr.sum()
    k = np.array([0, 1, 2, 1999, 2000, 2001, S_ - 1])
    np.testing.assert_array_equal(m.draw((k + 0.5) / S_), [0, 0, 1, 999, 2048, 2049, 2299])
    assert m.draw([0.0])[0] == 0 and m.draw([1.0])[0] == 2299  # a target AT S: the last slot that holds priority
    w = m.weights([0, 2048], 0.4, 2300)
    assert w.max() == 1.0 and w[1] == 1.0 and np.isclose(w[0], 2.0 ** -0.4)
    m.update([5, 5, 5, 7], [0.1, 3.0, 0.5, 0.0])
    assert np.isclose(m.prio[5], (3.0 + 1e-4) ** 0.6) and np.isclose(m.prio[7], 1e-4 ** 0.6) and m.pmax == max(2.0, (3.0 + 1e-4) ** 0.6)
    np.testing.assert_allclose(m.bsum().sum(), m.prio.sum())
    m2 = P.PerModel(100)
    m2.mark_new(30)
    assert (m2.prio[:30] == 1.0).all() and (m2.prio[30:] == 0).all() and m2.marked == 30
    m2.mark_new(250)  # more than cap rows between marks: the whole ring
    assert (m2.prio == 1.0).all() and m2.marked == 250


@pytest.mark.parametrize("extra,reason", [(["--agent", "SAC", "--type", "ESAC"], "drops the expert rows"),
                                          (["--agent", "SAC", "--type", "ISAC", "--bc_actor", "x", "--synthetic_expert"], "imitative branch is not built"),
                                          (["--agent", "HIRL"], "goes with --agent SAC"),
                                          (["--agent", "SAC", "--type", "SAC", "--dtype", "bf16"], "fp32 only"),
                                          (["--agent", "SAC", "--type", "SAC", "--gpus", "2"], "one GPU")])
def test_parse_args_refuses_per_where_it_is_not_built(extra, reason, capsys):
    from hirl4ucav_amd import train_all as T

    with pytest.raises(SystemExit):
        T.parse_args(["--per"] + extra)
    err = capsys.readouterr().err
    assert "--per" in err and reason in err, err


def test_parse_args_takes_per_with_its_defaults():
    from hirl4ucav_amd import train_all as T

    cfg = T.parse_args(["--agent", "SAC", "--type", "SAC", "--per"])
    assert cfg.per and (cfg.per_alpha, cfg.per_beta, cfg.per_beta_annealing) == (0.6, 0.4, 0.0001)
    assert T.per_refusal(cfg) is None and T.per_refusal(T.parse_args(["--agent", "SAC", "--type", "SAC"])) is None
    assert not T.parse_args(["--agent", "SAC", "--type", "SAC"]).per


def test_sac_agent_takes_per_but_not_with_the_imitative_branch(tmp_path):
    """(needs no GPU: the check precedes the engine)"""
    import types

    from hirl4ucav_amd.agents.SAC.agent import SacAgent

    box = lambda n: types.SimpleNamespace(shape=(n,))  # noqa: E731
    with pytest.raises(NotImplementedError, match="per with imitative"):
        SacAgent(box(13), box(4), str(tmp_path), hidden_units=[256, 512], imitative=True, per=True)


def test_uniform_memory_still_refuses_upsampling():
    from hirl4ucav_amd.utils.buffer import UniformMemory

    with pytest.raises(NotImplementedError):
        UniformMemory(100, upsample=True)
