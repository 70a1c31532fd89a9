"""CPU tests of the imitative SAC branch: the restatement tests/_isac_check.py PINNED against golden vectors recorded from the reference's
SacAgent.learn(imitative=True) (tests/golden/gen_isac_golden.py), and the host logic of the driver and the façade that needs no GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import sac_oracle as S
from tests import _hirl_data as D
from tests import _isac_check as C

torch.set_num_threads(1)


def expert_batch(data, idx):
    er = data["expert_rows"][idx]
    return er[:, 0:13], er[:, 13:17]


def test_isac_restatement_matches_reference(golden_dir):
    """the tolerances tests/test_oracle_sac.py applies to sac_learn.npz (rtol 1e-5, atol 1e-6; probes as there); bc_loss is O(10^3) and the
    combined policy loss inherits that scale: relative tolerance only for these two; bc_weight * 128 is an integer and equals the golden's"""
    g = np.load(os.path.join(golden_dir, "isac_learn.npz"))
    params, data = C.isac_params(int(g["seed"])), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"]) and D.checksum(data) == str(g["data_checksum"])
    w = g["out"][:, 7]
    assert ((w > 0) & (w < 1)).sum() >= 6 and len(set(np.round(w * 128).astype(int))) >= 4 and float(g["min_rel_gap"]) >= 1e-4  # the fixture's own conditions
    o = C.IsacCheck(params["policy"], params["q1"], params["q2"], params["bc_actor"])
    for k in range(g["out"].shape[0]):
        rows = data["replay"][g["idx"][k]]
        out = o.learn((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), g["eps"][k, 0], g["eps"][k, 1],
                      expert_batch(data, g["idx_expert"][k]))
        ref = g["out"][k]
        np.testing.assert_allclose(np.asarray(out)[[0, 1, 3, 4, 5]], ref[[0, 1, 3, 4, 5]], rtol=1e-5, atol=1e-6, err_msg=f"isac call {k}")
        np.testing.assert_allclose(np.asarray(out)[[2, 6]], ref[[2, 6]], rtol=1e-5, atol=0, err_msg=f"isac call {k} policy_loss / bc_loss")
        assert round(out[7] * 128) == round(ref[7] * 128) and out[7] * 128 == round(out[7] * 128), (k, out[7], ref[7])
        for j, net in enumerate((o.policy, o.q1, o.q2, o.q1_t, o.q2_t)):
            s, a, v = D.net_probe(S.flatten(net))
            np.testing.assert_allclose(v, g["probe_val"][k][j], rtol=1e-5, atol=2e-6, err_msg=f"call {k} net {j}")
            np.testing.assert_allclose(a, g["probe_abs"][k][j], rtol=1e-6)
    assert o.learning_steps == 8


def _parse(argv):
    from hirl4ucav_amd import train_all as T

    return T.parse_args(argv)


def test_train_all_parser_accepts_isac_and_refuses_what_it_cannot_run(tmp_path, capsys):
    bc = tmp_path / "bc_actor.pth"
    bc.write_bytes(b"x")
    base = ["--agent", "SAC", "--type", "ISAC", "--synthetic_expert", "--bc_actor", str(bc)]
    cfg = _parse(base)
    assert cfg.agent == "SAC" and cfg.type == "ISAC"
    for extra, word in ((["--dtype", "bf16"], "fp32"), (["--gpus", "2"], "one GPU")):
        with pytest.raises(SystemExit):
            _parse(base + extra)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse(["--agent", "SAC", "--type", "ISAC", "--synthetic_expert"])
    assert "--bc_actor" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse(["--agent", "SAC", "--type", "ISAC", "--bc_actor", str(bc)])
    assert "expert" in capsys.readouterr().err


@pytest.mark.parametrize("kw", [{"per": True}, {"multi_step": 3}, {"entropy_tuning": False}, {"grad_clip": 1.0}])
def test_sac_agent_still_refuses_what_is_not_built(kw, tmp_path):
    """(needs no GPU: the check precedes the engine)"""
    import types

    from hirl4ucav_amd.agents.SAC.agent import SacAgent

    box = lambda n: types.SimpleNamespace(shape=(n,))  # noqa: E731
    with pytest.raises(NotImplementedError) as e:
        SacAgent(box(13), box(4), str(tmp_path), hidden_units=[256, 512], imitative=True, **kw)
    assert "non-imitative" not in str(e.value)
