"""CPU tests of priorities at insert: the checker tests/_per_score.score against the reference's recorded run, the store model, the ABI version
and train_all's flag checks (no GPU needed)."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _hirl_data as D  # noqa: E402
from tests import _per_score as PS  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_checker_reproduces_the_references_errors(golden_dir, dtype):
    """errors[0] of the reference's SacAgent(per=True).learn run is |Q1(s, a) - y| on the UNTOUCHED networks (the first call computes its errors
    before any step; alpha = 1, the targets equal the critics) — exactly what agent.py:238-241 computes at append.  The bar is the one
    tests/test_per_gpu.py holds `errors` to against that file."""
    g = np.load(os.path.join(golden_dir, "sac_per_learn.npz"))
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"]) and D.checksum(data) == str(g["data_checksum"])
    rows = data["replay"][g["idx"][0]]
    got = PS.score(params, {"q1": params["q1"], "q2": params["q2"]}, 1.0, rows, g["eps"][0, 0], gamma=0.99, dtype=dtype)
    print(f"max abs {np.max(np.abs(got - g['errors'][0])):.2e}")
    np.testing.assert_allclose(got, g["errors"][0], rtol=5e-5, atol=2e-5)


def test_fixed_order_block_sums_are_sums():
    rng = np.random.default_rng(0)
    pr = rng.uniform(0.01, 3.0, 3 * 1024).astype(np.float32)
    pr[2500:] = 0
    got = PS.block_sums_fixed(pr)
    assert got.dtype == np.float32 and got.shape == (3,)
    np.testing.assert_allclose(got, pr.astype(np.float64).reshape(3, 1024).sum(1), rtol=1e-6)
    ints = rng.integers(0, 8, 2048).astype(np.float32)  # (exact in any order)
    np.testing.assert_array_equal(PS.block_sums_fixed(ints), ints.reshape(2, 1024).sum(1))


def test_store_model_wrap_around():
    m = PS.ScoreModel(2048)
    m.mark_new(2040)
    e = np.linspace(0.0, 3.0, 20)
    slots = m.score_new(2060, e)
    np.testing.assert_array_equal(slots, np.r_[2040:2048, 0:12])
    np.testing.assert_allclose(m.prio[slots], (e + 1e-4) ** 0.6)
    assert m.marked == 2060 and m.pmax == pytest.approx((3.0 + 1e-4) ** 0.6)
    assert (m.prio[12:2040] == 1.0).all()  # the others keep what mark_new gave them
    np.testing.assert_allclose(m.bsum32(), m.bsum(), rtol=1e-6)


def test_store_model_nothing_new_and_a_small_bound():
    m = PS.ScoreModel(2048)
    m.mark_new(100)
    before = m.prio.copy()
    assert m.score_new(100, np.zeros(0)).size == 0 and m.marked == 100 and m.pmax == 1.0
    np.testing.assert_array_equal(m.prio, before)
    # max_new smaller than the rows stored: the rest waits for the next call
    slots = m.score_new(150, np.full(64, 0.5), max_new=32)
    np.testing.assert_array_equal(slots, np.arange(100, 132))
    assert m.marked == 132 and (m.prio[132:150] == 0).all()
    slots = m.score_new(150, np.full(64, 0.25), max_new=32)
    np.testing.assert_array_equal(slots, np.arange(132, 150))
    assert m.marked == 150 and m.pmax == 1.0  # (0.5001^0.6 < 1: pmax never falls)


def test_store_model_more_than_the_ring_holds():
    m = PS.ScoreModel(1024)
    e = np.arange(1024) / 1024.0
    slots = m.score_new(1040, e)
    np.testing.assert_array_equal(slots, (1040 + np.arange(1024)) % 1024)  # row i = the row in slot (total + i) mod cap: the last cap rows stored
    assert slots[0] == 16 and m.marked == 1040 and (m.prio > 0).all()
    np.testing.assert_allclose(m.prio[slots], (e + 1e-4) ** 0.6)


def test_store_model_non_finite_errors_enter_at_pmax():
    m = PS.ScoreModel(2048)
    m.set([0], [2.5])  # pmax 2.5
    m.marked = 1
    e = np.array([0.3, np.nan, 9.0, np.inf, 0.1])
    slots = m.score_new(6, e)
    np.testing.assert_allclose(m.prio[slots], [(0.3 + 1e-4) ** 0.6, 2.5, (9.0 + 1e-4) ** 0.6, 2.5, (0.1 + 1e-4) ** 0.6])  # pmax AS IT WAS at entry
    assert m.pmax == pytest.approx((9.0 + 1e-4) ** 0.6) and m.marked == 6


def test_header_and_binding_versions():
    from hirl4ucav_amd import _lib

    hdr = open(os.path.join(REPO, "include", "hirl4ucav.h")).read()
    declared = int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1))
    assert declared == _lib.ABI_VERSION and declared >= 120
    assert "hx_per_score_new" in hdr and "hx_per_score_workspace_floats" in hdr and re.search(r"\* 120:", hdr)


@pytest.mark.parametrize("argv,reason", [
    (["--agent", "SAC", "--type", "SAC", "--per_new", "td"], "goes with --per"),
    (["--agent", "SAC", "--type", "SAC", "--per", "--per_new", "td", "--dtype", "bf16"], "fp32 only"),
    (["--agent", "SAC", "--type", "ISAC", "--per", "--per_new", "td", "--bc_actor", "x", "--synthetic_expert"], "imitative"),
])
def test_parse_args_refuses_per_new_td_where_it_is_not_built(argv, reason, capsys):
    from hirl4ucav_amd import train_all as T

    with pytest.raises(SystemExit):
        T.parse_args(argv)
    err = capsys.readouterr().err
    assert "--per" in err and reason in err, err


def test_parse_args_takes_per_new():
    from hirl4ucav_amd import train_all as T

    assert T.parse_args(["--agent", "SAC", "--type", "SAC", "--per"]).per_new == "max"
    cfg = T.parse_args(["--agent", "SAC", "--type", "SAC", "--per", "--per_new", "td"])
    assert cfg.per_new == "td" and T.per_refusal(cfg) is None
    assert T.per_refusal(T.parse_args(["--agent", "SAC", "--type", "SAC"])) is None
