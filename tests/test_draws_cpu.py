"""CPU tests of the host statement of the in-kernel draws (tests/_philox_model.py; the GPU is held to it value by value in tests/test_draws_gpu.py):
the Random123 known answers, agreement of every other host copy of Philox (tests/_upsample_model.py, tests/_noise_model.py, tests/_per_score.py, the
oracle library's ox_philox4x32_10 that the env's reset is pinned through), the counter map of DESIGN.md "Who draws where" as sets that must not meet,
the quality of the model's normals, the sampler model's invariants, and the one counter whose first uniform is exactly 1.0f."""
import os
import re

import numpy as np
import pytest

from tests import _philox_model as PM
from tests._ring_model import allowed_slots

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, words)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]

# the committed u01 == 1.0f edge: Philox(key = U1_SEED; (U1_ROW, U1_CALL, TAG_ACT, 0)) has word 0 >> 8 == 0xFFFFFF (found by an offline search over rows
# 0 .. 2^22 of call 1 with this model: one hit in 2^22 counters, at the expected rate of 2^-24 a lucky first chunk)
U1_SEED, U1_ROW, U1_CALL = 2024, 2733486, 1


def random_pairs(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64), rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64)


def test_known_answers():
    for c, k, want in KAT:
        assert tuple(int(x) for x in PM.philox4x32_10(c, k)) == want
    c, k = np.array([v[0] for v in KAT]), np.array([v[1] for v in KAT])
    np.testing.assert_array_equal(PM.philox4x32_10(c, k), np.array([v[2] for v in KAT], np.uint32))  # (the batched form)
    np.testing.assert_array_equal(PM.philox4x32_10(c[0], k), PM.philox4x32_10(np.repeat(c[:1], 3, 0), k))  # (one counter broadcast over keys)


def test_the_other_host_copies_agree_with_the_shared_model():
    """tests/_upsample_model.philox4x32_10 (which tests/_noise_model.py imports) word for word on the known answers and on 10^4 random (counter, key)
    pairs; tests/_per_score.philox_normals IS the shared model; tests/_noise_model.normal4 keeps its float64 uniforms — it may differ from the device's
    float32 ones by what u01's rounding moves a normal, at most sqrt(2 * 2^-25) = 2.45e-4 (at u >> 8 = 0xFFFFFF: 1 - 2^-25 against 1.0f)."""
    from tests import _noise_model as NM
    from tests import _per_score as PS
    from tests import _upsample_model as UM

    assert NM.philox4x32_10 is UM.philox4x32_10
    for c, k, want in KAT:
        assert UM.philox4x32_10(c, k) == want
    c, k = random_pairs(10_000)
    got = PM.philox4x32_10(c, k)
    for i in range(c.shape[0]):
        assert UM.philox4x32_10(c[i], k[i]) == tuple(int(x) for x in got[i]), i
    np.testing.assert_array_equal(PS.philox_normals(7, PS.SCORE_ROW0, 3, 48), PM.act_normals(7, PM.SCORE_ROW0, 48, 3, PM.TAG_GAUSS).astype(np.float32))
    assert (PS.SCORE_ROW0, PS.LEARN_NEXT_ROW0) == (PM.SCORE_ROW0, PM.LEARN_NEXT_ROW0) and (NM.TAG_STEP, NM.TAG_INIT) == (PM.BANK_STEP, PM.BANK_INIT)
    assert (UM.UPS_STREAM, UM.UPS_FIRE_ROW) == (PM.UPS_STREAM, PM.UPS_FIRE_ROW)
    seed = (5 << 32) | 77
    for row, step, pole in ((0, 0, 0), (3, 5, 1), (2 ** 32 - 1, (1 << 32) + 4, 7)):
        ctr = NM.step_counter(row, step, pole)
        key, mine = PM.bank_counters(seed, row, 1, step, pole)
        assert tuple(int(x) for x in mine[0]) == ctr
        np.testing.assert_allclose(NM.normal4(ctr, seed), PM.draw_normals((key, mine))[0], rtol=0, atol=2.45e-4)
    np.testing.assert_array_equal(PM.bank_counters(seed, 9, 2, 123, 3, init=True)[1], [[9, 0, 0, PM.BANK_INIT | 3], [10, 0, 0, PM.BANK_INIT | 3]])
    words = UM.philox_words(seed, 4, 3, fire=True)
    key, ctr = PM.upsample_counters(seed, 3, 4, fire=True)
    w = PM.philox4x32_10(ctr, key).astype(np.uint64)
    assert words == [int(x) for x in (w[:3, 0] << np.uint64(32)) | w[:3, 1]] + [int((w[3, 0] << np.uint64(32)) | w[3, 1]), int((w[3, 2] << np.uint64(32)) | w[3, 3])]


def test_the_oracle_librarys_philox_agrees_with_the_shared_model():
    """ox_philox4x32_10 (oracle/env_oracle.c): the env's random reset is pinned through it, so the device's second copy (csrc/hx_env_dev.h) is on the chain"""
    from tests import _oracle as ox

    L = ox.lib()
    c, k = random_pairs(10_000, seed=1)
    c = np.concatenate([np.array([v[0] for v in KAT], np.uint64), c])
    k = np.concatenate([np.array([v[1] for v in KAT], np.uint64), k])
    want = PM.philox4x32_10(c, k)
    c32, k32, o = np.ascontiguousarray(c.astype(np.uint32)), np.ascontiguousarray(k.astype(np.uint32)), np.zeros(4, np.uint32)
    for i in range(c.shape[0]):
        L.ox_philox4x32_10(c32[i].ctypes.data, k32[i].ctypes.data, ox.p(o))
        assert np.array_equal(o, want[i]), i
    key, ctr = PM.env_reset_counters(9, [5, 6], [2, 0])
    assert key == (9, 0) and ctr.tolist() == [[5, 2, 0, 0], [6, 0, 0, 0]]


def test_u01_is_the_devices_float32():
    """(float)(u >> 8) + 0.5f rounds to even from 2^23 on; the largest word gives exactly 1.0f"""
    w = np.array([0, 0xFF, 0x100, (1 << 31) - 1, 1 << 31, (1 << 31) | 0x100, 0xFFFFFE00, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    u = PM.u01(w)
    assert u.dtype == np.float32
    f = np.float32
    want = [f(0.5) * f(2.0 ** -24), f(0.5) * f(2.0 ** -24), f(1.5) * f(2.0 ** -24), f(2.0 ** 23 - 0.5) * f(2.0 ** -24), f(0.5),  # 2^23 + 0.5 -> 2^23 (even)
            f(2.0 ** 23 + 2) * f(2.0 ** -24),                                      # 2^23 + 1.5 -> 2^23 + 2
            f(2.0 ** 24 - 2) * f(2.0 ** -24), f(1.0), f(1.0)]                      # 2^24 - 1.5 -> 2^24 - 2; 2^24 - 0.5 -> 2^24
    np.testing.assert_array_equal(u, np.array(want, f))
    assert (u > 0).all() and (u <= 1).all()


def test_the_committed_edge_gives_two_zero_normals():
    key, ctr = PM.act_counters(U1_SEED, U1_ROW, 1, U1_CALL)
    w = PM.philox4x32_10(ctr, key)[0]
    assert int(w[0]) >> 8 == 0xFFFFFF and PM.u01(w)[0] == np.float32(1.0)
    for dt in (np.float64, np.float32):
        z = PM.act_normals(U1_SEED, U1_ROW, 1, U1_CALL, dtype=dt)[0]
        assert z[0] == 0 and z[1] == 0 and abs(z[2]) > 0.1 and abs(z[3]) > 0.1
    assert int(PM.philox4x32_10(PM.act_counters(U1_SEED, U1_ROW + 1, 1, U1_CALL)[1], key)[0, 0]) >> 8 != 0xFFFFFF  # (the row beside it is an ordinary one)


# ---- the counter map ---------------------------------------------------------------------------------------------------------------------------------
FULL = [(0, 0xFFFFFFFF)]
ROWS = [(0, (1 << 31) - 1)]           # rows / env ids of a launch: < 2^31
BATCH_ROWS = [(0, (1 << 30) - 1)]     # the i of 0x40000000 + i, 0x80000000 + i, 0xC0000000 + i (a minibatch or a scoring chunk)
WORLD, POLES, ROUNDS = 8, 8, PM.MAX_ROUNDS


def one(*v):
    return [(int(x), int(x)) for x in v]


def shifted(iv, by):
    return [(lo + by, hi + by) for lo, hi in iv]


# train_all.py's keys as offsets from the run's seed (checked against the source below): "rank" stands for 0 .. WORLD - 1
KEY_OFFSETS = {"env": "seed", "acting": "seed + 1", "sampler": "seed + 2 + rank", "scorer": "seed + 3 + rank", "bank": "seed + 4"}


def offsets(expr):
    base = sum(int(t) for t in re.findall(r"\+ (\d+)", expr))
    return set(range(base, base + WORLD)) if expr.endswith("rank") else {base}


# consumer -> (key offsets, the sets the four counter words can take in a run, each a list of closed intervals)
CONSUMERS = {
    "env reset": (KEY_OFFSETS["env"], [ROWS, FULL, one(0), one(0)]),                                           # (env id, episode, 0, 0)
    "acting, deterministic head": (KEY_OFFSETS["acting"], [ROWS, FULL, one(PM.TAG_ACT), one(0)]),              # (env id = row0 + row, call, tag, 0)
    "acting, Gaussian head": (KEY_OFFSETS["acting"], [ROWS, FULL, one(PM.TAG_GAUSS), one(0)]),
    "sampler": (KEY_OFFSETS["sampler"], [[(0, 1023)], FULL, one(0, 1), [(0, ROUNDS - 1)]]),                    # (t, call, stream, round)
    "smoothing noise": (KEY_OFFSETS["sampler"], [one(PM.SMOOTH_ROW), FULL, one(PM.SMOOTH_STREAM), one(0)]),
    "PER": (KEY_OFFSETS["sampler"], [ROWS, FULL, one(PM.PER_STREAM), one(0)]),
    "upsampling": (KEY_OFFSETS["sampler"], [ROWS + one(PM.UPS_FIRE_ROW), FULL, one(PM.UPS_STREAM), one(0)]),
    "SAC learn(), policy.sample(s')": (KEY_OFFSETS["sampler"], [shifted(BATCH_ROWS, PM.LEARN_NEXT_ROW0), FULL, one(PM.TAG_GAUSS), one(0)]),
    "SAC learn(), policy.sample(s)": (KEY_OFFSETS["sampler"], [shifted(BATCH_ROWS, 0x80000000), FULL, one(PM.TAG_GAUSS), one(0)]),
    "scorer": (KEY_OFFSETS["scorer"], [shifted(BATCH_ROWS, PM.SCORE_ROW0), FULL, one(PM.TAG_GAUSS), one(0)]),
    "noise bank": (KEY_OFFSETS["bank"], [FULL, FULL, FULL, [(PM.BANK_STEP, PM.BANK_STEP + POLES - 1), (PM.BANK_INIT, PM.BANK_INIT + POLES - 1)]]),
}


def meet(a, b):
    return any(lo1 <= hi2 and lo2 <= hi1 for lo1, hi1 in a for lo2, hi2 in b)


def test_key_offsets_are_train_alls():
    """the one-line table above against the source, as tests/test_host_logic.py does for flags: every place train_all hands a consumer its key"""
    src = open(os.path.join(REPO, "hirl4ucav_amd", "train_all.py")).read()
    norm = lambda s: re.sub(r"\s+", " ", s.replace("run.", "")).strip()  # noqa: E731
    found = {
        "env": re.findall(r"run\.env = BatchedHarfangEnv\(.*?seed=([^,)]+)", src),
        "acting": re.findall(r"act_seed=([^,)]+)", src) + re.findall(r"eng\.act(?:_step)?\(.*?seed=([^,)]+)", src),
        "sampler": re.findall(r"sample_seed=([^,)\n]+)", src) + re.findall(r"n_main, sample_seed = [^,]+, ([^\n]+)", src),
        "scorer": re.findall(r"score_new\(.*?seed=([^,)]+)", src),
        "bank": re.findall(r"sigma_max=.*?seed=([^,)]+)", src),
    }
    for name, exprs in found.items():
        assert exprs and {norm(e) for e in exprs} == {KEY_OFFSETS[name]}, (name, exprs)
    assert len(found["acting"]) >= 5 and len(found["sampler"]) >= 3 and len(found["scorer"]) >= 2
    # the draws that use the sampler's key are handed it, not one of their own: sample()'s seed reaches the PER / upsampling draw and SAC's learn()
    eng = open(os.path.join(REPO, "hirl4ucav_amd", "agents", "engine.py")).read()
    assert re.search(r"per\.sample_into\(.*?seed=seed,", eng) and re.search(r"draw_call\(.*?, seed, self\.upsample_calls", eng)
    sac = open(os.path.join(REPO, "hirl4ucav_amd", "agents", "sac_engine.py")).read()
    assert re.search(r"self\._seed = int\(seed\)", sac)


def test_the_counter_map_is_collision_free():
    """Any two consumers that can meet under one key (rank r's sampler key is rank r - 1's scorer key, and seed + 4 is the noise bank's as well as rank 2's
    sampler key and rank 1's scorer key) differ in at least one counter word's set.  A pair that no key brings together is named, so that a new key
    offset that does shows up here: the env's reset (env id, episode, 0, 0) has the shape of the sampler's (t, call, 0, round 0), and the Gaussian
    head's acting rows (env ids below 2^31) cover the rows 0x40000000 + i at which SAC's learn() draws policy.sample(s') with the same tag."""
    names = list(CONSUMERS)
    only_the_key_separates = []
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ka, wa), (kb, wb) = CONSUMERS[a], CONSUMERS[b]
            words_apart = any(not meet(x, y) for x, y in zip(wa, wb))
            if offsets(ka) & offsets(kb):
                assert words_apart, f"{a} and {b} share a key ({ka} / {kb}) and a counter"
            elif not words_apart:
                only_the_key_separates.append((a, b))
    assert set(only_the_key_separates) == {("env reset", "sampler"), ("acting, Gaussian head", "SAC learn(), policy.sample(s')")}, only_the_key_separates
    # the model's own counter functions stay inside the sets the table claims for them
    probes = {
        "acting, deterministic head": PM.act_counters(1, 2 ** 31 - 100, 100, 7)[1],
        "acting, Gaussian head": PM.gauss_counters(1, 5, 10, 7)[1],
        "scorer": PM.gauss_counters(1, PM.SCORE_ROW0, 1024, 7)[1],
        "SAC learn(), policy.sample(s')": PM.gauss_counters(1, PM.LEARN_NEXT_ROW0, 1024, 7)[1],
        "smoothing noise": PM.smoothing_counters(1, 7)[1],
        "sampler": PM.sampler_counters(1, np.arange(1024), 7, 1, 127)[1],
        "PER": PM.per_counters(1, 128, 7)[1],
        "upsampling": PM.upsample_counters(1, 128, 7, fire=True)[1],
        "noise bank": np.concatenate([PM.bank_counters(1, 0, 4, (1 << 40) + 3, 7)[1], PM.bank_counters(1, 0, 4, 0, 0, init=True)[1]]),
        "env reset": PM.env_reset_counters(1, [0, 2 ** 31 - 1], [0, 9])[1],
    }
    for name, ctr in probes.items():
        for j, allowed in enumerate(CONSUMERS[name][1]):
            assert all(meet(one(v), allowed) for v in np.unique(ctr[:, j])), (name, j)


# ---- the quality of the model's normals --------------------------------------------------------------------------------------------------------------
def test_quality_of_the_models_normals():
    """2^16 rows x 16 calls x 4 components under the acting tag (the GPU is pinned to these values, tests/test_draws_gpu.py): Kolmogorov-Smirnov against
    Phi, the counts beyond 3 and 4 sigma against their binomial, the six component-pair correlations, the lag-1 correlation along rows and along
    calls (r sqrt(N) is standard normal for independent draws).  Every p-value inside [1e-3, 1 - 1e-3] — too good a fit fails like too bad a one, the
    convention of test_device_draw_is_uniform; the statistics are constants of QUALITY_SEED = 4, one of the seeds whose eleven p-values all lie in
    [0.05, 0.95] (of 1 .. 11: 2, 4, 6, 8 and 9 — as many as independent uniform p-values would give) — checked below, so the window is not grazed."""
    from scipy import stats

    z = PM.normals(PM.quality_words())
    assert z.shape == (1 << 16, 16, 4) and np.isfinite(z).all()
    n = z.size
    pv = {"ks": stats.kstest(z.reshape(-1), "norm").pvalue}
    for s in (3.0, 4.0):
        pv[f"beyond {s:g} sigma"] = stats.binom.sf(int((np.abs(z) > s).sum()) - 1, n, 2 * stats.norm.sf(s))

    def corr_p(a, b):
        a, b = a.reshape(-1), b.reshape(-1)
        return stats.norm.sf(np.corrcoef(a, b)[0, 1] * np.sqrt(a.size))

    for i in range(4):
        for j in range(i + 1, 4):
            pv[f"components {i}, {j}"] = corr_p(z[..., i], z[..., j])
    pv["lag 1 along rows"] = corr_p(z[:-1], z[1:])
    pv["lag 1 along calls"] = corr_p(z[:, :-1], z[:, 1:])
    assert len(pv) == 11
    for name, p in pv.items():
        assert 1e-3 <= p <= 1 - 1e-3, (name, p)
        assert 0.05 <= p <= 0.95, (name, p, "QUALITY_SEED was to be chosen with every p-value in [0.05, 0.95]")
    # the float32 yardstick: one float32 evaluation of the same formula on the same uniforms.  2 pi u in float32 is off by up to 2^-24 * 2 pi = 3.7e-7
    # in the angle, times a radius of up to 5.8: about 2e-6 is what to expect
    e32 = PM.e32()
    print(f"E32 = {e32:.4g}")
    assert 1e-7 < e32 < 5e-6, e32


# ---- the sampler model -------------------------------------------------------------------------------------------------------------------------------
def test_draw_map_never_yields_a_guarded_slot():
    """slot_of_draw over the WHOLE population is exactly the allowed slots, in order (the ring part full, full, wrapped window, beyond 2^32)"""
    for cap, guard in ((700, 150), (64, 32), (50, 1), (512, 0)):
        for tot in (0, 1, guard, cap - guard, cap - guard + 1, cap - 1, cap, cap + 1, 2 * cap - guard, 2 * cap - 1, 3 * cap + cap - 80, (1 << 32) + 5, (1 << 40) + cap - 3):
            m = PM.draw_map(tot, cap, guard)
            got = PM.slot_of_draw(m, np.arange(m[0]))
            np.testing.assert_array_equal(got, allowed_slots(tot, cap, guard), err_msg=f"cap {cap} guard {guard} total {tot}")


def sampler_cases(n, seed=0):
    rng = np.random.default_rng(seed)
    for i in range(n):
        batch = int(rng.integers(1, 33))
        n_main = int(rng.integers(0, batch + 1))
        cap = int(rng.integers(80, 400))
        guard = int(rng.integers(0, cap // 2 + 1)) if i % 2 else 0
        total = int(rng.choice([rng.integers(guard + batch, cap), rng.integers(cap, 5 * cap), (1 << 32) + rng.integers(0, cap)]))
        expert_len = int(rng.integers(max(batch - n_main, 1), 200))
        bc_len = int(rng.integers(batch, 300))
        yield total, cap, guard, expert_len, bc_len, batch, n_main, int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 32))


def test_sampler_model_invariants():
    """2,000 seeded cases: indices inside the population (the guarded map never yields a guarded slot), distinct inside a group whenever the round cap
    was not reached; and the two streams of one (seed, call) are unrelated: over the cases whose two first groups draw from equally long tables the
    pooled rank correlation of idx against idx_bc is that of independent draws (were both streams keyed alike it would be 1)."""
    from scipy import stats

    pairs = []
    for k, (total, cap, guard, expert_len, bc_len, batch, n_main, seed, call) in enumerate(sampler_cases(2000)):
        if k % 4 == 0:  # the case the correlation needs: one group, both tables equally long, no guard (idx == idx_bc if the streams were one)
            guard, n_main = 0, batch
            bc_len = min(total, cap)
        idx, idx_bc, used = PM.sample_model(total, cap, guard, expert_len, bc_len, batch, n_main, seed, call)
        what = (total, cap, guard, expert_len, bc_len, batch, n_main, seed, call)
        assert idx.shape == idx_bc.shape == (batch,) and 1 <= used <= PM.MAX_ROUNDS
        assert np.isin(idx[:n_main], allowed_slots(total, cap, guard)).all(), what
        assert ((idx[n_main:] >= 0) & (idx[n_main:] < expert_len)).all() and ((idx_bc >= 0) & (idx_bc < bc_len)).all(), what
        if used < PM.MAX_ROUNDS:
            assert len(set(idx[:n_main])) == n_main and len(set(idx[n_main:])) == batch - n_main and len(set(idx_bc)) == batch, what
        if k % 4 == 0:
            pairs.append(np.stack([idx / bc_len, idx_bc / bc_len], 1))
    p = np.concatenate(pairs)
    rho = stats.spearmanr(p[:, 0], p[:, 1])[0]
    pv = stats.norm.sf(rho * np.sqrt(p.shape[0] - 1))
    assert p.shape[0] > 5000 and 1e-3 <= pv <= 1 - 1e-3, (rho, pv, p.shape)


def test_sampler_model_at_the_round_cap():
    """a group that asks for more than its table holds keeps duplicates after 128 rounds — every value still inside the table, every table entry taken, and
    the lowest row of a key never redraws (its index is its first draw); a group that asks for exactly its table ends with or without a survivor"""
    idx, idx_bc, used = PM.sample_model(5000, 5000, 0, 8, 150, 128, 112, 3, 1)
    assert used == PM.MAX_ROUNDS and set(idx[112:]) == set(range(8)) and len(set(idx[:112])) == 112 and len(set(idx_bc)) == 128
    key, ctr = PM.sampler_counters(3, [112], 1, 0, 0)
    assert idx[112] == (int(PM.philox4x32_10(ctr, key)[0, 0]) * 8) >> 32  # row 112, the lowest of its group, owns whatever it drew first
    ends = []
    for call in range(1, 5):  # (which calls end how is a constant of the seed: tests/test_draws_gpu.py takes this list — calls 2 and 4 keep a duplicate)
        idx, _, used = PM.sample_model(130, 5000, 0, 0, None, 128, 128, 22, call)
        assert (used == PM.MAX_ROUNDS) == (len(set(idx)) < 128) and idx.max() < 130
        ends.append(used == PM.MAX_ROUNDS)
    assert ends == [False, True, False, True]
    idx, idx_bc, used = PM.sample_model(0, 64, 0, 0, 0, 4, 4, 1, 1)  # empty tables: umulhi(word, 0) = 0 for everyone
    assert used == PM.MAX_ROUNDS and not idx.any() and not idx_bc.any()


@pytest.mark.parametrize("n_main", [0, 16])
def test_sampler_model_with_one_group(n_main):
    idx, idx_bc, used = PM.sample_model(300, 5000, 0, 200, 150, 16, n_main, 9, 1)
    assert used < PM.MAX_ROUNDS and len(set(idx)) == 16 and idx.max() < (300 if n_main else 200) and len(set(idx_bc)) == 16
