"""Every in-kernel random draw of the acting and sampling kernels BY VALUE against the host Philox model (tests/_philox_model.py, itself held to the
Random123 known answers, to the other host copies and to its own statistics by tests/test_draws_cpu.py; DESIGN.md "Who draws where").

Reached directly here: hx_actor_act's per-tile kernel (16- and 32-row tiles, philox_normal) and the persistent kernels of every acting format
(philox_normal_pair), hx_sac_act's in-kernel eps, hx_sample_batch[_guarded] (sample_kernel) and the deferred draw of hx_hirl_learn_sampled (draw_fused),
with their smoothing noise.  Reached through existing bit-identity tests, which tie the other kernels to those: test_persistent_act_equals_the_per_tile_kernel
(tests/test_actp_gpu.py), test_act_row_tilings_agree_bit_for_bit and test_act_step_in_one_launch_equals_act_then_step (tests/test_hirl_gpu.py: the
act + env launches), test_front_launch_equals_act_step_then_guarded_learn (tests/test_front_gpu.py: the front launch's acting roles, and the predraw
workgroup of hx_hirl_learn_back — its `_idx`, `_idx_bc`, `_noise`, `rows` and `bc_rows` are compared bit for bit with sample(defer=True) + learn() under a
guard, the deferred draw pinned here; so the predraw workgroup has no case of its own).

Tolerances.  Integers (indices, gathered rows): exact.  Normals formed with logf / sinf / cosf: against the float64 model, 4 x E32 on z, where E32 is the
largest distance between numpy's float32 evaluation of the same Box-Muller formula and the float64 one over the CPU test's 2^22 draws (computed, not
typed in: _philox_model.e32(), about 1.7e-6) — device and numpy libm may each be an ulp or two off in different places —, plus one fp32 rounding of the sum
clean + sigma z (2^-24: the sum is below 2 wherever the clamp leaves it alone).  No row is excluded: the clamp is modelled.
The smoothing noise uses the fast intrinsics (__logf / __sinf / __cosf: v_log_f32, v_sin_f32, v_cos_f32), whose error is not derived here: the first run
on an MI355X recorded max |got - sigma z64| / sigma = 1.158e-6 (SMOOTH_RECORDED; the same figure from the sampling launch and from the deferred form,
which are bit-identical) over 64 calls x 2 seeds x 4 components; the test asserts 4 x that, and that the recorded value itself is below 1e-3 (the bound
the SAC scorer's indirect pin uses).  It is no larger than the library functions' E32."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402
from tests import _philox_model as PM  # noqa: E402
from tests.test_draws_cpu import U1_CALL, U1_ROW, U1_SEED  # noqa: E402

SMOOTH_RECORDED = 1.16e-6  # max |got - sigma z64| / sigma of the smoothing noise, first run on an MI355X: 1.158e-6 in both forms (module docstring)
HALF_ULP_BELOW_2 = 2.0 ** -24
T_PAST_2_32 = ((1 << 32) // 700 + 1) * 700 + 620  # tests/test_hirl_gpu.py: the 64-bit counter past 2^32, congruent to 3 * 700 + 620 mod 700


@pytest.fixture(scope="module")
def eng_mod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


@pytest.fixture(scope="module")
def z_tol():
    """(E32, the tolerance on a standard-normal draw of the device's logf / sinf / cosf)"""
    e32 = PM.e32()
    return e32, 4.0 * e32


@pytest.fixture(scope="module")
def actor(eng_mod):
    params = D.make_params(D.PARAM_SEED)
    e = eng_mod.HirlEngine(batch=128)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    return e


def check_act(e, obs, sigma, seed, row0, call, z_tol, what):
    """act(obs, sigma) of call `call` against clip(clean + sigma z_model, -1, 1), every row and component -> (got, clean, z)"""
    e32, tz = z_tol
    clean = e.act(obs).cpu().numpy()
    e.act_calls = call - 1
    got = e.act(obs, sigma=sigma, seed=seed, row0=row0).cpu().numpy()
    assert e.act_calls == call
    z = PM.act_normals(seed, row0, obs.shape[0], call)
    s = float(np.float32(sigma))
    want = np.clip(clean.astype(np.float64) + s * z, -1.0, 1.0)
    tol = s * tz + HALF_ULP_BELOW_2
    diff = np.abs(got.astype(np.float64) - want)
    bad = np.argwhere(diff > tol)
    assert bad.size == 0, (f"{what}: {bad.shape[0]} entries off, first (row, component) {bad[0].tolist()} by {diff[tuple(bad[0])]:.3g}; worst {diff.max():.3g}; "
                           f"E32 {e32:.4g}, allowed sigma * 4 E32 + 2^-24 = {tol:.4g}")
    return got, clean, z


@pytest.mark.parametrize("seed,call", [(5, 10), ((9 << 32) | 5, 10), (5, 77)])
def test_acting_draw_by_value_ragged_tile(actor, z_tol, seed, call):
    """33 rows: two 16-row tiles and one row of a third; two calls, two seeds (the second differs in the key's HIGH word only)"""
    obs = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (33, 13)).astype(np.float32)).cuda()
    got, clean, z = check_act(actor, obs, 0.1, seed, 0, call, z_tol, f"33 rows seed {seed} call {call}")
    assert (got != clean).mean() > 0.9  # (the draws did move the actions)


def test_acting_draw_by_value_row_counter_wraps(actor, z_tol):
    """100 rows at row0 = 2^32 - 50: counter word 0 is (row0 + row) mod 2^32 — rows 50 .. 99 draw what rows 0 .. 49 of a call at row0 = 0 draw"""
    obs = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, (100, 13)).astype(np.float32)).cuda()
    _, _, z = check_act(actor, obs, 0.1, 5, 2 ** 32 - 50, 3, z_tol, "row0 = 2^32 - 50")
    np.testing.assert_array_equal(z[50:], PM.act_normals(5, 0, 50, 3))


def test_acting_draw_by_value_where_u01_is_one(actor, z_tol):
    """the committed counter whose first word has u >> 8 == 0xFFFFFF, as row 0 of a 16-row call: u01 is exactly 1.0f, the logarithm 0, both normals of
    the pair 0 — components 0 and 1 are the clean action bit for bit (a float64 u01 would give 1 - 2^-25 and normals of up to 2.4e-4)"""
    obs = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (16, 13)).astype(np.float32)).cuda()
    got, clean, z = check_act(actor, obs, 0.3, U1_SEED, U1_ROW, U1_CALL, z_tol, "u01 == 1.0f")
    assert z[0, 0] == 0 and z[0, 1] == 0
    np.testing.assert_array_equal(got[0, :2].view(np.uint32), clean[0, :2].view(np.uint32))
    assert (got[0, 2:] != clean[0, 2:]).all() and (got[1:] != clean[1:]).any(1).all()


@pytest.mark.parametrize("fmt", ["f32", "f32x9", "bf16"])
def test_acting_draw_by_value_persistent_kernels(eng_mod, z_tol, fmt):
    """8,193 rows: beyond one round of 32-row workgroups, the persistent kernel of each acting format (philox_normal_pair: one Philox evaluation per
    pair of components), at a row0 that is not zero.  sigma = 0.5 puts a share of the entries on the clamp, which the host models."""
    params = D.make_params(D.PARAM_SEED)
    e = eng_mod.HirlEngine(batch=128)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    if fmt == "f32":
        e.x9_rows = None  # (the fp32 image at every row count)
    else:
        e.set_act_dtype(fmt)
    n = 8193
    assert e._act_format(n)[0] == {"f32": "_f32i", "f32x9": "_x9", "bf16": "_bf16"}[fmt]
    obs = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (n, 13)).astype(np.float32)).cuda()
    got, clean, z = check_act(e, obs, 0.5, 7, 1000, 2, z_tol, f"8,193 rows {fmt}")
    clamped = np.abs(clean.astype(np.float64) + 0.5 * z) > 1.0
    assert clamped.any() and (np.abs(got[clamped]) == 1.0).all() and not clamped.all()


@pytest.mark.parametrize("n", [48, 1000])
def test_gaussian_heads_draw_by_value(n, z_tol):
    """hx_sac_act in explore mode: the in-kernel eps against the SAME call given eps = the model's normals (both on the device, so the networks' arithmetic
    is the same and only eps differs).  a = tanh(mu + exp(log_std) eps): |da| <= exp(log_std) |d eps| (tanh' <= 1), log_std from the float64 oracle;
    d eps = 4 E32 + the float32 rounding of the given eps (2^-24 |eps|); + 2^-22 for the fp32 sum and tanhf on both sides."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine as SE
    from oracle import sac_oracle as S
    from tests.test_oracle_sac import sac_params

    e32, tz = z_tol
    params = sac_params()
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], params["q1"], params["q2"])
    obs = np.random.default_rng(n).uniform(-1, 1, (n, 13)).astype(np.float32)
    dobs = torch.from_numpy(obs).cuda()
    seed, row0, call = (3 << 32) | 17, 2 ** 32 - 20, 6
    z = PM.act_normals(seed, row0, n, call, tag=PM.TAG_GAUSS)
    e.act_calls = call - 1
    got = e.act(dobs, seed=seed, row0=row0).cpu().numpy().astype(np.float64)
    e.act_calls = call - 1
    want = e.act(dobs, eps=torch.from_numpy(z.astype(np.float32)).cuda()).cpu().numpy().astype(np.float64)
    with torch.no_grad():
        _, log_std = S.policy_forward(S.to_t(params["policy"], dtype=torch.float64), torch.from_numpy(obs).double())
    tol = np.exp(log_std.numpy()) * (tz + 2.0 ** -24 * np.abs(z)) + 2.0 ** -22
    diff = np.abs(got - want)
    bad = np.argwhere(diff > tol)
    assert bad.size == 0, f"{bad.shape[0]} entries off, first {bad[0].tolist()} by {diff[tuple(bad[0])]:.3g} (allowed {tol[tuple(bad[0])]:.3g}); E32 {e32:.4g}"
    exploit = e.act(dobs, explore=False).cpu().numpy()
    assert (np.abs(got - exploit) > 1e-3).mean() > 0.9  # (the draws did move the actions)


# ---- the minibatch draw ------------------------------------------------------------------------------------------------------------------------------
class Tables:
    """a main ring of `cap` slots whose counter stands at `total`, an expert ring of `expert_len` rows, a BC table of `bc_len` rows (None: no BC)"""

    def __init__(self, cap, total, expert_len, bc_len, seed=0):
        from hirl4ucav_amd.utils.buffer import DeviceReplay

        rng = np.random.default_rng(seed)
        self.cap, self.total, self.expert_len, self.bc_len = cap, total, expert_len, bc_len
        self.rep = DeviceReplay(cap)
        self.rep.ring.copy_(torch.from_numpy(rng.normal(size=(cap, 32)).astype(np.float32)))
        self.rep.ring[:, 31] = (self.rep.ring[:, 31] > 1.0).float()  # done flags
        self.rep.total.fill_(total)
        self.exp = None
        if expert_len:
            self.exp = DeviceReplay(expert_len + 3)
            self.exp.store_rows(torch.from_numpy(rng.normal(size=(expert_len, 32)).astype(np.float32)))
        self.bc = torch.from_numpy(rng.normal(size=(bc_len, 32)).astype(np.float32)).cuda() if bc_len else None
        self.ring_h, self.exp_h = self.rep.ring.cpu().numpy(), (self.exp.ring.cpu().numpy() if self.exp is not None else None)
        self.bc_h = self.bc.cpu().numpy() if self.bc is not None else None


def new_engine(eng_mod, B, use_bc):
    params = D.make_params(31)
    e = eng_mod.HirlEngine(batch=B, use_bc=use_bc, slope=0.0 if use_bc else 0.01)
    e.load_params(params["actor"], params["critic"], params["bc_actor"] if use_bc else None)
    return e


def draw(e, T, n_main, seed, call, guard, deferred, sigma=0.2):
    """one draw of call `call` -> (idx, idx_bc, noise, rows, bc_rows) on the host.  deferred: sample(defer=True) + learn() (draw_fused inside the update's
    first launch, the guard through HxSample.guard as the front launch's twin sets it); else the sampling launch (hx_sample_batch, hx_sample_batch_guarded)"""
    from hirl4ucav_amd import _lib

    B = e.batch
    e.sample_calls = call - 1
    if deferred:
        e.sample(T.rep, T.exp, T.bc, n_main=n_main, seed=seed, sigma=sigma, defer=True)
        e._pending[0].guard = guard
        e.learn(bc_weight_now=0.3 if T.bc is not None else 0.0)
    elif guard == 0:
        e.sample(T.rep, T.exp, T.bc, n_main=n_main, seed=seed, sigma=sigma)
    else:
        e.sample_calls = call
        _lib.call("hx_sample_batch_guarded", T.rep.total.data_ptr(), T.cap, T.rep.ring.data_ptr(), T.exp.ring.data_ptr() if T.exp is not None else None,
                  T.expert_len, _lib.ptr(T.bc), T.bc_len or 0, B, n_main, 1, int(seed), call, float(sigma), e._idx.data_ptr(),
                  e._idx_bc.data_ptr() if T.bc is not None else None, e._noise.data_ptr(), e.rows.data_ptr(), e.bc_rows.data_ptr() if T.bc is not None else None,
                  guard, _lib.stream_ptr())
    assert e.sample_calls == call
    return (e._idx.cpu().numpy(), e._idx_bc.cpu().numpy() if T.bc is not None else None, e._noise.cpu().numpy(), e.rows.reshape(B, 32).cpu().numpy(),
            e.bc_rows.reshape(B, 32).cpu().numpy() if T.bc is not None else None)


def check_draw(e, T, n_main, seed, call, guard, deferred):
    B = e.batch
    idx, idx_bc, _, rows, bc_rows = draw(e, T, n_main, seed, call, guard, deferred)
    want, want_bc, used = PM.sample_model(T.total, T.cap, guard, T.expert_len, T.bc_len if T.bc is not None else None, B, n_main, seed, call)
    what = f"B {B} n_main {n_main} total {T.total} cap {T.cap} guard {guard} seed {seed} call {call} {'deferred' if deferred else 'launch'} ({used} rounds)"
    np.testing.assert_array_equal(idx, want, err_msg=what)
    np.testing.assert_array_equal(rows[:n_main], T.ring_h[want[:n_main]], err_msg=what)
    if n_main < B:
        np.testing.assert_array_equal(rows[n_main:], T.exp_h[want[n_main:]], err_msg=what)
    if T.bc is not None:
        np.testing.assert_array_equal(idx_bc, want_bc, err_msg=what)
        np.testing.assert_array_equal(bc_rows, T.bc_h[want_bc], err_msg=what)
    return idx, idx_bc, used


@pytest.mark.parametrize("deferred", [False, True])
def test_index_draw_by_value(eng_mod, deferred):
    """B = 128, n_main = 96, 300 live rows of 5,000, 200 expert rows, 150 BC rows (test_device_sampler's case): idx, idx_bc and both row tiles are the
    model's, for two seeds (the second differs in the key's high word only) and calls that differ in the low and in a high bit"""
    T = Tables(5000, 300, 200, 150)
    e = new_engine(eng_mod, 128, True)
    seen = []
    for seed, call in ((9, 1), (9, 2), ((1 << 32) | 9, 1), (9, (1 << 31) | 1)):
        idx, idx_bc, used = check_draw(e, T, 96, seed, call, 0, deferred)
        assert used < PM.MAX_ROUNDS and len(set(idx[:96])) == 96 and len(set(idx[96:])) == 32 and len(set(idx_bc)) == 128
        seen.append(idx)
    assert all(not np.array_equal(seen[0], s) for s in seen[1:])


@pytest.mark.parametrize("deferred", [False, True])
def test_index_draw_by_value_at_the_round_cap(eng_mod, deferred):
    """a group that asks for (nearly) its whole table.  128 of 130 live rows: calls 1 .. 4 of seed 22 were chosen with the model — calls 2 and 4 still hold
    a duplicate after 128 rounds and keep it, calls 1 and 3 end before (tests/test_draws_cpu.py asserts the same list).  n_main = 112 with 8 expert rows:
    16 rows from 8, duplicates forced.  Who survives must not depend on where the hash table keeps a key: the two forms use tables of 4,096 and 1,024 slots
    and other hashes, the model none."""
    e = new_engine(eng_mod, 128, False)
    T = Tables(5000, 130, 0, None, seed=1)
    ends = []
    for call in (1, 2, 3, 4):
        idx, _, used = check_draw(e, T, 128, 22, call, 0, deferred)
        assert (used == PM.MAX_ROUNDS) == (len(set(idx)) < 128)
        ends.append(used == PM.MAX_ROUNDS)
    assert ends == [False, True, False, True]
    e = new_engine(eng_mod, 128, True)
    T = Tables(5000, 5000, 8, 150, seed=2)
    for call in (1, 2):
        idx, idx_bc, used = check_draw(e, T, 112, 3, call, 0, deferred)
        assert used == PM.MAX_ROUNDS and set(idx[112:]) == set(range(8)) and len(set(idx[:112])) == 112


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("n_main", [0, 16])
def test_index_draw_by_value_one_group(eng_mod, deferred, n_main):
    """B = 16 with every row from the expert ring, and with every row from the main ring"""
    T = Tables(5000, 300, 200, 150, seed=3)
    e = new_engine(eng_mod, 16, True)
    for call in (1, 2):
        check_draw(e, T, n_main, 9, call, 0, deferred)


def test_index_draw_by_value_one_stream_per_pass(eng_mod):
    """B = 1,024 of 1,500 live rows and of 1,500 BC rows: beyond 512 rows the sampling launch draws the two streams one after the other with all 1,024
    threads (the deferred draw stops at 256 rows); collisions in the first round for certain"""
    T = Tables(1500, 1500, 0, 1500, seed=4)
    e = eng_mod.HirlEngine(batch=1024)
    for call in (1, 2):
        idx, idx_bc, used = check_draw(e, T, 1024, 3, call, 0, False)
        assert 1 < used < PM.MAX_ROUNDS and len(set(idx)) == 1024 and len(set(idx_bc)) == 1024


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("total", [400, 3 * 700 + 620, T_PAST_2_32, 2 * 700 + 200])
def test_guarded_index_draw_by_value(eng_mod, deferred, total):
    """cap 700, guard 150: the ring part full (no window to jump), full with the guard window wrapping round the end of the ring (every draw shifted up,
    none jumps), the same head with the counter past 2^32 — and full with the window inside the ring (head 200: a draw AT or beyond the head jumps the
    window; with 2 * 700 + 200 calls 10 and 11 were chosen with the model because a row draws exactly the head there, and lands on slot 350)"""
    T = Tables(700, total, 40, 150, seed=5)
    e = new_engine(eng_mod, 128, True)
    inside = total == 2 * 700 + 200
    for call in ((1, 10, 11) if inside else (1, 2, 3)):
        idx, _, used = check_draw(e, T, 96, 12345, call, 150, deferred)
        assert used < PM.MAX_ROUNDS
        if inside and call != 1:
            assert 350 in idx[:96]
    if total == T_PAST_2_32:  # the head is where 3 * 700 + 620 has it: the same slots
        want = PM.sample_model(3 * 700 + 620, 700, 150, 40, 150, 128, 96, 12345, 3)[0]
        np.testing.assert_array_equal(idx, want)


# ---- the smoothing noise -----------------------------------------------------------------------------------------------------------------------------
def test_smoothing_noise_by_value(eng_mod):
    """noise[4] of hx_sample_batch and of the deferred form (sample(defer=True) + learn(): smoothing_noise<> in launch A) over 64 calls x 2 seeds against
    sigma z of the float64 model (components 0 / 1 from words 0 / 1, components 2 / 3 from words 2 / 3).  Fast intrinsics: the bound is 4 x the deviation
    recorded on the first run (module docstring), which itself has to stay below 1e-3."""
    T = Tables(5000, 300, 200, 150, seed=6)
    sigma = 0.2
    s = float(np.float32(sigma))
    worst = {}
    for deferred in (False, True):
        e = new_engine(eng_mod, 128, True)
        dev = 0.0
        for seed in (9, (7 << 32) | 3):
            for call in range(1, 65):
                noise = draw(e, T, 96, seed, call, 0, deferred, sigma=sigma)[2]
                z = PM.smoothing_normals(seed, call)
                dev = max(dev, float(np.abs(noise.astype(np.float64) - s * z).max()) / s)
        worst["deferred" if deferred else "launch"] = dev
    print(f"smoothing noise: max |got - sigma z64| / sigma = {worst}")
    assert SMOOTH_RECORDED is not None and SMOOTH_RECORDED < 1e-3, "the recorded deviation is a finding, not a tolerance, from 1e-3 on"
    for form, dev in worst.items():
        assert dev <= 4.0 * SMOOTH_RECORDED, f"{form}: {dev:.4g} against 4 x the recorded {SMOOTH_RECORDED:.4g}"
