"""Is the reference of the peer-read all-reduce kernels right, and does the comparison discriminate?  (tests/_xchg_model.py; the kernels themselves:
tests/test_xchg_gpu.py.)  The model against fp64 and torch's bf16; the slices against the kernel's own owner search; four wrong models that the
inputs of EVERY (W, n) case of the GPU test must tell from the right one; the epoch words of exchange.epoch_word across the wrap."""
import numpy as np
import pytest

from tests import _xchg_model as X

torch = pytest.importorskip("torch")

SHAPES = sorted(set(X.CASES) | {(1, n) for n in X.RCCL_N})


def test_rank_order_sum_is_within_the_sequential_bound_of_the_fp64_sum():
    """|fl(((x0 + x1) + ...) + xW-1) - sum| <= (W - 1) u sum|x| (1 + O(u)) <= W 2^-24 sum|x|: W - 1 adds, each with a relative error of at most u = 2^-24"""
    rng = np.random.default_rng(5)
    wide = (rng.choice([-1.0, 1.0], (8, 1000)) * 10.0 ** rng.uniform(-6, 6, (8, 1000))).astype(np.float32)
    for W, n in [(8, None)] + SHAPES:
        bufs = wide if n is None else X.messages(W, n, X.case_seed(W, n))
        finite = np.isfinite(bufs).all(0)
        got = X.rank_order_sum(bufs)[finite].astype(np.float64)
        b64 = bufs[:, finite].astype(np.float64)
        assert finite.sum() >= min(bufs.shape[1], 4) // 2
        assert np.all(np.abs(got - b64.sum(0)) <= W * 2.0 ** -24 * np.abs(b64).sum(0)), (W, n)


def test_to_bf16_rne_is_torchs_conversion():
    rng = np.random.default_rng(6)
    x = X.from_bits(rng.integers(0, 1 << 32, 200000).astype(np.uint32))  # every exponent, denormals, infinities and NaNs among them
    edge = X.from_bits(np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0xFF7F8000, 0x00008000, 0x00018000,
                                 0x00007FFF, 0x007FFFFF, 0x80000000, 0, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001], np.uint32))
    for v in (x, edge, X.rank_order_sum(X.messages(8, 1028, 1))):
        want = torch.from_numpy(v.copy()).to(torch.bfloat16).to(torch.float32).numpy()
        got = X.to_bf16_rne(v)
        assert np.all(X.same(got, want))
        assert np.all((X.bits(got) & 0xFFFF) == 0)
    assert X.bits(X.to_bf16_rne(edge))[:8].tolist() == [0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0x7F800000, 0x7F7F0000, 0x7F800000, 0xFF800000]


@pytest.mark.parametrize("W", range(1, 9))
def test_slices_tile_the_message_and_the_kernels_owner_search_lands_on_them(W):
    for n4 in list(range(1, 71)) + [255, 256, 257, 65535, 65536, 65537, 69122]:
        sl = X.slices(n4, W)
        assert sl[0][0] == 0 and sl[-1][1] == n4 and all(lo <= hi for lo, hi in sl)
        assert all(sl[r][1] == sl[r + 1][0] for r in range(W - 1))
        by_slice = np.repeat(np.arange(W), [hi - lo for lo, hi in sl])
        start, landed = X.kernel_owner(n4, W)
        assert start.min() >= 0 and start.max() < W, (n4, start.min(), start.max())
        assert np.array_equal(landed, by_slice), n4
        probe = {0, n4 - 1} | {i for lo, hi in sl for i in (lo - 1, lo, hi - 1, hi) if 0 <= i < n4}
        assert all(X.owner(i, n4, W) == by_slice[i] for i in probe)


def test_every_input_class_occurs():
    for W, n in SHAPES:
        if n < 28:
            continue
        m = X.messages(W, n, X.case_seed(W, n))
        assert m.dtype == np.float32 and m.shape == (W, n)
        assert np.array_equal(X.bits(m), X.bits(X.messages(W, n, X.case_seed(W, n))))  # seeded
        s, cls = X.rank_order_sum(m), X.column_class(n)
        sb, mb = X.bits(s), X.bits(m)
        col = {name: np.flatnonzero(cls == c) for c, name in enumerate(X.CLASSES)}
        assert all(j.size >= 2 for j in col.values())
        j = col["normal"]
        assert np.all(np.isfinite(m[:, j]) & (np.abs(m[:, j]) >= 1e-6) & (np.abs(m[:, j]) < 1e7))
        j = col["cancel"]
        if W >= 2:
            assert np.all(m[1, j] == -m[0, j]) and np.all(m[0, j] != 0)
        if W >= 3:
            assert np.all((m[2:, j] != 0).sum(0) == 1) and np.all(s[j] != 0)
            assert np.all(sb[j] != X.bits(X.rank_order_sum(m, order=range(W - 1, -1, -1)))[j])  # the order of addition changes the bits
        for name, kept in (("tie_even", 0), ("tie_odd", 1)):
            j = col[name]
            assert np.all((sb[j] & 0xFFFF) == 0x8000) and np.all((sb[j] >> 16) & 1 == kept)
        assert np.all(mb[:, col["zero_pos"]] == 0) and np.all(sb[col["zero_pos"]] == 0)
        assert np.all(mb[:, col["zero_neg"]] == 0x80000000) and np.all(sb[col["zero_neg"]] == 0x80000000)
        j = col["zero_mixed"]
        assert np.all((mb[:, j] & 0x7FFFFFFF) == 0)
        if W >= 2:
            assert np.all(mb[:, j].min(0) == 0) and np.all(mb[:, j].max(0) == 0x80000000) and np.all(sb[j] == 0)
        j = col["denormal"]
        assert np.all((mb[:, j] & 0x7F800000) == 0) and np.all((mb[:, j] & 0x007FFFFF) != 0)
        j = col["overflow"]
        assert np.all(np.isfinite(s[j])) and np.all((sb[j] & 0x7FFFFFFF) >= 0x7F7F8000) and np.all(np.isinf(X.to_bf16_rne(s[j])))
        assert (sb[j] & 0x7FFFFFFF).min() == 0x7F7F8000  # the tie over the largest finite bf16 among them
        assert np.all(s[col["inf_pos"]] == np.inf) and np.all(s[col["inf_neg"]] == -np.inf)
        assert np.all(np.isinf(m[:, col["inf_pos"]]).sum(0) == 1) and np.all(np.isnan(m[:, col["nan"]]).sum(0) == 1)
        assert np.all(np.isnan(s[col["nan"]]))
        j = col["inf_nan"]
        if W >= 2:
            assert np.all((m[:, j] == np.inf).sum(0) == 1) and np.all((m[:, j] == -np.inf).sum(0) == 1) and np.all(np.isnan(s[j]))
        else:
            assert np.all(s[j] == np.inf)


def test_the_comparison_rejects_four_wrong_models_at_every_case():
    """Each wrong model must differ from the right one, under the GPU test's own comparison, in at least one element of the inputs of every case it applies to"""
    seen = dict.fromkeys(("ceil", "reverse", "trunc", "away"), 0)
    for W, n in X.CASES:
        m = X.messages(W, n, X.case_seed(W, n))
        s = X.rank_order_sum(m)
        assert np.all(X.same(s, s)) and np.all(X.same_image(X.red_image(m), X.red_image(m)))
        if (n // 4) % W != 0:
            for bf16 in (False, True):
                assert not np.all(X.same_image(X.red_image(m, bf16, part=X.slices_ceil), X.red_image(m, bf16), bf16)), ("ceil", W, n, bf16)
            seen["ceil"] += 1
        if W >= 3:
            rev = X.rank_order_sum(m, order=range(W - 1, -1, -1))
            assert not np.all(X.same(rev, s)), ("reverse", W, n)
            assert not np.all(X.same(X.to_bf16_rne(rev), X.to_bf16_rne(s))), ("reverse, bf16", W, n)
            seen["reverse"] += 1
        for name, wrong in (("trunc", X.to_bf16_trunc), ("away", X.to_bf16_ties_away)):
            assert not np.all(X.same(wrong(s), X.to_bf16_rne(s))), (name, W, n)
            assert not np.all(X.same_image(X.red_image(m, True, to_bf16=wrong), X.red_image(m, True), True)), (name, W, n)
            seen[name] += 1
    assert seen["trunc"] == seen["away"] == len(X.CASES) == 70 and seen["reverse"] == 54 and seen["ceil"] > 40, seen
    for n in X.RCCL_N:  # hx_rccl_allreduce_bf16 at world 1
        t = X.messages(1, n, X.case_seed(1, n))[0]
        assert not np.all(X.same(X.to_bf16_trunc(t), X.to_bf16_rne(t))) and not np.all(X.same(X.to_bf16_ties_away(t), X.to_bf16_rne(t)))


M = 0xFFFFFFFE
COUNTS = sorted(set(range(1, 6)) | {k * M + d for k in (1, 2, 3) for d in range(-3, 5)})


def test_epoch_words_are_never_reserved_and_stay_close_across_the_wrap():
    from hirl4ucav_amd.agents.exchange import epoch_word

    def int32(v):
        v &= 0xFFFFFFFF
        return v - (1 << 32) if v & 0x80000000 else v

    assert [epoch_word(c) for c in (1, 2, M, M + 1, 2 * M, 2 * M + 1)] == [1, 2, M, 1, M, 1]
    for c in COUNTS:
        w, nxt = epoch_word(c), epoch_word(c + 1)
        assert 0 < w < 0xFFFFFFFF and w == int(w)
        assert 0 < int32(nxt - w) <= 3, (c, w, nxt)       # the kernels' (int)(flag - epoch) >= 0 with a peer one exchange ahead ...
        assert int32(w - nxt) < 0                         # ... and the rank ahead keeps waiting for the one behind
        assert (c & 1) != ((c + 1) & 1)
    with pytest.raises(ValueError):
        epoch_word(0)


@pytest.mark.parametrize("two_stage", [False, True])
def test_oneshot_exchange_passes_the_epoch_word_and_keeps_the_counters_parity(two_stage, monkeypatch):
    """OneShotExchange.allreduce across the wrap, the library call recorded instead of made: the flag word is epoch_word(count), the buffer the parity of
    the unbounded count — two consecutive exchanges never take the same buffer — and write_buffer() names the buffer the next exchange reads"""
    from hirl4ucav_amd.agents import exchange as E

    calls = []
    monkeypatch.setattr(E._lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(E._lib, "stream_ptr", lambda: None)

    class Reduced:
        def data_ptr(self):
            return 0

    x = object.__new__(E.OneShotExchange)
    x.two_stage, x.bf16, x.world, x.rank, x.timeout_ms, x.status_ptr = two_stage, False, 2, 0, 200, 0
    x.n, x.reduced, x.flags, x.flags2, x.reds = {"g": 1024}, {"g": Reduced()}, {"g": "f"}, {"g": "f2"}, {"g": "r"}
    x.bufs, x.own = {("g", 0): "buf0", ("g", 1): "buf1"}, {("g", 0): "own0", ("g", 1): "own1"}
    for start in (0, M - 3, 2 * M - 3):
        x.epoch = {"g": start}
        last = None
        for c in range(start + 1, start + 8):
            del calls[:]
            assert x.write_buffer("g") == "own%d" % (c & 1)
            x.allreduce("g")
            (name, a), = calls
            assert name == ("hx_allreduce_twostage" if two_stage else "hx_allreduce_oneshot")
            buf, word = a[1], a[9 if two_stage else 7]
            assert word == E.epoch_word(c) and 0 < word < 0xFFFFFFFF and buf == "buf%d" % (c & 1) and buf != last
            last = buf
