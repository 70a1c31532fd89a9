"""The peer-read all-reduce kernels (hx_allreduce_oneshot, hx_allreduce_twostage and its bf16 form) and the bf16 cast pair of hx_rccl_allreduce_bf16
against the exact rank-order sum of tests/_xchg_model.py: every comparison in bits, NaN results by class.

All W "ranks" live in ONE process on ONE stream, and no wait ever spins: before each call every rank's flag word already holds that call's epoch (a
stream-ordered write).  The handshake between concurrent ranks stays the business of tests/test_sharded_gpu.py.  The reference has no exchange (one
process, hirl/agents/HIRL.py:52)."""
import ctypes

import numpy as np
import pytest

from tests import _xchg_model as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
TIMEOUT_MS = 200
PITCH = 16  # words between two ranks' flag (or status) words: a 64-byte line each


class Ranks:
    """flag, second-stage flag and status words of up to 8 ranks in fine-grained memory, as the kernels' pointer arrays and as one int32 tensor"""

    def __init__(self):
        from hirl4ucav_amd import _lib
        from hirl4ucav_amd.agents import exchange as E

        self.lib = _lib
        _lib.load()
        self.mem = VP()
        _lib.call("hx_ipc_alloc", 3 * X.MAX_WORLD * PITCH * 4, 1, ctypes.byref(self.mem))
        self.words = torch.as_tensor(E._DeviceWords(self.mem.value, 3 * X.MAX_WORLD * PITCH), device="cuda").view(torch.int32).view(3, X.MAX_WORLD, PITCH)

    def ptr(self, which, r):
        return self.mem.value + 4 * PITCH * (which * X.MAX_WORLD + r)

    def arrays(self, W):
        return [(VP * W)(*[self.ptr(which, r) for r in range(W)]) for which in (0, 1)]

    def zero(self):
        self.words.zero_()

    def announce(self, W, epoch, rank=None, peers=None):
        """both flag sets of every rank <- epoch (`peers`: what the ranks other than `rank` hold instead), on the stream"""
        as_i32 = lambda v: v - (1 << 32) if v & 0x80000000 else v  # noqa: E731
        self.words[0:2, :W, 0] = as_i32(epoch if peers is None else peers)
        if peers is not None:
            self.words[0:2, rank, 0] = as_i32(epoch)

    def assert_clean(self, W, what):
        torch.cuda.synchronize()
        assert self.words[2, :, 0].tolist() == [0] * X.MAX_WORLD, (what, "status words", self.words[2, :, 0].tolist())

    def free(self):
        torch.cuda.synchronize()
        del self.words
        self.lib.call("hx_ipc_free", self.mem)


@pytest.fixture(scope="module")
def ranks():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = Ranks()
    yield r
    r.free()


class Case:
    """one (W, n): the messages, dst with its guard floats and the red buffers on the device, the model's answers on the host"""

    def __init__(self, W, n, seed, messages=None):
        """messages: fp32 [W, n] to send instead of the seeded X.messages(W, n, seed)"""
        self.W, self.n = W, n
        self.host = X.messages(W, n, seed) if messages is None else np.ascontiguousarray(messages, np.float32)
        assert self.host.shape == (W, n)
        self.sum = X.rank_order_sum(self.host)
        self.msg = torch.from_numpy(self.host).cuda()
        self.dst = torch.full((W, n + X.GUARD), -7.0, dtype=torch.float32, device="cuda")
        self.red = torch.full((W, n), X.SENTINEL, dtype=torch.int32, device="cuda")
        self.bufs = (VP * W)(*[self.msg[r].data_ptr() for r in range(W)])
        self.reds = (VP * W)(*[self.red[r].data_ptr() for r in range(W)])

    def call(self, ranks, variant, r, epoch):
        flags, flags2 = ranks.arrays(self.W)
        if variant == "oneshot":
            ranks.lib.call("hx_allreduce_oneshot", self.dst[r].data_ptr(), self.bufs, flags, ranks.ptr(2, r), self.W, r, self.n, epoch, TIMEOUT_MS,
                           ranks.lib.stream_ptr())
        else:
            ranks.lib.call("hx_allreduce_twostage", self.dst[r].data_ptr(), self.bufs, self.reds, flags, flags2, ranks.ptr(2, r), self.W, r, self.n, epoch,
                           TIMEOUT_MS, int(variant == "twostage-bf16"), ranks.lib.stream_ptr())

    def check_red(self, variant):
        bf16 = variant == "twostage-bf16"
        got = self.red.cpu().numpy().view(np.uint32)
        ok = X.same_image(got, X.red_image(self.host, bf16), bf16)
        assert ok.all(), (variant, self.W, self.n, "red after pass A: first wrong (rank, word)", np.argwhere(~ok)[:4].tolist())

    def check_dst(self, variant):
        want = X.to_bf16_rne(self.sum) if variant == "twostage-bf16" else self.sum
        got = self.dst.cpu().numpy()
        assert np.all(got[:, self.n:] == -7.0), (variant, self.W, self.n, "guard floats written")
        for r in range(self.W):
            ok = X.same(got[r, :self.n], want)
            bad = np.flatnonzero(~ok)[:4]
            assert ok.all(), (variant, self.W, self.n, "rank", r, "columns", bad.tolist(), X.bits(got[r, bad]).tolist(), X.bits(want[bad]).tolist(),
                              [X.CLASSES[c] for c in X.column_class(self.n)[bad]])
            assert np.array_equal(X.bits(got[r, :self.n]), X.bits(got[0, :self.n])), (variant, self.W, self.n, "rank", r, "differs from rank 0")


def run_case(ranks, variant, W, n, seed, epoch=1, ahead=None, messages=None):
    """Every rank in turn.  Two-stage: one call launches both stages, so pass A leaves every red[r] slice written (checked: the partition itself) and
    pass B, one epoch later on the same messages, gives the dst to compare.  `ahead`: what the PEERS' flags hold at each call (a peer one exchange ahead).
    -> the Case (its dst rows hold every rank's result)"""
    c = Case(W, n, seed, messages)
    ranks.zero()
    passes = [epoch] if variant == "oneshot" else [epoch, epoch + 1]
    for k, e in enumerate(passes):
        for r in range(W):
            ranks.announce(W, e, r, None if ahead is None else ahead[k])
            c.call(ranks, variant, r, e)
        ranks.assert_clean(W, (variant, W, n, "pass", k))
        if variant != "oneshot" and k == 0:
            c.check_red(variant)
    c.check_dst(variant)
    return c


@pytest.mark.parametrize("variant", ["oneshot", "twostage", "twostage-bf16"])
def test_allreduce_equals_the_rank_order_sum_in_bits(ranks, variant):
    """70 (W, n) cases: W = 1..8 at n4 = 1, 2, 3, 5, 7 (empty slices, slices of one float4) and around one workgroup (n = 1020, 1024, 1028); W = 3, 5, 8
    across the 256-workgroup grid stride and at the engine's own length.  Status words 0 and guard floats intact after every case."""
    assert len(X.CASES) == 70
    for W, n in X.CASES:
        run_case(ranks, variant, W, n, X.case_seed(W, n))


@pytest.mark.parametrize("variant", ["oneshot", "twostage"])
def test_epoch_words_across_the_sign_change_and_the_wrap(ranks, variant):
    """the signed-distance comparison (int)(flag - epoch) >= 0 where it can go wrong: epoch 0x7FFFFFFF with the peer already at 0x80000000, 0x80000000
    itself, and the last word 0xFFFFFFFE with the peer already at 1 (exchange.epoch_word).  Two-stage needs a first pass to fill red: it runs at the word
    BEFORE each of these, with the peer at the word itself, so the compared pass is the one named here."""
    from hirl4ucav_amd.agents.exchange import epoch_word

    for k, (e, peer) in enumerate([(0x7FFFFFFF, 0x80000000), (0x80000000, None), (0xFFFFFFFE, 1)]):
        assert epoch_word(e) == e and (peer is None or peer == epoch_word(e + 1))
        if variant == "oneshot":
            run_case(ranks, variant, 2, 1024, 77 + k, epoch=e, ahead=None if peer is None else [peer])
        else:
            run_case(ranks, variant, 2, 1024, 77 + k, epoch=e - 1, ahead=None if peer is None else [e, peer])


def test_the_poison_value_is_refused_as_an_epoch(ranks):
    c = Case(2, 1024, 3)
    ranks.zero()
    for variant, name in (("oneshot", "hx_allreduce_oneshot"), ("twostage", "hx_allreduce_twostage")):
        with pytest.raises(ranks.lib.HxError, match=name + ": epoch 0xFFFFFFFF is reserved"):
            c.call(ranks, variant, 0, 0xFFFFFFFF)
    ranks.assert_clean(2, "refused epoch")
    assert torch.all(c.dst == -7.0) and ranks.words[0:2].abs().sum().item() == 0  # nothing was launched


def test_rccl_bf16_cast_pair_at_world_one():
    """hx_rccl_allreduce_bf16 with ONE rank: cast to bf16 (round to nearest even), ncclAllReduce of one rank, cast back — t must come back as
    to_bf16_rne(t) in bits; a length that is no multiple of 4 takes the fp32 path and comes back unchanged"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents.exchange import RcclDirect

    try:
        RcclDirect.available()
    except _lib.HxError as e:
        print("hx_rccl_available:", e)
        pytest.skip(f"RCCL cannot be bound in this process: {e}")
    comm = RcclDirect(RcclDirect.make_id(), 1, 0, bf16=True)
    try:
        for n in X.RCCL_N:
            host = X.messages(1, n, X.case_seed(1, n))[0]
            buf = torch.full((n + X.GUARD,), -7.0, dtype=torch.float32, device="cuda")
            buf[:n] = torch.from_numpy(host).cuda()
            comm.allreduce(buf[:n])
            torch.cuda.synchronize()
            got, want = buf.cpu().numpy(), X.to_bf16_rne(host)
            ok = X.same(got[:n], want)
            bad = np.flatnonzero(~ok)[:4]
            assert ok.all(), (n, bad.tolist(), X.bits(got[bad]).tolist(), X.bits(want[bad]).tolist(), [X.CLASSES[c] for c in X.column_class(n)[bad]])
            assert np.all(got[n:] == -7.0), (n, "guard floats written")
        host = X.messages(1, 28, 9)[0][[0, 2, 3, 7, 8, 12]]  # 6 elements: a normal, two bf16 ties, a denormal, an overflow, a NaN
        t = torch.from_numpy(host).cuda()
        comm.allreduce(t)
        torch.cuda.synchronize()
        assert np.all(X.same(t.cpu().numpy(), host))
    finally:
        comm.close()
