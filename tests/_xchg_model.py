"""The exact answer of the peer-read all-reduce kernels (hirl4ucav_amd/csrc/hx_xchg.hip) and of the bf16 cast pair of hx_rccl.hip, numpy only.

dst[i] = ((buf[0][i] + buf[1][i]) + ...) + buf[W-1][i] in plain fp32 adds has ONE right answer per bit (no fused operation is possible in a
chain of adds), and so has round-to-nearest-even to bf16: the GPU tests compare bits, NaN results by class.  tests/test_xchg_cpu.py holds this
model to fp64 and to torch's bf16 conversion, and shows that the comparison tells four wrong models from the right one."""
import numpy as np

MAX_WORLD = 8
SENTINEL = 0x7FA57FA5  # a signalling NaN with a payload, as fp32 AND in each bf16 half: no add and no conversion produces it
GUARD = 64             # floats behind dst that must stay untouched

CLASSES = ("normal", "cancel", "tie_even", "tie_odd", "zero_pos", "zero_neg", "zero_mixed", "denormal", "overflow", "inf_pos", "inf_neg",
           "inf_nan", "nan")
# (the first four columns — all a message of n = 4 has — are the ones the mutants of test_xchg_cpu.py need: an order-dependent sum, a bf16 tie
# with the kept bit even (ties away from zero differ) and one with it odd (truncation differs))


def column_class(n):
    """index into CLASSES of every column of messages(W, n, seed)"""
    return np.arange(n) % len(CLASSES)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def rank_order_sum(bufs, order=None):
    """fp32 [W, n] -> fp32 [n]: left to right in rank order, one elementwise fp32 add per rank (`order`: another order, for the mutants)"""
    bufs = np.asarray(bufs)
    assert bufs.dtype == np.float32 and bufs.ndim == 2
    order = range(bufs.shape[0]) if order is None else order
    with np.errstate(all="ignore"):
        s = None
        for r in order:
            s = bufs[r].copy() if s is None else (s + bufs[r]).astype(np.float32)
    return s


def slices(n4, W):
    """(lo, hi) per rank, in float4s: rank r reduces [n4 r / W, n4 (r + 1) / W)"""
    return [(n4 * r // W, n4 * (r + 1) // W) for r in range(W)]


def slices_ceil(n4, W):
    """the MUTANT partition: boundaries rounded up instead of down"""
    return [(-(-n4 * r // W), -(-n4 * (r + 1) // W)) for r in range(W)]


def owner(i, n4, W):
    """the rank whose slice holds float4 i"""
    for r, (lo, hi) in enumerate(slices(n4, W)):
        if lo <= i < hi:
            return r
    raise ValueError((i, n4, W))


def kernel_owner(n4, W):
    """what twostage_kernel's stage 2 computes for every float4 i < n4: (the start guess (i W + W - 1) / n4, the rank after its two correction loops)"""
    i = np.arange(n4, dtype=np.int64)
    start = (i * W + W - 1) // n4
    r = start.copy()
    while True:
        down = (r > 0) & (i < n4 * r // W)
        if not down.any():
            break
        r[down] -= 1
    while True:
        up = (r + 1 < W) & (i >= n4 * (r + 1) // W)
        if not up.any():
            break
        r[up] += 1
    return start, r


def to_bf16_rne(x):
    """fp32 -> bf16 bits -> fp32, round to nearest even, on the integer bits (NaN stays a quiet NaN of the same sign)"""
    b = bits(x).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (b & 0xFFFF0000) | 0x00400000, r)
    return from_bits(r.astype(np.uint32))


def to_bf16_trunc(x):
    """MUTANT: the low 16 bits dropped"""
    return from_bits(bits(x) & np.uint32(0xFFFF0000))


def to_bf16_ties_away(x):
    """MUTANT: round to nearest, ties away from zero"""
    b = bits(x).astype(np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (b & 0xFFFF0000) | 0x00400000, (b + 0x8000) & 0xFFFF0000)
    return from_bits(r.astype(np.uint32))


def same(got, want):
    """elementwise: NaN results compare as "is NaN", everything else as bits (so -0 != +0)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.where(np.isnan(want), np.isnan(got), bits(got) == bits(want))


def red_image(bufs, bf16=False, part=slices, to_bf16=to_bf16_rne):
    """The ranks' `red` buffers after stage 1 of hx_allreduce_twostage on buffers pre-filled with SENTINEL words: uint32 [W, n].  Rank r has
    written its slice of the sum — as fp32 at float4 i, or with bf16 as 8 bytes at uint2 i (the first 2 n bytes) — and nothing else."""
    W, n = bufs.shape
    s = rank_order_sum(bufs)
    img = np.full((W, n), SENTINEL, np.uint32)
    for r, (lo, hi) in enumerate(part(n // 4, W)):
        if bf16:
            half = img[r].view(np.uint16)
            half[4 * lo:4 * hi] = (bits(to_bf16(s[4 * lo:4 * hi])) >> 16).astype(np.uint16)
        else:
            img[r, 4 * lo:4 * hi] = bits(s[4 * lo:4 * hi])
    return img


def same_image(got, want, bf16=False):
    """red buffers as uint32 [W, n] against red_image: the same words written (everything else still SENTINEL), the written values by `same`"""
    got, want = np.ascontiguousarray(got, np.uint32), np.ascontiguousarray(want, np.uint32)
    if not bf16:
        return np.where(want == SENTINEL, got == SENTINEL, (got != SENTINEL) & same(from_bits(got), from_bits(want)))
    g, w = got.view(np.uint16), want.view(np.uint16)
    half = np.uint16(SENTINEL & 0xFFFF)
    val = same(from_bits(g.astype(np.uint32) << 16), from_bits(w.astype(np.uint32) << 16))
    return np.where(w == half, g == half, (g != half) & val)


def _wide(rng, shape):
    """normals over twelve decades, either sign"""
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 10.0, shape) * 10.0 ** rng.integers(-6, 6, shape)).astype(np.float32)


def _integer_parts(rng, total, W, spread, positive=False):
    """W integers that add up to `total` ([k] each), every partial sum far below 2^24: their fp32 sum is exact in any order"""
    k = total.shape[0]
    parts = rng.integers(0 if positive else -spread, spread + 1, (W, k))
    parts[0] = total - parts[1:].sum(0)
    return parts


def messages(W, n, seed):
    """The seeded inputs: fp32 [W, n], column j of class CLASSES[j % 13].  Where a class needs more ranks than there are (W = 1: no pair to
    cancel, no second infinity) the column keeps what W allows."""
    assert 1 <= W <= MAX_WORLD and n > 0
    rng = np.random.default_rng([int(seed), W, n])
    cls = column_class(n)
    out = np.zeros((W, n), np.float32)
    cols = {name: np.flatnonzero(cls == c) for c, name in enumerate(CLASSES)}

    j = cols["normal"]
    out[:, j] = _wide(rng, (W, j.size))

    j = cols["cancel"]  # rank 0: x, rank 1: -x, a later rank: 1e-8 x (below half an ulp of x), the others 0: left to right 1e-8 x, any other order not
    x = _wide(rng, j.size)
    out[0, j] = x
    if W >= 2:
        out[1, j] = -x
    if W >= 3:
        out[2 + np.arange(j.size) % (W - 2), j] = np.float32(1e-8) * x

    for name, low2 in (("tie_even", 1), ("tie_odd", 3)):  # the sum is M 2^e with M odd in [257, 511]: exactly between two bf16; kept bit = bit 1 of M
        j = cols[name]
        M = 256 + 4 * rng.integers(0, 64, j.size) + low2
        parts = _integer_parts(rng, M, W, 1000)
        scale = np.ldexp(rng.choice([-1.0, 1.0], j.size), rng.integers(-20, 21, j.size))
        out[:, j] = (parts * scale).astype(np.float32)

    out[:, cols["zero_neg"]] = -0.0
    j = cols["zero_mixed"]
    z = np.where(rng.integers(0, 2, (W, j.size)) == 1, -0.0, 0.0).astype(np.float32)
    z[0] = -0.0
    if W >= 2:
        z[1] = 0.0
    out[:, j] = z

    j = cols["denormal"]
    d = rng.integers(1, 0x800000, (W, j.size)).astype(np.uint32) | (rng.integers(0, 2, (W, j.size)).astype(np.uint32) << 31)
    out[:, j] = from_bits(d)

    j = cols["overflow"]  # M 2^104 with 2^24 - 2^15 <= M < 2^24: finite in fp32, at or above the tie over the largest finite bf16 (0x7F7F, odd) -> inf
    M = (1 << 24) - 1 - rng.integers(0, 1 << 15, j.size)
    if j.size:
        M[0] = (1 << 24) - (1 << 15)  # the tie itself
    parts = _integer_parts(rng, M, W, 1 << 20, positive=True)
    out[:, j] = (parts * np.ldexp(rng.choice([-1.0, 1.0], j.size), 104)).astype(np.float32)

    for name, vals in (("inf_pos", (np.inf,)), ("inf_neg", (-np.inf,)), ("inf_nan", (np.inf, -np.inf)), ("nan", (np.nan,))):
        j = cols[name]
        out[:, j] = _wide(rng, (W, j.size))
        a = np.arange(j.size) % W
        out[a, j] = vals[0]
        if len(vals) > 1 and W >= 2:
            out[(a + 1 + np.arange(j.size) // W % (W - 1)) % W, j] = vals[1]
    return out


# ---- the (W, n) cases of tests/test_xchg_gpu.py (kept here so that the CPU test holds the mutants to the same list) ----------------------------------
SMALL_N = (4, 8, 12, 20, 28)          # n4 = 1, 2, 3, 5, 7: empty slices, slices of one float4
BLOCK_N = (1020, 1024, 1028)          # around one 256-thread workgroup
STRIDE_N = 4 * (65536 + 5)            # crosses the 256-workgroup grid stride
ENGINE_N = 276488                     # the engine's critic message
CASES = [(W, n) for W in range(1, MAX_WORLD + 1) for n in SMALL_N + BLOCK_N] + [(W, n) for n in (STRIDE_N, ENGINE_N) for W in (3, 5, 8)]
RCCL_N = (4, 1020, 1024, 1028, ENGINE_N)


def case_seed(W, n):
    return 1000 * W + n % 997
