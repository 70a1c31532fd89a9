"""Seeded inputs of the bf16 update's ragged-batch cases, shared by tests/test_bf16_ragged_cpu.py (are the bf16 bars FAIR at these batches, i.e. does
fp32 accumulation in the kernel's grouping itself stay within them of the fp64 sums, and do they still REJECT a wrong batch tail?) and
tests/test_bf16_ragged_gpu.py (the engine against the rounded-operand oracle).  Networks D.make_params(11), tables D.make_data(12, outliers=True):
those of tests/test_hirl_gpu.py::test_learn_ragged_batches_and_outlier_rows (rows with the +600 kill bonus, 100x TD errors).

Cases (every call's minibatch indices, BC-table indices and smoothing noise are a function of (case, B) alone):
  soft     HIRL, bc_weight_now = 100 (the soft estimate) with warm-up weight 0.1, four calls (two actor calls); also the inputs of the staged path
  expert   the same with the last B - n_main rows drawn from the expert ring
  td3      LeakyReLU 0.01, no BC, four calls
  bc       BC pre-training (bc_train_actor), three steps
Every minibatch holds a done = 1 row at index 0 and a done = 0 row at index 1.

The CPU stand-ins for a correct kernel (KernelSums: fp32 accumulation in the kernels' grouping; KernelSumsNearMisses: the same, with every operand
on the edge of a bf16 rounding boundary rounded the other way) and the capture of the rounded operands (Captured) live here too: they replace
hirl_oracle._RoundedLinear2 for the time of a `with`, so that Bf16Layer2 and tests/test_sac_bf16_gpu.RoundedSac pick them up unchanged."""
import numpy as np
import torch

from oracle import hirl_oracle as H
from tests import _hirl_data as D

PARAM_SEED, DATA_SEED = 11, 12
# hx_wgrad.hip, the bf16 branch of wgrad_kernel: dW2 contracts over the batch rows, 32 per MFMA; a wave pair splits the rows at
# hr = ((B + 7) >> 3) << 2 and each wave walks its half in 64-row chunks of two MFMAs; rows past the half's end are loaded clamped and zeroed.
BATCHES = (
    16,   # hr = 8: each half is a quarter of ONE MFMA, 24 of its 32 rows are tail
    48,   # hr = 24: half 1 starts at row 24, inside what would be MFMA 0's row range; MFMA 1 of either half is all tail
    144,  # hr = 72: one full 64-row chunk, then 8 rows
    272,  # hr = 136: two full chunks, then 8 rows — and the batch crosses kWgRowChunk = 256, the rows whose scalars the layer-1 and head jobs stage at a time
)
N_MAIN = {("expert", 48): 32, ("expert", 144): 80}
HIRL_CASES = [("soft", B) for B in BATCHES] + [("expert", 48), ("expert", 144), ("td3", 48), ("td3", 272), ("bc", 16), ("bc", 144)]
STAGED_BATCHES = (48, 272)     # the staged path runs the inputs of ("soft", B)
SAC_BATCHES = (16, 144, 272)   # tests/_sac_edges.py case "ragged"
N_CALLS = {"soft": 4, "expert": 4, "td3": 4, "bc": 3}
# seeds of the draws: SEED[case] + B + 10000 x (the number of seeds REJECTED for that (case, B)).  A seed is rejected when a CPU stand-in for a
# correct kernel (tests/test_bf16_ragged_cpu.py) misses a bar on its inputs, never for what the engine gives.  Rejected, all by the
# KernelSumsNearMisses stand-in (the plain fp32 sums passed everywhere) and all on TIGHT's 99.8 % share:
#   ("soft", 16)    seed 1016   call 2, actor gradient: 0.24 % of full1.weight outside TIGHT.  (The engine missed on the same call: one h1 element
#                               of actor(s_bc) and one of actor(s) rounded the other way, 0.47 % of full2.weight outside TIGHT, 0.50 x LOOSE —
#                               one row is 1/16 of this batch, not 1/128.)
#   ("expert", 144) seed 2144   call 3, critic gradient: 3 of the 256 entries of layernorm3.weight outside TIGHT (one miss is 0.39 % of such a tensor)
#                   seed 12144  call 0, critic gradient: 0.53 % of full3.weight outside TIGHT
SEED = {"soft": 1000, "expert": 2000, "td3": 3000, "bc": 4000}
REJECTED = {("soft", 16): 1, ("expert", 144): 2}
SOFT, WARM = 100, 0.1

_cache = {}


def params():
    if "params" not in _cache:
        _cache["params"] = D.make_params(PARAM_SEED)
    return _cache["params"]


def data():
    if "data" not in _cache:
        _cache["data"] = D.make_data(DATA_SEED, outliers=True)
    return _cache["data"]


def n_main(case, B):
    return N_MAIN.get((case, B), B)


def calls(case, B):
    """-> N_CALLS[case] x (idx int32 [B]: n_main(case, B) replay rows, then expert-ring rows; idx_bc int32 [B]; noise float32 [4])"""
    d, rng = data(), np.random.default_rng(SEED[case] + B + 10000 * REJECTED.get((case, B), 0))
    done, live = np.flatnonzero(d["replay"][:, 31] == 1), np.flatnonzero(d["replay"][:, 31] == 0)
    nm, out = n_main(case, B), []
    for k in range(N_CALLS[case]):
        idx = np.concatenate([rng.integers(0, D.N_REPLAY, nm), rng.integers(0, D.N_EXPERT_ROWS, B - nm)]).astype(np.int32)
        idx[0], idx[1] = done[k], live[k]
        out.append((idx, rng.integers(0, D.N_EXPERT, B).astype(np.int32), rng.normal(0, 0.2, 4).astype(np.float32)))
    return out


def batch_of(case, B, idx):
    """the oracle's (s, a, s', r, d) of a minibatch"""
    d, nm = data(), n_main(case, B)
    rows = np.concatenate([d["replay"][idx[:nm]], d["expert_rows"][idx[nm:]]], 0)
    return rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]


def bc_batch_of(idx_bc):
    d = data()
    return d["expert_s"][idx_bc], d["expert_a"][idx_bc]


def new_oracle(case):
    p = params()
    if case == "td3":
        return H.HirlOracle(p["actor"], p["critic"], None, slope=0.01, use_bc=False)
    o = H.HirlOracle(p["actor"], p["critic"], p["bc_actor"], slope=0.01 if case == "bc" else 0.0)
    o.split_actor_grads = True
    return o


# ---- stand-ins for hirl_oracle._RoundedLinear2 -----------------------------------------------------------------------------------------------------

def _f32_slabs(a, b, width=32):
    """a b^T of bf16-valued fp32 matrices (every product exact in fp32), the contraction index in slabs of `width` (one bf16 MFMA's k), each slab
    an fp32 matmul, the slabs added in fp32 in order"""
    acc = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32)
    for k0 in range(0, a.shape[1], width):
        acc = acc + a[:, k0:k0 + width] @ b[:, k0:k0 + width].t()
    return acc


def half_rows(B):
    """rows per half of the weight-gradient kernel's wave pair (hx_wgrad.hip)"""
    return ((B + 7) >> 3) << 2


class KernelSums(torch.autograd.Function):
    """_RoundedLinear2 with the kernels' fp32 accumulation in the place of the fp64 sums: z2 and dh1 in 32-wide slabs of their contraction index;
    dW2 = (rows [0, hr) in 32-row groups) + (rows [hr, B) in 32-row groups), hr = half_rows(B), every partial sum and the final one fp32."""

    @staticmethod
    def forward(ctx, h, w, b):
        hb, wb = h.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
        ctx.save_for_backward(hb, wb)
        return _f32_slabs(hb, wb) + b

    @staticmethod
    def backward(ctx, g):
        hb, wb = ctx.saved_tensors
        gb = g.to(torch.bfloat16).float()
        hr = half_rows(g.shape[0])
        dw = _f32_slabs(gb[:hr].t().contiguous(), hb[:hr].t().contiguous()) + _f32_slabs(gb[hr:].t().contiguous(), hb[hr:].t().contiguous())
        return _f32_slabs(gb, wb.t().contiguous()), dw, g.sum(0)


def round_bf16_other_way(x, eps):
    """bf16(x) as fp32 — except that an element within `eps` (absolute, broadcast against x) of the midpoint between its two bf16 neighbours
    goes to the neighbour round-to-nearest does NOT choose: the operand another correct fp32 evaluation of x, off by up to eps, may round to"""
    bits = x.contiguous().view(torch.int32)
    down_bits = bits & -65536                                 # towards zero
    down, up = down_bits.view(torch.float32), (down_bits + 65536).view(torch.float32)
    mid = (down_bits | 32768).view(torch.float32)
    rne = x.to(torch.bfloat16).float()
    near = ((x - mid).abs() <= eps) & (x != 0)
    return torch.where(near, torch.where(rne == down, up, down), rne)


ULP1 = 2.0 ** -23  # one fp32 ulp of 1.0


class KernelSumsNearMisses(torch.autograd.Function):
    """KernelSums, and every operand the kernel rounds to bf16 itself that sits on the edge of a rounding boundary rounded the OTHER way.  The
    kernels' fp32 h1 and dz2 are correct but not torch's bits: h1 = act(LayerNorm(.)) is O(1), so two fp32 evaluations differ by about one ulp of
    1.0 (2^-23, absolute); dz2 comes out of the LayerNorm backward, whose subtractions are of the size of the row's largest entries, so by about
    2^-23 of the row's max |dz2|.  An element closer than that to the midpoint of its bf16 neighbours may be rounded either way by a correct
    kernel (tests/test_bf16_update_gpu.py counts about one such element in 2 x 10^4 at B = 128), and all of its row's later values move with it.
    Here ALL such elements go the other way at once."""

    @staticmethod
    def forward(ctx, h, w, b):
        hb, wb = round_bf16_other_way(h, ULP1), w.to(torch.bfloat16).float()
        ctx.save_for_backward(hb, wb)
        return _f32_slabs(hb, wb) + b

    @staticmethod
    def backward(ctx, g):
        hb, wb = ctx.saved_tensors
        gb = round_bf16_other_way(g, ULP1 * g.abs().amax(1, keepdim=True))
        hr = half_rows(g.shape[0])
        dw = _f32_slabs(gb[:hr].t().contiguous(), hb[:hr].t().contiguous()) + _f32_slabs(gb[hr:].t().contiguous(), hb[hr:].t().contiguous())
        return _f32_slabs(gb, wb.t().contiguous()), dw, g.sum(0)


class Captured:
    """`with Captured() as log:` _RoundedLinear2 unchanged, and every backward appends (data_ptr of W2, bf16(dz2) [B, 512], bf16(h1) [B, 256]) in fp64"""

    def __enter__(self):
        log, orig = [], H._RoundedLinear2

        class Capture(orig):
            @staticmethod
            def forward(ctx, h, w, b):
                ctx.w_ptr = w.data_ptr()
                return orig.forward(ctx, h, w, b)

            @staticmethod
            def backward(ctx, g):
                log.append((ctx.w_ptr, g.to(torch.bfloat16).double(), ctx.saved_tensors[0]))
                return orig.backward(ctx, g)

        self._swap = Swapped(Capture)
        self._swap.__enter__()
        return log

    def __exit__(self, *exc):
        self._swap.__exit__(*exc)


class Swapped:
    """`with Swapped(cls):` hirl_oracle._RoundedLinear2 is `cls`"""

    def __init__(self, cls):
        self.cls = cls

    def __enter__(self):
        self._orig = H._RoundedLinear2
        H._RoundedLinear2 = self.cls
        return self

    def __exit__(self, *exc):
        H._RoundedLinear2 = self._orig


class RecordedMasks:
    """`with RecordedMasks() as masks:` masks[c] = (pre-activation > 0) of activation call c of the oracle module `mod` (its _act calls, in order)"""

    def __init__(self, mod=H):
        self.mod = mod

    def __enter__(self):
        self._orig, masks = self.mod._act, {}

        def act(x, slope=0.0):
            masks[len(masks)] = (x > 0).detach().clone()
            return self._orig(x, slope)

        self.mod._act = act
        return masks

    def __exit__(self, *exc):
        self.mod._act = self._orig


def learn_mask_calls(was_actor_call, soft, use_bc=True):
    """the activation calls of HirlOracle.learn for which tests/test_bf16_update_gpu.learn_masks hands the kernel's masks to the oracle"""
    c = [6, 7, 8, 9]
    if was_actor_call:
        c += [10, 11, 12, 13]
        if use_bc:
            c += [18, 19] if soft else [14, 15]
    return c
