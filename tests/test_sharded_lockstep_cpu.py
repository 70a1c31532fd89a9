"""The count words of the merged actor message (include/hirl4ucav.h hx_hirl_actor_wgrad_split; numpy model in tests/_sharded_lockstep.py) without a GPU:
the soft count travels as base-32 digits so that every partial sum over up to 8 ranks stays within 256 — exact in bf16 in ANY order of summation —
while the count word itself does not survive a bf16 transport."""
import itertools
import os
import re

import numpy as np
import torch

from tests import _sharded_lockstep as LS
from tests import _xchg_model as X

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WORLD = X.MAX_WORLD  # kMaxWorld of hx_xchg.hip


def bf16_sum(words, order):
    """[W, k] fp32 -> [k]: every rank's words cast to bf16 (what hx_rccl_allreduce_bf16 puts on the wire), then added one rank at a time in `order`, every
    partial sum rounded to bf16 (torch's bf16 add) — a chain; trees are covered by bf16_tree_sum"""
    t = torch.from_numpy(np.ascontiguousarray(words)).to(torch.bfloat16)
    s = t[order[0]].clone()
    for r in order[1:]:
        s = s + t[r]
    return s.float().numpy()


def bf16_tree_sum(words, order):
    """the same ranks added pairwise (a reduction tree over `order`), every node rounded to bf16"""
    nodes = [torch.from_numpy(np.ascontiguousarray(words[r])).to(torch.bfloat16) for r in order]
    while len(nodes) > 1:
        nodes = [nodes[i] + nodes[i + 1] if i + 1 < len(nodes) else nodes[i] for i in range(0, len(nodes), 2)]
    return nodes[0].float().numpy()


def test_digit_words_round_trip():
    for c in (0, 1, 31, 32, 255, 256, 257, 1023, 1024, 65535, (1 << 31) - 1):
        w = LS.count_words(c)
        assert w.shape == (1 + LS.COUNT_DIGITS,) and w[0] == np.float32(c) and w[1:].max() <= 31 and LS.count_from_words(w) == c
    assert 32 ** LS.COUNT_DIGITS >= 1 << 31  # every non-negative int32 count has its digits


def test_every_partial_sum_of_digit_words_is_exact_in_bf16():
    """31 x 8 = 248 <= 256 = the last integer below which bf16 holds every integer"""
    assert 31 * MAX_WORLD <= 256
    ints = torch.arange(0, 257, dtype=torch.float32)
    assert torch.equal(ints.to(torch.bfloat16).float(), ints) and float(torch.tensor(257.0).to(torch.bfloat16)) != 257.0


def test_global_count_survives_bf16_sums_in_shuffled_orders():
    """per-rank counts up to the headline's 128 rows, up to 2^20 and up to int32's end; worlds 1..8; chains in shuffled rank orders and pairwise trees: the
    count rebuilt from the bf16-summed digit words is the integer sum, every time — and so is the fp32 rank-order sum's and its bf16 image (what
    twostage-bf16 delivers: ONE rounding of the fp32 sum)"""
    rng = np.random.default_rng(3)
    for W in range(1, MAX_WORLD + 1):
        for top in (128, 1 << 20, (1 << 31) - 1):
            for trial in range(12):
                counts = rng.integers(0, top + 1, W)
                if trial == 0:
                    counts[:] = top  # every rank at the top: the largest digit sums
                words = np.stack([LS.count_words(c) for c in counts])
                total = int(counts.astype(np.int64).sum())
                for _ in range(4):
                    order = list(rng.permutation(W))
                    assert LS.count_from_words(bf16_sum(words, order)) == total, (W, counts, order)
                    assert LS.count_from_words(bf16_tree_sum(words, order)) == total, (W, counts, order)
                s = X.rank_order_sum(words)
                assert LS.count_from_words(s) == total and LS.count_from_words(X.to_bf16_rne(s)) == total


def test_the_count_word_alone_does_not_survive_bf16():
    """why nothing computes with tail word 0: eight ranks of 128 rows reach 1,024, and bf16 keeps 8 bits"""
    counts = (120, 127, 1, 128, 77, 64, 33, 15)
    words = np.stack([LS.count_words(c) for c in counts])
    assert sum(counts) == 565
    assert X.to_bf16_rne(X.rank_order_sum(words))[0] != 565.0          # twostage-bf16: the fp32 sum, rounded once
    assert bf16_sum(words, list(range(8)))[0] != 565.0                 # rccl-bf16: summed in bf16
    assert float(X.to_bf16_rne(np.float32([1023.0]))[0]) == 1024.0     # and with one rank: the cast alone
    seen = {float(bf16_sum(words, list(p))[0]) for p in itertools.islice(itertools.permutations(range(8)), 0, 5040, 97)}
    assert 565.0 not in seen


def test_soft_weight_model_rounds_once():
    """LS.soft_weight_f32 = ONE rounding of count * float32(1 / batch) + warm, clipped at 1: equal to the two-rounding form wherever that is exact, and
    different from it somewhere (otherwise the GPU test could not tell the two)"""
    assert LS.soft_weight_f32(0, 1024, 0.0) == 0 and LS.soft_weight_f32(1024, 1024, 0.0) == 1 and LS.soft_weight_f32(1023, 1024, 0.05) == 1
    assert LS.soft_weight_f32(513, 1024, 0.0) == np.float32(513.0 / 1024.0)
    two = lambda c, b, w: min(np.float32(np.float32(np.float32(c) * (np.float32(1.0) / np.float32(b))) + np.float32(w)), np.float32(1.0))  # noqa: E731
    diff = [(c, b) for b in (48, 96, 144, 384) for c in range(1, b) if LS.soft_weight_f32(c, b, 0.05) != two(c, b, 0.05)]
    assert diff and all(abs(float(LS.soft_weight_f32(c, b, 0.05)) - float(two(c, b, 0.05))) < 1.2e-7 for c, b in diff)


def test_abi_version_names_the_message_change():
    hdr = open(os.path.join(REPO, "include", "hirl4ucav.h")).read()
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 124 and "124: the merged actor message" in hdr
    src = open(os.path.join(REPO, "hirl4ucav_amd", "csrc", "hx_update.h")).read()
    assert int(re.search(r"constexpr int kCountDigits = (\d+);", src).group(1)) == LS.COUNT_DIGITS
