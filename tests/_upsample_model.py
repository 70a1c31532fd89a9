"""Success upsampling in numpy and Python integers (include/hirl4ucav.h "Success upsampling"): the counts per block of 1,024 slots, W, the target
t = (word W) >> 64, the slot from the cumulative integer weights, the BC minibatch's fire row, Philox4x32-10 as the kernels key it, and a seeded
generator of labels and words that covers the edges the tests name.  No GPU, no library."""
import numpy as np

BLOCK = 1024
MASK64 = (1 << 64) - 1
UPS_STREAM, UPS_FIRE_ROW = 0x55505331, 0xFFFFFFF1


def live_len(total, cap):
    return min(int(total), int(cap))


def slot_weights(labels, total, cap, boost):
    """explicit per-slot integer weights [cap]: boost for a live label == 1, 1 for any other live slot, 0 beyond the live length"""
    labels = np.asarray(labels)
    n = live_len(total, cap)
    w = np.zeros(int(cap), np.int64)
    w[:n] = np.where(labels[:n] == 1, int(boost), 1)
    return w


def counts(labels, total, cap):
    """cnt[ceil(cap / 1024)]: live slots per block whose label is exactly 1"""
    labels = np.asarray(labels)
    n = live_len(total, cap)
    nb = (int(cap) + BLOCK - 1) // BLOCK
    hit = np.zeros(nb * BLOCK, np.int64)
    hit[:n] = labels[:n] == 1
    return hit.reshape(nb, BLOCK).sum(1).astype(np.uint32)


def touched_blocks(marked, total, cap, max_new):
    """-> (blocks recounted by mark_new, the new marked): the blocks holding slots of [marked, marked + len) mod cap, len = min(total - marked, max_new);
    len >= cap: every block and marked = total"""
    marked, total, cap = int(marked), int(total), int(cap)
    nb = (cap + BLOCK - 1) // BLOCK
    ln = min(max(total - marked, 0), int(max_new))
    if ln >= cap:
        return list(range(nb)), total
    return sorted({((marked + i) % cap) // BLOCK for i in range(ln)}), marked + ln


def mark_new(cnt, marked, labels, total, cap, max_new):
    """the state after hx_ups_mark_new: only the touched blocks are recounted (from the labels and the live length as they are NOW)"""
    blocks, new_marked = touched_blocks(marked, total, cap, max_new)
    fresh = counts(labels, total, cap)
    out = np.array(cnt, np.uint32, copy=True)
    out[blocks] = fresh[blocks]
    return out, new_marked


def weight_total(cnt, total, cap, boost):
    return live_len(total, cap) + (int(boost) - 1) * int(np.asarray(cnt, np.int64).sum())


def target(word, W):
    return (int(word) * int(W)) >> 64


def draw_slots(labels, cnt, total, cap, boost, words):
    """idx of every word: the block from the cumulative block weights live_in_block + (boost - 1) cnt, the slot from the block's labels.  With
    consistent counts this is the slot whose interval of the running per-slot weight holds t; a target past the end of its block's labels (stale
    counts) resolves to the block's last live slot; W == 0: slot 0."""
    labels = np.asarray(labels)
    n, cap, boost = live_len(total, cap), int(cap), int(boost)
    nb = (cap + BLOCK - 1) // BLOCK
    live = [min(max(n - b * BLOCK, 0), BLOCK) for b in range(nb)]
    bw = [live[b] + (boost - 1) * int(cnt[b]) for b in range(nb)]
    W = sum(bw)
    out = []
    for word in words:
        if W == 0:
            out.append(0)
            continue
        t = target(word, W)
        b = 0
        while t >= bw[b]:
            t -= bw[b]
            b += 1
        slot, c = None, 0
        for j in range(live[b]):
            c += boost if labels[b * BLOCK + j] == 1 else 1
            if c > t:
                slot = j
                break
        if slot is None:
            slot = live[b] - 1 if live[b] > 0 else 0
        out.append(min(b * BLOCK + slot, cap - 1))
    return np.array(out, np.int32)


def brute_slots(labels, total, cap, boost, words):
    """the same draw from explicit per-slot weights and ONE cumulative sum over the whole ring (no blocks, no counts)"""
    w = slot_weights(labels, total, cap, boost)
    cum = np.cumsum(w)
    W = int(cum[-1]) if len(cum) else 0
    return np.array([0 if W == 0 else int(np.searchsorted(cum, target(x, W), side="right")) for x in words], np.int32)


def slot_interval(labels, total, cap, boost, slot):
    """[first, last] target of a live slot"""
    w = slot_weights(labels, total, cap, boost)
    lo = int(w[:slot].sum())
    return lo, lo + int(w[slot]) - 1


def word_for_target(t, W):
    """the smallest 64-bit word whose target is t: ceil(t 2^64 / W)"""
    x = -((-int(t) << 64) // int(W))
    assert 0 <= x <= MASK64 and target(x, W) == t
    return x


def fire_replacement(w0, w1, n_fire, batch):
    """-> (j, k): idx_bc[k] <- fire_idx[j]"""
    return (int(w0) * int(n_fire)) >> 64, (int(w1) * int(batch)) >> 64


def philox4x32_10(c, k):
    c0, c1, c2, c3 = (int(v) & 0xFFFFFFFF for v in c)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_words(seed, call, n_main, fire=False):
    """the words hx_ups_draw takes with x = NULL: one per row, then the fire row's two"""
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    out = []
    for r in range(n_main):
        p = philox4x32_10((r, call, UPS_STREAM, 0), key)
        out.append((p[0] << 32) | p[1])
    if fire:
        p = philox4x32_10((UPS_FIRE_ROW, call, UPS_STREAM, 0), key)
        out += [(p[0] << 32) | p[1], (p[2] << 32) | p[3]]
    return out


def words_tensor(words):
    """64-bit words as the int64 array the binding hands over (two's complement)"""
    return np.array([w - (1 << 64) if w >= (1 << 63) else w for w in words], np.int64)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "last_live", "beyond_live", "boundaries", "mixed")


def make_labels(pattern, cap, live, seed=0):
    """labels [cap] int8 for a live length `live`.  none: no success row (the draw is the plain uniform one); all: every row a success; last_live:
    one success in the last live slot; beyond_live: labels 1 only at or beyond the live length; boundaries: successes on both sides of every block
    boundary (and at slot 0 / the last live slot); mixed: -1, 0 and 1 mixed by a seeded generator, stale 1s beyond the live length too"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(cap, np.int8)
    if pattern == "none":
        lab[:] = rng.choice(np.array([-1, 0], np.int8), cap)
    elif pattern == "all":
        lab[:] = 1
    elif pattern == "last_live":
        lab[live - 1] = 1
    elif pattern == "beyond_live":
        lab[:live] = rng.choice(np.array([-1, 0], np.int8), live)
        lab[live:] = 1
    elif pattern == "boundaries":
        for e in range(BLOCK, cap, BLOCK):
            lab[e - 1], lab[e] = 1, 1
        lab[0], lab[live - 1] = 1, 1
    elif pattern == "mixed":
        lab[:] = rng.choice(np.array([-1, 0, 0, 0, 1], np.int8), cap)
    else:
        raise ValueError(pattern)
    return lab


def make_words(labels, total, cap, boost, count, seed=0, every_slot=False):
    """`count` words: 0 and 2^64 - 1 first, then — as far as `count` reaches, all of them with every_slot — for the live slots in order the two words
    whose targets are the first and the last integer of the slot's interval, then seeded random words"""
    W = int(slot_weights(labels, total, cap, boost).sum())
    words = [0, MASK64]
    if W:
        n = live_len(total, cap)
        w = slot_weights(labels, total, cap, boost)
        lo = np.concatenate([[0], np.cumsum(w)[:-1]])
        slots = range(n) if every_slot else [s for s in (0, n - 1, n // 2) if 0 <= s < n]
        for s in slots:
            words += [word_for_target(int(lo[s]), W), word_for_target(int(lo[s] + w[s] - 1), W)]
    rng = np.random.default_rng(seed)
    if not every_slot:
        words = words[:count]
        words += [int(v) for v in rng.integers(0, 1 << 64, count - len(words), dtype=np.uint64)]
    return words
