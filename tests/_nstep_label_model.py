"""numpy model of the n-step relabelling of a labelled expert table (include/hirl4ucav.h "n-step returns for a labelled expert table", hx_nstep_label):
the same fp32 arithmetic in the same order, row by row, and a seeded table maker whose segments cover every length the kernel can get wrong."""
import numpy as np

W_S2, W_R, W_D = 17, 30, 31


def segment_ends(last):
    """per row j: the index of the final row of j's segment (the table's last row ends one whatever its byte says: the kernel never reads past E)"""
    last = np.asarray(last).reshape(-1) != 0
    E = last.size
    end = np.empty(E, np.int64)
    e = E - 1
    for j in range(E - 1, -1, -1):
        if last[j]:
            e = j
        end[j] = e
    return end


def steps_of(last, n):
    """m per row: min(n, rows from j to the end of j's segment, inclusive)"""
    end = segment_ends(last)
    return np.minimum(int(n), end - np.arange(end.size) + 1)


def relabel(rows, last, n, gamma):
    """-> rows_out [E, 32] float32: per row j, acc = 0; boot = 1; for k < m: w = k == 0 ? 1 : boot * gamma; acc = acc + w * r[j + k]; boot = w"""
    rows = np.asarray(rows, np.float32).reshape(-1, 32)
    g, one = np.float32(gamma), np.float32(1.0)
    m = steps_of(last, n)
    out = rows.copy()
    for j in range(rows.shape[0]):
        acc, boot = np.float32(0.0), one
        for k in range(int(m[j])):
            w = one if k == 0 else np.float32(boot * g)
            acc = np.float32(acc + np.float32(w * rows[j + k, W_R]))
            boot = w
        e = j + int(m[j]) - 1
        out[j, W_S2:W_R] = rows[e, W_S2:W_R]
        out[j, W_R] = acc
        out[j, W_D] = one if rows[e, W_D] != 0 else np.float32(one - boot)
    return out


def segment_lengths(n, E):
    """the seeded table's segments: 1, 2, n - 1, n, n + 1, a filler that ends exactly at row 63, a segment of one row that ends exactly at row 64, 70 rows
    (longer than a workgroup), then a cycle of short ones up to E; the final segment is cut at E"""
    head = [k for k in (1, 2, n - 1, n, n + 1) if k >= 1]
    lens = head + [64 - sum(head), 1, 70]
    cycle = [n + 1, 2, n, 1, 3, max(n - 1, 1), 5]
    i = 0
    while sum(lens) < E:
        lens.append(cycle[i % len(cycle)])
        i += 1
    out, left = [], E
    for k in lens:
        if left <= 0:
            break
        out.append(min(k, left))
        left -= out[-1]
    return out


def make_table(n, E=300, seed=0):
    """-> rows [E, 32], last [E] uint8, segs: per segment (first row, length, ends with done).  Within a segment row j + 1 starts where row j ended;
    rewards are finite and negative but for the +600 on every second terminal row; every third segment, and the final one, ends WITHOUT done (a file's end,
    a gap)."""
    rng = np.random.default_rng([n, E, seed])
    rows = np.zeros((E, 32), np.float32)
    last = np.zeros(E, np.uint8)
    segs, j = [], 0
    lens = segment_lengths(n, E)
    for i, k in enumerate(lens):
        s = rng.normal(size=13).astype(np.float32)
        terminal = i % 3 != 2 and i != len(lens) - 1
        for t in range(k):
            s2 = rng.normal(size=13).astype(np.float32)
            rows[j + t, 0:13], rows[j + t, 13:17], rows[j + t, W_S2:W_R] = s, rng.uniform(-1, 1, 4).astype(np.float32), s2
            rows[j + t, W_R] = np.float32(rng.uniform(-2.0, -0.01))
            s = s2
        if terminal:
            rows[j + k - 1, W_D] = 1.0
            if i % 2 == 0:
                rows[j + k - 1, W_R] = np.float32(600.0) + rows[j + k - 1, W_R]  # the kill step: the rare +600 on top of the shaping term
        last[j + k - 1] = 1
        segs.append((j, k, terminal))
        j += k
    assert j == E
    return rows, last, segs
