"""Checkers for priorities at insert (test infrastructure only; include/hirl4ucav.h "Priorities at insert").

score       — the reference's |Q1(s, a) - y| for stored rows with the networks as they stand (SAC/agent.py:198-210, 238-241), built from
              oracle.sac_oracle.sample and mlp, in fp32 or fp64.  Pinned by tests/test_per_score_cpu.py against the reference's recorded run.
ScoreModel  — tests/_per_check.PerModel with score_new(total, errors): the store rule of hx_per_score_new (this project's own definition, so the
              model IS its statement), the non-finite fallback, and the block sums in the device's fixed order, in fp32 bits."""
import numpy as np
import torch

from oracle import sac_oracle as S
from tests import _per_check as P


def score(params, targets, alpha, rows, eps, gamma=0.99, dtype=torch.float32):
    """errors [n] of the rows [n, 32] (s[13] a[4] s'[13] r d).  params: {"policy", "q1", "q2"} (only Q1 of the critics is used: agent.py:241),
    targets: {"q1", "q2"} the target critics, alpha: the entropy coefficient, eps [n, 4]: the draws of policy.sample(s')."""
    rows = np.asarray(rows)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)  # noqa: E731
    s, a, ns, r, d = t(rows[:, 0:13]), t(rows[:, 13:17]), t(rows[:, 17:30]), t(rows[:, 30:31]), t(rows[:, 31:32])
    pol, q1 = S.to_t(params["policy"], dtype=dtype), S.to_t(params["q1"], dtype=dtype)
    t1, t2 = S.to_t(targets["q1"], dtype=dtype), S.to_t(targets["q2"], dtype=dtype)
    with torch.no_grad():
        na, nh, _ = S.sample(pol, ns, t(eps))                                       # calc_target_q, agent.py:202-210
        nsa = torch.cat([ns, na], 1)
        next_q = torch.min(S.mlp(t1, nsa), S.mlp(t2, nsa)) + float(alpha) * nh
        y = r + (1.0 - d) * float(gamma) * next_q
        cur_q1 = S.mlp(q1, torch.cat([s, a], 1))                                   # calc_current_q, agent.py:198-200
        return torch.abs(cur_q1 - y).reshape(-1).numpy().copy()                     # agent.py:241


def assert_errors(got, params, targets, alpha, rows, eps, gamma=0.99, what="errors"):
    """`got` (fp32 arithmetic) against the fp64 evaluation of `score`, per row within
        5e-6 + 2e-5 |ref|                              the project's HIP-vs-checker bar for this quantity (tests/test_per_gpu.py)
      + gamma alpha sum_j 4 * 2^-24 / (1 - a'_j^2 + 1e-6)   what ONE fp32 evaluation of a' = tanh(x) costs the entropy H' = ... - log(1 - a'^2 + 1e-6):
    below 1 the fp32 grid is 2^-24 wide, tanhf is good to about an ulp, so 1 - a'^2 carries up to ~4 * 2^-24 of absolute error whatever computes it,
    and log turns that into 4 * 2^-24 / (1 - a'^2 + 1e-6).  The term is below 1e-6 unless an action saturates (|a'| > 0.9); where one does, fp32
    torch itself misses the plain bar against fp64 (3 of the first 2,064 table rows do, by up to 1.2e-4), so the plain bar cannot be asked of any
    fp32 evaluation there.  Rows whose reference is not finite are skipped (the caller checks them)."""
    ref = score(params, targets, alpha, rows, eps, gamma=gamma, dtype=torch.float64)
    with torch.no_grad():
        na, _, _ = S.sample(S.to_t(params["policy"], dtype=torch.float64), torch.as_tensor(np.asarray(rows)[:, 17:30], dtype=torch.float64),
                            torch.as_tensor(np.asarray(eps), dtype=torch.float64))
    cond = (4.0 * 2.0 ** -24 / (1.0 - na.numpy() ** 2 + 1e-6)).sum(1)
    d = 1.0 - np.asarray(rows, np.float64)[:, 31]
    tol = 5e-6 + 2e-5 * np.abs(ref) + np.abs(d) * float(gamma) * float(alpha) * cond
    ok = np.isfinite(ref)
    diff = np.abs(np.asarray(got, np.float64) - ref)
    bad = np.flatnonzero(ok & ~(diff <= tol))
    assert bad.size == 0, f"{what}: rows {bad[:8]} differ by {diff[bad[:8]]} (allowed {tol[bad[:8]]})"
    return ref


def block_sums_fixed(prio32):
    """the block sums of fp32 priorities [nblocks * 1024] in the order of resum_block (hx_per.hip), every add in fp32: thread t of 256 holds slots
    4 t .. 4 t + 3 as (x + y) + (z + w); in each 16-lane row the quads Q_k = (p0 + p1) + (p2 + p3), the row (Q0 + Q3) + (Q2 + Q1) (two quad
    permutes, then rotations by 4 and by 8 lanes, read at lane 0); the wave (r0 + r1) + (r2 + r3); the block (w0 + w1) + (w2 + w3)"""
    f = np.float32
    v = np.asarray(prio32, f).reshape(-1, 256, 4)
    p = (v[:, :, 0] + v[:, :, 1]).astype(f) + (v[:, :, 2] + v[:, :, 3]).astype(f)   # [nb, 256]
    p = p.astype(f).reshape(-1, 4, 4, 4, 4)                                        # block, wave, row, quad, lane
    q = (p[..., 0] + p[..., 1]).astype(f) + (p[..., 2] + p[..., 3]).astype(f)       # [nb, 4, 4, 4]
    q = q.astype(f)
    r = (q[..., 0] + q[..., 3]).astype(f) + (q[..., 2] + q[..., 1]).astype(f)       # [nb, 4, 4]
    r = r.astype(f)
    w = (r[..., 0] + r[..., 1]).astype(f) + (r[..., 2] + r[..., 3]).astype(f)       # [nb, 4]
    w = w.astype(f)
    return ((w[:, 0] + w[:, 1]).astype(f) + (w[:, 2] + w[:, 3]).astype(f)).astype(f)


def bsum_bits(prio, cap):
    """fixed-order block sums of the live priorities prio[:cap] (the padding behind cap holds zeros)"""
    nb = (cap + P.BLOCK - 1) // P.BLOCK
    pad = np.zeros(nb * P.BLOCK, np.float32)
    pad[:cap] = np.asarray(prio, np.float32)[:cap]
    return block_sums_fixed(pad)


class ScoreModel(P.PerModel):
    """PerModel + score_new.  The rule: new = total - marked rows are waiting, len = min(new, max_new) of them are covered.  len < cap: row i sits in
    slot (marked + i) mod cap and marked advances by len.  len >= cap ("whole"): only the last cap rows are still in the ring — row i is the one in
    slot (total + i) mod cap, i < cap, every slot gets a priority and marked = total.  A finite error e >= 0 stores (e + 1e-4)^alpha and raises
    pmax to it; any other error stores pmax as it was when the call started."""

    def plan(self, total, max_new=None):
        new = max(total - self.marked, 0)
        n = new if max_new is None else min(new, int(max_new))
        if n >= self.cap:
            return (total + np.arange(self.cap)) % self.cap, total
        return (self.marked + np.arange(n)) % self.cap, self.marked + n

    def score_new(self, total, errors, max_new=None):
        """errors[i] = the error of row i of the call (at least as many as the rows covered) -> the slots written"""
        slots, marked = self.plan(total, max_new)
        e = np.asarray(errors, np.float64)[:slots.size]
        assert e.size == slots.size, "one error per row covered"
        ok = np.isfinite(e) & (e >= 0)
        with np.errstate(invalid="ignore"):
            p = np.where(ok, (np.where(ok, e, 0.0) + P.EPS) ** self.alpha, self.pmax)
        self.prio[slots] = p
        if ok.any():
            self.pmax = max(self.pmax, float(p[ok].max()))
        self.marked = marked
        return slots

    def bsum32(self):
        return bsum_bits(self.prio.astype(np.float32), self.cap)


SCORE_ROW0, LEARN_NEXT_ROW0 = 0xC0000000, 0x40000000  # the Philox rows of the scorer and of learn()'s policy.sample(s') (include/hirl4ucav.h)


def philox_normals(seed, row0, call, n):
    """the Gaussian head's in-kernel draws on the host: Philox4x32-10(key = seed; counter = (row0 + row, call, 0x53414331, 0)) -> Box-Muller, [n, 4]
    (tests/_philox_model.py: the device's float32 uniforms, float64 transcendentals — equal to the device's up to its logf / sinf / cosf rounding)"""
    from tests import _philox_model as PM

    return PM.act_normals(seed, row0, n, call, tag=PM.TAG_GAUSS).astype(np.float32)
