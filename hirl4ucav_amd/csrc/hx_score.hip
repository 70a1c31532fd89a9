// hx_score.hip — priorities at insert for SAC's prioritized replay (gfx950): every row stored since the last call is scored with the networks as they
// stand, |Q1(s, a) - y| (SAC/agent.py:198-210, 234-246: what train_episode hands to memory.append), and enters the store at (error + 1e-4)^alpha
// instead of at pmax (hx_per_mark_new).  include/hirl4ucav.h "Prioritized replay, priorities at insert".
//
// The call works through the range [marked, *total) in CHUNKS of exactly chunk_rows rows, every chunk the same six launches of the same shape:
//     per_new_index   the chunk's slots from *total / *marked (device words: nothing is read on the host), its rows gathered into a compact tile
//     fwd_l2          policy(s') and Q1(s, a), values only                                  (launch_fwd: the update's forward kernel, unchanged)
//     gauss_head      a', H' = policy.sample(s'), one draw per row                          (hx_sac.hip's kernel, unchanged)
//     fwd_l2          target Q1 / Q2 (s', a')
//     td_score        y = r + (1 - d) gamma (min Q_target + alpha H'), error = |Q1 - y|     one wave per row
//     per_score_commit  prio[slot] <- (error + 1e-4)^alpha, the touched blocks re-summed, pmax raised; the LAST chunk's publishes `marked`
// launch_fwd picks its column tiling (and with it the K-split) from the row tiles of the launch, so a row's bits depend on the launch shape: the last
// chunk is padded to chunk_rows with a live row whose results are dropped, never shortened — a row's score depends on the row, the networks and its
// draw, not on how many rows were stored with it.  fwd_l2's compact job form carries no row index (pack_fwd), hence the gathered tile.
#include <cmath>

#include "hx_per_dev.h"

using namespace hxnn;
using namespace hxu;

namespace {

constexpr uint32_t kScoreRow0 = 0xC0000000u;  // the scorer's Philox rows: learn() draws at 0x40000000 + r and 0x80000000 + r, acting at env ids from 0

// What a call covers, from the device words as they stand when it starts (`marked` moves only in the last chunk's commit, `total` not at all while the
// call's launches run): rows i < len, row i in slot (start + i) mod cap.  More than cap new rows ("whole"): only the last cap of them are still in
// the ring — those are scored, which gives every slot a priority, and marked <- total.
struct ScorePlan {
    unsigned long long tot, mk, start, len;
    bool whole;
};
__device__ __forceinline__ ScorePlan score_plan(const PerDev& P, long long max_new) {
    ScorePlan s;
    const unsigned long long cap = (unsigned long long)P.cap;
    s.tot = *P.total; s.mk = *P.marked;
    s.len = s.tot > s.mk ? s.tot - s.mk : 0ull;
    if (s.len > (unsigned long long)max_new) s.len = (unsigned long long)max_new;  // (a bound that was too small: the rest is scored by the next call)
    s.whole = s.len >= cap;
    s.start = s.whole ? s.tot - cap : s.mk;
    if (s.whole) s.len = cap;
    return s;
}

// hdr[0] = len (int), hdr[1] = pmax as it was when the call started (float): what a non-finite error stores
struct IndexArgs {
    PerDev P;
    long long max_new;
    int row_base, rows;  // this chunk: rows [row_base, row_base + rows) of the call
    const float* ring;
    int* idx;            // [rows]
    float* tile;         // [rows][32]
    float* hdr;
};
// 8 lanes per row, one 16-byte piece each.  A padding row (i >= len) takes the range's first slot: inside the ring whatever the counters say.
__global__ __launch_bounds__(kPerThreads) void per_new_index_kernel(IndexArgs A) {
    const ScorePlan s = score_plan(A.P, A.max_new);
    const int e = blockIdx.x * kPerThreads + threadIdx.x;
    if (e == 0) {
        reinterpret_cast<int*>(A.hdr)[0] = (int)s.len;  // (len <= cap <= 2^24)
        if (A.row_base == 0) A.hdr[1] = *A.P.pmax;
    }
    const int r = e >> 3, c = e & 7;
    if (r >= A.rows) return;
    const unsigned long long i = (unsigned long long)A.row_base + (unsigned long long)r;
    const unsigned long long slot = (s.start + (i < s.len ? i : 0ull)) % (unsigned long long)A.P.cap;
    if (c == 0) A.idx[r] = (int)slot;
    reinterpret_cast<float4*>(A.tile)[e] = reinterpret_cast<const float4*>(A.ring + (size_t)slot * 32)[c];
}

// y and error per row from the three critic z2 rows (sac_td_heads, sac_td_target; no gradients, no sums).  One wave per row.
struct TdScoreArgs {
    const float* q1net; const float* t1net; const float* t2net;
    Mlp m;
    const float* z2_q1; const float* z2_t1; const float* z2_t2;
    const float* tile;         // [rows][32]: reward, done in columns 30, 31
    const float* ent_next;     // [rows] H'
    const float* alpha_state;
    const float* hdr;
    int row_base, rows;
    float gamma;
    float* err;                // [rows]
    float* errors_out;         // [max_new] or nullptr
};
__global__ __launch_bounds__(kThreads) void td_score_kernel(TdScoreArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    const int len = reinterpret_cast<const int*>(A.hdr)[0];
    if (r >= A.rows || A.row_base + r >= len) return;
    float qmin, q1, q2;
    sac_td_heads<false>(A.m, r, {A.t1net, A.z2_t1, nullptr}, {A.t2net, A.z2_t2, nullptr}, {A.q1net, A.z2_q1, nullptr}, {}, qmin, q1, q2);
    if (lane == 0) {
        const float lab0 = A.tile[(size_t)r * 32 + 30], lab1 = A.tile[(size_t)r * 32 + 31];
        const float e = fabsf(q1 - sac_td_target(lab0, lab1, A.gamma, qmin, A.ent_next[r], A.alpha_state[3]));
        A.err[r] = e;
        if (A.errors_out) A.errors_out[A.row_base + r] = e;
    }
}

// per_mark_kernel's ownership: workgroup g owns block (first touched block + g) mod nblocks — it writes its slots of the chunk, then re-sums, and waits
// for nobody.  publish (the call's last chunk): the last workgroup to finish (a ticket) moves `marked`; every other one has read it by then.
struct CommitArgs {
    PerDev P;
    long long max_new;
    int row_base, rows;
    const float* err;  // [rows]
    const float* hdr;
    float alpha;
    int publish;
};
__global__ __launch_bounds__(kPerThreads) void per_score_commit_kernel(CommitArgs A) {
    __shared__ float part[4];
    const PerDev& P = A.P;
    const int tid = threadIdx.x;
    const ScorePlan s = score_plan(P, A.max_new);
    const unsigned long long cap = (unsigned long long)P.cap;
    unsigned long long n = s.len > (unsigned long long)A.row_base ? s.len - (unsigned long long)A.row_base : 0ull;  // this chunk's live rows
    if (n > (unsigned long long)A.rows) n = (unsigned long long)A.rows;
    const unsigned long long s0 = (s.start + (unsigned long long)A.row_base) % cap;
    const int b = (int)(((long long)(s0 / kPerBlock) + blockIdx.x) % P.nblocks);
    const float pm = A.hdr[1];
    bool touched = false;
    float top = 0.0f;
    if (n > 0) {
        float4* q = reinterpret_cast<float4*>(P.prio + (size_t)b * kPerBlock) + tid;
        const float4 v = *q;
        float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned long long sl = (unsigned long long)b * kPerBlock + tid * 4 + c;
            const unsigned long long off = sl >= s0 ? sl - s0 : sl + cap - s0;
            if (sl < cap && off < n) {
                const float x = A.err[off];
                float p;
                const bool storable = per_priority(x, A.alpha, p);
                const bool ok = x >= 0.0f && x <= 3.0e38f && storable;  // (the error itself finite too: with alpha 0 any x gives p = 1)
                e[c] = ok ? p : pm;  // never skipped: a live slot holds a priority
                if (ok) top = fmaxf(top, p);
                touched = true;
            }
        }
        if (touched) *q = make_float4(e[0], e[1], e[2], e[3]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) top = fmaxf(top, __shfl_xor(top, d));
    if ((tid & 63) == 0 && top > 0.0f) atomicMax(reinterpret_cast<unsigned*>(P.pmax), __float_as_uint(top));  // (the bits of a non-negative float: order-independent)
    if (__syncthreads_or(touched)) resum_block(P, b, part);  // (the barrier also orders this workgroup's stores before its re-sum's loads)
    if (A.publish && tid == 0) {
        __threadfence();
        if (atomicAdd(P.ticket, 1u) == gridDim.x - 1) {
            *P.ticket = 0u;
            *P.marked = s.whole ? s.tot : s.mk + s.len;
        }
    }
}

enum { SC_PN = 0, SC_Q1, SC_T1, SC_T2, SC_COUNT };  // slots of a chunk: policy(s'), Q1(s, a), target Q1 / Q2 (s', a')
// behind the slots: tile [C][32], a' [C][4], H' [C], err [C], idx [C], hdr [8]
constexpr size_t score_floats(size_t C) { return (size_t)SC_COUNT * kSlotFloats * C + (32 + 4 + 1 + 1 + 1) * C + 8; }

}  // namespace

extern "C" {

int64_t hx_per_score_workspace_floats(int32_t chunk_rows) { return chunk_rows > 0 && chunk_rows % 16 == 0 ? (int64_t)score_floats((size_t)chunk_rows) : 0; }

int hx_per_score_new(const HxPer* per, const float* ring, const HxSacNets* N, const HxHyper* Hy, int64_t max_new, int32_t chunk_rows, float per_alpha,
                     const float* eps, uint64_t seed, uint32_t call, float* ws, float* errors_out, void* stream) {
    PerDev P;
    if (int rc = per_dev(per, "hx_per_score_new", &P)) return rc;
    HX_REQUIRE(ring && N && Hy && ws, "hx_per_score_new: ring, nets, hyper and ws (hx_per_score_workspace_floats(chunk_rows) floats)");
    HX_REQUIRE(N->policy && N->critic && N->target_critic && N->alpha_state, "hx_per_score_new: nets needs policy, critic, target_critic and alpha_state");
    HX_REQUIRE(!N->w2_bf16_all, "hx_per_score_new: scoring is fp32 only (nets->w2_bf16_all must be NULL)");
    HX_REQUIRE(chunk_rows > 0 && chunk_rows % 16 == 0, "hx_per_score_new: chunk_rows is a positive multiple of 16 (got %d)", (int)chunk_rows);
    HX_REQUIRE(max_new > 0, "hx_per_score_new: max_new is the caller's upper bound on the rows stored since the last call (> 0)");
    HX_REQUIRE(per_alpha >= 0.0f && per_alpha <= 1.0f, "hx_per_score_new: per_alpha in [0, 1] (got %g)", (double)per_alpha);
    HX_REQUIRE((reinterpret_cast<uintptr_t>(ring) & 15u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 15u) == 0, "hx_per_score_new: ring and ws must be 16-byte aligned");
    if (int rc = sac_check_formats(N, "hx_per_score_new")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int C = chunk_rows;
    const long long rows_all = max_new < per->cap ? (long long)max_new : (long long)per->cap;  // (a call never covers more than the ring holds)
    const int nchunks = (int)((rows_all + C - 1) / C);
    Slot s[SC_COUNT];
    for (int i = 0; i < SC_COUNT; ++i) s[i] = carve_slot(ws + (size_t)i * kSlotFloats * C, C);
    float* const tile = ws + (size_t)SC_COUNT * kSlotFloats * C;
    float* const act = tile + 32 * (size_t)C;
    float* const ent = act + 4 * (size_t)C;
    float* const err = ent + C;
    int* const idx = reinterpret_cast<int*>(err + C);
    float* const hdr = err + 2 * (size_t)C;
    const float* q1 = N->critic;
    const float* t1 = N->target_critic; const float* t2 = N->target_critic + kQs.padded();
    const RowSrc src{tile, nullptr, nullptr, 0, 32};
    const long long cblocks = C / kPerBlock + 3;  // a range of C slots touches at most this many blocks (ragged last block, wrap)
    const unsigned cgrid = (unsigned)(cblocks < P.nblocks ? cblocks : P.nblocks);
    for (int c = 0; c < nchunks; ++c) {
        const int base = c * C;
        const int given = (int)(rows_all - base < C ? rows_all - base : C);  // rows of this chunk the caller's eps / errors_out cover
        {
            const IndexArgs A{P, (long long)max_new, base, C, ring, idx, tile, hdr};
            hipLaunchKernelGGL(per_new_index_kernel, dim3((unsigned)((C * 8 + kPerThreads - 1) / kPerThreads)), dim3(kPerThreads), 0, st, A);
        }
        {   // policy(s'), Q1(s, a): values only
            FwdArgs F{};
            F.njobs = 2; F.slope = 0.0f;
            F.job[0] = FwdJob{N->policy, kPolicy, src, 17, 0, Head{}, nullptr, 0.f, s[SC_PN], C, 0, IM_ACTOR};
            F.job[1] = FwdJob{q1, kQs, src, 0, 0, Head{}, nullptr, 0.f, s[SC_Q1], C, 0, IM_C1};
            launch_fwd(F, st);
        }
        // a', H' = policy.sample(s'): per-row waves, so the rows behind `given` (padding: dropped) may keep what an earlier chunk left
        launch_sac_gauss_rows(N->policy, s[SC_PN].z2, eps ? eps + 4 * (size_t)base : nullptr, given, act, ent, seed, kScoreRow0 + (uint32_t)base, call, st);
        launch_target_q(s + SC_T1, N->target_critic, src, act, C, nullptr, st);
        {
            const TdScoreArgs T{q1, t1, t2, kQs, s[SC_Q1].z2, s[SC_T1].z2, s[SC_T2].z2, tile, ent, N->alpha_state, hdr, base, given, Hy->gamma, err, errors_out};
            hipLaunchKernelGGL(td_score_kernel, dim3((unsigned)((C + 3) / 4)), dim3(kThreads), 0, st, T);
        }
        {
            const CommitArgs A{P, (long long)max_new, base, C, err, hdr, per_alpha, c == nchunks - 1 ? 1 : 0};
            hipLaunchKernelGGL(per_score_commit_kernel, dim3(cgrid), dim3(kPerThreads), 0, st, A);
        }
    }
    HX_CHECK_LAUNCH("hx_per_score_new");
    return 0;
}

}  // extern "C"
