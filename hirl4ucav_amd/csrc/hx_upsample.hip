// hx_upsample.hip — success upsampling beside a DeviceReplay ring (gfx950): the per-block counts of live success rows, the proportional draw with
// INTEGER weights boost : 1 (the reference's 1.0 : 0.1, buffer.py:18-29, 39-43) and the BC minibatch's fire row (HIRL.py:253-257, BC.py:171-176).
// Every sum is an exact count: no float arithmetic, no atomics — include/hirl4ucav.h "Success upsampling"; tests/_upsample_model.py is the rule in Python.
#include "hx_update.h"

using namespace hxnn;
using namespace hxu;

namespace {

constexpr int kUpsBlock = 1024;     // slots per count
constexpr int kUpsScanMax = 8192;   // entries of the block-weight scan the draw holds in LDS (cap <= 2^24: at most two blocks per entry)
constexpr uint32_t kUpsStream = 0x55505331u;  // the draw's own Philox stream word
constexpr uint32_t kUpsFireRow = 0xFFFFFFF1u; // the counter row of the BC replacement's words

struct UpsDev {
    uint32_t* cnt;
    unsigned long long* marked;
    const unsigned long long* total;
    const int8_t* succ;
    long long cap;
    int boost, nblocks;
};

// The 16 labels of slots [base, base + 16) as four words, in two steps so that the loads of several blocks can be in flight together: labels_load is
// one unconditional 16-byte load — of chunk 0 for a lane whose chunk does not lie wholly below cap: nothing at or behind cap is read (the label array
// is cap bytes: a ragged last block) —, labels_fix then reads the ONE chunk of the ring that straddles cap byte by byte.  A lane whose chunk lies
// wholly at or behind cap keeps chunk 0's labels: none of its slots is live, and success_bits masks by the live length.
__device__ __forceinline__ uint4 labels_load(const int8_t* succ, long long base, long long cap) {
    if (cap < 16) return make_uint4(0u, 0u, 0u, 0u);  // (uniform)
    return *reinterpret_cast<const uint4*>(succ + (base + 16 <= cap ? base : 0));
}
__device__ __forceinline__ uint4 labels_fix(uint4 v, const int8_t* succ, long long base, long long cap) {
    if (base < cap && base + 16 > cap) {
        unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll 1
        for (int j = 0; base + j < cap; ++j) {
            const unsigned long long byte = (unsigned long long)(uint8_t)succ[base + j];
            if (j < 8) lo |= byte << (8 * j);
            else hi |= byte << (8 * (j - 8));
        }
        v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    return v;
}
__device__ __forceinline__ uint4 load_labels(const int8_t* succ, long long base, long long cap) { return labels_fix(labels_load(succ, base, cap), succ, base, cap); }
// bit j: slot base + j is live (< n) and its label is exactly 1;  live16: bit j: the slot is live.  Per word: 0x80 in every byte that equals 1 (the exact
// zero-byte test on w ^ 0x01010101), the four flags gathered into four bits by one multiplication (no two partial products meet: no carries).
__device__ __forceinline__ uint32_t ones4(uint32_t w) {
    const uint32_t x = w ^ 0x01010101u;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 where the byte of x is 0
    return (((z >> 7) * 0x01020408u) >> 24) & 0xFu;
}
__device__ __forceinline__ uint32_t success_bits(const uint4& v, long long base, long long n, uint32_t& live16) {
    const long long l = n - base;
    live16 = l <= 0 ? 0u : (l >= 16 ? 0xFFFFu : (1u << (int)l) - 1u);
    return (ones4(v.x) | (ones4(v.y) << 4) | (ones4(v.z) << 8) | (ones4(v.w) << 12)) & live16;
}
// one wave: the live success rows of block b, lane l holding slots 16 l .. 16 l + 15 — sixteen ballots, popcounts added in bit order
__device__ __forceinline__ uint32_t count_block(const UpsDev& U, int b, long long n) {
    const int lane = threadIdx.x & 63;
    const long long base = (long long)b * kUpsBlock + lane * 16;
    uint32_t live16;
    const uint32_t m = success_bits(load_labels(U.succ, base, U.cap), base, n, live16);
    uint32_t c = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) c += (uint32_t)__popcll(__ballot((m >> j) & 1u));
    return c;
}

// ---------------------------------------------------------------------------------------------------------------
// mark_new: ONE workgroup; wave w takes the touched blocks w, w + 16, ... (counted from the block of slot marked mod cap).  Every wave reads
// marked before the barrier, thread 0 stores it behind the barrier.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ups_mark_kernel(UpsDev U, long long max_new) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long tot = *U.total, mk = *U.marked, cap = (unsigned long long)U.cap;
    unsigned long long len = tot > mk ? tot - mk : 0ull;
    if (len > (unsigned long long)max_new) len = (unsigned long long)max_new;  // (a bound that was too small: the rest is covered by the next call)
    const bool whole = len >= cap;
    const long long n = (long long)(tot < cap ? tot : cap);
    __syncthreads();  // every wave holds marked
    if (len > 0) {
        const unsigned long long s0 = mk % cap;
        const int b0 = (int)(s0 / kUpsBlock);
        // blocks touched by [s0, s0 + len) mod cap, in ring order from b0 (a range that wraps into b0 again does not count it twice)
        long long nt;
        if (whole) nt = U.nblocks;
        else {
            const unsigned long long e = s0 + len;  // exclusive end, unwrapped
            if (e <= cap) nt = (long long)((e - 1) / kUpsBlock) - b0 + 1;
            else {
                nt = (U.nblocks - b0) + (long long)((e - cap - 1) / kUpsBlock) + 1;
                if (nt > U.nblocks) nt = U.nblocks;
            }
        }
        for (long long g = wave; g < nt; g += 16) {
            const int b = (int)((b0 + g) % U.nblocks);
            const uint32_t c = count_block(U, b, n);
            if (lane == 0) U.cnt[b] = c;
        }
    }
    if (threadIdx.x == 0) *U.marked = whole ? tot : mk + len;
}

// recount: one wave per block, 16 blocks per workgroup; nobody reads marked
__global__ __launch_bounds__(1024) void ups_recount_kernel(UpsDev U) {
    const int b = blockIdx.x * 16 + (threadIdx.x >> 6);
    const unsigned long long tot = *U.total, cap = (unsigned long long)U.cap;
    if (b < U.nblocks) {
        const uint32_t c = count_block(U, b, (long long)(tot < cap ? tot : cap));
        if ((threadIdx.x & 63) == 0) U.cnt[b] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *U.marked = tot;
}

// ---------------------------------------------------------------------------------------------------------------
// draw: one workgroup of 1,024 threads (as per_sample_kernel).  Row r: t = (x_r W) >> 64; the block by binary search in the inclusive scan of the
// block weights (LDS), the slot by one wave's scan of the block's 1,024 labels; the rows gathered into the [batch][32] tile.  Then the fire row.
// ---------------------------------------------------------------------------------------------------------------
struct UpsDrawArgs {
    UpsDev U;
    int has_ups;
    const float* ring;
    int batch, n_main;
    const unsigned long long* x;
    uint64_t seed;
    uint32_t call;
    int* idx; float* rows;
    const int* fire_idx; int n_fire;
    const float* bc_table; int* idx_bc; float* bc_rows;
};

__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint32_t block_live(long long n, int b) {
    const long long l = n - (long long)b * kUpsBlock;
    return (uint32_t)(l < 0 ? 0 : (l > kUpsBlock ? kUpsBlock : l));
}
__device__ __forceinline__ uint32_t block_weight(const UpsDev& U, long long n, int b) { return block_live(n, b) + (uint32_t)(U.boost - 1) * U.cnt[b]; }

// one wave: the slot of block b whose interval of the block's running weight holds tl; lane l holds the labels of slots 16 l .. 16 l + 15 in `lab`
__device__ __forceinline__ int row_slot(const UpsDev& U, long long n, int b, uint32_t tl, uint4 lab, int lane) {
    const long long base = (long long)b * kUpsBlock + lane * 16;
    uint32_t live16;
    const uint32_t m = success_bits(labels_fix(lab, U.succ, base, U.cap), base, n, live16);
    const uint32_t mine = (uint32_t)__popc(live16) + (uint32_t)(U.boost - 1) * (uint32_t)__popc(m);
    const uint32_t inc = wave_scan_incl_u32(mine);
    const unsigned long long above = __ballot(inc > tl);
    if (!above) {  // the counts were stale (rows stored since the last mark_new): the block's last live slot
        const int live = (int)block_live(n, b);
        return live > 0 ? live - 1 : 0;
    }
    const int L = __ffsll((long long)above) - 1;  // the first lane whose inclusive weight is above the target
    // the lane's first slot whose inclusive weight is above the target, by bisection over its 16 slots (the weight of slots 0 .. j grows with j; lane L
    // holds such a slot)
    const uint32_t c0 = inc - mine;  // the weight before this lane's slots
    int j = 0;
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1) {
        const uint32_t upto = (1u << (j + h)) - 1u;  // slots 0 .. j + h - 1
        if (c0 + (uint32_t)__popc(live16 & upto) + (uint32_t)(U.boost - 1) * (uint32_t)__popc(m & upto) <= tl) j += h;
    }
    return L * 16 + (__shfl(j, L) & 15);
}

__global__ __launch_bounds__(1024) void ups_draw_kernel(UpsDrawArgs A) {
    __shared__ uint32_t scan[kUpsScanMax];  // inclusive scan of the (grouped) block weights
    __shared__ uint32_t wsum[16];
    __shared__ int rblk[1024];              // per row: the block, the target inside it, the slot
    __shared__ uint32_t rtgt[1024];
    __shared__ int fin[1024];
    const UpsDev& U = A.U;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int M = A.has_ups ? A.n_main : 0;
    if (M > 0) {  // (uniform over the workgroup: the barriers below are reached by all or by none)
        const int nb = U.nblocks;
        const int G = (nb + kUpsScanMax - 1) / kUpsScanMax;  // blocks per scan entry (1; 2 beyond 2^23 slots)
        const int E = (nb + G - 1) / G;
        const int per = (E + 1023) / 1024;                   // scan entries per thread (<= 8)
        const unsigned long long tot = *U.total;
        const long long n = (long long)(tot < (unsigned long long)U.cap ? tot : (unsigned long long)U.cap);
        // ---- inclusive scan of the block weights: a thread's entries in order, the 64 thread sums of a wave by shuffles, the 16 wave sums in wave order
        uint32_t run = 0u;
#pragma unroll 1
        for (int k = 0; k < per; ++k) {
            const int e = tid * per + k;
            if (e < E) {
                for (int g = 0; g < G; ++g)
                    if (e * G + g < nb) run += block_weight(U, n, e * G + g);
                scan[e] = run;  // inclusive among this thread's entries
            }
        }
        const uint32_t inw = wave_scan_incl_u32(run);
        if (lane == 63) wsum[wave] = inw;
        __syncthreads();
        uint32_t before = inw - run;  // the weight before this thread's entries
        for (int w = 0; w < wave; ++w) before += wsum[w];
#pragma unroll 1
        for (int k = 0; k < per; ++k) {
            const int e = tid * per + k;
            if (e < E) scan[e] += before;
        }
        __syncthreads();
        const uint32_t W = scan[E - 1];
        // ---- per row: the target and its block
        if (tid < M) {
            unsigned long long word;
            if (A.x) word = A.x[tid];
            else {
                uint32_t p[4];
                philox4x32_10((uint32_t)tid, A.call, kUpsStream, 0u, (uint32_t)A.seed, (uint32_t)(A.seed >> 32), p);
                word = ((unsigned long long)p[0] << 32) | p[1];
            }
            int b = 0;
            uint32_t tl = 0u;
            if (W > 0u) {
                const uint32_t t = (uint32_t)__umul64hi(word, (unsigned long long)W);  // < W
                int lo = 0, hi = E - 1;  // the first entry whose inclusive weight is above t (the last one's is W > t)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (scan[mid] <= t) lo = mid + 1;
                    else hi = mid;
                }
                tl = t - (lo ? scan[lo - 1] : 0u);
                b = lo * G;
                for (int g = 0; g + 1 < G && b + 1 < nb; ++g) {  // inside a grouped entry: its blocks in order
                    const uint32_t w = block_weight(U, n, b);
                    if (tl < w) break;
                    tl -= w;
                    ++b;
                }
            }
            rblk[tid] = b;
            rtgt[tid] = tl;
        }
        __syncthreads();
        // ---- per row, one wave: the slot inside the block.  Lane l holds slots 16 l .. 16 l + 15: one 16-byte load, scanned in slot order.  A wave
        // takes rows wave, wave + 16, ...; the loads of eight of them are in flight together.  (Row and block are wave-uniform: scalar branches.)
        const bool empty = __builtin_amdgcn_readfirstlane(W) == 0u;  // nothing holds weight (drawn from an empty ring: the caller's error): slot 0
        for (int r0 = __builtin_amdgcn_readfirstlane(wave); r0 < M; r0 += 16 * 8) {
            uint4 lab[8];
            int blk[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = r0 + 16 * q;
                blk[q] = r < M ? __builtin_amdgcn_readfirstlane(rblk[r]) : 0;
                lab[q] = labels_load(U.succ, (long long)blk[q] * kUpsBlock + lane * 16, U.cap);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = r0 + 16 * q;
                if (r < M) {
                    const int slot = row_slot(U, n, blk[q], rtgt[r], lab[q], lane);
                    if (lane == 0) {
                        const long long s = (long long)blk[q] * kUpsBlock + slot;
                        fin[r] = empty ? 0 : (int)(s < U.cap ? s : U.cap - 1);
                    }
                }
            }
        }
        __syncthreads();
        if (tid < M) A.idx[tid] = fin[tid];
        // gather: 8 lanes per row, one 16-B piece each (sample_kernel's)
        for (int e = tid; e < M * 8; e += 1024) {
            const int r = e >> 3, c = e & 7;
            reinterpret_cast<float4*>(A.rows)[e] = reinterpret_cast<const float4*>(A.ring + (size_t)fin[r] * 32)[c];
        }
    }
    // ---- the BC minibatch's fire row: one wave, 8 lanes copy the row
    if (A.fire_idx && wave == 0) {
        unsigned long long w0, w1;
        if (A.x) { w0 = A.x[A.n_main]; w1 = A.x[A.n_main + 1]; }
        else {
            uint32_t p[4];
            philox4x32_10(kUpsFireRow, A.call, kUpsStream, 0u, (uint32_t)A.seed, (uint32_t)(A.seed >> 32), p);
            w0 = ((unsigned long long)p[0] << 32) | p[1];
            w1 = ((unsigned long long)p[2] << 32) | p[3];
        }
        const int j = (int)__umul64hi(w0, (unsigned long long)A.n_fire);  // < n_fire
        const int k = (int)__umul64hi(w1, (unsigned long long)A.batch);   // < batch
        const int f = A.fire_idx[j];
        if (lane == 0) A.idx_bc[k] = f;
        if (lane < 8) reinterpret_cast<float4*>(A.bc_rows + (size_t)k * 32)[lane] = reinterpret_cast<const float4*>(A.bc_table + (size_t)f * 32)[lane];
    }
}

int ups_dev(const HxUps* u, const char* who, UpsDev* out) {
    HX_REQUIRE(u && u->cnt && u->marked && u->total && u->ring_success && u->cap > 0, "%s: ups needs cnt, marked, total, ring_success and cap > 0", who);
    HX_REQUIRE(u->cap <= ((int64_t)1 << 24), "%s: success upsampling holds at most 2^24 slots (cap = %lld): 16,384 block weights is what the draw scans", who,
               (long long)u->cap);
    HX_REQUIRE(u->boost >= 2 && u->boost <= 255, "%s: boost is 2 .. 255 (the weight of a success row against 1), got %d", who, (int)u->boost);
    HX_REQUIRE((reinterpret_cast<uintptr_t>(u->ring_success) & 15u) == 0, "%s: ring_success must be 16-byte aligned", who);
    *out = UpsDev{u->cnt, (unsigned long long*)u->marked, (const unsigned long long*)u->total, u->ring_success, (long long)u->cap, (int)u->boost,
                  (int)((u->cap + kUpsBlock - 1) / kUpsBlock)};
    return 0;
}

}  // namespace

extern "C" {

int hx_ups_sizeof(void) { return (int)sizeof(HxUps); }
int64_t hx_ups_words(int64_t cap) { return cap > 0 && cap <= ((int64_t)1 << 24) ? (cap + kUpsBlock - 1) / kUpsBlock : 0; }

int hx_ups_mark_new(const HxUps* ups, int64_t max_new, void* stream) {
    UpsDev U;
    if (int rc = ups_dev(ups, "hx_ups_mark_new", &U)) return rc;
    HX_REQUIRE(max_new > 0, "hx_ups_mark_new: max_new is the caller's upper bound on the rows stored since the last call (> 0)");
    hipLaunchKernelGGL(ups_mark_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, U, (long long)max_new);
    HX_CHECK_LAUNCH("hx_ups_mark_new");
    return 0;
}

int hx_ups_recount(const HxUps* ups, void* stream) {
    UpsDev U;
    if (int rc = ups_dev(ups, "hx_ups_recount", &U)) return rc;
    hipLaunchKernelGGL(ups_recount_kernel, dim3((unsigned)((U.nblocks + 15) / 16)), dim3(1024), 0, (hipStream_t)stream, U);
    HX_CHECK_LAUNCH("hx_ups_recount");
    return 0;
}

int hx_ups_draw(const HxUps* ups, const float* ring, int32_t batch, int32_t n_main, const uint64_t* x, uint64_t seed, uint32_t call, int32_t* idx,
                float* rows, const int32_t* fire_idx, int32_t n_fire, const float* bc_table, int32_t* idx_bc, float* bc_rows, void* stream) {
    HX_REQUIRE(batch > 0 && batch <= 1024 && n_main >= 0 && n_main <= batch, "hx_ups_draw: 0 < batch <= 1024 and 0 <= n_main <= batch");
    HX_REQUIRE(n_main > 0 || fire_idx, "hx_ups_draw: nothing to do (n_main = 0 and no fire_idx)");
    UpsDrawArgs A{};
    if (n_main > 0) {
        HX_REQUIRE(ups, "hx_ups_draw: n_main > 0 needs ups (NULL goes with n_main = 0: the BC replacement alone)");
        if (int rc = ups_dev(ups, "hx_ups_draw", &A.U)) return rc;
        HX_REQUIRE(ring && idx && rows, "hx_ups_draw: ring, idx and rows");
        HX_REQUIRE(((reinterpret_cast<uintptr_t>(ring) | reinterpret_cast<uintptr_t>(rows)) & 15u) == 0, "hx_ups_draw: ring and rows must be 16-byte aligned");
        A.has_ups = 1;
    }
    if (fire_idx) {
        HX_REQUIRE(n_fire > 0 && bc_table && idx_bc && bc_rows, "hx_ups_draw: fire_idx goes with n_fire > 0, bc_table, idx_bc and bc_rows");
        HX_REQUIRE(((reinterpret_cast<uintptr_t>(bc_table) | reinterpret_cast<uintptr_t>(bc_rows)) & 15u) == 0, "hx_ups_draw: bc_table and bc_rows must be 16-byte aligned");
    } else {
        HX_REQUIRE(n_fire == 0, "hx_ups_draw: n_fire > 0 without fire_idx");
    }
    A.ring = ring; A.batch = batch; A.n_main = n_main; A.x = (const unsigned long long*)x; A.seed = seed; A.call = call; A.idx = idx; A.rows = rows;
    A.fire_idx = fire_idx; A.n_fire = n_fire; A.bc_table = bc_table; A.idx_bc = idx_bc; A.bc_rows = bc_rows;
    hipLaunchKernelGGL(ups_draw_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_ups_draw");
    return 0;
}

}  // extern "C"
