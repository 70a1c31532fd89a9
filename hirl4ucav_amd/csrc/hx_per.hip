// hx_per.hip — prioritized replay beside a DeviceReplay ring (gfx950): the priority store with its per-block sums, the proportional sampler with
// importance weights, and the priority update (SacAgent(per=True): SAC/agent.py:112-118, 281-284, 329-331; the memory class itself lives in the
// un-vendored rltorch, so the draw rule here is this project's own — include/hirl4ucav.h "Prioritized replay").
#include <cmath>

#include "hx_per_dev.h"

using namespace hxnn;
using namespace hxu;

namespace {

constexpr int kScanMax = 8192;      // entries of the block-sum scan the sampler holds in LDS (cap <= 2^24: at most two blocks per entry)

// ---------------------------------------------------------------------------------------------------------------
// mark_new: every slot in [marked, *total) mod cap <- pmax; workgroup g owns block (first touched block + g) mod nblocks — it writes, then re-sums,
// so no workgroup depends on another one's stores.  The last workgroup to finish (a ticket) publishes marked: every other one has read it by then.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPerThreads) void per_mark_kernel(PerDev P, long long max_new) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const unsigned long long tot = *P.total, mk = *P.marked, cap = (unsigned long long)P.cap;
    unsigned long long len = tot > mk ? tot - mk : 0ull;
    if (len > (unsigned long long)max_new) len = (unsigned long long)max_new;  // (a bound that was too small: the rest is marked by the next call)
    const bool whole = len >= cap;
    const unsigned long long s0 = mk % cap;
    const int b = (int)(((long long)(s0 / kPerBlock) + blockIdx.x) % P.nblocks);
    const float pm = *P.pmax;
    bool touched = false;
    if (len > 0) {
        float4* q = reinterpret_cast<float4*>(P.prio + (size_t)b * kPerBlock) + tid;
        float4 v = *q;
        float* e = &v.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned long long s = (unsigned long long)b * kPerBlock + tid * 4 + c;
            if (s < cap && (whole || (s >= s0 ? s - s0 : s + cap - s0) < len)) { e[c] = pm; touched = true; }
        }
        if (touched) *q = v;
    }
    if (__syncthreads_or(touched)) resum_block(P, b, part);  // (the barrier also orders this workgroup's stores before its re-sum's loads)
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(P.ticket, 1u) == gridDim.x - 1) {
            *P.ticket = 0u;
            *P.marked = whole ? tot : mk + len;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// set / update: n (slot, value) pairs; workgroup b owns block b: it looks through the pairs for its own slots, clears them, takes the MAXIMUM of the
// values given for each (unsigned atomicMax on the bits of a non-negative float: order-independent), re-sums if it was touched, raises pmax.
// mode 0: value = p[i] as given (already raised to alpha); mode 1: value = (|err[i]| + 1e-4)^alpha (powf).  A pair whose slot is outside [0, cap) or
// whose value is not finite (or negative) is skipped: the slot keeps the priority it had.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool per_value(const float* val, int i, int mode, float alpha, float& p) {
    if (mode) return per_priority(fabsf(val[i]), alpha, p);
    p = val[i];
    return p >= 0.0f && p <= 3.0e38f;  // (false for NaN)
}
__global__ __launch_bounds__(kPerThreads) void per_write_kernel(PerDev P, const int* __restrict__ slots, const float* __restrict__ val, int n, int mode, float alpha) {
    __shared__ float part[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const long long lo = (long long)b * kPerBlock, hi = lo + kPerBlock < P.cap ? lo + kPerBlock : P.cap;
    bool touched = false;
    for (int i = tid; i < n; i += kPerThreads) {
        const long long s = slots[i];
        float p;
        if (s >= lo && s < hi && per_value(val, i, mode, alpha, p)) { P.prio[s] = 0.0f; touched = true; }
    }
    if (!__syncthreads_or(touched)) return;
    float top = 0.0f;
    for (int i = tid; i < n; i += kPerThreads) {
        const long long s = slots[i];
        float p;
        if (s >= lo && s < hi && per_value(val, i, mode, alpha, p)) {
            atomicMax(reinterpret_cast<unsigned*>(P.prio + s), __float_as_uint(p));
            top = fmaxf(top, p);
        }
    }
    if (top > 0.0f) atomicMax(reinterpret_cast<unsigned*>(P.pmax), __float_as_uint(top));
    __syncthreads();
    resum_block(P, b, part);
}
__global__ __launch_bounds__(kPerThreads) void per_resum_kernel(PerDev P) {
    __shared__ float part[4];
    resum_block(P, blockIdx.x, part);
}

// ---------------------------------------------------------------------------------------------------------------
// sample: one workgroup of 1,024 threads (as sample_kernel).  Row r: target = u_r S; the block by binary search in the inclusive scan of bsum (LDS),
// the slot by one wave's scan of the block's 1,024 priorities; weights (n p / S)^-beta over their maximum; the rows gathered into the [batch][32] tile.
// ---------------------------------------------------------------------------------------------------------------
struct PerSampleArgs {
    PerDev P;
    const float* ring;
    const float* u;  // [batch] in [0, 1] (1 resolves as a target that rounded to S), or nullptr: Philox4x32-10(seed; row, call, kPerStream)
    int batch;
    uint64_t seed;
    uint32_t call;
    float beta;
    int* idx; float* weights; float* rows;
};
constexpr uint32_t kPerStream = 0x50455231u;  // the draw's own Philox stream word

// inclusive scan over the 64 lanes of a wave (Hillis-Steele on ds_bpermute: a fixed order)
__device__ __forceinline__ float wave_scan_incl(float v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(1024) void per_sample_kernel(PerSampleArgs A) {
    __shared__ float scan[kScanMax];   // inclusive scan of the (grouped) block sums
    __shared__ float tsum[2][1024];
    __shared__ int rblk[1024];         // per row: the block, the target inside it, the slot, the unnormalised weight
    __shared__ float rtgt[1024];
    __shared__ int fin[1024];
    __shared__ float rw[1024];
    __shared__ unsigned wmax;
    const PerDev& P = A.P;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = A.batch, nb = P.nblocks;
    const int G = (nb + kScanMax - 1) / kScanMax;  // blocks per scan entry (1; 2 beyond 2^23 slots)
    const int E = (nb + G - 1) / G;
    const int per = (E + 1023) / 1024;             // scan entries per thread (<= 8)
    if (tid == 0) wmax = 0u;
    // ---- inclusive scan of bsum: a thread's entries in order, the 1,024 thread sums by Hillis-Steele, every sum in a fixed order
    float loc[8];
    float run = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = tid * per + k;
        float v = 0.0f;
        if (k < per && e < E)
            for (int g = 0; g < G; ++g)
                if (e * G + g < nb) v += P.bsum[e * G + g];
        run += v;
        loc[k] = run;
    }
    tsum[0][tid] = run;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < 1024; d <<= 1) {
        tsum[cur ^ 1][tid] = tid >= d ? tsum[cur][tid] + tsum[cur][tid - d] : tsum[cur][tid];
        cur ^= 1;
        __syncthreads();
    }
    const float before = tid ? tsum[cur][tid - 1] : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = tid * per + k;
        if (k < per && e < E) scan[e] = before + loc[k];
    }
    __syncthreads();
    const float S = scan[E - 1];
    if (!(S > 0.0f)) {  // nothing holds priority (sampled before anything was marked: the caller's error): every row is slot 0 with weight 1, nothing is searched
        if (tid < B) { A.idx[tid] = 0; A.weights[tid] = 1.0f; }
        for (int e = tid; e < B * 8; e += 1024) reinterpret_cast<float4*>(A.rows)[e] = reinterpret_cast<const float4*>(A.ring)[e & 7];
        return;
    }
    const unsigned long long tot = *P.total;
    const float nlive = (float)(tot < (unsigned long long)P.cap ? tot : (unsigned long long)P.cap);
    // ---- per row: the target and its block
    if (tid < B) {
        float u;
        if (A.u) u = A.u[tid];
        else {
            uint32_t x[4];
            philox4x32_10((uint32_t)tid, A.call, kPerStream, 0u, (uint32_t)A.seed, (uint32_t)(A.seed >> 32), x);
            u = u01(x[0]);
        }
        const float t = u * S;
        int lo = 0, hi = E;  // entries whose inclusive sum is <= t  (searchsorted, side = right)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (scan[mid] <= t) lo = mid + 1;
            else hi = mid;
        }
        int e = lo < E ? lo : E - 1;  // (t rounded up to S: the last entry; the walk below finds the last block that holds anything)
        float tl = t - (e ? scan[e - 1] : 0.0f);
        int b = e * G;
        for (int g = 0; g + 1 < G && b + 1 < nb; ++g) {  // inside a grouped entry: its blocks in order
            const float s = P.bsum[b];
            if (tl < s) break;
            tl -= s;
            ++b;
        }
        // a block without priority mass (the target rounded past the end, or sat in a run of empty blocks): the nearest LOWER block that has some,
        // its whole mass below the target; with nothing below, the nearest higher one from its start
        if (!(P.bsum[b] > 0.0f)) {
            int c = b;
            while (c >= 0 && !(P.bsum[c] > 0.0f)) --c;
            if (c >= 0) { b = c; tl = 3.0e38f; }
            else {
                c = b;
                while (c < nb - 1 && !(P.bsum[c] > 0.0f)) ++c;
                b = c; tl = 0.0f;
            }
        }
        rblk[tid] = b;
        rtgt[tid] = fmaxf(tl, 0.0f);
    }
    __syncthreads();
    // ---- per row, one wave: the slot inside the block.  Lane l holds slots q * 256 + 4 l + c (q, c < 4) of the block: float4 loads, scanned in slot order.
    for (int r = wave; r < B; r += 16) {
        const int b = rblk[r];
        const float tl = rtgt[r];
        const float4* q4 = reinterpret_cast<const float4*>(P.prio + (size_t)b * kPerBlock);
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = q4[q * 64 + lane];
        float carry = 0.0f;
        int below = 0, first_nz = kPerBlock;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
            const float mine = (p[0] + p[1]) + (p[2] + p[3]);
            const float inc = wave_scan_incl(mine);
            float c0 = carry + (inc - mine);  // the sum of everything before this lane's four slots
            // (inc - mine is the exclusive scan up to rounding; the fallbacks below keep a rounding slip from ever selecting an empty slot)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                c0 += p[c];
                below += c0 <= tl ? 1 : 0;
                if (p[c] > 0.0f) first_nz = min(first_nz, q * 256 + lane * 4 + c);
            }
            carry += __shfl(inc, 63);
        }
        int slot = wave_sum_int(below);  // slots whose inclusive sum is <= the target = the index of the first one above it
        // the target at or past the block's mass, or (rounding) on an empty slot: the nearest LOWER slot that holds priority, else the first one
        const int s_here = slot < kPerBlock ? slot : kPerBlock - 1;
        int lower = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int s = q * 256 + lane * 4 + c;
                if (p[c] > 0.0f && s <= s_here) lower = max(lower, s);
            }
        }
        lower = wave_max_int(lower);
        first_nz = wave_min_int(first_nz);
        slot = lower >= 0 ? lower : (first_nz < kPerBlock ? first_nz : 0);  // (a slot that holds priority is its own nearest lower one)
        if (lane == 0) {
            const long long s = (long long)b * kPerBlock + slot;
            const long long sc = s < P.cap ? s : P.cap - 1;  // (never taken while the padding holds zeros)
            const float p = P.prio[sc];
            const float w = (S > 0.0f && p > 0.0f) ? powf(nlive * p / S, -A.beta) : 1.0f;
            fin[r] = (int)sc;
            rw[r] = w;
            atomicMax(&wmax, __float_as_uint(w));
        }
    }
    __syncthreads();
    if (tid < B) {
        const float m = __uint_as_float(wmax), w = rw[tid];
        A.idx[tid] = fin[tid];
        A.weights[tid] = w == m ? 1.0f : __fdiv_rn(w, m);  // the largest weight is exactly 1
    }
    // gather: 8 lanes per row, one 16-B piece each (sample_kernel's)
    for (int e = tid; e < B * 8; e += 1024) {
        const int r = e >> 3, c = e & 7;
        reinterpret_cast<float4*>(A.rows)[e] = reinterpret_cast<const float4*>(A.ring + (size_t)fin[r] * 32)[c];
    }
}

}  // namespace

extern "C" {

int hx_per_sizeof(void) { return (int)sizeof(HxPer); }
int64_t hx_per_prio_floats(int64_t cap) { return cap > 0 ? (cap + kPerBlock - 1) / kPerBlock * kPerBlock : 0; }

int hx_per_mark_new(const HxPer* per, int64_t max_new, void* stream) {
    PerDev P;
    if (int rc = per_dev(per, "hx_per_mark_new", &P)) return rc;
    HX_REQUIRE(max_new > 0, "hx_per_mark_new: max_new is the caller's upper bound on the rows stored since the last call (> 0)");
    const long long blocks = max_new / kPerBlock + 3;  // a range of max_new slots touches at most this many blocks (ragged last block, wrap)
    const unsigned grid = (unsigned)(blocks < P.nblocks ? blocks : P.nblocks);
    hipLaunchKernelGGL(per_mark_kernel, dim3(grid), dim3(kPerThreads), 0, (hipStream_t)stream, P, (long long)max_new);
    HX_CHECK_LAUNCH("hx_per_mark_new");
    return 0;
}

int hx_per_set(const HxPer* per, const int32_t* slots, const float* p, int32_t n, void* stream) {
    PerDev P;
    if (int rc = per_dev(per, "hx_per_set", &P)) return rc;
    HX_REQUIRE(slots && p && n > 0, "hx_per_set: slots, p and n > 0");
    hipLaunchKernelGGL(per_write_kernel, dim3((unsigned)P.nblocks), dim3(kPerThreads), 0, (hipStream_t)stream, P, slots, p, n, 0, 1.0f);
    HX_CHECK_LAUNCH("hx_per_set");
    return 0;
}

int hx_per_update(const HxPer* per, const int32_t* idx, const float* errors, int32_t n, float alpha, void* stream) {
    PerDev P;
    if (int rc = per_dev(per, "hx_per_update", &P)) return rc;
    HX_REQUIRE(idx && errors && n > 0 && alpha >= 0.0f, "hx_per_update: idx, errors, n > 0 and alpha >= 0");
    hipLaunchKernelGGL(per_write_kernel, dim3((unsigned)P.nblocks), dim3(kPerThreads), 0, (hipStream_t)stream, P, idx, errors, n, 1, alpha);
    HX_CHECK_LAUNCH("hx_per_update");
    return 0;
}

int hx_per_resum(const HxPer* per, void* stream) {
    PerDev P;
    if (int rc = per_dev(per, "hx_per_resum", &P)) return rc;
    hipLaunchKernelGGL(per_resum_kernel, dim3((unsigned)P.nblocks), dim3(kPerThreads), 0, (hipStream_t)stream, P);
    HX_CHECK_LAUNCH("hx_per_resum");
    return 0;
}

int hx_per_sample(const HxPer* per, const float* ring, int32_t batch, const float* u, uint64_t seed, uint32_t call, float beta, int32_t* idx,
                  float* weights, float* rows, void* stream) {
    PerDev P;
    if (int rc = per_dev(per, "hx_per_sample", &P)) return rc;
    HX_REQUIRE(ring && idx && weights && rows && batch > 0 && batch <= 1024 && beta >= 0.0f, "hx_per_sample: ring, idx, weights, rows, 0 < batch <= 1024, beta >= 0");
    PerSampleArgs A{P, ring, u, batch, seed, call, beta, idx, weights, rows};
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_per_sample");
    return 0;
}

}  // extern "C"
