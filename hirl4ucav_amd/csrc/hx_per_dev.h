// hx_per_dev.h — the priority store's device view, shared by hx_per.hip (mark, set / update, re-sum, sample) and hx_score.hip (priorities at insert):
// the buffers, the fixed-order block sum, the priority rule and the host check that builds the view from an HxPer (gfx950).
#pragma once
#include <cmath>

#include "hx_update.h"

namespace hxu {

constexpr int kPerBlock = 1024;     // slots per block sum
constexpr int kPerThreads = 256;    // workgroup of the store kernels: one float4 of the block per thread

struct PerDev {
    float* prio; float* bsum; float* pmax;
    unsigned long long* marked; unsigned* ticket;
    const unsigned long long* total;
    long long cap;
    int nblocks;
};

// bsum[b] <- the sum of block b in a FIXED order ((x + y) + (z + w) per thread, the DPP tree per wave, ((w0 + w1) + (w2 + w3)) over the four waves):
// the same bits for the same priorities, whoever re-sums.  All kPerThreads threads of the workgroup call it; `part` = 4 floats of LDS.
__device__ __forceinline__ void resum_block(const PerDev& P, int b, float* part) {
    const int tid = threadIdx.x;
    const float4 v = reinterpret_cast<const float4*>(P.prio + (size_t)b * kPerBlock)[tid];  // (the padding behind cap holds zeros)
    const float s = wave_sum((v.x + v.y) + (v.z + v.w));
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) P.bsum[b] = (part[0] + part[1]) + (part[2] + part[3]);
}

// the priority of a TD error: p = (err + 1e-4)^alpha (powf) -> whether it may be stored: finite and not negative (false for NaN)
__device__ __forceinline__ bool per_priority(float err, float alpha, float& p) {
    p = powf(err + 1e-4f, alpha);
    return p >= 0.0f && p <= 3.0e38f;
}

inline int per_dev(const HxPer* p, const char* who, PerDev* out) {
    HX_REQUIRE(p && p->prio && p->bsum && p->pmax && p->marked && p->ticket && p->total && p->cap > 0, "%s: per needs prio, bsum, pmax, marked, ticket, total and cap > 0", who);
    HX_REQUIRE(p->cap <= ((int64_t)1 << 24), "%s: prioritized replay holds at most 2^24 slots (cap = %lld): 16,384 block sums is what the sampler scans", who, (long long)p->cap);
    HX_REQUIRE((reinterpret_cast<uintptr_t>(p->prio) & 15u) == 0, "%s: prio must be 16-byte aligned", who);
    *out = PerDev{p->prio, p->bsum, p->pmax, (unsigned long long*)p->marked, p->ticket, (const unsigned long long*)p->total, (long long)p->cap,
                  (int)((p->cap + kPerBlock - 1) / kPerBlock)};
    return 0;
}

}  // namespace hxu
