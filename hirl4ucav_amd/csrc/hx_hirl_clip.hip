// hx_hirl_clip.hip — gradient-norm clipping for HIRL and TD3 (gfx950): torch.nn.utils.clip_grad_norm_ once per optimizer, in front of its step.  The
// reference's HIRL.py / TD3.py have no clip: a declared extension, the rule is SAC's (SAC/utils.py:15-21).
//   hirl_grad_sumsq   sums of squares of a gradient, one partial per fixed 4,096-word chunk (no atomics, a fixed order)
//   hirl_adam_clip    adam_kernel's step on (g * gscale) * coef; every workgroup re-adds the partials and forms coef itself
// HIRL's update already runs as stages where ranks exchange gradients (HirlEngine._learn_staged), the optimizer step after the exchange: the norm
// launch goes in front of that step and sees the summed gradient — the data-parallel meaning, the norm of the averaged gradient.
// An optimizer covers ALL of its parameters: both Q heads AND the LayerNorm weights (HIRL trains them; hx_clip.hip's clip_live leaves SAC's untrained
// slots out), the whole actor.  The padding behind size() never counts.
#include <cmath>

#include "hx_update.h"

using namespace hxnn;
using namespace hxu;

namespace {

// The summation shape of one block's sum of squares (tests/test_hirl_clip_gpu.py derives its rounding bound from these, through hx_hirl_clip_shape):
//   a thread squares 4 float4 (kClipVecs) of its chunk: (x^2 + y^2) + (z^2 + w^2) per float4 (depth 2), added one after the other (kClipVecs - 1 deep),
//   the wave's 64 sums by wave_sum's DPP tree (6 deep), the workgroup's 4 waves as (w0 + w1) + (w2 + w3) (2 deep),
//   a block's <= 64 partials by ONE wave_sum (6 deep) — in the stepping kernel, by every workgroup alike —, the critic's two heads head 0 + head 1 (1 deep).
constexpr int kClipVecs = 4;                          // float4 per thread
constexpr int kClipChunk = kThreads * 4 * kClipVecs;  // 4,096 words per workgroup
constexpr int kClipMaxParts = 64;                     // partials per block: one wave re-adds them
constexpr int kClipOutWords = 8;                      // clip_ws[0..1] norms (critic, actor), [2..3] coefficients, four spare
constexpr int kClipWsFloats = kClipOutWords + 3 * kClipMaxParts;  // partials: Q head 0 | Q head 1 | actor
constexpr int kDepthBlock = 1 + 2 + (kClipVecs - 1) + 6 + 2 + 6;  // square, float4 tree, the thread's sequence, wave tree, four waves, the partials' wave tree

// g = w dL_bc + (1 - w) dL_rl (HIRL.py:321) with the roundings adam_kernel's `wmix * b + (1.0f - wmix) * g` compiles to — the product w b rounded, then
// ONE fused multiply-add — spelled out, so that both kernels here form the bits hx_adam_mixed steps on whatever the compiler would contract
__device__ __forceinline__ float mix(float w, float b, float g) { return __builtin_fmaf(1.0f - w, g, w * b); }

struct SumsqArgs {
    float* parts;               // [nblk][kClipMaxParts]
    int nblk, nchunks;          // blocks of the gradient (critic 2, actor 1), chunks per block
    int stride, live;           // words from one block to the next (padded()), words that count in each (size())
};

// A.g (and with A.g2 the mix w g2 + (1 - w) g, adam_kernel's roundings with adam_w's w) squared and summed per chunk
__global__ __launch_bounds__(kThreads) void hirl_grad_sumsq_kernel(AdamArgs A, SumsqArgs S) {
    __shared__ float part[4];
    const int tid = threadIdx.x, blk = blockIdx.x / S.nchunks, chunk = blockIdx.x % S.nchunks;
    const float wmix = A.g2 ? adam_w(A) : 0.0f;
    const float* g = A.g + (size_t)blk * S.stride;
    float4 v[kClipVecs];
#pragma unroll
    for (int q = 0; q < kClipVecs; ++q) {  // every load in flight before the first square; past the block's end: zeros, nothing read
        const int e = chunk * kClipChunk + (q * kThreads + tid) * 4;
        const bool in = e + 4 <= S.stride;
        v[q] = in ? *reinterpret_cast<const float4*>(g + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (A.g2) {  // (the message form has one block: the actor)
            const float4 b4 = in ? *reinterpret_cast<const float4*>(A.g2 + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[q].x = mix(wmix, b4.x, v[q].x);
            v[q].y = mix(wmix, b4.y, v[q].y);
            v[q].z = mix(wmix, b4.z, v[q].z);
            v[q].w = mix(wmix, b4.w, v[q].w);
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < kClipVecs; ++q) {
        const int e = chunk * kClipChunk + (q * kThreads + tid) * 4;
        const float x = e < S.live ? v[q].x : 0.0f, y = e + 1 < S.live ? v[q].y : 0.0f;
        const float z = e + 2 < S.live ? v[q].z : 0.0f, w = e + 3 < S.live ? v[q].w : 0.0f;
        const float t = (x * x + y * y) + (z * z + w * w);
        s = q == 0 ? t : s + t;
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) S.parts[blk * kClipMaxParts + chunk] = (part[0] + part[1]) + (part[2] + part[3]);
}

struct ClipArgs {
    const float* parts;  // this optimizer's first block's partials
    float* out;          // clip_ws: norms at [0..1], coefficients at [2..3]
    int nblk, nparts, slot;  // blocks (critic 2: ONE norm over both), partials per block, output word (0 critic, 1 actor)
    float max_norm;
};

// adam_kernel (hx_wgrad.hip) with the gradient scaled by the optimizer's clip coefficient: (g * gscale) * coef, and coef == 1.0f multiplies exactly,
// so a max_norm that never binds leaves adam_kernel's bits in parameters, moments, targets and every image.
__global__ __launch_bounds__(kThreads) void hirl_adam_clip_kernel(AdamArgs A, ClipArgs K) {
    __shared__ float sum_s[2];
    if (A.guard && __hip_atomic_load(A.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;  // failed exchange: fail-stop (launch-uniform)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float wmix = A.g2 ? adam_w(A) : 0.0f;  // (read before thread 0 of block 0 may store the new weight: same value either way)
    if (wave < K.nblk) {  // (wave-uniform) wave b: block b's partials in one fixed-order tree
        const float p = lane < K.nparts ? K.parts[wave * kClipMaxParts + lane] : 0.0f;
        const float s = wave_sum(p);
        if (lane == 0) sum_s[wave] = s;
    }
    __syncthreads();
    const float sum = K.nblk > 1 ? sum_s[0] + sum_s[1] : sum_s[0];
    const float norm = sqrtf(sum) * A.gscale;
    const float coef = fminf(1.0f, K.max_norm / (norm + 1e-6f));  // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
    if (blockIdx.x == 0 && tid == 0) {
        K.out[K.slot] = norm;
        K.out[2 + K.slot] = coef;
        if (A.finish_actor) {
            if (A.use_bc) {
                const float w = adam_w(A);
                A.losses[1] = A.losses[2] * w + A.losses[3] * (1.0f - w);  // HIRL.py:321
                A.losses[5] = w;
                *A.wstate = w;
            } else {
                A.losses[1] = A.losses[3];  // TD3.py:236
            }
        }
    }
    const int i = (blockIdx.x * kThreads + tid) * 4;
    if (i >= A.n) return;
    if (i + 4 <= A.n) {  // the flat buffers are 16-B aligned and a multiple of 4 floats long: one 16-B access per array
        float4 g4 = *reinterpret_cast<const float4*>(A.g + i);
        if (A.g2) {  // g = w dL_bc + (1 - w) dL_rl  (HIRL.py:321), combined AFTER the exchange
            const float4 b4 = *reinterpret_cast<const float4*>(A.g2 + i);
            g4.x = mix(wmix, b4.x, g4.x);
            g4.y = mix(wmix, b4.y, g4.y);
            g4.z = mix(wmix, b4.z, g4.z);
            g4.w = mix(wmix, b4.w, g4.w);
        }
        adam_step4(A, i, make_float4((g4.x * A.gscale) * coef, (g4.y * A.gscale) * coef, (g4.z * A.gscale) * coef, (g4.w * A.gscale) * coef));
        return;
    }
    for (int c = 0; c < A.n - i; ++c) {  // ragged tail
        float pv = A.p[i + c], mv = A.m[i + c], vv = A.v[i + c];
        const float gv = A.g2 ? mix(wmix, A.g2[i + c], A.g[i + c]) : A.g[i + c];
        adam_update(pv, mv, vv, (gv * A.gscale) * coef, A.b1, A.b2, A.eps, A.step_size, A.bc2_sqrt);
        A.p[i + c] = pv; A.m[i + c] = mv; A.v[i + c] = vv;
        if (A.target) A.target[i + c] = polyak_update(A.target[i + c], pv, A.tau);
    }
}

inline int clip_chunks(const Mlp& m) { return (m.padded() + kClipChunk - 1) / kClipChunk; }

// which (0 critic | 1 actor) and the message -> the AdamArgs both launches read and where the optimizer's partials and results lie
int clip_fill(AdamArgs& A, SumsqArgs& S, ClipArgs& K, const HxNets* N, const HxHyper* Hy, int which, bool polyak, int step, float grad_scale, int w_kind,
              float w_given, float warm, int batch, const float* msg, float max_norm, float* clip_ws, const char* who) {
    HX_REQUIRE(N && Hy && clip_ws && step >= 1, "%s: bad arguments (nets, hyper, clip_ws, step >= 1)", who);
    HX_REQUIRE(which == 0 || which == 1, "%s: which is 0 (critic) or 1 (actor): the actor alone (2, BC pre-training) has no clip", who);
    HX_REQUIRE(!msg || which == 1, "%s: the merged message belongs to the actor step (which 1)", who);
    HX_REQUIRE(grad_scale > 0.0f, "%s: grad_scale must be positive", who);
    HX_REQUIRE((reinterpret_cast<uintptr_t>(clip_ws) & 15u) == 0, "%s: clip_ws must be 16-byte aligned", who);
    if (int rc = hirl_adam_fill(A, N, Hy, which, polyak, step, grad_scale, w_kind, w_given, warm, batch, msg, who, who)) return rc;
    HX_REQUIRE(A.p && A.g && A.m && A.v && A.n % 4 == 0, "%s: parameters, gradients and moments must be set (16-byte aligned buffers)", who);
    const Mlp m = which == 0 ? kQ : kActor;
    static_assert(kClipMaxParts <= 64, "one wave re-adds a block's partials");
    float* parts = clip_ws + kClipOutWords + (which == 0 ? 0 : 2) * kClipMaxParts;
    S = SumsqArgs{parts, which == 0 ? 2 : 1, clip_chunks(m), m.padded(), m.size()};
    HX_REQUIRE(S.nchunks <= kClipMaxParts, "%s: a block has more chunks than one wave re-adds", who);
    K = ClipArgs{parts, clip_ws, S.nblk, S.nchunks, which, max_norm};
    return 0;
}

}  // namespace

extern "C" {

int64_t hx_hirl_clip_floats(void) { return kClipWsFloats; }
/* shape[0..7] (host) <- the summation shape of the two norms: float4 per thread, words per chunk, partials re-added by one wave at most, chunks of a Q
 * head, chunks of the actor, the depth of the critic's and of the actor's whole sum in additions (squares included) — what a rounding bound is derived
 * from —, and the word of clip_ws at which the partials begin (Q head 0 | Q head 1 | actor, shape[2] words each) */
int hx_hirl_clip_shape(int32_t* shape) {
    HX_REQUIRE(shape, "hx_hirl_clip_shape: null output");
    shape[0] = kClipVecs; shape[1] = kClipChunk; shape[2] = kClipMaxParts; shape[3] = clip_chunks(kQ); shape[4] = clip_chunks(kActor);
    shape[5] = kDepthBlock + 1;  // ... and head 0 + head 1
    shape[6] = kDepthBlock;
    shape[7] = kClipOutWords;
    return 0;
}
int hx_hirl_grad_norm(const HxNets* N, const HxHyper* Hy, int32_t which, int32_t w_kind, float w_given, float warm, int32_t batch, const float* msg,
                      float* clip_ws, void* stream) {
    AdamArgs A{}; SumsqArgs S{}; ClipArgs K{};
    if (int rc = clip_fill(A, S, K, N, Hy, which, false, 1, 1.0f, w_kind, w_given, warm, batch, msg, 1.0f, clip_ws, "hx_hirl_grad_norm")) return rc;
    hipLaunchKernelGGL(hirl_grad_sumsq_kernel, dim3((unsigned)(S.nblk * S.nchunks)), dim3(kThreads), 0, (hipStream_t)stream, A, S);
    HX_CHECK_LAUNCH("hx_hirl_grad_norm");
    return 0;
}
int hx_adam_clipped(const HxNets* N, const HxHyper* Hy, int32_t which, int32_t step, float grad_scale, int32_t w_kind, float w_given, float warm,
                    int32_t batch, const float* msg, float max_norm, float* clip_ws, void* stream) {
    const bool polyak = (which & 16) != 0;  // + 16: soft_update of this network's target in the same launch
    which &= 15;
    HX_REQUIRE(max_norm > 0.0f, "hx_adam_clipped: max_norm must be positive (and not NaN)");
    AdamArgs A{}; SumsqArgs S{}; ClipArgs K{};
    if (int rc = clip_fill(A, S, K, N, Hy, which, polyak, step, grad_scale, w_kind, w_given, warm, batch, msg, max_norm, clip_ws, "hx_adam_clipped")) return rc;
    hipLaunchKernelGGL(hirl_adam_clip_kernel, dim3((unsigned)((A.n / 4 + kThreads) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, A, K);
    HX_CHECK_LAUNCH("hx_adam_clipped");
    return 0;
}

}  // extern "C"
