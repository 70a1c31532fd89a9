// hx_clip.hip — gradient-norm clipping for SAC (gfx950): update_params(optim, network, loss, grad_clip) = clip_grad_norm_ before optimizer.step()
// (SAC/utils.py:15-21, SAC/agent.py:310-320).
//   grad_sumsq    per-segment sums of squares of a flat gradient buffer, one partial per fixed 4,096-word chunk (no atomics, a fixed order)
//   adam_clip     the optimizer step (adam_step4) on g * gscale * coef[segment]; every workgroup re-adds its segments' partials and forms coef itself
// On one GPU the unclipped update steps every parameter inside the launch that produces its gradient (wgrad_kernel<ADAM>); a global norm is a grid-wide
// dependency between "all gradients written" and "any parameter stepped", so the clipped update runs wgrad (no Adam), grad_sumsq, adam_clip.
#include <cmath>

#include "hx_update.h"

using namespace hxnn;
using namespace hxu;

namespace {

// The summation shape of one segment's sum of squares (tests/test_sac_clip_gpu.py derives its rounding bound from these, through hx_sac_clip_shape):
//   a thread squares 4 float4 (kClipVecs) of its chunk: (x^2 + y^2) + (z^2 + w^2) per float4 (depth 2), added one after the other (kClipVecs - 1 deep),
//   the wave's 64 sums by wave_sum's DPP tree (6 deep), the workgroup's 4 waves as (w0 + w1) + (w2 + w3) (2 deep),
//   the segment's <= 64 partials by ONE wave_sum (6 deep) — in the stepping kernel, by every workgroup alike.
constexpr int kClipVecs = 4;                                  // float4 per thread
constexpr int kClipChunk = kThreads * 4 * kClipVecs;          // 4,096 words per workgroup
constexpr int kClipMaxParts = 64;                             // partials per segment: one wave re-adds them
constexpr int kClipOutWords = 8;                              // clip_ws[0..2] norms, [3..5] coefficients, two spare
constexpr int kClipWsFloats = kClipOutWords + 3 * kClipMaxParts;

struct SumsqArgs {
    const float* g;   // the flat gradient buffer: nseg blocks of m.padded() words
    float* parts;     // [nseg][kClipMaxParts]
    Mlp m;
    int nseg, nchunks;  // chunks per segment
};

// word e of a block counts: W1, b1 | W2, b2 | W3, b3 — not the LayerNorm slots (g1, be1 | g2, be2), not the padding behind size()
__device__ __forceinline__ bool clip_live(const Mlp& m, int e) { return e < m.g1() || (e >= m.W2() && e < m.g2()) || (e >= m.W3() && e < m.size()); }

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(SumsqArgs A) {
    __shared__ float part[4];
    const int tid = threadIdx.x, seg = blockIdx.x / A.nchunks, chunk = blockIdx.x % A.nchunks;
    const int padded = A.m.padded();
    const float* g = A.g + (size_t)seg * padded;
    float4 v[kClipVecs];
#pragma unroll
    for (int q = 0; q < kClipVecs; ++q) {  // every load in flight before the first square; past the block's end: zeros, nothing read
        const int e = chunk * kClipChunk + (q * kThreads + tid) * 4;
        v[q] = e + 4 <= padded ? *reinterpret_cast<const float4*>(g + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < kClipVecs; ++q) {
        const int e = chunk * kClipChunk + (q * kThreads + tid) * 4;
        const float x = clip_live(A.m, e) ? v[q].x : 0.0f, y = clip_live(A.m, e + 1) ? v[q].y : 0.0f;
        const float z = clip_live(A.m, e + 2) ? v[q].z : 0.0f, w = clip_live(A.m, e + 3) ? v[q].w : 0.0f;
        const float t = (x * x + y * y) + (z * z + w * w);
        s = q == 0 ? t : s + t;
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) A.parts[seg * kClipMaxParts + chunk] = (part[0] + part[1]) + (part[2] + part[3]);
}

struct ClipArgs {
    const float* parts;  // this launch's first segment's partials
    float* out;          // clip_ws: norms at [0..2], coefficients at [3..5]
    int nseg, nparts, seg_len, out_lo;  // segments of this launch, partials per segment, words per segment, first output word (0: Q1, Q2; 2: policy)
    float max_norm;
};

// adam_step4 for the SAC networks (no BC mix, no exchange guard; A.target is NULL: SAC steps no target here) with the gradient scaled by its
// segment's clip coefficient: (g * gscale) * coef, and coef == 1.0f multiplies exactly, so a max_norm that never binds leaves adam_kernel's bits in
// parameters, moments and every image.
__global__ __launch_bounds__(kThreads) void adam_clip_kernel(AdamArgs A, ClipArgs K) {
    __shared__ float coef_s[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (wave < K.nseg) {  // (wave-uniform) wave s: segment s — its partials in one fixed-order tree, the norm, the coefficient
        const float p = lane < K.nparts ? K.parts[wave * kClipMaxParts + lane] : 0.0f;
        const float norm = sqrtf(wave_sum(p)) * A.gscale;
        const float c = fminf(1.0f, K.max_norm / (norm + 1e-6f));  // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
        if (lane == 0) {
            coef_s[wave] = c;
            if (blockIdx.x == 0) { K.out[K.out_lo + wave] = norm; K.out[3 + K.out_lo + wave] = c; }
        }
    }
    __syncthreads();
    if (A.alpha_state && blockIdx.x == 0 && tid == 0)  // the log-alpha step: never clipped (update_params(self.alpha_optim, None, entropy_loss))
        sac_alpha_step(A.alpha_state, A.losses, A.losses[4], A.target_entropy, A.b1, A.b2, A.eps, A.alpha_step_size, A.bc2_sqrt);
    const int i = (blockIdx.x * kThreads + tid) * 4;
    if (i + 4 > A.n) return;  // (A.n is a multiple of 4: the blocks are padded)
    const float coef = coef_s[K.nseg > 1 && i >= K.seg_len ? 1 : 0];  // (segments start at multiples of 4 words: a float4 lies in one)
    const float4 g4 = *reinterpret_cast<const float4*>(A.g + i);
    adam_step4(A, i, make_float4((g4.x * A.gscale) * coef, (g4.y * A.gscale) * coef, (g4.z * A.gscale) * coef, (g4.w * A.gscale) * coef));
}

inline int clip_chunks(const Mlp& m) { return (m.padded() + kClipChunk - 1) / kClipChunk; }

}  // namespace

namespace hxu {

int sac_grad_norm(const HxSacNets* N, int which, float* clip_ws, hipStream_t st, const char* who) {
    HX_REQUIRE(N && (which == 0 || which == 1) && clip_ws, "%s: bad arguments (nets, which 0 critic | 1 policy, clip_ws)", who);
    const float* g = which == 0 ? N->grad_critic : N->grad_policy;
    HX_REQUIRE(g && (((uintptr_t)g | (uintptr_t)clip_ws) & 15u) == 0, "%s: the gradient buffer and clip_ws must be 16-byte aligned", who);
    const Mlp m = which == 0 ? kQs : kPolicy;
    static_assert(kClipMaxParts <= 64, "one wave re-adds a segment's partials");
    SumsqArgs A{g, clip_ws + kClipOutWords + (which == 0 ? 0 : 2) * kClipMaxParts, m, which == 0 ? 2 : 1, clip_chunks(m)};
    HX_REQUIRE(A.nchunks <= kClipMaxParts, "%s: a segment has more chunks than one wave re-adds", who);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)(A.nseg * A.nchunks)), dim3(kThreads), 0, st, A);
    HX_CHECK_LAUNCH(who);
    return 0;
}

int sac_clipped_step(const HxSacNets* N, const HxHyper* Hy, int which, int step, float grad_scale, float target_entropy, float max_norm, float* clip_ws,
                     bool alpha_step, hipStream_t st, const char* who) {
    HX_REQUIRE(N && Hy && step >= 1 && (which == 0 || which == 1) && clip_ws, "%s: bad arguments (nets, hyper, step >= 1, which 0 | 1, clip_ws)", who);
    HX_REQUIRE(max_norm > 0.0f, "%s: max_norm must be positive (and not NaN)", who);
    HX_REQUIRE(grad_scale > 0.0f, "%s: grad_scale must be positive", who);
    AdamArgs A{};
    if (int rc = sac_adam_fill(A, N, Hy, which, step, grad_scale, target_entropy, alpha_step, who)) return rc;
    HX_REQUIRE(A.p && A.g && A.m && A.v && (((uintptr_t)A.p | (uintptr_t)A.g | (uintptr_t)A.m | (uintptr_t)A.v | (uintptr_t)clip_ws) & 15u) == 0 && A.n % 4 == 0,
               "%s: parameters, gradients, moments and clip_ws must be 16-byte aligned buffers", who);
    const Mlp m = which == 0 ? kQs : kPolicy;
    ClipArgs K{clip_ws + kClipOutWords + (which == 0 ? 0 : 2) * kClipMaxParts, clip_ws, which == 0 ? 2 : 1, clip_chunks(m), m.padded(), which == 0 ? 0 : 2, max_norm};
    hipLaunchKernelGGL(adam_clip_kernel, dim3((unsigned)((A.n / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, A, K);
    HX_CHECK_LAUNCH(who);
    return 0;
}

}  // namespace hxu

extern "C" {

int64_t hx_sac_clip_floats(void) { return kClipWsFloats; }
/* shape[0..5] (host) <- the summation shape of a segment's sum of squares: float4 per thread, words per chunk, partials re-added by one wave at most,
 * chunks of a Q segment, chunks of the policy segment, the depth of the whole sum in additions (squares included) — what a rounding bound is derived from */
int hx_sac_clip_shape(int32_t* shape6) {
    HX_REQUIRE(shape6, "hx_sac_clip_shape: null output");
    shape6[0] = kClipVecs; shape6[1] = kClipChunk; shape6[2] = kClipMaxParts; shape6[3] = clip_chunks(kQs); shape6[4] = clip_chunks(kPolicy);
    shape6[5] = 1 + 2 + (kClipVecs - 1) + 6 + 2 + 6;  // square, float4 tree, the thread's sequence, wave tree, four waves, the partials' wave tree
    return 0;
}
int hx_sac_grad_norm(const HxSacNets* N, int32_t which, float* clip_ws, void* stream) {
    return sac_grad_norm(N, which, clip_ws, (hipStream_t)stream, "hx_sac_grad_norm");
}
int hx_sac_adam_clipped(const HxSacNets* N, const HxHyper* Hy, int32_t which, int32_t step, float grad_scale, float target_entropy, float max_norm,
                        float* clip_ws, void* stream) {
    return sac_clipped_step(N, Hy, which, step, grad_scale, target_entropy, max_norm, clip_ws, /*alpha_step=*/true, (hipStream_t)stream, "hx_sac_adam_clipped");
}

}  // extern "C"
