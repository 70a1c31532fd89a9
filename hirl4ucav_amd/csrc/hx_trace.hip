// hx_trace.hip — the record of validation episodes, kept on the device (gfx950): behind every env step of a batched validation one small launch
// appends the step of each tracked env whose episode is still running to a log and latches what the reference's validate() reads when it SEES
// done (train_all.py:22-102: the score so far, the step, the flags, the launch counters).  The kernels keep simulating an env after its done;
// nothing after the first done enters the record or the score.  The rule is stated in include/hirl4ucav.h ("Episode record") and, in numpy, in
// tests/_trace_model.py.
//
// One tracked env per lane, 64 per workgroup.  The log is field-major, then step, then tracked env, and the summaries are struct-of-arrays, so
// every store of a wave is one contiguous run; with env_ids == NULL the seven state words and the three step outputs are contiguous reads too
// (with a list: gathers).  Memory-bound and tiny: per running env and step 40 B read, 32 B of log and 12 B of summary written.  No LDS, no
// float atomics, at most one integer atomic per wave.
#include "hx_common.h"

#pragma clang fp contract(off)
namespace {

constexpr int kEnvs = 64;  // tracked envs per workgroup = one wave
constexpr int kAllyPos = 0, kOppoPos = 13, kFlags = 35;  // state words (hirl4ucav.h "Env state layout")

struct PushArgs {
    HxTrace T;
    const uint32_t* state; int64_t n, stride;
    const float* reward; const uint8_t* done; const int8_t* success; const int32_t* env_ids;
    int t;
};

__global__ __launch_bounds__(kEnvs) void trace_reset_kernel(HxTrace T) {
    const int64_t j = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    if (j == 0) *T.alive = (int32_t)T.k;
    if (j >= T.k) return;
    T.total[j] = 0.f;
    T.nrec[j] = 0;
    T.end_step[j] = -1;
    T.end_flags[j] = 0u;
    T.launches[j] = 0;
    T.hits[j] = 0;
}

__global__ __launch_bounds__(kEnvs) void trace_push_kernel(PushArgs A) {
    const HxTrace& T = A.T;
    const int64_t j = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    bool ending = false;
    if (j < T.k && T.end_step[j] < 0) {
        const int64_t i = A.env_ids ? (int64_t)A.env_ids[j] : j;
        if (i >= 0 && i < A.n) {  // (an id outside the env records nothing: never an address outside the state)
            const float r = A.reward[i];
            const int succ = A.success[i];
            const uint32_t flags = A.state[kFlags * A.stride + i];
            const int64_t fs = (int64_t)T.cap_steps * T.k, at = (int64_t)A.t * T.k + j;  // + field * fs
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                T.log[f * fs + at] = A.state[(kAllyPos + f) * A.stride + i];
                T.log[(3 + f) * fs + at] = A.state[(kOppoPos + f) * A.stride + i];
            }
            T.log[6 * fs + at] = __float_as_uint(r);
            T.log[7 * fs + at] = (flags & 0xffffu) | ((uint32_t)(uint8_t)succ << 16);
            T.total[j] = T.total[j] + r;
            T.nrec[j] = A.t + 1;
            if (succ != 0) T.launches[j] += 1;
            if (succ == 1) T.hits[j] += 1;
            ending = A.done[i] != 0;
            if (ending) {
                T.end_step[j] = A.t;
                T.end_flags[j] = flags;
            }
        }
    }
    const unsigned long long b = __ballot(ending);
    if (b != 0ull && threadIdx.x == 0) atomicSub(T.alive, __popcll(b));
}

int check(const HxTrace* tr, const char* who) {
    HX_REQUIRE(tr && tr->log && tr->total && tr->nrec && tr->end_step && tr->end_flags && tr->launches && tr->hits && tr->alive,
               "%s: an HxTrace with its log, six summary arrays and the alive word", who);
    HX_REQUIRE(tr->k > 0 && tr->k < (1ll << 31), "%s: 0 < k < 2^31", who);
    HX_REQUIRE(tr->cap_steps > 0, "%s: cap_steps > 0, got %d", who, tr->cap_steps);
    return 0;
}

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

int hx_trace_sizeof(void) { return (int)sizeof(HxTrace); }

int64_t hx_trace_workspace_words(int64_t k, int32_t cap_steps) {
    if (k <= 0 || k >= (1ll << 31) || cap_steps <= 0) return 0;
    return k * ((int64_t)HX_TRACE_FIELDS * cap_steps + HX_TRACE_SUMMARIES) + 1;
}

int hx_trace_reset(const HxTrace* tr, void* stream) {
    if (int rc = check(tr, "hx_trace_reset")) return rc;
    const unsigned grid = (unsigned)((tr->k + kEnvs - 1) / kEnvs);
    hipLaunchKernelGGL(trace_reset_kernel, dim3(grid), dim3(kEnvs), 0, (hipStream_t)stream, *tr);
    HX_CHECK_LAUNCH("hx_trace_reset");
    return 0;
}

int hx_trace_push(const HxTrace* tr, const float* state, int64_t n, int64_t stride, const float* reward, const uint8_t* done, const int8_t* success,
                  const int32_t* env_ids, int32_t t, void* stream) {
    if (int rc = check(tr, "hx_trace_push")) return rc;
    HX_REQUIRE(state && reward && done && success, "hx_trace_push: state, reward, done and success");
    HX_REQUIRE(n > 0 && n < (1ll << 31) && stride >= n, "hx_trace_push: 0 < n < 2^31 and stride >= n, got n = %lld, stride = %lld", (long long)n,
               (long long)stride);
    HX_REQUIRE(env_ids || tr->k <= n, "hx_trace_push: without env_ids the tracked envs are 0..k-1: k = %lld > n = %lld", (long long)tr->k, (long long)n);
    HX_REQUIRE(t >= 0 && t < tr->cap_steps, "hx_trace_push: step %d is outside the log's 0..%d", t, tr->cap_steps - 1);
    PushArgs A{*tr, reinterpret_cast<const uint32_t*>(state), n, stride, reward, done, success, env_ids, (int)t};
    const unsigned grid = (unsigned)((tr->k + kEnvs - 1) / kEnvs);
    hipLaunchKernelGGL(trace_push_kernel, dim3(grid), dim3(kEnvs), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_trace_push");
    return 0;
}

}  // extern "C"
