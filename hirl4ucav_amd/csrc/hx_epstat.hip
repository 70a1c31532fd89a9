// hx_epstat.hip — per-episode statistics of a training population, binned by scenario (gfx950): behind every acting launch one small launch adds
// each env's reward to its running return and, where an episode left (done, or the time limit), adds return, length and the way it ended to the
// statistics of the env's scenario — the reference's totalReward / step of an episode (train_all.py:341-354, 383-385), which the vector loop never
// had.  The rule is stated in include/hirl4ucav.h ("Episode statistics") and, in numpy, in tests/_epstat_model.py.
//
// One env per lane, 64 per workgroup.  The per-env words are struct-of-arrays, so every load and store of a wave is one contiguous run; the
// workgroup's 64 lanes meet in LDS (10 values per lane, 4,672 B; the lanes' bins travel as two ballots), and lanes 0..35 each own ONE 8-byte word
// of the workgroup's slot of `part`: they add the lanes of their bin in lane order 0..63 and the slot is stored as one 288-byte run.  The same
// workgroup sees the same envs on every call, so there is no atomic of any kind, no workgroup waits for another, and the same inputs give the same
// bits.  Memory-bound and tiny: per env and call 22 B read, 12 B written, and 576 B of partials per workgroup.
#include "hx_common.h"

#pragma clang fp contract(off)
namespace {

constexpr int kEnvs = 64;     // envs per workgroup = one wave
constexpr int kFlags = 35;    // state word (hirl4ucav.h "Env state layout"); the scenario id is bits 8..9
constexpr int kSums = HX_EPSTAT_SUMS, kBins = HX_EPSTAT_BINS, kSlot = HX_EPSTAT_SLOT_WORDS;
static_assert(kSlot == kBins * kSums + kBins && kSlot <= kEnvs, "one lane per word of a workgroup's slot");
enum { S_COUNT = 0, S_DONE, S_TIME_LIMIT, S_LEN, S_RET, S_RET_SQ, S_FIRE_GOOD, S_FIRE_BAD };
static_assert(S_FIRE_BAD + 1 == kSums, "hirl4ucav.h HX_EPSTAT_SUMS");

struct PushArgs {
    HxEpStat E;
    const uint32_t* state; int64_t n, stride;
    const float* reward; const uint8_t* done; const int8_t* success; const uint32_t* episode_ctr;
};

__device__ __forceinline__ unsigned long long pack_min_max(float mn, float mx) {
    return (unsigned long long)__float_as_uint(mn) | ((unsigned long long)__float_as_uint(mx) << 32);
}

__device__ __forceinline__ void clear_slot(const HxEpStat& E, int tid) {
    if (tid >= kSlot) return;
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(E.part) + (int64_t)blockIdx.x * kSlot;
    slot[tid] = tid < kBins * kSums ? 0ull : pack_min_max(__builtin_inff(), -__builtin_inff());
}

__global__ __launch_bounds__(kEnvs) void epstat_clear_kernel(HxEpStat E) { clear_slot(E, threadIdx.x); }

__global__ __launch_bounds__(kEnvs) void epstat_reset_kernel(HxEpStat E, const uint32_t* episode_ctr) {
    const int64_t i = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    clear_slot(E, threadIdx.x);
    if (i >= E.n_envs) return;
    E.acc[i] = 0.f;
    E.len[i] = 0u;
    E.last_ctr[i] = episode_ctr[i];
}

__global__ __launch_bounds__(kEnvs) void epstat_push_kernel(PushArgs A) {
    __shared__ double s_val[kSums][kEnvs + 1];  // each lane's contribution to the sums of ITS bin (+1: the eight fields of a lane in eight banks)
    __shared__ float s_min[kEnvs], s_max[kEnvs];
    const HxEpStat& E = A.E;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kEnvs + tid;
    int bin = 0;
    bool leaves = false, dn = false;
    float ret = 0.f;
    uint32_t len = 0u;
    int succ = 0;
    // the word of the workgroup's slot this lane owns, requested before everything else: its round trip hides behind the per-env loads
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(E.part) + (int64_t)blockIdx.x * kSlot;
    const bool owns = tid < kSlot;
    const unsigned long long old = owns ? slot[tid] : 0ull;
    if (i < E.n_envs) {
        bin = (int)((A.state[kFlags * A.stride + i] >> 8) & 3u);
        succ = A.success[i];
        dn = A.done[i] != 0;
        const float r = A.reward[i];
        const uint32_t ctr = A.episode_ctr[i];
        const bool trunc = ctr != E.last_ctr[i] && !dn;
        ret = E.acc[i];
        len = E.len[i];
        if (!trunc) {  // (the time-limit step's reward stays out of the return: train_all.py:346-354 breaks before totalReward += reward)
            ret = ret + r;
            len += 1u;
        }
        leaves = trunc || dn;
        E.acc[i] = leaves ? 0.f : ret;
        E.len[i] = leaves ? 0u : len;
        E.last_ctr[i] = ctr;
    }
    const double dret = (double)ret;
    const unsigned long long bin_lo = __ballot(bin & 1), bin_hi = __ballot(bin & 2);  // every lane's bin, in scalar registers
    s_val[S_COUNT][tid] = leaves ? 1.0 : 0.0;
    s_val[S_DONE][tid] = (leaves && dn) ? 1.0 : 0.0;
    s_val[S_TIME_LIMIT][tid] = (leaves && !dn) ? 1.0 : 0.0;
    s_val[S_LEN][tid] = leaves ? (double)len : 0.0;
    s_val[S_RET][tid] = leaves ? dret : 0.0;
    s_val[S_RET_SQ][tid] = leaves ? dret * dret : 0.0;
    s_val[S_FIRE_GOOD][tid] = succ == 1 ? 1.0 : 0.0;
    s_val[S_FIRE_BAD][tid] = succ == -1 ? 1.0 : 0.0;
    s_min[tid] = leaves ? ret : __builtin_inff();
    s_max[tid] = leaves ? ret : -__builtin_inff();
    __syncthreads();
    // word `tid` of the slot: a sum of bin tid / 8 (words 0..31), or the packed (min, max) of bin tid - 32 (words 32..35); lanes 0..63 in order.  One
    // loop for both kinds (a lane keeps what its word needs), so that the wave walks the 64 lanes once.
    const bool is_sum = tid < kBins * kSums;
    const int b = is_sum ? tid / kSums : (tid & (kBins - 1)), f = tid % kSums;
    double c = 0.0;
    float mn = __uint_as_float((uint32_t)old), mx = __uint_as_float((uint32_t)(old >> 32));
#pragma unroll
    for (int l = 0; l < kEnvs; ++l) {  // (c is never -0.0, so the + 0.0 of another bin's lane changes no bit)
        const bool mine = ((int)((bin_lo >> l) & 1ull) | ((int)((bin_hi >> l) & 1ull) << 1)) == b;
        const double v = s_val[f][l];
        const float lo = s_min[l], hi = s_max[l];
        c = c + (mine ? v : 0.0);
        mn = (mine && lo < mn) ? lo : mn;
        mx = (mine && hi > mx) ? hi : mx;
    }
    if (owns) slot[tid] = is_sum ? (unsigned long long)__double_as_longlong(__longlong_as_double((long long)old) + c) : pack_min_max(mn, mx);
}

int check(const HxEpStat* es, const char* who) {
    HX_REQUIRE(es && es->part && es->acc && es->len && es->last_ctr, "%s: an HxEpStat with its partials and three per-env arrays", who);
    HX_REQUIRE(es->n_envs > 0 && es->n_envs < (1ll << 31), "%s: 0 < n_envs < 2^31", who);
    HX_REQUIRE(((uintptr_t)es->part & 7u) == 0, "%s: part is 8-byte aligned", who);
    return 0;
}

unsigned grid_of(const HxEpStat* es) { return (unsigned)((es->n_envs + kEnvs - 1) / kEnvs); }

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

int hx_epstat_sizeof(void) { return (int)sizeof(HxEpStat); }

int64_t hx_epstat_workspace_words(int64_t n_envs) {
    if (n_envs <= 0 || n_envs >= (1ll << 31)) return 0;
    return ((n_envs + kEnvs - 1) / kEnvs) * (2 * kSlot) + 3 * n_envs;
}

int hx_epstat_reset(const HxEpStat* es, const uint32_t* episode_ctr, void* stream) {
    if (int rc = check(es, "hx_epstat_reset")) return rc;
    HX_REQUIRE(episode_ctr, "hx_epstat_reset: episode_ctr [n_envs]");
    hipLaunchKernelGGL(epstat_reset_kernel, dim3(grid_of(es)), dim3(kEnvs), 0, (hipStream_t)stream, *es, episode_ctr);
    HX_CHECK_LAUNCH("hx_epstat_reset");
    return 0;
}

int hx_epstat_clear(const HxEpStat* es, void* stream) {
    if (int rc = check(es, "hx_epstat_clear")) return rc;
    hipLaunchKernelGGL(epstat_clear_kernel, dim3(grid_of(es)), dim3(kEnvs), 0, (hipStream_t)stream, *es);
    HX_CHECK_LAUNCH("hx_epstat_clear");
    return 0;
}

int hx_epstat_push(const HxEpStat* es, const float* state, int64_t n, int64_t stride, const float* reward, const uint8_t* done, const int8_t* success,
                   const uint32_t* episode_ctr, void* stream) {
    if (int rc = check(es, "hx_epstat_push")) return rc;
    HX_REQUIRE(state && reward && done && success && episode_ctr, "hx_epstat_push: state, reward, done, success and episode_ctr");
    HX_REQUIRE(n == es->n_envs && stride >= n, "hx_epstat_push: n = n_envs and stride >= n, got n = %lld, n_envs = %lld, stride = %lld", (long long)n,
               (long long)es->n_envs, (long long)stride);
    PushArgs A{*es, reinterpret_cast<const uint32_t*>(state), n, stride, reward, done, success, episode_ctr};
    hipLaunchKernelGGL(epstat_push_kernel, dim3(grid_of(es)), dim3(kEnvs), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_epstat_push");
    return 0;
}

}  // extern "C"
