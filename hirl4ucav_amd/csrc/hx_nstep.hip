// hx_nstep.hip — truncated n-step returns behind an acting launch that runs WITHOUT a replay ring (gfx950): a window of the last n steps per env,
// finished rows written into the ordinary ring in the ordinary 32-word format (SacAgent(multi_step=n): SAC/agent.py:121-124; the memory class itself
// lives in the un-vendored rltorch, so the rule here is this project's own — include/hirl4ucav.h "n-step returns").
//
// One env per lane, 64 envs per workgroup.  Everything a lane touches in global memory is struct-of-arrays over envs, so a wave-instruction reads
// or writes one 256-B run; the row-major observations and the finished rows meet in LDS (the staging pattern of hx_env_block.h).  Memory-bound:
// per env and step about 110 B of inputs, 120 B of obs_prev / head words, 8 B per pending head, and — in the steady state of one finished row per
// env and step — 80 B of window read, 72 B of window written and one 128-B ring line.
#include "hx_common.h"
#include "hx_env_block.h"

#pragma clang fp contract(off)
namespace {

using hxenv::ring_slot;
using hxenv::wrap_slot;

constexpr int kEnvs = 64;                      // envs per workgroup = one wave
constexpr int kRowPitch = HX_ROW_WORDS + 1;    // +1: conflict-free per-lane row writes
constexpr int kObsTile = kEnvs * HX_OBS_DIM;
// fields of a head in the window, win[field][head][env]
enum { F_S = 0, F_A = HX_OBS_DIM, F_ACC = F_A + HX_ACT_DIM, F_BOOT, F_SUCC, F_COUNT };
static_assert(F_COUNT == HX_NSTEP_FIELDS, "hirl4ucav.h HX_NSTEP_FIELDS");
typedef float ns_v4f __attribute__((ext_vector_type(4)));

struct PushArgs {
    float* win; uint32_t* hc; float* obs_prev; uint32_t* last_ctr;
    int64_t n_envs;
    int n;
    float gamma;
    const float* obs_new; const float* actions; const float* reward; const uint8_t* done; const int8_t* success; const uint32_t* episode_ctr;
    float* ring; int8_t* ring_success;
    int64_t cap;
    unsigned long long* total;
    double inv_cap;
};

__global__ __launch_bounds__(kEnvs) void nstep_reset_kernel(float* win, int n, uint32_t* hc, float* obs_prev, uint32_t* last_ctr, int64_t n_envs,
                                                            const float* obs, const uint32_t* episode_ctr) {
    const int64_t i = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    if (i >= n_envs) return;
    for (int k = 0; k < F_COUNT * n; ++k) win[(int64_t)k * n_envs + i] = 0.f;  // (every field of every head position: a snapshot holds no stale word)
    hc[i] = 0u;
    last_ctr[i] = episode_ctr[i];
#pragma unroll
    for (int f = 0; f < HX_OBS_DIM; ++f) obs_prev[(int64_t)f * n_envs + i] = obs[i * HX_OBS_DIM + f];
}

// inclusive scan of small non-negative counts over the 64 lanes of the wave
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__global__ __launch_bounds__(kEnvs) void nstep_push_kernel(PushArgs A) {
    __shared__ float s_obs[kObsTile];            // the workgroup's next observations, row-major as the env leaves them
    __shared__ float s_row[kEnvs * kRowPitch];   // one finished row per lane and round
    __shared__ unsigned s_slot[kEnvs];           // its ring slot
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * kEnvs, i = i0 + tid, N = A.n_envs;
    const int nblk = (int)((N - i0) < kEnvs ? (N - i0) : kEnvs);
    const bool active = tid < nblk;
    const int n = A.n;

    hxenv::tile_copy<kEnvs, kObsTile>(s_obs, A.obs_new + i0 * HX_OBS_DIM, nblk * HX_OBS_DIM, tid);

    float op[HX_OBS_DIM];  // obs_prev: the state this step started from
    float4 act = {0.f, 0.f, 0.f, 0.f};
    float r = 0.f, succ = 0.f;
    bool dn = false, trunc = false;
    int head = 0, count = 0, nemit = 0;
    uint32_t ctr = 0u;
    if (active) {
#pragma unroll
        for (int f = 0; f < HX_OBS_DIM; ++f) op[f] = A.obs_prev[(int64_t)f * N + i];
        act = reinterpret_cast<const float4*>(A.actions)[i];
        r = A.reward[i];
        succ = (float)A.success[i];
        dn = A.done[i] != 0;
        ctr = A.episode_ctr[i];
        trunc = ctr != A.last_ctr[i] && !dn;
        const uint32_t hc = A.hc[i];
        head = (int)(hc & 0xffu);
        count = (int)(hc >> 8);
        if (head >= n || count >= n) head = count = 0;  // (words that were never reset: an empty window, never an index outside it)
        if (!trunc) ++count;                            // the new head is head number count - 1
        nemit = (trunc || dn) ? count : (count == n ? 1 : 0);
    } else {
#pragma unroll
        for (int f = 0; f < HX_OBS_DIM; ++f) op[f] = 0.f;
    }
    // ring slots: rows by env, then oldest head first -> a prefix over the lanes' counts, ONE atomic per workgroup
    const int incl = wave_scan_incl(nemit, tid);
    const int wg_rows = __shfl(incl, 63), first = incl - nemit;
    unsigned slot0 = 0u;
    if (wg_rows > 0) {
        unsigned long long t0 = 0ull;
        if (tid == 0) t0 = atomicAdd(A.total, (unsigned long long)wg_rows);
        t0 = ((unsigned long long)(unsigned)__shfl((int)(t0 >> 32), 0) << 32) | (unsigned)__shfl((int)t0, 0);
        slot0 = ring_slot(t0, (unsigned long long)A.cap, A.inv_cap);
    }
    int maxcount = count;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) maxcount = max(maxcount, __shfl_xor(maxcount, d));
    __syncthreads();  // s_obs complete

    const unsigned cap = (unsigned)A.cap;
    for (int j = 0; j < maxcount; ++j) {  // head j of every lane, oldest first (a uniform trip count)
        const bool live = j < count;
        const bool emit = j < nemit;
        if (live) {
            int pos = head + j;
            pos = pos >= n ? pos - n : pos;
            const int64_t at = (int64_t)pos * N + i;           // + field * n * N
            const int64_t fs = (int64_t)n * N;
            const bool fresh = !trunc && j == count - 1;       // the head pushed by this call: still in registers
            float acc = 0.f, boot = 0.f;
            if (!fresh) { acc = A.win[F_ACC * fs + at]; boot = A.win[F_BOOT * fs + at]; }
            if (!trunc) {
                const float w = fresh ? 1.0f : boot * A.gamma;
                acc = acc + w * r;
                boot = w;
            }
            if (emit) {
                float* row = s_row + tid * kRowPitch;
                if (fresh) {
#pragma unroll
                    for (int f = 0; f < HX_OBS_DIM; ++f) row[f] = op[f];
                    row[13] = act.x; row[14] = act.y; row[15] = act.z; row[16] = act.w;
                } else {
#pragma unroll
                    for (int f = 0; f < HX_OBS_DIM + HX_ACT_DIM; ++f) row[f] = A.win[(int64_t)f * fs + at];
                }
                const float* sp = s_obs + tid * HX_OBS_DIM;
#pragma unroll
                for (int f = 0; f < HX_OBS_DIM; ++f) row[17 + f] = trunc ? op[f] : sp[f];
                row[30] = acc;
                row[31] = (dn && !trunc) ? 1.0f : 1.0f - boot;
                const unsigned slot = wrap_slot(slot0 + (unsigned)(first + j), cap);
                s_slot[tid] = slot;
                if (A.ring_success) A.ring_success[slot] = (int8_t)(fresh ? succ : A.win[F_SUCC * fs + at]);
            } else {
                A.win[F_ACC * fs + at] = acc;
                A.win[F_BOOT * fs + at] = boot;
                if (fresh) {
#pragma unroll
                    for (int f = 0; f < HX_OBS_DIM; ++f) A.win[(int64_t)f * fs + at] = op[f];
                    A.win[(F_A + 0) * fs + at] = act.x; A.win[(F_A + 1) * fs + at] = act.y;
                    A.win[(F_A + 2) * fs + at] = act.z; A.win[(F_A + 3) * fs + at] = act.w;
                    A.win[F_SUCC * fs + at] = succ;
                }
            }
        }
        const unsigned long long b = __ballot(emit && live);
        if (b == 0ull) continue;  // (uniform)
        __syncthreads();
        // the round's rows as whole 128-B lines: 8 lanes per row, 16 B each
        float4* ring4 = reinterpret_cast<float4*>(A.ring);
#pragma unroll
        for (int it = 0; it < kEnvs * (HX_ROW_WORDS / 4) / kEnvs; ++it) {
            const int k = tid + it * kEnvs;
            const int rr = k >> 3, c = (k & 7) * 4;
            if ((b >> rr) & 1ull) {
                const float* src = s_row + rr * kRowPitch + c;
                const ns_v4f v = {src[0], src[1], src[2], src[3]};
                __builtin_nontemporal_store(v, reinterpret_cast<ns_v4f*>(ring4) + (size_t)s_slot[rr] * (HX_ROW_WORDS / 4) + (k & 7));
            }
        }
        __syncthreads();  // s_row / s_slot are free for the next round
    }
    if (active) {
        int h = head, c = count;
        if (trunc || dn) { h = 0; c = 0; }
        else if (c == n) { h = h + 1 >= n ? 0 : h + 1; c = n - 1; }
        A.hc[i] = (uint32_t)h | ((uint32_t)c << 8);
        A.last_ctr[i] = ctr;
        const float* sp = s_obs + tid * HX_OBS_DIM;
#pragma unroll
        for (int f = 0; f < HX_OBS_DIM; ++f) A.obs_prev[(int64_t)f * N + i] = sp[f];
    }
}

int check(const HxNStep* ns, const char* who) {
    HX_REQUIRE(ns && ns->win && ns->hc && ns->obs_prev && ns->last_ctr, "%s: an HxNStep with its four buffers", who);
    HX_REQUIRE(ns->n_envs > 0 && ns->n_envs < (1ll << 31), "%s: 0 < n_envs < 2^31", who);
    HX_REQUIRE(ns->n >= 1 && ns->n <= HX_NSTEP_MAX, "%s: n is 1..%d, got %d", who, HX_NSTEP_MAX, ns->n);
    HX_REQUIRE(ns->gamma >= 0.0f && ns->gamma <= 1.0f, "%s: gamma in [0, 1]", who);
    return 0;
}

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

int hx_nstep_sizeof(void) { return (int)sizeof(HxNStep); }

int64_t hx_nstep_workspace_floats(int64_t n_envs, int32_t n) {
    if (n_envs <= 0 || n < 1 || n > HX_NSTEP_MAX) return 0;
    return n_envs * ((int64_t)HX_NSTEP_FIELDS * n + HX_OBS_DIM + 2);
}

int hx_nstep_reset(const HxNStep* ns, const float* obs, const uint32_t* episode_ctr, void* stream) {
    if (int rc = check(ns, "hx_nstep_reset")) return rc;
    HX_REQUIRE(obs && episode_ctr, "hx_nstep_reset: obs [n_envs][13] and episode_ctr [n_envs]");
    const unsigned grid = (unsigned)((ns->n_envs + kEnvs - 1) / kEnvs);
    hipLaunchKernelGGL(nstep_reset_kernel, dim3(grid), dim3(kEnvs), 0, (hipStream_t)stream, ns->win, (int)ns->n, ns->hc, ns->obs_prev, ns->last_ctr, ns->n_envs,
                       obs, episode_ctr);
    HX_CHECK_LAUNCH("hx_nstep_reset");
    return 0;
}

int hx_nstep_push(const HxNStep* ns, const float* obs_new, const float* actions, const float* reward, const uint8_t* done, const int8_t* success,
                  const uint32_t* episode_ctr, float* ring, int8_t* ring_success, int64_t cap, uint64_t* total, void* stream) {
    if (int rc = check(ns, "hx_nstep_push")) return rc;
    HX_REQUIRE(obs_new && actions && reward && done && success && episode_ctr, "hx_nstep_push: obs_new, actions, reward, done, success and episode_ctr");
    HX_REQUIRE(ring && total, "hx_nstep_push: the ring and its counter");
    HX_REQUIRE(cap >= (int64_t)ns->n * ns->n_envs, "hx_nstep_push: one call can emit n * n_envs = %lld rows, the ring holds %lld", (long long)ns->n * ns->n_envs,
               (long long)cap);
    HX_REQUIRE(cap < (1ll << 31), "hx_nstep_push: cap < 2^31");
    PushArgs A{ns->win, ns->hc, ns->obs_prev, ns->last_ctr, ns->n_envs, ns->n, ns->gamma, obs_new, actions, reward, done, success, episode_ctr,
               ring, ring_success, cap, (unsigned long long*)total, 1.0 / (double)cap};
    const unsigned grid = (unsigned)((ns->n_envs + kEnvs - 1) / kEnvs);
    hipLaunchKernelGGL(nstep_push_kernel, dim3(grid), dim3(kEnvs), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_nstep_push");
    return 0;
}

}  // extern "C"
