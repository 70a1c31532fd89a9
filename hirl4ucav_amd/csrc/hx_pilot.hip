// hx_pilot.hip — the scripted pursuit pilot (data/expert_pilot.py pursuit_actions) as kernels (gfx950), so that the expert can be asked what it would do
// in the states the learner reaches: hx_pilot_act flies a population, hx_pilot_refresh relabels a few envs' observations behind every acting launch
// and writes them as (s, a) rows into the online region of the BC table (dataset aggregation; no counterpart in the reference, whose expert lives in
// an external simulator).  The rule is stated in include/hirl4ucav.h ("The pilot as a kernel") and, in numpy, in tests/_pilot_model.py.
//
// Both kernels: one env per lane, 64 per workgroup, fp32 without contraction, correctly rounded divide and square root (hipcc's default; no fast
// intrinsics).  hx_pilot_act reads each of its ten state words as one contiguous run per wave and stores one float4 per lane.  hx_pilot_refresh gathers
// its k picks (they are spread over the population on purpose), stages the finished rows in LDS (8 KB) and writes each as one whole 128-byte line,
// eight lanes of 16 bytes.  No atomics, no workgroup waits for another, no scratch; the slots of one call are distinct (k <= M), so no two lanes write
// the same line.
#include "hx_common.h"
#include "hx_pilot_dev.h"  // pursuit_levels, clamp1, finite_word: the pilot's law, shared with hx_branch.hip

#pragma clang fp contract(off)
namespace {

using namespace hxpilot;

constexpr int kEnvs = 64;  // envs (act) or picks (refresh) per workgroup = one wave

__global__ __launch_bounds__(kEnvs) void pilot_act_kernel(const float* __restrict__ state, int64_t n, int64_t stride, const float* __restrict__ obs,
                                                          const float* __restrict__ noise, float* __restrict__ actions) {
    const int64_t i = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    if (i >= n) return;
    float l0, l1, l2;
    pursuit_levels(state, stride, i, l0, l1, l2);
    if (noise) {
        l0 = l0 + noise[i * 3 + 0];
        l1 = l1 + noise[i * 3 + 1];
        l2 = l2 + noise[i * 3 + 2];
    }
    const float fire = (obs[i * kObs + 7] > 0.f && obs[i * kObs + 8] > 0.f) ? 1.f : -1.f;
    reinterpret_cast<float4*>(actions)[i] = make_float4(clamp1(l0), clamp1(l1), clamp1(l2), fire);
}

struct RefreshArgs {
    const float* state; int64_t n, stride;
    const float* obs; float* table;
    int64_t offline_rows, online_rows;
    int32_t per_call;
    uint32_t step;       // floor(n / per_call)
    uint32_t call_mod_n; // call mod n
    uint32_t base_mod_m; // (call * per_call) mod online_rows
};

__global__ __launch_bounds__(kEnvs) void pilot_refresh_kernel(RefreshArgs A) {
    __shared__ float4 s_row[kEnvs][kRow / 4];
    __shared__ int64_t s_slot[kEnvs];  // the table row of pick j, or -1: nothing is written
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kEnvs + tid;
    int64_t slot = -1;
    if (j < A.per_call) {
        uint32_t e32 = A.call_mod_n + (uint32_t)j * A.step;  // both terms below n < 2^31: one conditional subtraction is the mod
        if (e32 >= (uint32_t)A.n) e32 -= (uint32_t)A.n;
        const int64_t e = (int64_t)e32;
        float l0, l1, l2;
        pursuit_levels(A.state, A.stride, e, l0, l1, l2);
        float v[kRow];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < kObs; ++c) {
            v[c] = A.obs[e * kObs + c];
            ok = ok && finite_word(v[c]);
        }
        v[13] = clamp1(l0);
        v[14] = clamp1(l1);
        v[15] = clamp1(l2);
        v[16] = (v[7] > 0.f && v[8] > 0.f) ? 1.f : -1.f;
        ok = ok && finite_word(v[13]) && finite_word(v[14]) && finite_word(v[15]);
#pragma unroll
        for (int c = 17; c < kRow; ++c) v[c] = 0.f;
#pragma unroll
        for (int q = 0; q < kRow / 4; ++q) s_row[tid][q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        uint32_t o32 = A.base_mod_m + (uint32_t)j;  // j < per_call <= M < 2^31, likewise
        if (o32 >= (uint32_t)A.online_rows) o32 -= (uint32_t)A.online_rows;
        if (ok) slot = A.offline_rows + (int64_t)o32;
    }
    s_slot[tid] = slot;
    __syncthreads();
    // the workgroup's rows as whole 128-byte lines: 8 lanes per row, 16 bytes each
    float4* table4 = reinterpret_cast<float4*>(A.table);
    const int q = tid & 7;
#pragma unroll
    for (int r0 = 0; r0 < kEnvs; r0 += 8) {
        const int r = r0 + (tid >> 3);
        const int64_t to = s_slot[r];
        if (to >= 0) table4[to * (kRow / 4) + q] = s_row[r][q];
    }
}

int check_env(const char* who, const float* state, int64_t n, int64_t stride, const float* obs) {
    HX_REQUIRE(state && obs, "%s: state [37][stride] and obs [n][13]", who);
    HX_REQUIRE(n > 0 && n < (1ll << 31) && stride >= n, "%s: 0 < n < 2^31 and stride >= n, got n = %lld, stride = %lld", who, (long long)n, (long long)stride);
    return 0;
}

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

int hx_pilot_act(const float* state, int64_t n, int64_t stride, const float* obs, const float* noise, float* actions, void* stream) {
    if (int rc = check_env("hx_pilot_act", state, n, stride, obs)) return rc;
    HX_REQUIRE(actions && ((uintptr_t)actions & 15u) == 0, "hx_pilot_act: actions [n][4], 16-byte aligned");
    hipLaunchKernelGGL(pilot_act_kernel, dim3((unsigned)((n + kEnvs - 1) / kEnvs)), dim3(kEnvs), 0, (hipStream_t)stream, state, n, stride, obs, noise, actions);
    HX_CHECK_LAUNCH("hx_pilot_act");
    return 0;
}

int hx_pilot_refresh(const float* state, int64_t n, int64_t stride, const float* obs, float* table, int64_t offline_rows, int64_t online_rows,
                     int32_t per_call, uint64_t call, void* stream) {
    if (int rc = check_env("hx_pilot_refresh", state, n, stride, obs)) return rc;
    HX_REQUIRE(table && ((uintptr_t)table & 127u) == 0, "hx_pilot_refresh: table [offline_rows + online_rows][32], 128-byte aligned");
    HX_REQUIRE(offline_rows >= 0 && online_rows >= 1 && offline_rows + online_rows < (1ll << 31),
               "hx_pilot_refresh: offline_rows >= 0, online_rows >= 1, fewer than 2^31 rows in all, got %lld and %lld", (long long)offline_rows, (long long)online_rows);
    HX_REQUIRE(per_call >= 1 && per_call <= n && per_call <= online_rows, "hx_pilot_refresh: 1 <= per_call <= min(n, online_rows), got per_call = %d, n = %lld, "
               "online_rows = %lld", (int)per_call, (long long)n, (long long)online_rows);
    // (call * per_call) mod M from the residues: exact for every 64-bit call, the product stays below 2^62
    const uint64_t m = (uint64_t)online_rows;
    RefreshArgs A{state, n, stride, obs, table, offline_rows, online_rows, per_call, (uint32_t)(n / per_call), (uint32_t)(call % (uint64_t)n),
                  (uint32_t)(((call % m) * (uint64_t)per_call) % m)};
    hipLaunchKernelGGL(pilot_refresh_kernel, dim3((unsigned)((per_call + kEnvs - 1) / kEnvs)), dim3(kEnvs), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_pilot_refresh");
    return 0;
}

}  // extern "C"
