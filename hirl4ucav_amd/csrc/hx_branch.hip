// hx_branch.hip — expert branches (gfx950): behind an acting launch, a few envs of the population are loaded into registers, flown ONE step under the
// scripted pursuit pilot's noise-free action (hx_pilot_dev.h) by the env's own step (hx_env_dev.h hxenv::Stepper<false>: what hx_env_step runs), and
// written down as full transitions (s, a_E, s'_E, r, done) + step_success over the oldest rows of the online region of the labelled expert ring.
// Nothing is stored back to the env state or its observations: the learner's own trajectory is untouched.  No counterpart in the reference, whose
// expert lives in an external simulator.  The rule is stated in include/hirl4ucav.h ("Expert branches") and, on the CPU, in tests/_branch_model.py.
//
// Shape (that of pilot_refresh_kernel, hx_pilot.hip): one pick per lane, 64 per workgroup.  The 37 state words and 13 observation words of a pick are
// gathers (the picks are spread over the population on purpose); finished rows are staged in LDS (8 KB) and written as whole 128-byte lines, eight
// lanes of 16 bytes; the success bytes are one store per lane.  No atomics, no workgroup waits for another, no scratch; the slots of one call are
// distinct (k <= M), so no two lanes write the same line or byte.
//
// Numerics: compiled with hx_env.hip's flags (no contraction); the step is hx_env_dev.h's text on the same inputs, so s', r, done and step_success
// carry hx_env_step's bits.
#include "hx_common.h"
#include "hx_env_dev.h"
#include "hx_pilot_dev.h"

#pragma clang fp contract(off)
namespace {

using namespace hxpilot;

constexpr int kPicks = 64;  // picks per workgroup = one wave

struct BranchArgs {
    const float* state; int64_t n, stride;
    const float* obs; float* ring; int8_t* success;
    int64_t offline_rows, online_rows;
    int32_t per_call;
    uint32_t step;       // floor(n / per_call)
    uint32_t call_mod_n; // call mod n
    uint32_t base_mod_m; // (call * per_call) mod online_rows
};

__global__ __launch_bounds__(kPicks) void pilot_branch_kernel(BranchArgs A) {
    __shared__ float4 s_row[kPicks][kRow / 4];
    __shared__ int64_t s_slot[kPicks];  // the ring row of pick j, or -1: nothing is written
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * kPicks + tid;
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
        // one step of env e in registers: the env is the lane's own base (a gather), nothing of T is ever stored
        hxenv::Stepper<false> T;
        T.load(A.state, A.stride, e, 0u, false);
        hxenv::Wrapped W{};
        hxenv::V3 eu{}, eu2{};
        T.step(make_float4(v[13], v[14], v[15], v[16]), false, eu, eu2, W);
        v[17] = W.o0; v[18] = W.o1; v[19] = W.o2;
        v[20] = eu.x; v[21] = eu.y; v[22] = eu.z;
        v[23] = W.o6; v[24] = W.o7; v[25] = W.o8;
        v[26] = eu2.x; v[27] = eu2.y; v[28] = eu2.z;
        v[29] = W.o12;
        v[30] = W.reward;
        v[31] = W.done ? 1.f : 0.f;
#pragma unroll
        for (int c = kObs; c < kRow; ++c) ok = ok && finite_word(v[c]);
#pragma unroll
        for (int q = 0; q < kRow / 4; ++q) s_row[tid][q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        uint32_t o32 = A.base_mod_m + (uint32_t)j;  // j < per_call <= M < 2^31, likewise
        if (o32 >= (uint32_t)A.online_rows) o32 -= (uint32_t)A.online_rows;
        if (ok) {
            slot = A.offline_rows + (int64_t)o32;
            A.success[slot] = (int8_t)W.success;
        }
    }
    s_slot[tid] = slot;
    __syncthreads();
    // the workgroup's rows as whole 128-byte lines: 8 lanes per row, 16 bytes each
    float4* ring4 = reinterpret_cast<float4*>(A.ring);
    const int q = tid & 7;
#pragma unroll
    for (int r0 = 0; r0 < kPicks; r0 += 8) {
        const int r = r0 + (tid >> 3);
        const int64_t to = s_slot[r];
        if (to >= 0) ring4[to * (kRow / 4) + q] = s_row[r][q];
    }
}

#ifdef HX_HOST_DRYRUN
uint32_t g_last_packed[3];  // the asan-host build keeps what the last call packed (tools/asan_branch_host.cpp compares it with 128-bit arithmetic)
#endif

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

#ifdef HX_HOST_DRYRUN
// asan-host build only (never in the shipped library, not in the public header): step, call mod n and (call * per_call) mod M of the last hx_pilot_branch
void hx_pilot_branch_last_packed(uint32_t out[3]) { out[0] = g_last_packed[0]; out[1] = g_last_packed[1]; out[2] = g_last_packed[2]; }
#endif

int hx_pilot_branch(const float* state, int64_t n, int64_t stride, const float* obs, float* ring, int8_t* success, int64_t offline_rows,
                    int64_t online_rows, int32_t per_call, uint64_t call, void* stream) {
    HX_REQUIRE(state && obs, "hx_pilot_branch: state [37][stride] and obs [n][13]");
    HX_REQUIRE(n > 0 && n < (1ll << 31) && stride >= n, "hx_pilot_branch: 0 < n < 2^31 and stride >= n, got n = %lld, stride = %lld", (long long)n, (long long)stride);
    HX_REQUIRE(ring && ((uintptr_t)ring & 127u) == 0 && success, "hx_pilot_branch: ring [offline_rows + online_rows][32], 128-byte aligned, and success "
               "[offline_rows + online_rows]");
    HX_REQUIRE(offline_rows >= 0 && online_rows >= 1 && offline_rows + online_rows < (1ll << 31),
               "hx_pilot_branch: offline_rows >= 0, online_rows >= 1, fewer than 2^31 rows in all, got %lld and %lld", (long long)offline_rows, (long long)online_rows);
    HX_REQUIRE(per_call >= 1 && per_call <= n && per_call <= online_rows, "hx_pilot_branch: 1 <= per_call <= min(n, online_rows), got per_call = %d, n = %lld, "
               "online_rows = %lld", (int)per_call, (long long)n, (long long)online_rows);
    // (call * per_call) mod M from the residues: exact for every 64-bit call, the product stays below 2^62
    const uint64_t m = (uint64_t)online_rows;
    BranchArgs A{state, n, stride, obs, ring, success, offline_rows, online_rows, per_call, (uint32_t)(n / per_call), (uint32_t)(call % (uint64_t)n),
                 (uint32_t)(((call % m) * (uint64_t)per_call) % m)};
#ifdef HX_HOST_DRYRUN
    g_last_packed[0] = A.step; g_last_packed[1] = A.call_mod_n; g_last_packed[2] = A.base_mod_m;
#endif
    hipLaunchKernelGGL(pilot_branch_kernel, dim3((unsigned)((per_call + kPicks - 1) / kPicks)), dim3(kPicks), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_pilot_branch");
    return 0;
}

}  // extern "C"
