// hx_branch_steps.hip — expert branches of up to H steps (gfx950): hx_branch.hip's one-step branch as a CONVEYOR.  The k branches stay resident in a
// small device workspace; every call advances each of them ONE step — pilot_branch_kernel's work plus a coalesced load and store — and writes that step's
// (s, a_E, s', r, done) + step_success over the oldest online rows of the labelled expert ring.  A branch that ends (done, a non-finite row, or H steps
// flown) is reseeded from the learner's population on the next call.  The cost per call is one launch and one env step whatever H is; the rows of one
// pilot flight reach the ring one per call.  Nothing is stored back to the env state or its observations.  The rule is stated in
// include/hirl4ucav.h ("Expert branches") and, on the CPU, in tests/_branch_steps_model.py.
//
// Shape (pilot_branch_kernel's): one branch per lane, 64 per workgroup.  A seeded lane gathers the 37 state words and 13 observation words of its env;
// a resident lane reads column j of the workspace, struct-of-arrays over branches, so a wave's access of one word is one contiguous run.  The pilot's
// law runs on the Stepper's registers (hx_pilot_dev.h, the register form).  Finished rows are staged in LDS (8 KB) and written as whole 128-byte lines;
// the stepped state goes back to the workspace through Stepper::store, one contiguous run per word.  Each lane adds to its own three 64-bit counters.
// No atomics, no workgroup waits for another, no scratch; columns >= k of the workspace are never touched.
//
// Numerics: compiled with hx_env.hip's flags (no contraction); the step is hx_env_dev.h's text, so a branch's rows carry the bits of hx_pilot_act +
// hx_env_step flown on a clone of the picked env.
#include "hx_common.h"
#include "hx_env_dev.h"
#include "hx_pilot_dev.h"

#pragma clang fp contract(off)
namespace {

using namespace hxpilot;

constexpr int kPicks = 64;                  // branches per workgroup = one wave
constexpr int kStateWords = 37;             // hirl4ucav.h "Env state layout"
constexpr int kWorkWords = kStateWords + kObs + 1;  // bstate, bobs, age: 32-bit words per column, in front of the three 64-bit counters

struct StepsArgs {
    const float* state; int64_t n, stride;
    const float* obs; float* ring; int8_t* success;
    int64_t offline_rows, online_rows;
    int32_t per_call;
    uint32_t step;       // floor(n / per_call)
    uint32_t call_mod_n; // call mod n
    uint32_t base_mod_m; // (call * per_call) mod online_rows
    uint32_t max_steps;
    float* work; int64_t ws;  // the workspace and its columns (hirl4ucav.h: bstate[37][ws] bobs[13][ws] age[ws] counters[3][ws])
};

__global__ __launch_bounds__(kPicks) void pilot_branch_steps_kernel(StepsArgs A) {
    __shared__ float4 s_row[kPicks][kRow / 4];
    __shared__ int64_t s_slot[kPicks];  // the ring row of branch j, or -1: nothing is written
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * kPicks;
    const int64_t j = j0 + tid;
    int64_t slot = -1;
    if (j < A.per_call) {
        float* bstate = A.work;
        float* bobs = A.work + kStateWords * A.ws;
        uint32_t* age = reinterpret_cast<uint32_t*>(A.work + (kStateWords + kObs) * A.ws);
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(A.work + kWorkWords * A.ws);
        const bool resident = A.max_steps > 1u;  // max_steps == 1: hx_pilot_branch's rule, the workspace's state, observations and ages are not read
        const uint32_t a = resident ? age[j] : 0u;
        const bool seed = a == 0u;
        uint32_t e32 = A.call_mod_n + (uint32_t)j * A.step;  // both terms below n < 2^31: one conditional subtraction is the mod
        if (e32 >= (uint32_t)A.n) e32 -= (uint32_t)A.n;
        const int64_t e = (int64_t)e32;
        // the branch's source: env e of the population (a gather) or column j of the workspace (one contiguous run per word)
        hxenv::Stepper<false> T;
        T.load(seed ? A.state : bstate, seed ? A.stride : A.ws, seed ? e : j, 0u, false);
        const float* op = seed ? A.obs + e * kObs : bobs + j;
        const int64_t os = seed ? 1 : A.ws;
        float v[kRow];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < kObs; ++c) {
            v[c] = op[c * os];
            ok = ok && finite_word(v[c]);
        }
        float l0, l1, l2;
        pursuit_levels(T.mine.qw, T.mine.qx, T.mine.qy, T.mine.qz, T.other.p.x - T.mine.p.x, T.other.p.y - T.mine.p.y, T.other.p.z - T.mine.p.z, l0, l1, l2);
        v[13] = clamp1(l0);
        v[14] = clamp1(l1);
        v[15] = clamp1(l2);
        v[16] = (v[7] > 0.f && v[8] > 0.f) ? 1.f : -1.f;
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
            // the lane's own words: rows written, rows with done, kills (wrap_step's comparison for the +600, on the flags and health it left)
            cnt[j] += 1ull;
            if (W.done) cnt[A.ws + j] += 1ull;
            if (W.done && T.S.health < 0.1f && (T.S.flags & HX_F_FIRE_SUCCESS)) cnt[2 * A.ws + j] += 1ull;
        }
        if (resident) {
            if (ok && !W.done && a + 1u < A.max_steps) {  // the flight goes on: the stepped state and s' to column j
                T.store(bstate, A.ws, j0, (uint32_t)tid, false);
#pragma unroll
                for (int c = 0; c < kObs; ++c) bobs[c * A.ws + j] = v[17 + c];
                age[j] = a + 1u;
            } else {
                age[j] = 0u;  // ended: the column is left as it is, the next call reseeds
            }
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

int64_t pad64(int64_t k) { return (k + 63) / 64 * 64; }

#ifdef HX_HOST_DRYRUN
uint32_t g_last_packed[4];  // the asan-host build keeps what the last call packed (tools/asan_branch_steps_host.cpp compares it with 128-bit arithmetic)
#endif

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

#ifdef HX_HOST_DRYRUN
// asan-host build only (never in the shipped library, not in the public header): step, call mod n, (call * per_call) mod M and max_steps of the last
// hx_pilot_branch_steps
void hx_pilot_branch_steps_last_packed(uint32_t out[4]) { for (int i = 0; i < 4; ++i) out[i] = g_last_packed[i]; }
#endif

int64_t hx_branch_workspace_bytes(int32_t per_call) {
    if (per_call < 1) return 0;
    return pad64(per_call) * (kWorkWords * 4 + 3 * 8);
}

int hx_pilot_branch_steps(const float* state, int64_t n, int64_t stride, const float* obs, float* ring, int8_t* success, int64_t offline_rows,
                          int64_t online_rows, int32_t per_call, int32_t max_steps, uint64_t call, void* work, int64_t work_stride, void* stream) {
    HX_REQUIRE(state && obs, "hx_pilot_branch_steps: state [37][stride] and obs [n][13]");
    HX_REQUIRE(n > 0 && n < (1ll << 31) && stride >= n, "hx_pilot_branch_steps: 0 < n < 2^31 and stride >= n, got n = %lld, stride = %lld", (long long)n, (long long)stride);
    HX_REQUIRE(ring && ((uintptr_t)ring & 127u) == 0 && success, "hx_pilot_branch_steps: ring [offline_rows + online_rows][32], 128-byte aligned, and success "
               "[offline_rows + online_rows]");
    HX_REQUIRE(offline_rows >= 0 && online_rows >= 1 && offline_rows + online_rows < (1ll << 31),
               "hx_pilot_branch_steps: offline_rows >= 0, online_rows >= 1, fewer than 2^31 rows in all, got %lld and %lld", (long long)offline_rows, (long long)online_rows);
    HX_REQUIRE(per_call >= 1 && per_call <= n && per_call <= online_rows, "hx_pilot_branch_steps: 1 <= per_call <= min(n, online_rows), got per_call = %d, n = %lld, "
               "online_rows = %lld", (int)per_call, (long long)n, (long long)online_rows);
    HX_REQUIRE(max_steps >= 1 && max_steps <= 65535, "hx_pilot_branch_steps: 1 <= max_steps <= 65535, got %d", (int)max_steps);
    HX_REQUIRE(work && ((uintptr_t)work & 15u) == 0, "hx_pilot_branch_steps: work is hx_branch_workspace_bytes(per_call) bytes, 16-byte aligned");
    HX_REQUIRE(work_stride == pad64(per_call), "hx_pilot_branch_steps: work_stride is per_call rounded up to 64 = %lld, got %lld", (long long)pad64(per_call),
               (long long)work_stride);
    // (call * per_call) mod M from the residues: exact for every 64-bit call, the product stays below 2^62
    const uint64_t m = (uint64_t)online_rows;
    StepsArgs A{state, n, stride, obs, ring, success, offline_rows, online_rows, per_call, (uint32_t)(n / per_call), (uint32_t)(call % (uint64_t)n),
                (uint32_t)(((call % m) * (uint64_t)per_call) % m), (uint32_t)max_steps, static_cast<float*>(work), work_stride};
#ifdef HX_HOST_DRYRUN
    g_last_packed[0] = A.step; g_last_packed[1] = A.call_mod_n; g_last_packed[2] = A.base_mod_m; g_last_packed[3] = A.max_steps;
#endif
    hipLaunchKernelGGL(pilot_branch_steps_kernel, dim3((unsigned)((per_call + kPicks - 1) / kPicks)), dim3(kPicks), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_pilot_branch_steps");
    return 0;
}

}  // extern "C"
