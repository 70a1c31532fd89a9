// hx_selfimit.hip — self-imitation (gfx950): an episode tape keeps the last L executed steps of every env; behind an acting launch the episodes that
// have just ended in a kill (done with reward > 0: the +600 of hx_env_dev.h) are written, oldest step first, as full transitions (s, a, s', r, done) +
// step_success over the oldest rows of the online region of the labelled expert ring, and optionally as (s, a, zeros) rows into the online region of the
// BC table.  The learner's own successful episodes become demonstrations (Oh et al. 2018).  No counterpart in the reference.  The rule is stated in
// include/hirl4ucav.h ("Self-imitation") and, on the CPU, in tests/_selfimit_model.py.
//
// Two launches per call, and the same inputs give the same bits however workgroups are scheduled: no workgroup waits for another, no float atomics, no
// atomic at all — a slot is a function of the cursor and of klen[0 .. env], nothing else.
//   record  one env per lane, 64 per workgroup: the step goes into tape position p = call mod L (the tape is indexed by the CALL, tape[L][19][n_envs], so
//           a wave's store is one contiguous 256-byte run per field), len / obs_prev / last_ctr move, klen[env] = rows to emit (0: none) and the
//           workgroup's sums wcount[g] (rows) / wkills[g] (episodes) are stored.  Every word has one writer.
//   flush   one workgroup of four waves per 64-env group.  wcount[g] == 0: gone after one load (but the last workgroup, which owns the cursor).  The
//           others add wcount[0 .. g) (integers: any order gives the same sum), take the lane prefix of klen, apply the acceptance rule and copy: 8 lanes
//           per row, each gathers its 4 words from the tape into registers and stores 16 bytes, so a row leaves as one whole 128-byte line; the row's 32
//           finite tests meet in one ballot, so nothing is staged in LDS.  The cursor is double-buffered by call parity: every workgroup reads
//           cursor[call & 1], the last one writes cursor[(call + 1) & 1] — no workgroup reads a word that another writes in the same launch.
// A one-launch form would need the group prefix inside the launch that produces the counts, i.e. a workgroup waiting for another: not taken.
//
// Numerics: rows are copies; built without contraction like hx_nstep.hip although no sum is formed here (the only comparison is reward > 0).
#include "hx_common.h"
#include "hx_env_block.h"

#pragma clang fp contract(off)
namespace {

constexpr int kEnvs = 64;        // envs per workgroup of both launches = one wave of the record launch
constexpr int kFlushWaves = 4;   // waves of a flush workgroup: 32 rows per pass
constexpr int kFields = HX_SELF_FIELDS;
constexpr int kObsTile = kEnvs * HX_OBS_DIM;
enum { F_S = 0, F_A = HX_OBS_DIM, F_R = F_A + HX_ACT_DIM, F_SUCC, F_COUNT };
static_assert(F_COUNT == HX_SELF_FIELDS, "hirl4ucav.h HX_SELF_FIELDS");
static_assert(HX_OBS_DIM + HX_ACT_DIM + HX_OBS_DIM + 2 == HX_ROW_WORDS && HX_ROW_WORDS == 32, "a row is s[13] a[4] s'[13] r done");

__device__ __forceinline__ bool finite_word(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// inclusive scan of small non-negative counts over the 64 lanes of the wave
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// the workspace, carved as include/hirl4ucav.h lays it out
struct SelfWs {
    float* tape; float* obs_prev; uint32_t* len; uint32_t* last_ctr; uint32_t* klen; uint32_t* wcount; uint32_t* wkills;
    uint64_t* cursor; uint64_t* counters;
    int64_t n_envs;
    int32_t L;
};

// grid (groups, L): workgroup (g, p) zeroes tape position p of its 64 envs; the workgroups of p == 0 also set the per-env words and the group sums
__global__ __launch_bounds__(kEnvs) void self_reset_kernel(SelfWs S, const float* obs, const uint32_t* episode_ctr) {
    const int64_t N = S.n_envs, i = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (i < N) {
#pragma unroll
        for (int f = 0; f < kFields; ++f) S.tape[(p * kFields + f) * N + i] = 0.f;
    }
    if (p != 0) return;
    if (threadIdx.x == 0) S.wcount[blockIdx.x] = S.wkills[blockIdx.x] = 0u;
    if (i >= N) return;
    S.len[i] = 0u;
    S.klen[i] = 0u;
    S.last_ctr[i] = episode_ctr[i];
#pragma unroll
    for (int f = 0; f < HX_OBS_DIM; ++f) S.obs_prev[(int64_t)f * N + i] = obs[i * HX_OBS_DIM + f];
}

struct PushArgs {
    SelfWs S;
    const float* obs_new; const float* actions; const float* reward; const uint8_t* done; const int8_t* success; const uint32_t* episode_ctr;
    float* ring; int8_t* ring_success;
    int64_t offline_rows, online_rows;
    float* bc_table;
    int64_t bc_offline_rows;
    uint32_t pos;     // call mod L
    uint32_t parity;  // call & 1
    uint32_t groups;
};

__global__ __launch_bounds__(kEnvs) void self_record_kernel(PushArgs A) {
    __shared__ float s_obs[kObsTile];  // the workgroup's next observations, row-major as the env leaves them
    const int tid = threadIdx.x;
    const SelfWs& S = A.S;
    const int64_t N = S.n_envs, i0 = (int64_t)blockIdx.x * kEnvs, i = i0 + tid;
    const int nblk = (int)((N - i0) < kEnvs ? (N - i0) : kEnvs);
    const bool active = tid < nblk;
    hxenv::tile_copy<kEnvs, kObsTile>(s_obs, A.obs_new + i0 * HX_OBS_DIM, nblk * HX_OBS_DIM, tid);
    unsigned emit = 0u;
    uint32_t ctr = 0u, len = 0u;
    if (active) {
        const float r = A.reward[i];
        const bool dn = A.done[i] != 0;
        ctr = A.episode_ctr[i];
        const bool trunc = ctr != S.last_ctr[i] && !dn;
        len = S.len[i];
        if (trunc) {
            len = 0u;
        } else {
            const float4 act = reinterpret_cast<const float4*>(A.actions)[i];
            float* at = S.tape + (int64_t)A.pos * kFields * N + i;
#pragma unroll
            for (int f = 0; f < HX_OBS_DIM; ++f) at[(int64_t)f * N] = S.obs_prev[(int64_t)f * N + i];
            at[(int64_t)(F_A + 0) * N] = act.x; at[(int64_t)(F_A + 1) * N] = act.y;
            at[(int64_t)(F_A + 2) * N] = act.z; at[(int64_t)(F_A + 3) * N] = act.w;
            at[(int64_t)F_R * N] = r;
            at[(int64_t)F_SUCC * N] = (float)A.success[i];
            len = len >= (uint32_t)S.L ? (uint32_t)S.L : len + 1u;  // min(len + 1, L); a word that was never reset cannot leave [1, L]
            if (dn) {
                emit = r > 0.f ? len : 0u;  // the kill test: every term of the reward but the +600 is <= 0
                len = 0u;
            }
        }
    }
    __syncthreads();  // s_obs complete
    if (active) {
        S.len[i] = len;
        S.klen[i] = emit;
        S.last_ctr[i] = ctr;
        const float* sp = s_obs + tid * HX_OBS_DIM;
#pragma unroll
        for (int f = 0; f < HX_OBS_DIM; ++f) S.obs_prev[(int64_t)f * N + i] = sp[f];
    }
    const int rows = __shfl(wave_scan_incl((int)emit, tid), 63);  // <= 64 * 65,535 < 2^23
    const int kills = __popcll(__ballot(emit > 0u));
    if (tid == 0) {
        S.wcount[blockIdx.x] = (uint32_t)rows;
        S.wkills[blockIdx.x] = (uint32_t)kills;
    }
}

// The acceptance rule for the 64 envs of group g, with `base` rows of kill episodes in front of the group: kl = the lane's rows (0: no kill; never more than
// L, so never an index outside the tape), incl = their inclusive lane prefix; the lane's episode is accepted iff P_e = base + incl <= M — a function of
// the prefix alone.  Whole wave.
__device__ __forceinline__ bool group_accept(const SelfWs& S, unsigned g, unsigned long long base, unsigned long long M, int lane, int& kl, int& incl) {
    const int64_t e = (int64_t)g * kEnvs + lane;
    kl = e < S.n_envs ? (int)S.klen[e] : 0;
    kl = kl > S.L ? S.L : kl;
    incl = wave_scan_incl(kl, lane);
    return kl > 0 && base + (unsigned long long)incl <= M;
}

__global__ __launch_bounds__(kEnvs * kFlushWaves) void self_flush_kernel(PushArgs A) {
    __shared__ unsigned s_written[kFlushWaves];
    const SelfWs& S = A.S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned g = blockIdx.x, G = A.groups;
    const bool owner = g == G - 1u;  // the last workgroup owns the cursor
    const uint32_t wc = S.wcount[g];
    if (wc == 0u && !owner) return;  // (uniform over the workgroup)
    const int64_t N = S.n_envs;
    const unsigned long long M = (unsigned long long)A.online_rows;
    const int L = S.L;
    // rows of the kill episodes in front of this group: every wave adds the same words (integers: the sum does not depend on the order)
    unsigned long long base = 0ull;
    for (unsigned h = (unsigned)lane; h < g; h += 64u) base += S.wcount[h];
    base = wave_sum_u64(base);
    const unsigned long long cursor = S.cursor[A.parity];

    unsigned written = 0u, eps_ok = 0u;
    if (wc != 0u) {
        int kl, incl;
        const bool acc_lane = group_accept(S, g, base, M, lane, kl, incl);
        const int first = incl - kl;
        eps_ok = (unsigned)__popcll(__ballot(acc_lane));
        const unsigned c0 = (unsigned)(cursor % M);
        const int sub = lane >> 3, q = lane & 7;
        unsigned long long todo = __ballot(acc_lane);
        while (todo) {  // the accepted episodes of the group in env order (uniform over the wave)
            const int el = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const int m = __shfl(kl, el);
            const unsigned k0 = (unsigned)base + (unsigned)__shfl(first, el);  // rows accepted in front of this episode: k0 + m <= M < 2^31
            const int64_t e = (int64_t)g * kEnvs + el;
            for (int j0 = wave * 8; j0 < m; j0 += 8 * kFlushWaves) {
                const int j = j0 + sub;
                const bool live = j < m;
                float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, succ = 0.f;
                if (live) {
                    int pos = (int)A.pos - (m - 1 - j);
                    pos = pos < 0 ? pos + L : pos;
                    int pos1 = pos + 1;
                    pos1 = pos1 >= L ? 0 : pos1;
                    const float* at = S.tape + (int64_t)pos * kFields * N + e;
                    const float* at1 = S.tape + (int64_t)pos1 * kFields * N + e;
                    const bool lastrow = j == m - 1;
                    // word w of the row [s 0..12 | a 13..16 | s' 17..29 | r 30 | done 31]
                    auto word = [&](int w) -> float {
                        if (w < F_R) return at[(int64_t)w * N];
                        if (w < F_R + HX_OBS_DIM) return lastrow ? A.obs_new[e * HX_OBS_DIM + (w - F_R)] : at1[(int64_t)(w - F_R) * N];
                        if (w == 30) return at[(int64_t)F_R * N];
                        return lastrow ? 1.f : 0.f;
                    };
                    v0 = word(4 * q); v1 = word(4 * q + 1); v2 = word(4 * q + 2); v3 = word(4 * q + 3);
                    if (q == 7) succ = at[(int64_t)F_SUCC * N];
                }
                const bool fin = finite_word(v0) && finite_word(v1) && finite_word(v2) && finite_word(v3);
                const unsigned long long okb = __ballot(fin);
                const bool ok = live && ((okb >> (lane & 56)) & 0xFFull) == 0xFFull;  // all 32 words of the row are finite
                if (ok) {
                    unsigned o = c0 + k0 + (unsigned)j;  // both terms below M < 2^31: one conditional subtraction is the mod
                    if (o >= (unsigned)M) o -= (unsigned)M;
                    const int64_t slot = A.offline_rows + (int64_t)o;
                    reinterpret_cast<float4*>(A.ring)[slot * (HX_ROW_WORDS / 4) + q] = make_float4(v0, v1, v2, v3);
                    if (q == 7) A.ring_success[slot] = (int8_t)succ;
                    if (A.bc_table) {  // (s, a, zeros): words 0 .. 16 of the row
                        const int64_t bslot = A.bc_offline_rows + (int64_t)o;
                        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (q < 4) b = make_float4(v0, v1, v2, v3);
                        else if (q == 4) b.x = v0;
                        reinterpret_cast<float4*>(A.bc_table)[bslot * (HX_ROW_WORDS / 4) + q] = b;
                    }
                }
                written += (unsigned)__popcll(__ballot(ok && q == 0));
            }
        }
    }
    if (lane == 0) s_written[wave] = written;
    __syncthreads();
    if (wave != 0) return;
    if (wc != 0u && lane == 0) {  // the group's own counter words
        const unsigned kills = S.wkills[g];
        unsigned rows = 0u;
#pragma unroll
        for (int w = 0; w < kFlushWaves; ++w) rows += s_written[w];
        uint64_t* cnt = S.counters;
        cnt[(size_t)HX_SELF_KILLS * G + g] += kills;
        cnt[(size_t)HX_SELF_EPISODES * G + g] += eps_ok;
        cnt[(size_t)HX_SELF_ROWS * G + g] += rows;
        cnt[(size_t)HX_SELF_DROPPED * G + g] += kills - eps_ok;
    }
    if (!owner) return;
    // the cursor: the rows of the leading run of accepted episodes over ALL groups
    unsigned long long accepted = base + wc;
    if (accepted > M) {  // a drop somewhere: the group the bound falls into (a wave-wide scan of wcount, 64 groups per pass), then the rule on its lanes
        unsigned long long run = 0ull;
        unsigned h = 0u;
        for (unsigned h0 = 0u; h0 < G; h0 += 64u) {
            const unsigned hh = h0 + (unsigned)lane;
            const int w = hh < G ? (int)S.wcount[hh] : 0;  // <= 64 * 65,535 < 2^23: a pass sums to less than 2^29
            const int inc = wave_scan_incl(w, lane);
            const unsigned long long over = __ballot(run + (unsigned long long)inc > M);
            if (over) {  // (uniform; it is reached: the total exceeds M)
                const int l = __ffsll((long long)over) - 1;
                run += (unsigned long long)__shfl(inc - w, l);
                h = h0 + (unsigned)l;
                break;
            }
            run += (unsigned long long)__shfl(inc, 63);
        }
        int kl, incl;
        int best = group_accept(S, h, run, M, lane, kl, incl) ? incl : 0;  // accepted lanes are a leading run of the kill lanes: the last one's prefix
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d));
        accepted = run + (unsigned long long)best;
    }
    if (lane == 0) S.cursor[A.parity ^ 1u] = cursor + accepted;
}

int carve(void* work, int64_t work_words, int64_t n_envs, int32_t L, SelfWs& s, const char* who) {
    HX_REQUIRE(work && ((uintptr_t)work & 15u) == 0, "%s: the workspace, 16-byte aligned", who);
    HX_REQUIRE(n_envs > 0 && n_envs < (1ll << 31), "%s: 0 < n_envs < 2^31, got %lld", who, (long long)n_envs);
    HX_REQUIRE(L >= 1 && L <= HX_SELF_MAX_STEPS, "%s: L is 1..%d, got %d", who, HX_SELF_MAX_STEPS, (int)L);
    HX_REQUIRE(work_words == hx_self_workspace_words(n_envs, L), "%s: work_words is hx_self_workspace_words(n_envs, L) = %lld, got %lld", who,
               (long long)hx_self_workspace_words(n_envs, L), (long long)work_words);
    const int64_t n = n_envs, groups = (n + kEnvs - 1) / kEnvs, gpad = (groups + 1) / 2 * 2;
    uint32_t* w = (uint32_t*)work;
    int64_t at = 0;
    s.tape = (float*)(w + at); at += (int64_t)kFields * L * n;
    s.obs_prev = (float*)(w + at); at += (int64_t)HX_OBS_DIM * n;
    s.len = w + at; at += n;
    s.last_ctr = w + at; at += n;
    s.klen = w + at; at += n;
    s.wcount = w + at; at += gpad;
    s.wkills = w + at; at += gpad;
    at = (at + 1) / 2 * 2;  // the 64-bit part starts on an 8-byte boundary
    s.cursor = (uint64_t*)(w + at); at += 4;
    s.counters = (uint64_t*)(w + at);
    s.n_envs = n;
    s.L = L;
    return 0;
}

#ifdef HX_HOST_DRYRUN
uint32_t g_last_packed[3];  // the asan-host build keeps what the last hx_self_push packed: call mod L, call & 1, groups
#endif

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

#ifdef HX_HOST_DRYRUN
// asan-host build only (never in the shipped library, not in the public header)
void hx_self_push_last_packed(uint32_t out[3]) { out[0] = g_last_packed[0]; out[1] = g_last_packed[1]; out[2] = g_last_packed[2]; }
#endif

int64_t hx_self_workspace_words(int64_t n_envs, int32_t L) {
    if (n_envs <= 0 || n_envs >= (1ll << 31) || L < 1 || L > HX_SELF_MAX_STEPS) return 0;
    const int64_t groups = (n_envs + kEnvs - 1) / kEnvs, gpad = (groups + 1) / 2 * 2;
    int64_t words = n_envs * ((int64_t)kFields * L + HX_OBS_DIM + 3) + 2 * gpad;
    words = (words + 1) / 2 * 2;       // the 64-bit part starts on an 8-byte boundary
    return words + 2 * 2 + 2 * HX_SELF_COUNTERS * groups;
}

int hx_self_reset(void* work, int64_t work_words, int64_t n_envs, int32_t L, const float* obs, const uint32_t* episode_ctr, void* stream) {
    SelfWs ws{};
    const SelfWs* self = &ws;
    if (int rc = carve(work, work_words, n_envs, L, ws, "hx_self_reset")) return rc;
    HX_REQUIRE(obs && episode_ctr, "hx_self_reset: obs [n_envs][13] and episode_ctr [n_envs]");
    const unsigned groups = (unsigned)((self->n_envs + kEnvs - 1) / kEnvs);
    hipLaunchKernelGGL(self_reset_kernel, dim3(groups, (unsigned)self->L), dim3(kEnvs), 0, (hipStream_t)stream, *self, obs, episode_ctr);
    HX_CHECK_LAUNCH("hx_self_reset");
    return 0;
}

int hx_self_push(void* work, int64_t work_words, int64_t n_envs, int32_t L, const float* obs_new, const float* actions, const float* reward, const uint8_t* done, const int8_t* success,
                 const uint32_t* episode_ctr, float* ring, int8_t* ring_success, int64_t offline_rows, int64_t online_rows, float* bc_table,
                 int64_t bc_offline_rows, uint64_t call, void* stream) {
    SelfWs ws{};
    const SelfWs* self = &ws;
    if (int rc = carve(work, work_words, n_envs, L, ws, "hx_self_push")) return rc;
    HX_REQUIRE(obs_new && ((uintptr_t)obs_new & 15u) == 0 && actions && ((uintptr_t)actions & 15u) == 0 && reward && done && success && episode_ctr,
               "hx_self_push: obs_new [n_envs][13] and actions [n_envs][4], 16-byte aligned, reward, done, success and episode_ctr");
    HX_REQUIRE(ring && ((uintptr_t)ring & 127u) == 0 && ring_success, "hx_self_push: ring [offline_rows + online_rows][32], 128-byte aligned, and ring_success "
               "[offline_rows + online_rows]");
    HX_REQUIRE(offline_rows >= 0 && online_rows >= 1 && offline_rows + online_rows < (1ll << 31),
               "hx_self_push: offline_rows >= 0, online_rows >= 1, fewer than 2^31 rows in all, got %lld and %lld", (long long)offline_rows, (long long)online_rows);
    HX_REQUIRE(self->L <= online_rows, "hx_self_push: L <= online_rows (an episode of L rows must fit), got L = %d, online_rows = %lld", (int)self->L,
               (long long)online_rows);
    HX_REQUIRE(!bc_table || (((uintptr_t)bc_table & 127u) == 0 && bc_offline_rows >= 0 && bc_offline_rows + online_rows < (1ll << 31)),
               "hx_self_push: bc_table NULL or [bc_offline_rows + online_rows][32], 128-byte aligned, bc_offline_rows >= 0, fewer than 2^31 rows in all, got %lld",
               (long long)bc_offline_rows);
    const unsigned groups = (unsigned)((self->n_envs + kEnvs - 1) / kEnvs);
    PushArgs A{*self, obs_new, actions, reward, done, success, episode_ctr, ring, ring_success, offline_rows, online_rows, bc_table, bc_offline_rows,
               (uint32_t)(call % (uint64_t)self->L), (uint32_t)(call & 1u), groups};
#ifdef HX_HOST_DRYRUN
    g_last_packed[0] = A.pos; g_last_packed[1] = A.parity; g_last_packed[2] = A.groups;
#endif
    hipLaunchKernelGGL(self_record_kernel, dim3(groups), dim3(kEnvs), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_self_push (record)");
    hipLaunchKernelGGL(self_flush_kernel, dim3(groups), dim3(kEnvs * kFlushWaves), 0, (hipStream_t)stream, A);
    HX_CHECK_LAUNCH("hx_self_push (flush)");
    return 0;
}

}  // extern "C"
