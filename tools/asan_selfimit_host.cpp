// tools/asan_selfimit_host.cpp — the host path of hx_self_push, hx_self_reset and hx_self_workspace_words (self-imitation,
// hx_selfimit.hip) under AddressSanitizer, as a stand-alone program on a box WITHOUT a GPU: the argument checks and refusals, the workspace arithmetic up
// to 2^31 - 1 envs and 65,535 steps, the host path at 64-bit call counts (2^32 - 1, 2^32, 2^40, 2^64 - 1), the packing of the two launches (dry runs in
// the asan-host build).  CPU only.  The asan-host build of hx_selfimit.hip keeps the three words the last call packed for its kernels — call mod L, call & 1,
// the number of 64-env groups — and hands them out (hx_self_push_last_packed: that build only, not in the public header).  On the GPU the same values are
// held to the model by tests/test_selfimit_gpu.py.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_selfimit_host.cpp -o /tmp/asan_selfimit_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_selfimit_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ != HX_ERR_ARG) { printf("NOT REFUSED (rc %d): %s\n", rc_, #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
#define EQ(a, b) do { long long a_ = (long long)(a), b_ = (long long)(b); if (a_ != b_) { printf("%s = %lld, expected %lld\n", #a, a_, b_); ++fails; } } while (0)
extern "C" void hx_self_push_last_packed(uint32_t out[3]);
static void packed(uint64_t call, uint64_t L, uint64_t n) {
    uint32_t got[3];
    hx_self_push_last_packed(got);
    if (got[0] != (uint32_t)(call % L) || got[1] != (uint32_t)(call & 1) || got[2] != (uint32_t)((n + 63) / 64)) {
        printf("PACKED: call %llu L %llu n %llu -> %u %u %u\n", (unsigned long long)call, (unsigned long long)L, (unsigned long long)n, got[0], got[1], got[2]);
        ++fails;
    }
}
// the header's layout, restated: tape, obs_prev, len, last_ctr, klen, wcount[Gp], wkills[Gp], pad to even, cursor[2], counters[4][G]
static int64_t words(int64_t n, int64_t L) {
    const int64_t g = (n + 63) / 64, gp = (g + 1) / 2 * 2;
    int64_t w = n * (19 * L + 13 + 3) + 2 * gp;
    w = (w + 1) / 2 * 2;
    return w + 4 + 8 * g;
}
int main() {
    const int64_t N = 300, E0 = 40, M = 50;
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 133) ++fails;
    EQ(hx_self_workspace_words(0, 1), 0); EQ(hx_self_workspace_words(-3, 1), 0); EQ(hx_self_workspace_words(1ll << 31, 1), 0);
    EQ(hx_self_workspace_words(8, 0), 0); EQ(hx_self_workspace_words(8, -1), 0); EQ(hx_self_workspace_words(8, 65536), 0);
    const int64_t shapes[][2] = {{1, 1}, {63, 2}, {64, 5}, {65, 5}, {130, 5}, {4096, 256}, {131072, 256}, {(1ll << 31) - 1, 65535}, {(1ll << 31) - 1, 1}, {1, 65535}};
    for (auto& s : shapes) EQ(hx_self_workspace_words(s[0], (int32_t)s[1]), words(s[0], s[1]));
    EQ(hx_self_workspace_words(1, 1), 52); EQ(hx_self_workspace_words(4096, 256) * 4 - 76ll * 256 * 4096, 4 * (16 * 4096 + 128 + 4 + 512));
    uint32_t* w = (uint32_t*)dev((size_t)hx_self_workspace_words(N, 7) * 4);
    const int32_t L = 7;
    float* obs = (float*)dev(N * 13 * 4); float* act = (float*)dev(N * 4 * 4); float* rew = (float*)dev(N * 4);
    uint8_t* done = (uint8_t*)dev(N); int8_t* succ = (int8_t*)dev(N); uint32_t* ctr = (uint32_t*)dev(N * 4);
    float* ring = (float*)dev((E0 + M) * 32 * 4); int8_t* rs = (int8_t*)dev(E0 + M); float* bc = (float*)dev((9 + M) * 32 * 4);
    OK(hx_self_reset(w, hx_self_workspace_words(N, L), N, L, obs, ctr, nullptr));
    const uint64_t calls[] = {0, 1, 6, 7, 0xFFFFFFFFull, 0x100000000ull, 1ull << 40, ~0ull};
    for (uint64_t c : calls) {
        OK(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, c, nullptr)); packed(c, 7, N);
        OK(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, bc, 9, c, nullptr)); packed(c, 7, N);
    }
    {
        OK(hx_self_reset(w, hx_self_workspace_words(1, 1), 1, 1, obs, ctr, nullptr));  // (a smaller carving of the same memory)
        OK(hx_self_push(w, hx_self_workspace_words(1, 1), 1, 1, obs, act, rew, done, succ, ctr, ring, rs, 0, 1, nullptr, 0, 1ull << 40, nullptr)); packed(1ull << 40, 1, 1);
        OK(hx_self_push(w, hx_self_workspace_words(64, 50), 64, 50, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 99, nullptr)); packed(99, 50, 64);
        REFUSED(hx_self_push(w, hx_self_workspace_words(64, 51), 64, 51, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 99, nullptr));  // L > online_rows
    }
    // the workspace, n_envs and L
    REFUSED(hx_self_push(nullptr, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w + 1, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w + 2, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_reset(nullptr, hx_self_workspace_words(N, L), N, L, obs, ctr, nullptr));
    REFUSED(hx_self_reset(w + 1, hx_self_workspace_words(N, L), N, L, obs, ctr, nullptr));
    REFUSED(hx_self_reset(w, hx_self_workspace_words(N, L), N, L, nullptr, ctr, nullptr));
    REFUSED(hx_self_reset(w, hx_self_workspace_words(N, L), N, L, obs, nullptr, nullptr));
    const int64_t bad_n[] = {0, -1, 1ll << 31};
    for (int64_t n : bad_n) { REFUSED(hx_self_push(w, hx_self_workspace_words(n, L), n, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr)); REFUSED(hx_self_reset(w, hx_self_workspace_words(n, L), n, L, obs, ctr, nullptr)); }
    const int32_t bad_l[] = {0, -1, 65536};
    for (int32_t l : bad_l) { REFUSED(hx_self_push(w, hx_self_workspace_words(N, l), N, l, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr)); REFUSED(hx_self_reset(w, hx_self_workspace_words(N, l), N, l, obs, ctr, nullptr)); }
    // work_words that is not the count of (n_envs, L): a wrong pair cannot write outside the buffer
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L) - 1, N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L + 1, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N + 1, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, 0, N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_reset(w, hx_self_workspace_words(N, L) + 1, N, L, obs, ctr, nullptr));
    REFUSED(hx_self_reset(w, hx_self_workspace_words(N, L), N, L - 1, obs, ctr, nullptr));
    // the inputs
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, nullptr, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs + 1, act, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, nullptr, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act + 2, rew, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, nullptr, done, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, nullptr, succ, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, nullptr, ctr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, nullptr, ring, rs, E0, M, nullptr, 0, 0, nullptr));
    // the destinations: hx_pilot_branch's alignment and range checks
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, nullptr, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring + 1, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring + 16, rs, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, nullptr, E0, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, -1, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, 0, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, 6, nullptr, 0, 0, nullptr));  // L = 7 > online_rows
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, (int64_t)1 << 31, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, ((int64_t)1 << 31) - M, M, nullptr, 0, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, bc + 1, 9, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, bc + 16, 9, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, bc, -1, 0, nullptr));
    REFUSED(hx_self_push(w, hx_self_workspace_words(N, L), N, L, obs, act, rew, done, succ, ctr, ring, rs, E0, M, bc, ((int64_t)1 << 31) - M, 0, nullptr));
    printf(fails ? "FAILED: %d\n" : "hx_self_push and hx_self_reset ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
