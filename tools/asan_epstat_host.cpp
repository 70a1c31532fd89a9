// tools/asan_epstat_host.cpp — the host paths of the episode-statistics entry points (hx_epstat_*) under AddressSanitizer, as a stand-alone program
// on a box WITHOUT a GPU: the workspace size, the argument checks and refusals, the packing of the three launches (dry runs in the asan-host build).
// CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_epstat_host.cpp -o /tmp/asan_epstat_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_epstat_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t N = 300, stride = 320, groups = (N + 63) / 64;
    const int64_t words = hx_epstat_workspace_words(N);
    printf("sizeof(HxEpStat) %d / %zu, workspace %lld words\n", hx_epstat_sizeof(), sizeof(HxEpStat), (long long)words);
    if (hx_epstat_sizeof() != (int)sizeof(HxEpStat) || words != groups * 2 * HX_EPSTAT_SLOT_WORDS + 3 * N) ++fails;
    if (hx_epstat_workspace_words(0) != 0 || hx_epstat_workspace_words(-5) != 0 || hx_epstat_workspace_words((int64_t)1 << 31) != 0) ++fails;
    if (HX_EPSTAT_SLOT_WORDS != HX_EPSTAT_BINS * HX_EPSTAT_SUMS + HX_EPSTAT_BINS) ++fails;
    uint32_t* ws = (uint32_t*)dev(words * 4);
    const int64_t k = groups * 2 * HX_EPSTAT_SLOT_WORDS;
    HxEpStat S{(double*)ws, (float*)(ws + k), ws + k + N, ws + k + 2 * N, N};
    float* state = (float*)dev(37 * stride * 4); float* rew = (float*)dev(N * 4);
    uint8_t* done = (uint8_t*)dev(N); int8_t* succ = (int8_t*)dev(N); uint32_t* ctr = (uint32_t*)dev(N * 4);
    OK(hx_epstat_reset(&S, ctr, nullptr));
    OK(hx_epstat_push(&S, state, N, stride, rew, done, succ, ctr, nullptr));
    OK(hx_epstat_push(&S, state, N, N, rew, done, succ, ctr, nullptr));
    OK(hx_epstat_clear(&S, nullptr));
    REFUSED(hx_epstat_reset(nullptr, ctr, nullptr));
    REFUSED(hx_epstat_reset(&S, nullptr, nullptr));
    REFUSED(hx_epstat_clear(nullptr, nullptr));
    REFUSED(hx_epstat_push(nullptr, state, N, stride, rew, done, succ, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, nullptr, N, stride, rew, done, succ, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N, stride, nullptr, done, succ, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N, stride, rew, nullptr, succ, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N, stride, rew, done, nullptr, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N, stride, rew, done, succ, nullptr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N + 1, stride, rew, done, succ, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N - 1, stride, rew, done, succ, ctr, nullptr));
    REFUSED(hx_epstat_push(&S, state, N, N - 1, rew, done, succ, ctr, nullptr));
    HxEpStat bad = S; bad.part = nullptr;
    REFUSED(hx_epstat_push(&bad, state, N, stride, rew, done, succ, ctr, nullptr));
    bad = S; bad.part = (double*)(ws + 1);
    REFUSED(hx_epstat_clear(&bad, nullptr));
    bad = S; bad.acc = nullptr;
    REFUSED(hx_epstat_reset(&bad, ctr, nullptr));
    bad = S; bad.len = nullptr;
    REFUSED(hx_epstat_clear(&bad, nullptr));
    bad = S; bad.last_ctr = nullptr;
    REFUSED(hx_epstat_push(&bad, state, N, stride, rew, done, succ, ctr, nullptr));
    bad = S; bad.n_envs = 0;
    REFUSED(hx_epstat_reset(&bad, ctr, nullptr));
    bad = S; bad.n_envs = (int64_t)1 << 31;
    REFUSED(hx_epstat_clear(&bad, nullptr));
    printf(fails ? "FAILED: %d\n" : "episode-statistics entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
