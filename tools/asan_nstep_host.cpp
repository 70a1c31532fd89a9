// tools/asan_nstep_host.cpp — the host paths of the n-step entry points (hx_nstep_*) under AddressSanitizer, as a stand-alone program on a box
// WITHOUT a GPU: the workspace size, the argument checks and refusals, the packing of the two launches (dry runs in the asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_nstep_host.cpp -o /tmp/asan_nstep_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_nstep_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t N = 300, cap = 1024;
    const int n = 3;
    const int64_t words = hx_nstep_workspace_floats(N, n);
    printf("sizeof(HxNStep) %d / %zu, workspace %lld words\n", hx_nstep_sizeof(), sizeof(HxNStep), (long long)words);
    if (hx_nstep_sizeof() != (int)sizeof(HxNStep) || words != N * (HX_NSTEP_FIELDS * n + 15)) ++fails;
    if (hx_nstep_workspace_floats(N, 0) != 0 || hx_nstep_workspace_floats(N, HX_NSTEP_MAX + 1) != 0 || hx_nstep_workspace_floats(0, n) != 0) ++fails;
    float* ws = (float*)dev(words * 4);
    const int64_t k = (int64_t)HX_NSTEP_FIELDS * n * N;
    HxNStep S{ws, (uint32_t*)(ws + k), ws + k + N, (uint32_t*)(ws + k + 14 * N), N, n, 0.99f};
    float* obs = (float*)dev(N * 13 * 4); float* act = (float*)dev(N * 16); float* rew = (float*)dev(N * 4);
    uint8_t* done = (uint8_t*)dev(N); int8_t* succ = (int8_t*)dev(N); uint32_t* ctr = (uint32_t*)dev(N * 4);
    float* ring = (float*)dev(cap * 128); int8_t* rs = (int8_t*)dev(cap); uint64_t* total = (uint64_t*)dev(8);
    OK(hx_nstep_reset(&S, obs, ctr, nullptr));
    OK(hx_nstep_push(&S, obs, act, rew, done, succ, ctr, ring, rs, cap, total, nullptr));
    OK(hx_nstep_push(&S, obs, act, rew, done, succ, ctr, ring, nullptr, cap, total, nullptr));
    REFUSED(hx_nstep_reset(nullptr, obs, ctr, nullptr));
    REFUSED(hx_nstep_reset(&S, nullptr, ctr, nullptr));
    REFUSED(hx_nstep_push(&S, obs, act, rew, done, succ, ctr, ring, rs, n * N - 1, total, nullptr));
    REFUSED(hx_nstep_push(&S, obs, act, rew, done, succ, ctr, ring, rs, (int64_t)1 << 31, total, nullptr));
    REFUSED(hx_nstep_push(&S, obs, act, rew, done, succ, ctr, nullptr, rs, cap, total, nullptr));
    REFUSED(hx_nstep_push(&S, obs, act, rew, done, succ, ctr, ring, rs, cap, nullptr, nullptr));
    REFUSED(hx_nstep_push(&S, obs, nullptr, rew, done, succ, ctr, ring, rs, cap, total, nullptr));
    HxNStep bad = S; bad.n = 9;
    REFUSED(hx_nstep_push(&bad, obs, act, rew, done, succ, ctr, ring, rs, cap * 4, total, nullptr));
    bad = S; bad.n = 0;
    REFUSED(hx_nstep_reset(&bad, obs, ctr, nullptr));
    bad = S; bad.hc = nullptr;
    REFUSED(hx_nstep_push(&bad, obs, act, rew, done, succ, ctr, ring, rs, cap, total, nullptr));
    bad = S; bad.gamma = 1.5f;
    REFUSED(hx_nstep_push(&bad, obs, act, rew, done, succ, ctr, ring, rs, cap, total, nullptr));
    bad = S; bad.n_envs = 0;
    REFUSED(hx_nstep_reset(&bad, obs, ctr, nullptr));
    printf(fails ? "FAILED: %d\n" : "n-step entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
