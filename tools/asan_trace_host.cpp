// tools/asan_trace_host.cpp — the host paths of the episode record's entry points (hx_trace_*) under AddressSanitizer, as a stand-alone program on a
// box WITHOUT a GPU: the workspace size, the argument checks and refusals, the packing of the two launches (dry runs in the asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_trace_host.cpp -o /tmp/asan_trace_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_trace_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t N = 300, stride = 320, k = 130;
    const int cap = 24;
    const int64_t words = hx_trace_workspace_words(k, cap);
    printf("sizeof(HxTrace) %d / %zu, workspace %lld words\n", hx_trace_sizeof(), sizeof(HxTrace), (long long)words);
    if (hx_trace_sizeof() != (int)sizeof(HxTrace) || words != k * (HX_TRACE_FIELDS * cap + HX_TRACE_SUMMARIES) + 1) ++fails;
    if (hx_trace_workspace_words(0, cap) != 0 || hx_trace_workspace_words(-5, cap) != 0 || hx_trace_workspace_words(k, 0) != 0 ||
        hx_trace_workspace_words(k, -1) != 0 || hx_trace_workspace_words((int64_t)1 << 31, cap) != 0) ++fails;
    uint32_t* ws = (uint32_t*)dev(words * 4);
    uint32_t* s = ws + (int64_t)HX_TRACE_FIELDS * cap * k;
    HxTrace T{ws, (float*)s, (int32_t*)(s + k), (int32_t*)(s + 2 * k), s + 3 * k, (int32_t*)(s + 4 * k), (int32_t*)(s + 5 * k), (int32_t*)(s + 6 * k), k, cap};
    float* state = (float*)dev(HX_ENV_WORDS * stride * 4); float* rew = (float*)dev(N * 4);
    uint8_t* done = (uint8_t*)dev(N); int8_t* succ = (int8_t*)dev(N); int32_t* ids = (int32_t*)dev(k * 4);
    OK(hx_trace_reset(&T, nullptr));
    OK(hx_trace_push(&T, state, N, stride, rew, done, succ, nullptr, 0, nullptr));
    OK(hx_trace_push(&T, state, N, stride, rew, done, succ, ids, cap - 1, nullptr));
    REFUSED(hx_trace_push(&T, state, N, stride, rew, done, succ, ids, cap, nullptr));
    REFUSED(hx_trace_push(&T, state, N, stride, rew, done, succ, ids, -1, nullptr));
    REFUSED(hx_trace_reset(nullptr, nullptr));
    REFUSED(hx_trace_push(nullptr, state, N, stride, rew, done, succ, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, nullptr, N, stride, rew, done, succ, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, state, N, stride, nullptr, done, succ, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, state, N, stride, rew, nullptr, succ, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, state, N, stride, rew, done, nullptr, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, state, 0, stride, rew, done, succ, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, state, N, N - 1, rew, done, succ, ids, 0, nullptr));
    REFUSED(hx_trace_push(&T, state, k - 1, stride, rew, done, succ, nullptr, 0, nullptr));  // envs 0..k-1 of fewer than k
    OK(hx_trace_push(&T, state, k - 1, stride, rew, done, succ, ids, 0, nullptr));           // ... a list may name an env of a smaller env
    HxTrace bad = T; bad.k = 0;
    REFUSED(hx_trace_reset(&bad, nullptr));
    bad = T; bad.k = -3;
    REFUSED(hx_trace_push(&bad, state, N, stride, rew, done, succ, ids, 0, nullptr));
    bad = T; bad.cap_steps = 0;
    REFUSED(hx_trace_reset(&bad, nullptr));
    bad = T; bad.cap_steps = -1;
    REFUSED(hx_trace_push(&bad, state, N, stride, rew, done, succ, ids, 0, nullptr));
    bad = T; bad.log = nullptr;
    REFUSED(hx_trace_push(&bad, state, N, stride, rew, done, succ, ids, 0, nullptr));
    bad = T; bad.end_step = nullptr;
    REFUSED(hx_trace_reset(&bad, nullptr));
    bad = T; bad.alive = nullptr;
    REFUSED(hx_trace_reset(&bad, nullptr));
    printf(fails ? "FAILED: %d\n" : "episode-record entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
