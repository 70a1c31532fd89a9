// tools/asan_pilot_host.cpp — the host paths of the pilot entry points (hx_pilot_act, hx_pilot_refresh) under AddressSanitizer, as a stand-alone
// program on a box WITHOUT a GPU: the argument checks and refusals, the residues of a 64-bit call count, the packing of the two launches (dry runs in
// the asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_pilot_host.cpp -o /tmp/asan_pilot_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_pilot_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ != HX_ERR_ARG) { printf("NOT REFUSED (rc %d): %s\n", rc_, #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t N = 300, stride = 320, E0 = 40, M = 50;
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 126) ++fails;
    float* state = (float*)dev(37 * stride * 4); float* obs = (float*)dev(N * 13 * 4); float* noise = (float*)dev(N * 3 * 4);
    float* act = (float*)dev(N * 4 * 4); float* table = (float*)dev((E0 + M) * 32 * 4);
    OK(hx_pilot_act(state, N, stride, obs, nullptr, act, nullptr));
    OK(hx_pilot_act(state, N, N, obs, noise, act, nullptr));
    OK(hx_pilot_act(state, 1, 1, obs, noise, act, nullptr));
    REFUSED(hx_pilot_act(nullptr, N, stride, obs, nullptr, act, nullptr));
    REFUSED(hx_pilot_act(state, N, stride, nullptr, nullptr, act, nullptr));
    REFUSED(hx_pilot_act(state, N, stride, obs, nullptr, nullptr, nullptr));
    REFUSED(hx_pilot_act(state, N, stride, obs, nullptr, act + 1, nullptr));
    REFUSED(hx_pilot_act(state, 0, stride, obs, nullptr, act, nullptr));
    REFUSED(hx_pilot_act(state, -1, stride, obs, nullptr, act, nullptr));
    REFUSED(hx_pilot_act(state, N, N - 1, obs, nullptr, act, nullptr));
    REFUSED(hx_pilot_act(state, (int64_t)1 << 31, (int64_t)1 << 31, obs, nullptr, act, nullptr));
    const uint64_t calls[] = {0, 1, 299, 300, 0xFFFFFFFFull, 0x100000000ull, 1ull << 40, ~0ull};
    for (uint64_t c : calls) {
        OK(hx_pilot_refresh(state, N, stride, obs, table, E0, M, 7, c, nullptr));
        OK(hx_pilot_refresh(state, N, stride, obs, table, E0, M, 50, c, nullptr));
    }
    OK(hx_pilot_refresh(state, N, stride, obs, table, 0, M, 1, 3, nullptr));
    OK(hx_pilot_refresh(state, 1, 1, obs, table, 3, 1, 1, 1ull << 40, nullptr));
    OK(hx_pilot_refresh(state, N, stride, obs, table, 1, 89, 89, 5, nullptr));
    REFUSED(hx_pilot_refresh(nullptr, N, stride, obs, table, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, nullptr, table, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, nullptr, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table + 1, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table + 16, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, 0, stride, obs, table, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, N - 1, obs, table, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table, -1, M, 7, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table, E0, 0, 1, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table, E0, M, 0, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table, E0, M, -4, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table, E0, M, 51, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, 40, stride, obs, table, E0, M, 41, 0, nullptr));
    REFUSED(hx_pilot_refresh(state, N, stride, obs, table, (int64_t)1 << 31, M, 7, 0, nullptr));
    printf(fails ? "FAILED: %d\n" : "pilot entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
