// tools/asan_nstep_label_host.cpp — the host path of hx_nstep_label (the n-step relabelling of a labelled expert table) under AddressSanitizer, as a
// stand-alone program on a box WITHOUT a GPU: the argument checks and refusals, the packing of the launch (a dry run in the asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_nstep_label_host.cpp -o /tmp/asan_nstep_label_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_nstep_label_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t E = 300;
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 132) ++fails;
    float* both = (float*)dev(2 * E * 128);  // rows_in, and rows_out right behind it
    float* in = both; float* out = both + E * 32;
    uint8_t* last = (uint8_t*)dev(E);
    for (int n = 1; n <= HX_NSTEP_MAX; ++n) OK(hx_nstep_label(in, last, E, n, 0.99f, out, nullptr));
    OK(hx_nstep_label(in, last, 1, 3, 0.0f, out, nullptr));
    OK(hx_nstep_label(out, last, E, 3, 1.0f, in, nullptr));  // (back to back either way round is no overlap)
    REFUSED(hx_nstep_label(in, last, E, 0, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, E, HX_NSTEP_MAX + 1, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, 0, 3, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, -1, 3, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, (int64_t)1 << 31, 3, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, E, 3, 1.5f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, E, 3, -0.5f, out, nullptr));
    REFUSED(hx_nstep_label(nullptr, last, E, 3, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, nullptr, E, 3, 0.99f, out, nullptr));
    REFUSED(hx_nstep_label(in, last, E, 3, 0.99f, nullptr, nullptr));
    REFUSED(hx_nstep_label(in + 1, last, E - 1, 3, 0.99f, out, nullptr));   // misaligned
    REFUSED(hx_nstep_label(in, last, E - 1, 3, 0.99f, out + 2, nullptr));
    REFUSED(hx_nstep_label(in, last, E, 3, 0.99f, in, nullptr));            // in place
    REFUSED(hx_nstep_label(in, last, E, 3, 0.99f, out - 4, nullptr));       // the last 16 bytes of rows_in
    REFUSED(hx_nstep_label(in + 32, last, E, 3, 0.99f, in, nullptr));       // one row apart
    printf(fails ? "FAILED: %d\n" : "hx_nstep_label ran its host path under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
