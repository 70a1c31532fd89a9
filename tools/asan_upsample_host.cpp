// tools/asan_upsample_host.cpp — the host paths of the success-upsampling entry points (hx_ups_*) under AddressSanitizer, as a stand-alone program on a
// box WITHOUT a GPU: the sizes, the argument checks and refusals, the packing of the three launches (dry runs in the asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_upsample_host.cpp -o /tmp/asan_upsample_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_upsample_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t cap = 3000;
    const int B = 128;
    printf("sizeof(HxUps) %d / %zu, words(3000) %lld, version %d\n", hx_ups_sizeof(), sizeof(HxUps), (long long)hx_ups_words(cap), hx_version());
    if (hx_ups_sizeof() != (int)sizeof(HxUps) || hx_ups_words(cap) != 3 || hx_ups_words(1024) != 1 || hx_ups_words(1025) != 2) ++fails;
    if (hx_ups_words(0) != 0 || hx_ups_words(-5) != 0 || hx_ups_words(((int64_t)1 << 24) + 1) != 0 || hx_ups_words((int64_t)1 << 24) != 16384) ++fails;
    if (hx_version() != HX_ABI_VERSION) ++fails;
    uint32_t* cnt = (uint32_t*)dev(3 * 4);
    uint64_t* marked = (uint64_t*)dev(8); uint64_t* total = (uint64_t*)dev(8);
    int8_t* labels = (int8_t*)dev(cap);
    float* ring = (float*)dev(cap * 128); float* rows = (float*)dev(B * 128); int32_t* idx = (int32_t*)dev(B * 4);
    uint64_t* x = (uint64_t*)dev((B + 2) * 8);
    int32_t* fire = (int32_t*)dev(5 * 4); float* table = (float*)dev(400 * 128); int32_t* idx_bc = (int32_t*)dev(B * 4); float* bc_rows = (float*)dev(B * 128);
    HxUps U{cnt, marked, total, labels, cap, 10};
    OK(hx_ups_mark_new(&U, 64, nullptr));
    OK(hx_ups_mark_new(&U, (int64_t)1 << 40, nullptr));
    OK(hx_ups_recount(&U, nullptr));
    OK(hx_ups_draw(&U, ring, B, B, nullptr, 7, 1, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    OK(hx_ups_draw(&U, ring, B, 100, x, 0, 0, idx, rows, fire, 5, table, idx_bc, bc_rows, nullptr));
    OK(hx_ups_draw(nullptr, nullptr, B, 0, x, 0, 0, nullptr, nullptr, fire, 1, table, idx_bc, bc_rows, nullptr));  // the BC replacement alone
    OK(hx_ups_draw(&U, ring, 1, 1, x, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    OK(hx_ups_draw(&U, ring, 1024, 1024, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));  // (dry run: nothing is written)
    REFUSED(hx_ups_mark_new(nullptr, 64, nullptr));
    REFUSED(hx_ups_mark_new(&U, 0, nullptr));
    REFUSED(hx_ups_mark_new(&U, -1, nullptr));
    REFUSED(hx_ups_recount(nullptr, nullptr));
    HxUps bad = U; bad.boost = 1;
    REFUSED(hx_ups_recount(&bad, nullptr));
    bad = U; bad.boost = 256;
    REFUSED(hx_ups_mark_new(&bad, 64, nullptr));
    bad = U; bad.cap = ((int64_t)1 << 24) + 1;
    REFUSED(hx_ups_recount(&bad, nullptr));
    bad = U; bad.cap = 0;
    REFUSED(hx_ups_recount(&bad, nullptr));
    bad = U; bad.cnt = nullptr;
    REFUSED(hx_ups_draw(&bad, ring, B, B, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    bad = U; bad.marked = nullptr;
    REFUSED(hx_ups_mark_new(&bad, 64, nullptr));
    bad = U; bad.total = nullptr;
    REFUSED(hx_ups_recount(&bad, nullptr));
    bad = U; bad.ring_success = labels + 1;  // not 16-byte aligned
    REFUSED(hx_ups_recount(&bad, nullptr));
    bad = U; bad.ring_success = nullptr;
    REFUSED(hx_ups_recount(&bad, nullptr));
    REFUSED(hx_ups_draw(&U, ring, 0, 0, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, 1025, 1, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B + 1, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, -1, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, 0, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));  // nothing to do
    REFUSED(hx_ups_draw(nullptr, ring, B, 4, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, nullptr, B, B, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, nullptr, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring + 1, B, B, nullptr, 0, 0, idx, rows, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, rows, fire, 0, table, idx_bc, bc_rows, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, rows, fire, 5, nullptr, idx_bc, bc_rows, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, rows, fire, 5, table, nullptr, bc_rows, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, rows, fire, 5, table, idx_bc, nullptr, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, rows, nullptr, 5, table, idx_bc, bc_rows, nullptr));
    REFUSED(hx_ups_draw(&U, ring, B, B, nullptr, 0, 0, idx, rows, fire, 5, table + 1, idx_bc, bc_rows, nullptr));
    printf(fails ? "FAILED: %d\n" : "success-upsampling entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
