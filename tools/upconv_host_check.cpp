// Stand-alone HOST check of the nearest-x2 fold's host code under AddressSanitizer / UBSan: tnr_pack_dims of the two
// TNR_PACK_UP2_* packings, tnr_upconv_fold_table and the argument checks of tnr_upconv_wgrad_unfold.  No device is needed and no
// kernel is launched: every call below returns before its launch.  Build and run (CPU only):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/upconv_host_check.cpp trainner_amd/csrc/pack_api.hip trainner_amd/csrc/elementwise.hip -o /tmp/upconv_host_check
//   /tmp/upconv_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/trainner_hip.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, tnr_last_error()); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

int main() {
    int32_t ko = 0, ki = 0;
    int64_t n = 0;
    // the folded S of a Cin -> Cout 3x3 layer: its data-gradient produces Cout channels, S itself Cin channels
    const int dims[][2] = {{64, 64}, {32, 32}, {64, 32}, {3, 64}, {100, 12}, {4, 4}};
    for (const auto &d : dims) {
        const int cout = d[0], cin = d[1];
        CHECK(tnr_pack_dims(cout, cin, 3, 3, TNR_PACK_UP2_DGRAD_S2, &ko, &ki, &n) == TNR_OK);
        CHECK(ko >= cout && ko % 32 == 0 && ki >= cin && ki % 16 == 0 && n == (int64_t)16 * ko * ki);
        int32_t ko4 = 0, ki4 = 0;
        int64_t n4 = 0;      // the same slab shape as the 4x4 layer S would get
        CHECK(tnr_pack_dims(cin, cout, 4, 4, TNR_PACK_DGRAD_S2, &ko4, &ki4, &n4) == TNR_OK && ko4 == ko && ki4 == ki && n4 == n);
        CHECK(tnr_pack_dims(cout, cin, 3, 3, TNR_PACK_UP2_FWD_S2D, &ko, &ki, &n) == TNR_OK);
        CHECK(ko >= cin && ko % 32 == 0 && ki >= cout && ki % 16 == 0 && n == (int64_t)16 * ko * ki);
        CHECK(tnr_pack_dims(cin, cout, 4, 4, TNR_PACK_FWD_S2D, &ko4, &ki4, &n4) == TNR_OK && ko4 == ko && ki4 == ki && n4 == n);
        CHECK(tnr_pack_dims(cout, cin, 3, 3, TNR_PACK_UP2_DGRAD_S2, nullptr, nullptr, nullptr) == TNR_OK);      // every output is optional
    }
    CHECK(tnr_pack_dims(64, 64, 4, 4, TNR_PACK_UP2_DGRAD_S2, &ko, &ki, &n) == TNR_EINVAL);
    CHECK(tnr_pack_dims(64, 64, 3, 1, TNR_PACK_UP2_FWD_S2D, &ko, &ki, &n) == TNR_EINVAL);
    CHECK(tnr_pack_dims(64, 64, 3, 3, 10, &ko, &ki, &n) == TNR_EINVAL && strstr(tnr_last_error(), "bad kind") != nullptr);

    int32_t *tab = (int32_t *)malloc(144 * sizeof(int32_t));      // exactly 144 entries: a write past the end is the sanitizer's to find
    CHECK(tnr_upconv_fold_table(tab) == TNR_OK);
    int ones = 0;
    for (int i = 0; i < 144; ++i) {
        CHECK(tab[i] == 0 || tab[i] == 1);
        ones += tab[i];
    }
    CHECK(ones == 36);                                            // every 3x3 tap lands in 2 x 2 folded taps
    CHECK(tab[0 * 9 + 8] == 1 && tab[15 * 9 + 0] == 1 && tab[5 * 9 + 4] == 1 && tab[5 * 9 + 0] == 0);
    free(tab);
    CHECK(tnr_upconv_fold_table(nullptr) == TNR_EINVAL);

    float *buf = (float *)aligned_alloc(64, 64 * sizeof(float));
    CHECK(tnr_upconv_wgrad_unfold(nullptr, buf, 1, 1, 1.f, 0.f, nullptr) == TNR_EINVAL);
    CHECK(tnr_upconv_wgrad_unfold(buf, nullptr, 1, 1, 1.f, 0.f, nullptr) == TNR_EINVAL);
    CHECK(tnr_upconv_wgrad_unfold(buf, buf + 16, 0, 1, 1.f, 0.f, nullptr) == TNR_EINVAL);
    CHECK(tnr_upconv_wgrad_unfold(buf, buf + 16, 1, -1, 1.f, 0.f, nullptr) == TNR_EINVAL);
    CHECK(tnr_upconv_wgrad_unfold(buf, buf + 16, 1 << 14, 1 << 14, 1.f, 0.f, nullptr) == TNR_EINVAL);
    CHECK(tnr_upconv_wgrad_unfold(buf + 1, buf + 32, 1, 1, 1.f, 0.f, nullptr) == TNR_EINVAL && strstr(tnr_last_error(), "aligned") != nullptr);
    free(buf);
    printf("upconv host check ok\n");
    return 0;
}
