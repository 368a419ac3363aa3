// Stand-alone driver of the host emulation of csrc/score.hip: eab_energy_ratios_f32 on rows allocated at their exact size (the
// batch's last row ends where its allocation ends) and poisoned with NaN past every signal's own length, and
// eab_com_mag_mse_loss_lens_f32 on spectra of exactly B * 2 * T * F floats (the caller poisons the frames past frames[b]), so that
// AddressSanitizer sees a read past a row and the scores see a read past a length.
//   score_emulation IN OUT UNALIGNED
// IN:  int32 B, B x (int32 est, clean, noisy samples), the est rows, the clean rows, the noisy rows (fp32, own lengths, back to
//      back); int32 Bl, F, T_esti, T_label, Bl x int32 frames, esti [Bl][2][T_esti][F], label [Bl][2][T_label][F] (Bl = 0: no loss)
// OUT: double [B][8] ratios and energies, double [Bl] losses
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eabnet_hip.h"

#define SPAN 4096                                                     /* EAB_SPAN of csrc/rows.h */

template <class T>
static bool take(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int B = 0;
    if (!take(f, &B, 1) || B < 1) return 2;
    std::vector<int> lens(3 * B);
    if (!take(f, lens.data(), lens.size())) return 2;
    int cap[3] = {0, 0, 0};
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 3; ++k) cap[k] = std::max(cap[k], lens[3 * b + k]);
    const int odd = atoi(argv[3]);                                    // 1: the rows start 4 bytes past a 16-byte boundary, 0: on one
    float* sig[3];
    for (int k = 0; k < 3; ++k) {
        const size_t n = (size_t)B * cap[k] + odd;
        void* p = nullptr;
        if (posix_memalign(&p, 16, n * sizeof(float))) return 2;
        std::fill_n((float*)p, n, NAN);
        sig[k] = (float*)p + odd;
        for (int b = 0; b < B; ++b)
            if (!take(f, sig[k] + (size_t)b * cap[k], lens[3 * b + k])) return 2;
    }
    int hd[4] = {0, 0, 0, 0};                                         // Bl, F, T_esti, T_label
    if (!take(f, hd, 4)) return 2;
    const int Bl = hd[0], F = hd[1], Te = hd[2], Tl = hd[3];
    std::vector<int> frames(Bl);
    std::vector<float> esti((size_t)Bl * 2 * Te * F), label((size_t)Bl * 2 * Tl * F);
    if (!take(f, frames.data(), frames.size()) || !take(f, esti.data(), esti.size()) || !take(f, label.data(), label.size())) return 2;
    fclose(f);

    const int spans = (std::max(cap[0], std::max(cap[1], cap[2])) + SPAN - 1) / SPAN;
    std::vector<double> partial((size_t)B * spans * 6), out((size_t)B * 8), loss(Bl);
    int rc = eab_energy_ratios_f32(sig[0], cap[0], cap[0], sig[1], cap[1], cap[1], sig[2], cap[2], cap[2], lens.data(), B,
                                   partial.data(), spans, out.data(), nullptr);
    if (rc) {
        printf("eab_energy_ratios_f32 returned %d\n", rc);
        return 1;
    }
    if (Bl) {
        const int lspans = (std::min(Te, Tl) * F + SPAN - 1) / SPAN;
        std::vector<double> lpartial((size_t)Bl * lspans * 2);
        rc = eab_com_mag_mse_loss_lens_f32(esti.data(), label.data(), frames.data(), Bl, Te, Tl, F, lpartial.data(), lspans, loss.data(),
                                           nullptr);
        if (rc) {
            printf("eab_com_mag_mse_loss_lens_f32 returned %d\n", rc);
            return 1;
        }
    }
    for (int k = 0; k < 3; ++k) free(sig[k] - odd);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    fwrite(loss.data(), 8, loss.size(), o);
    fclose(o);
    return 0;
}
