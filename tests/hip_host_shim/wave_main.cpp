// Stand-alone driver of the host emulation of csrc/wave_loss.hip and of the ISTFT adjoint of csrc/istft.hip, on arrays allocated at
// their exact sizes (AddressSanitizer sees a read or a write past a row) and poisoned with NaN past every signal's own length (the
// results see a read past a length).
//   wave_emulation loss  IN OUT UNALIGNED
//     IN:  int32 B, double eps, B x (int32 est, clean samples), B x float weights, the est rows, the clean rows (fp32, own lengths)
//     OUT: double [B][3] (loss, a, c), float [B] loss, float [2] (sum, mean), float [B][cap_e] gradient
//   wave_emulation istft IN OUT 0
//     IN:  int32 B, T, n_fft, hop, has_lens, B x int32 lens, float window[n_fft], float dwav[B][hop (T-1)]
//     OUT: float [B][2][T][F]
// istft.hip keeps its LDS in one dynamic array (`extern __shared__ float smem[]`), which the shim's `static` cannot spell: this file
// compiles istft.hip itself with __shared__ empty and defines the array -- correct because one workgroup runs at a time.
#include <hip/hip_runtime.h>
#undef __shared__
#define __shared__
#include "../../eabnet_amd/csrc/istft.hip"
alignas(16) float smem[(2 * 512 + 2 * 8 * 512 + 512 + 8 * 2 * 257)];   // the larger of the two kernels at n_fft = 512

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define SPAN 4096                                                     /* EAB_SPAN of csrc/rows.h */

template <class T>
static bool take(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

static int run_loss(FILE* f, FILE* o, int odd) {
    int B = 0;
    double eps = 0.0;
    if (!take(f, &B, 1) || B < 1 || !take(f, &eps, 1)) return 2;
    std::vector<int> lens(2 * B);
    std::vector<float> weights(B);
    if (!take(f, lens.data(), lens.size()) || !take(f, weights.data(), weights.size())) return 2;
    int cap[2] = {0, 0};
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 2; ++k) cap[k] = std::max(cap[k], lens[2 * b + k]);
    float* sig[2];
    for (int k = 0; k < 2; ++k) {                                     // rows `cap` apart, the last one ends with its allocation
        const size_t n = (size_t)B * cap[k] + odd;
        void* p = nullptr;
        if (posix_memalign(&p, 16, n * sizeof(float))) return 2;
        std::fill_n((float*)p, n, NAN);
        sig[k] = (float*)p + odd;                                     // odd: 4 bytes past a 16-byte boundary
        for (int b = 0; b < B; ++b)
            if (!take(f, sig[k] + (size_t)b * cap[k], lens[2 * b + k])) return 2;
    }
    void* gp = nullptr;
    const size_t gn = (size_t)B * cap[0] + odd;
    if (posix_memalign(&gp, 16, gn * sizeof(float))) return 2;
    std::fill_n((float*)gp, gn, NAN);
    float* grad = (float*)gp + odd;
    const int spans = (std::max(cap[0], cap[1]) + SPAN - 1) / SPAN;
    std::vector<double> partial((size_t)B * spans * 3), out((size_t)B * 3);
    std::vector<float> loss(B), total(2);
    int rc = eab_si_sdr_loss_f32(sig[0], cap[0], cap[0], sig[1], cap[1], cap[1], lens.data(), B, eps, partial.data(), spans, out.data(),
                                 loss.data(), total.data(), nullptr);
    if (rc) {
        printf("eab_si_sdr_loss_f32 returned %d\n", rc);
        return 1;
    }
    rc = eab_si_sdr_loss_bwd_f32(sig[0], cap[0], cap[0], sig[1], cap[1], cap[1], lens.data(), B, out.data(), weights.data(), 1, 1.0, grad,
                                 cap[0], nullptr);
    if (rc) {
        printf("eab_si_sdr_loss_bwd_f32 returned %d\n", rc);
        return 1;
    }
    fwrite(out.data(), 8, out.size(), o);
    fwrite(loss.data(), 4, loss.size(), o);
    fwrite(total.data(), 4, total.size(), o);
    fwrite(grad, 4, (size_t)B * cap[0], o);
    for (int k = 0; k < 2; ++k) free(sig[k] - odd);
    free(gp);
    return 0;
}

static int run_istft(FILE* f, FILE* o) {
    int hd[5];
    if (!take(f, hd, 5)) return 2;
    const int B = hd[0], T = hd[1], n_fft = hd[2], hop = hd[3], F = n_fft / 2 + 1;
    std::vector<int> lens(B);
    std::vector<float> window(n_fft), dwav((size_t)B * hop * (T - 1)), twiddle(2 * (size_t)n_fft);
    if (!take(f, lens.data(), lens.size()) || !take(f, window.data(), window.size()) || !take(f, dwav.data(), dwav.size())) return 2;
    for (int k = 0; k < n_fft; ++k) {
        twiddle[2 * k] = (float)std::cos(2.0 * M_PI * k / n_fft);
        twiddle[2 * k + 1] = (float)std::sin(2.0 * M_PI * k / n_fft);
    }
    std::vector<float> dspec((size_t)B * 2 * T * F, NAN);
    const int rc = eab_istft_bwd_f32(dwav.data(), window.data(), twiddle.data(), dspec.data(), hd[4] ? lens.data() : nullptr, B, T, n_fft,
                                     hop, nullptr);
    if (rc) {
        printf("eab_istft_bwd_f32 returned %d\n", rc);
        return 1;
    }
    fwrite(dspec.data(), 4, dspec.size(), o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    FILE* f = fopen(argv[2], "rb");
    FILE* o = fopen(argv[3], "wb");
    if (!f || !o) return 2;
    const int rc = strcmp(argv[1], "loss") == 0 ? run_loss(f, o, atoi(argv[4])) : run_istft(f, o);
    fclose(f);
    fclose(o);
    return rc;
}
