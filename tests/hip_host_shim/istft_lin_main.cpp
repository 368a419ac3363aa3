// Stand-alone driver of the host emulation of the linear-domain back end of csrc/istft.hip (eab_istft_lin_f32 and its adjoint
// eab_istft_lin_bwd_f32), on arrays allocated at their exact sizes (AddressSanitizer sees a read or a write past a row); the test
// poisons `spec` and `dwav` with NaN behind every length (the results see a read behind a length).
//   istft_lin_emulation IN OUT
//     IN:  int32 B, T, n_fft, hop, has_lens, B x int32 lens, float window[n_fft], float spec[B][2][T][F], float dwav[B][hop (T-1)]
//     OUT: float wav[B][hop (T-1)], float dspec[B][2][T][F]
// istft.hip keeps its LDS in one dynamic array (`extern __shared__ float smem[]`), which the shim's `static` cannot spell: this file
// compiles istft.hip itself with __shared__ empty and defines the array -- correct because one workgroup runs at a time.
#include <hip/hip_runtime.h>
#undef __shared__
#define __shared__
#include "istft.hip"
alignas(16) float smem[(2 * 512 + 2 * 8 * 512 + 512 + 8 * 2 * 257)];   // the larger of the kernels at n_fft = 512

#include <cmath>
#include <cstdio>
#include <vector>

template <class T>
static bool take(FILE* f, std::vector<T>& dst) { return fread(dst.data(), sizeof(T), dst.size(), f) == dst.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    std::vector<int> hd(5);
    if (!take(f, hd)) return 2;
    const int B = hd[0], T = hd[1], n_fft = hd[2], hop = hd[3], F = n_fft / 2 + 1;
    std::vector<int> lens(B);
    std::vector<float> window(n_fft), spec((size_t)B * 2 * T * F), dwav((size_t)B * hop * (T - 1)), twiddle(2 * (size_t)n_fft);
    if (!take(f, lens) || !take(f, window) || !take(f, spec) || !take(f, dwav)) return 2;
    for (int k = 0; k < n_fft; ++k) {
        twiddle[2 * k] = (float)std::cos(2.0 * M_PI * k / n_fft);
        twiddle[2 * k + 1] = (float)std::sin(2.0 * M_PI * k / n_fft);
    }
    const int* lp = hd[4] ? lens.data() : nullptr;
    std::vector<float> wav(dwav.size(), NAN), dspec(spec.size(), NAN);
    int rc = eab_istft_lin_f32(spec.data(), window.data(), twiddle.data(), wav.data(), lp, B, T, n_fft, hop, nullptr);
    if (rc) {
        printf("eab_istft_lin_f32 returned %d\n", rc);
        return 1;
    }
    rc = eab_istft_lin_bwd_f32(dwav.data(), spec.data(), window.data(), twiddle.data(), dspec.data(), lp, B, T, n_fft, hop, nullptr);
    if (rc) {
        printf("eab_istft_lin_bwd_f32 returned %d\n", rc);
        return 1;
    }
    fwrite(wav.data(), 4, wav.size(), o);
    fwrite(dspec.data(), 4, dspec.size(), o);
    fclose(f);
    fclose(o);
    return 0;
}
