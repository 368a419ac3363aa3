// Stand-alone driver of the host emulation of csrc/spec_loss.hip on arrays allocated at their exact sizes (AddressSanitizer sees a
// read or a write past a row, a table or a workspace); the caller poisons the rows with NaN past every length (the results see a
// read past a length).
//   mrstft_emulation IN OUT UNALIGNED
//     IN:  int32 B, R, cap_e, cap_s; double factor_sc, factor_mag, floor; R x int32 (n_fft, hop, win); B x int32 lens;
//          B x float weights; float est[B][cap_e]; float clean[B][cap_s]
//     OUT: double coef[B][R][2], float loss[B], float total[2], float grad[B][cap_e]
// spec_loss.hip keeps its LDS in one dynamic array (`extern __shared__ float mr_smem[]`), which the shim's `static` cannot spell:
// this file compiles spec_loss.hip itself with __shared__ empty and defines the array -- correct because one workgroup runs at a
// time.
#include <hip/hip_runtime.h>
#undef __shared__
#define __shared__
#include "../../eabnet_amd/csrc/spec_loss.hip"
alignas(16) float mr_smem[(72 * MR_MAX_NFFT + (MR_MAX_THREADS / 64) * 24) / 4];

#include <cstdio>
#include <cstdlib>
#include <vector>

template <class T>
static bool take(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

static float* rows_alloc(FILE* f, size_t n, int odd, bool read) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, (n + odd) * sizeof(float))) return nullptr;
    float* q = (float*)p + odd;                                       // odd: 4 bytes past a 16-byte boundary
    for (size_t i = 0; i < n; ++i) q[i] = NAN;
    if (read && !take(f, q, n)) return nullptr;
    return q;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    const int odd = atoi(argv[3]) ? 1 : 0;
    if (!f || !o) return 2;
    int hd[4];
    double par[3];
    if (!take(f, hd, 4) || !take(f, par, 3)) return 2;
    const int B = hd[0], R = hd[1], cap_e = hd[2], cap_s = hd[3];
    if (B < 1 || R < 1 || R > 8 || cap_e < 1 || cap_s < 1) return 2;
    std::vector<int32_t> res(3 * (size_t)R), lens(B);
    std::vector<float> weights(B);
    if (!take(f, res.data(), res.size()) || !take(f, lens.data(), lens.size()) || !take(f, weights.data(), weights.size())) return 2;
    float* est = rows_alloc(f, (size_t)B * cap_e, odd, true);
    float* clean = rows_alloc(f, (size_t)B * cap_s, odd, true);
    float* grad = rows_alloc(f, (size_t)B * cap_e, odd, false);
    if (!est || !clean || !grad) return 2;
    std::vector<float> tables;
    for (int r = 0; r < R; ++r) {
        const int N = res[3 * r], W = res[3 * r + 2], left = (N - W) / 2;
        if (N < 2 || W < 1 || W > N) return 2;
        for (int i = 0; i < N; ++i) tables.push_back(i >= left && i < left + W ? (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (i - left) / W)) : 0.0f);
        for (int k = 0; k < N; ++k) {
            tables.push_back((float)std::cos(2.0 * M_PI * k / N));
            tables.push_back((float)std::sin(2.0 * M_PI * k / N));
        }
    }
    const int cap = std::min(cap_e, cap_s);
    const long long wf = eab_mrstft_workspace_bytes(res.data(), R, B, cap, 0), wb = eab_mrstft_workspace_bytes(res.data(), R, B, cap, 1);
    if (wf < 0 || wb < 0) {
        printf("eab_mrstft_workspace_bytes refused the arguments\n");
        return 1;
    }
    std::vector<double> work_f((size_t)wf / 8), coef((size_t)B * R * 2);
    std::vector<float> work_b((size_t)wb / 4, NAN), loss(B), total(2);
    int rc = eab_mrstft_loss_f32(est, cap_e, cap_e, clean, cap_s, cap_s, lens.data(), B, res.data(), R, tables.data(), par[0], par[1], par[2],
                                 work_f.data(), wf, coef.data(), loss.data(), total.data(), nullptr);
    if (rc) {
        printf("eab_mrstft_loss_f32 returned %d\n", rc);
        return 1;
    }
    rc = eab_mrstft_loss_bwd_f32(est, cap_e, cap_e, clean, cap_s, cap_s, lens.data(), B, res.data(), R, tables.data(), par[2], coef.data(),
                                 weights.data(), 1, 1.0, work_b.data(), wb, grad, cap_e, nullptr);
    if (rc) {
        printf("eab_mrstft_loss_bwd_f32 returned %d\n", rc);
        return 1;
    }
    fwrite(coef.data(), 8, coef.size(), o);
    fwrite(loss.data(), 4, loss.size(), o);
    fwrite(total.data(), 4, total.size(), o);
    fwrite(grad, 4, (size_t)B * cap_e, o);
    fclose(f);
    fclose(o);
    free(est - odd);
    free(clean - odd);
    free(grad - odd);
    return 0;
}
