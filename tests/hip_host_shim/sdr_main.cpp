// Stand-alone driver of the host emulation of csrc/sdr.hip: the three kernels (correlations, Levinson solve, gradient filter) on the
// CPU under AddressSanitizer and UBSan.
//   sdr_emulation IN OUT
//     IN:  int32 B, int32 K, double load_diag, double eps, B x (int32 est, clean samples), B x float weights, the est rows, the
//          clean rows (fp32, own lengths)
//     OUT: per row ALONE (B = 1): double [6] out, double [K] h, float [est samples] gradient; then of the BATCH: double [B][6],
//          double [B][K], float [B][cap_e]
// Alone, every array of a row -- est, clean, lengths, partials, out, h, weight, gradient -- is an allocation of exactly its size, the
// row's capacity being its own length: a read or a write past a length or a capacity is a sanitizer report.  In the batch the rows
// lie `cap` apart, 4 bytes off a 16-byte boundary, the last one ending with its allocation, and NaN fills what lies past a length.
// The solve kernel adds across a wave with __shfl_xor, which the shim's header does not have: it is defined here, before the kernel
// file is included (two alternating halves of the shim's slots, so one barrier per exchange is enough).
#include <hip/hip_runtime.h>

static inline double __shfl_xor(double v, int mask, int) {
    static thread_local unsigned turn = 0;
    const int t = threadIdx.x;
    double* slot = shim.slot + 512 * (turn++ & 1);
    slot[t] = v;
    pthread_barrier_wait(&shim.wave[t >> 6]);
    return slot[t ^ mask];                                            // mask < 64: a lane of the same wave
}

#include "sdr.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class T>
static bool take(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

template <class T>
static T* exact(size_t n) { return (T*)malloc(n * sizeof(T)); }

static int fail(const char* what, int rc) {
    printf("%s returned %d\n", what, rc);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int B = 0, K = 0;
    double load_diag = 0.0, eps = 0.0;
    if (!take(f, &B, 1) || !take(f, &K, 1) || B < 1 || K < 1 || !take(f, &load_diag, 1) || !take(f, &eps, 1)) return 2;
    std::vector<int> lens(2 * B);
    std::vector<float> weights(B);
    if (!take(f, lens.data(), lens.size()) || !take(f, weights.data(), weights.size())) return 2;
    std::vector<std::vector<float>> sig[2];
    int cap[2] = {0, 0};
    for (int k = 0; k < 2; ++k)
        for (int b = 0; b < B; ++b) {
            sig[k].emplace_back(lens[2 * b + k]);
            if (!take(f, sig[k][b].data(), sig[k][b].size())) return 2;
            cap[k] = std::max(cap[k], lens[2 * b + k]);
        }
    // every row alone
    for (int b = 0; b < B; ++b) {
        const int le = lens[2 * b], ls = lens[2 * b + 1], spans = (std::max(le, ls) + EAB_SPAN - 1) / EAB_SPAN;
        float* e = exact<float>(le);
        float* s = exact<float>(ls);
        float* g = exact<float>(le);
        float* w = exact<float>(1);
        int* l2 = exact<int>(2);
        double* partial = exact<double>((size_t)spans * (2 * K + 1));
        double* out = exact<double>(SDR_OUT);
        double* h = exact<double>(K);
        memcpy(e, sig[0][b].data(), 4 * (size_t)le);
        memcpy(s, sig[1][b].data(), 4 * (size_t)ls);
        std::fill_n(g, le, NAN);
        w[0] = weights[b];
        l2[0] = le;
        l2[1] = ls;
        int rc = eab_sdr_f32(e, le, le, s, ls, ls, l2, 1, K, load_diag, eps, partial, spans, out, h, nullptr);
        if (rc) return fail("eab_sdr_f32", rc);
        rc = eab_sdr_loss_bwd_f32(e, le, le, s, ls, ls, l2, 1, K, out, h, w, 1, 1.0, g, le, nullptr);
        if (rc) return fail("eab_sdr_loss_bwd_f32", rc);
        fwrite(out, 8, SDR_OUT, o);
        fwrite(h, 8, K, o);
        fwrite(g, 4, le, o);
        free(e); free(s); free(g); free(w); free(l2); free(partial); free(out); free(h);
    }
    // the batch
    float* rows[2];
    void* raw[3];
    for (int k = 0; k < 2; ++k) {
        const size_t n = (size_t)B * cap[k] + 1;
        if (posix_memalign(&raw[k], 16, n * sizeof(float))) return 2;
        std::fill_n((float*)raw[k], n, NAN);
        rows[k] = (float*)raw[k] + 1;
        for (int b = 0; b < B; ++b) memcpy(rows[k] + (size_t)b * cap[k], sig[k][b].data(), 4 * sig[k][b].size());
    }
    const size_t gn = (size_t)B * cap[0] + 1;
    if (posix_memalign(&raw[2], 16, gn * sizeof(float))) return 2;
    std::fill_n((float*)raw[2], gn, NAN);
    float* grad = (float*)raw[2] + 1;
    const int spans = (std::max(cap[0], cap[1]) + EAB_SPAN - 1) / EAB_SPAN;
    std::vector<double> partial((size_t)B * spans * (2 * K + 1), NAN), out((size_t)B * SDR_OUT, NAN), h((size_t)B * K, NAN);
    int rc = eab_sdr_f32(rows[0], cap[0], cap[0], rows[1], cap[1], cap[1], lens.data(), B, K, load_diag, eps, partial.data(), spans,
                         out.data(), h.data(), nullptr);
    if (rc) return fail("eab_sdr_f32", rc);
    rc = eab_sdr_loss_bwd_f32(rows[0], cap[0], cap[0], rows[1], cap[1], cap[1], lens.data(), B, K, out.data(), h.data(), weights.data(), 1,
                              1.0, grad, cap[0], nullptr);
    if (rc) return fail("eab_sdr_loss_bwd_f32", rc);
    fwrite(out.data(), 8, out.size(), o);
    fwrite(h.data(), 8, h.size(), o);
    fwrite(grad, 4, (size_t)B * cap[0], o);
    for (void* p : raw) free(p);
    fclose(f);
    fclose(o);
    return 0;
}
