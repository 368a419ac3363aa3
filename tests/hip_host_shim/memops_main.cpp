// Stand-alone driver of the host emulation of csrc/norm.hip and csrc/cln.hip (inference side): one entry point per run, every
// array allocated at EXACTLY its size (16-byte aligned, as the arenas are), so that AddressSanitizer sees any access outside
// one; the outputs start from a sentinel, so a write outside the rows of the launch shows in the file.
//   memops_emulation IN OUT
// IN: int32 [12] header, float eps, int32 [B] lens, then the fp32 arrays of the entry point; OUT: its outputs.
//   header[0] = 1  norm_act[_win]:  B T rows_per_t C two use_win pos count use_lens
//        in  a [B][P][C], xfa [B][C][2], slopea [C] (, b, xfb, slopeb)                      out  out [B][P][C]
//   header[0] = 2  in_finalize[_mr]: B C nsets tiles count with_mr
//        in  stats [B][tiles][nsets][C][4], gamma0 [C], beta0 [C] (, gamma1, beta1)         out  xf0 (, xf1) (, mr0 (, mr1)) [B][C][2]
//   header[0] = 3  cLN unit:  B T P C mode use_slope use_add chunk
//        chunk 0: cln_stats + cln_apply on the whole utterance; chunk k > 0: windows of k frames with the state carried (the last
//        one clipped by the end); chunk -1: eab_cln_step_f32 frame by frame
//        in  x [B][T][P], slope [C], gain [C], bias [C], add [B][T][P]
//        out sums [B][T][2] and state [3B] (doubles), mr [B][T][2], y [B][T][P]
//   header[0] = 4  gate_rows:  B T row use_win pos count
//        in  a, r [B][T][row]                                                               out  z [B][T][row]
#include <hip/hip_runtime.h>

// (the device's two-argument form: the width is the wave)
static inline double __shfl_down(double v, int off) { return __shfl_down(v, off, 64); }

#include "norm.hip"
#include "cln.hip"

#include <cstdio>
#include <cstdlib>

#define SENTINEL 7.25f

template <typename T>
static T* exact(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * sizeof(T))) exit(2);
    return static_cast<T*>(p);
}

static FILE* fin;
static FILE* fout;

static float* rd(size_t n) {
    float* p = exact<float>(n);
    if (fread(p, 4, n, fin) != n) exit(2);
    return p;
}

template <typename T>
static T* fresh(size_t n) {
    T* p = exact<T>(n);
    for (size_t k = 0; k < n; ++k) p[k] = (T)SENTINEL;
    return p;
}

template <typename T>
static void put(T* p, size_t n) {
    fwrite(p, sizeof(T), n, fout);
    free(p);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    fin = fopen(argv[1], "rb");
    if (!fin) return 2;
    int h[12];
    float eps;
    if (fread(h, 4, 12, fin) != 12 || fread(&eps, 4, 1, fin) != 1) return 2;
    const int kind = h[0], B = h[1];
    if (B < 1 || B > 4096) return 2;
    int32_t* lens = exact<int32_t>(B);                                         // exactly B counts
    if (fread(lens, 4, B, fin) != (size_t)B) return 2;
    int32_t* pos = exact<int32_t>(1);
    fout = fopen(argv[2], "wb");
    if (!fout) return 2;
    int rc = 0;
    if (kind == 1) {
        const int T = h[2], rpt = h[3], C = h[4], two = h[5], use_win = h[6], use_lens = h[9];
        const size_t n = (size_t)B * T * rpt * C;
        float *a = rd(n), *xfa = rd((size_t)B * C * 2), *sla = rd(C), *b = nullptr, *xfb = nullptr, *slb = nullptr;
        if (two) b = rd(n), xfb = rd((size_t)B * C * 2), slb = rd(C);
        float* out = fresh<float>(n);
        *pos = h[7];
        const eab_time_window win{use_win ? pos : nullptr, use_win ? h[8] : 0, use_lens ? lens : nullptr};
        rc = use_win || use_lens ? eab_norm_act_win_f32(a, xfa, sla, b, xfb, slb, out, B, T, rpt, C, win, nullptr)
                                 : eab_norm_act_f32(a, xfa, sla, b, xfb, slb, out, B, T * rpt, C, nullptr);
        put(out, n);
        for (float* p : {a, xfa, sla, b, xfb, slb}) free(p);
    } else if (kind == 2) {
        const int C = h[2], nsets = h[3], tiles = h[4], count = h[5], with_mr = h[6];
        float* stats = rd((size_t)B * tiles * nsets * C * 4);
        float *g[2] = {nullptr, nullptr}, *be[2] = {nullptr, nullptr}, *xf[2] = {nullptr, nullptr}, *mr[2] = {nullptr, nullptr};
        const size_t n = (size_t)B * C * 2;
        for (int s = 0; s < nsets; ++s) g[s] = rd(C), be[s] = rd(C), xf[s] = fresh<float>(n), mr[s] = with_mr ? fresh<float>(n) : nullptr;
        rc = with_mr ? eab_in_finalize_mr_f32(stats, B, C, nsets, tiles, count, eps, g[0], be[0], xf[0], g[1], be[1], xf[1], mr[0], mr[1], nullptr)
                     : eab_in_finalize_f32(stats, B, C, nsets, tiles, count, eps, g[0], be[0], xf[0], g[1], be[1], xf[1], nullptr);
        for (int s = 0; s < nsets; ++s) put(xf[s], n);
        for (int s = 0; s < nsets && with_mr; ++s) put(mr[s], n);
        for (float* p : {stats, g[0], g[1], be[0], be[1]}) free(p);
    } else if (kind == 3) {
        const int T = h[2], P = h[3], C = h[4], mode = h[5], use_slope = h[6], use_add = h[7], chunk = h[8];
        const size_t n = (size_t)B * T * P, rows = (size_t)B * T;
        float *x = rd(n), *slope = rd(C), *gain = rd(C), *bias = rd(C), *add = rd(n);
        double *sums = fresh<double>(rows * 2), *state = fresh<double>(3 * (size_t)B);
        float *mr = fresh<float>(rows * 2), *y = fresh<float>(n);
        const float* st_slope = use_slope ? slope : nullptr;
        const float* ad = use_add ? add : nullptr;
        if (chunk == 0) {
            const eab_time_window win{nullptr, 0, nullptr};
            rc = eab_cln_stats_f32(x, st_slope, B, T, P, C, eps, sums, state, mr, win, nullptr);
            if (!rc) rc = eab_cln_apply_f32(x, mr, gain, bias, slope, ad, y, B, T, P, C, mode, win, nullptr);
        } else if (chunk > 0) {
            for (*pos = 0; *pos < T && !rc; *pos += chunk) {
                const eab_time_window win{pos, chunk, nullptr};
                rc = eab_cln_stats_f32(x, st_slope, B, T, P, C, eps, sums, state, mr, win, nullptr);
                if (!rc) rc = eab_cln_apply_f32(x, mr, gain, bias, slope, ad, y, B, T, P, C, mode, win, nullptr);
            }
        } else {
            for (*pos = 0; *pos < T && !rc; ++*pos) {
                const eab_time_window win{pos, 1, nullptr};
                rc = eab_cln_step_f32(x, st_slope, sums, state, mr, gain, bias, slope, ad, y, B, T, P, C, mode, eps, win, nullptr);
            }
        }
        put(sums, rows * 2);
        put(state, 3 * (size_t)B);
        put(mr, rows * 2);
        put(y, n);
        for (float* p : {x, slope, gain, bias, add}) free(p);
    } else if (kind == 4) {
        const int T = h[2], row = h[3], use_win = h[4];
        const size_t n = (size_t)B * T * row;
        float *a = rd(n), *r = rd(n), *z = fresh<float>(n);
        *pos = h[5];
        const eab_time_window win{use_win ? pos : nullptr, use_win ? h[6] : 0, nullptr};
        rc = eab_gate_rows_f32(a, r, z, B, T, row, win, nullptr);
        put(z, n);
        free(a);
        free(r);
    } else {
        return 2;
    }
    fclose(fin);
    fclose(fout);
    free(lens);
    free(pos);
    if (rc) {
        printf("memops entry point returned %d\n", rc);
        return 1;
    }
    return 0;
}
