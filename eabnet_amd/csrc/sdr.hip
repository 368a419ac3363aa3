// BSS-eval SDR per utterance of a padded batch, value and gradient: the estimate projected on the K shifts of the clean wave
// (the single-source SDR of mir_eval / fast_bss_eval in exact arithmetic; K = 1 is the SI-SDR of wave_loss.hip).  DESIGN §4.25.
//
// With e the estimate, s the clean wave (each zero from its own length up to N = the longer of the two, never read there),
// K = filter_length <= 512 and k10 = 10 / ln 10:
//     r[k] = sum_n s[n] s[n+k]    c[k] = sum_n s[n] e[n+k]    ee = sum_n e[n]^2              k = 0 .. K-1
//     R = Toeplitz(r) + load_diag r[0] I     h = R^-1 c     tgt = c . h     res = max(ee - tgt, 0)
//     sdr_b = 10 log10(tgt / res)            loss_b = -k10 [ ln(tgt + eps) - ln(res + eps) ]
//     d loss_b / d e[n] = a_b e[n] + c_b p[n],   p[n] = sum_k h[k] s[n-k],   a_b = 2 k10 / (res + eps),
//                                                c_b = -2 k10 [ 1 / (tgt + eps) + 1 / (res + eps) ]
// sdr_corr_kernel: workgroup (span, b) holds span `span` (EAB_SPAN samples, rows.h) of s with K-1 samples of look-ahead and the
// matching samples of e in LDS -- zeros at and past a signal's length, which is never read -- and lane t owns the lags t and
// t + 256: the fp64 product of two fp32 samples is exact, and a lag adds its products in ascending n.  ee by the scheme of
// score.hip (eab_span_reduce).  Partials are [B][spans][2K + 1] doubles: r, c, ee.
// sdr_solve_kernel: ONE WAVE per utterance adds the spans in index order and runs the symmetric Levinson recursion with a
// right-hand side in fp64.  Lane l owns the elements l, l + 64, .. (eight at K = 512) of the predictor a and of the solution x in
// registers; a copy of a in LDS serves the reversed reads a[m-j], and the two dot products of a step (the reflection numerator and
// the right-hand side's defect) go through one xor butterfly, after which every lane holds the same bits and the control flow stays
// uniform.  Order m+1 from order m:
//     num = sum_{j<m} a[j] r[m-j]   def = c[m] - sum_{j<m} x[j] r[m-j]   k = -num / E   E' = E (1 - k^2)   q = def / E'
//     a'[j] = a[j] + k a[m-j]   x'[j] = x[j] + q a'[m-j]   (a'[m-j] = a[m-j] + k a[j] from the same two registers)
// A row is NOT scored -- NaN in its value, its filter and its gradient row, no other row touched -- when r[0] is not positive, a
// prediction error E' is not positive (or not a number), or the clean wave has fewer than K samples.
// sdr_bwd_kernel: workgroup (span, b) filters s with h: taps, sums and a_b e + c_b p in fp64, rounded to fp32 once (e - p cancels
// at high SDR); a lane owns quads of outputs and slides a window of four samples down the taps.  grad_output is read on the
// device; exactly 0 from est's length to the row's end.  No atomics; every sum has one order: a row has the same bits alone, in any
// batch and in a second call.
#include "rows.h"

#define SDR_MAX_TAPS 512
#define SDR_WAVE 64
#define SDR_OWN (SDR_MAX_TAPS / SDR_WAVE)       /* elements of a and x a lane owns */
#define SDR_OUT 6                               /* doubles per utterance: sdr_dB, tgt, ee, loss, a_b, c_b */

typedef EabRows<2> SdrRows;         // estimate, clean

__global__ __launch_bounds__(EAB_SPAN_THREADS) void sdr_corr_kernel(const SdrRows rows, const int32_t* __restrict__ lens, int spans, int K,
                                                                    double* __restrict__ partial) {
    __shared__ float S[EAB_SPAN + SDR_MAX_TAPS - 1], E[EAB_SPAN + SDR_MAX_TAPS - 1];
    const int b = blockIdx.y, span = blockIdx.x, t = threadIdx.x;
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1);
    const int longest = max(le, ls);
    if ((long long)span * EAB_SPAN >= longest) return;           // (workgroup-uniform) the solve does not read this row
    const float* e = rows.p[0] + (long long)b * rows.stride[0];
    const float* s = rows.p[1] + (long long)b * rows.stride[1];
    const int n0 = span * EAB_SPAN;
    for (int i = t; i < EAB_SPAN + K - 1; i += EAB_SPAN_THREADS) {
        const long long idx = (long long)n0 + i;
        S[i] = idx < ls ? s[idx] : 0.0f;
        E[i] = idx < le ? e[idx] : 0.0f;
    }
    __syncthreads();
    double* P = partial + ((long long)b * spans + span) * (2 * K + 1);
    const int nv = min(EAB_SPAN, ls - n0);                        // s[n] = 0 from here on: every product is zero
    if (t + EAB_SPAN_THREADS < K) {                               // two lags
        const int k1 = t + EAB_SPAN_THREADS;
        double r0 = 0.0, c0 = 0.0, r1 = 0.0, c1 = 0.0;
        for (int n = 0; n < nv; ++n) {
            const double ds = (double)S[n];
            r0 = fma(ds, (double)S[n + t], r0);
            c0 = fma(ds, (double)E[n + t], c0);
            r1 = fma(ds, (double)S[n + k1], r1);
            c1 = fma(ds, (double)E[n + k1], c1);
        }
        P[t] = r0;
        P[K + t] = c0;
        P[k1] = r1;
        P[K + k1] = c1;
    } else if (t < K) {
        double r0 = 0.0, c0 = 0.0;
        for (int n = 0; n < nv; ++n) {
            const double ds = (double)S[n];
            r0 = fma(ds, (double)S[n + t], r0);
            c0 = fma(ds, (double)E[n + t], c0);
        }
        P[t] = r0;
        P[K + t] = c0;
    }
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < EAB_SPAN / (4 * EAB_SPAN_THREADS); ++j) {
        const int i = j * 4 * EAB_SPAN_THREADS + 4 * t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double de = (double)E[i + k];
            acc[0] = fma(de, de, acc[0]);
        }
    }
    eab_span_reduce<1>(acc, P + 2 * K);
}

// a and b of all 64 lanes -> their sums in every lane, the same bits in each (a + b is commutative at every stage)
__device__ __forceinline__ void sdr_wave_sum2(double& a, double& b) {
#pragma unroll
    for (int off = 1; off < SDR_WAVE; off <<= 1) {
        a += __shfl_xor(a, off, SDR_WAVE);
        b += __shfl_xor(b, off, SDR_WAVE);
    }
}

__global__ __launch_bounds__(SDR_WAVE) void sdr_solve_kernel(const double* __restrict__ partial, const int32_t* __restrict__ lens,
                                                             const SdrRows rows, int spans, int K, double load_diag, double eps,
                                                             double* __restrict__ out, double* __restrict__ h) {
    __shared__ double R[SDR_MAX_TAPS], Cc[SDR_MAX_TAPS], A[SDR_MAX_TAPS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1);
    const int longest = max(le, ls);
    const int used = (int)(((long long)longest + EAB_SPAN - 1) / EAB_SPAN);
    const int W = 2 * K + 1;
    const double* P = partial + (long long)b * spans * W;
    double a[SDR_OWN], x[SDR_OWN];
#pragma unroll
    for (int i = 0; i < SDR_OWN; ++i) {
        const int j = lane + SDR_WAVE * i;
        a[i] = j == 0 ? 1.0 : 0.0;
        x[i] = 0.0;
        if (j < K) {
            double rr = 0.0, cc = 0.0;
            for (int sp = 0; sp < used; ++sp) {
                rr += P[(long long)sp * W + j];
                cc += P[(long long)sp * W + K + j];
            }
            R[j] = rr;
            Cc[j] = cc;
            A[j] = a[i];
        }
    }
    double ee = 0.0;
    for (int sp = 0; sp < used; ++sp) ee += P[(long long)sp * W + 2 * K];
    __syncthreads();
    const double r0 = R[0];
    bool bad = !(r0 > 0.0) || ls < K;                             // (every lane decides alike: the same loads, the same bits)
    double Ep = r0 + load_diag * r0;
    if (lane == 0) x[0] = Cc[0] / Ep;
    for (int m = 1; m < K && !bad; ++m) {
        double arev[SDR_OWN], pn = 0.0, pd = 0.0;
#pragma unroll
        for (int i = 0; i < SDR_OWN; ++i) {
            const int j = lane + SDR_WAVE * i;
            arev[i] = 0.0;
            if (j <= m) {
                arev[i] = A[m - j];                               // (A[m] is still 0)
                if (j < m) {
                    const double rv = R[m - j];
                    pn = fma(a[i], rv, pn);
                    pd = fma(x[i], rv, pd);
                }
            }
        }
        sdr_wave_sum2(pn, pd);
        const double k = -pn / Ep;
        const double En = Ep * (1.0 - k * k);
        if (!(En > 0.0)) {
            bad = true;
            break;
        }
        const double q = (Cc[m] - pd) / En;
        Ep = En;
        __syncthreads();                                          // every lane has read the old A
#pragma unroll
        for (int i = 0; i < SDR_OWN; ++i) {
            const int j = lane + SDR_WAVE * i;
            if (j <= m) {
                const double an = a[i] + k * arev[i], ar = arev[i] + k * a[i];
                x[i] += q * ar;
                a[i] = an;
                A[j] = an;
            }
        }
        __syncthreads();
    }
    double tgt = 0.0, unused = 0.0;
#pragma unroll
    for (int i = 0; i < SDR_OWN; ++i) {
        const int j = lane + SDR_WAVE * i;
        if (j < K) tgt = fma(Cc[j], x[i], tgt);
    }
    sdr_wave_sum2(tgt, unused);
    const double nan = __builtin_nan("");
    if (h) {
#pragma unroll
        for (int i = 0; i < SDR_OWN; ++i) {
            const int j = lane + SDR_WAVE * i;
            if (j < K) h[(long long)b * K + j] = bad ? nan : x[i];
        }
    }
    if (lane == 0) {
        const double k10 = 4.342944819032518;                     // 10 / ln 10
        double res = ee - tgt;
        if (res < 0.0) res = 0.0;
        double* o = out + (long long)b * SDR_OUT;
        o[0] = bad ? nan : 10.0 * log10(tgt / res);
        o[1] = bad ? nan : tgt;
        o[2] = bad ? nan : ee;
        o[3] = bad ? nan : -k10 * (log(tgt + eps) - log(res + eps));
        o[4] = bad ? nan : 2.0 * k10 / (res + eps);
        o[5] = bad ? nan : -2.0 * k10 * (1.0 / (tgt + eps) + 1.0 / (res + eps));
    }
}

// grad row b: cap[0] floats, `gstride` floats between two rows; workgroup (span, b) writes span `span` of it
__global__ __launch_bounds__(EAB_SPAN_THREADS) void sdr_bwd_kernel(const SdrRows rows, const int32_t* __restrict__ lens, int K,
                                                                   const double* __restrict__ coef, const double* __restrict__ h,
                                                                   const float* __restrict__ gout, int gout_stride, double scale,
                                                                   float* __restrict__ grad, long long gstride) {
    __shared__ double H[SDR_MAX_TAPS];
    __shared__ float S[EAB_SPAN + SDR_MAX_TAPS];                  // S[i] = s[n0 - K + i]
    const int b = blockIdx.y, span = blockIdx.x, t = threadIdx.x;
    const int cap = rows.cap[0];
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1);
    const float* e = rows.p[0] + (long long)b * rows.stride[0];
    const float* s = rows.p[1] + (long long)b * rows.stride[1];
    float* g = grad + (long long)b * gstride;
    const bool ae = eab_aligned16(e), ag = eab_aligned16(g);
    const int n0 = span * EAB_SPAN;
    if (n0 < le) {                                                // (workgroup-uniform) a span past est's length filters nothing
        for (int i = t; i < K; i += EAB_SPAN_THREADS) H[i] = h[(long long)b * K + i];
        for (int i = t; i < EAB_SPAN + K; i += EAB_SPAN_THREADS) {
            const long long idx = (long long)n0 - K + i;
            S[i] = idx >= 0 && idx < ls ? s[idx] : 0.0f;
        }
    }
    __syncthreads();
    const double w = (double)gout[(long long)b * gout_stride] * scale;
    const double ca = w * coef[SDR_OUT * b + 4], cc = w * coef[SDR_OUT * b + 5];
#pragma unroll 1
    for (int j = 0; j < EAB_SPAN / (4 * EAB_SPAN_THREADS); ++j) {
        const int i0 = j * 4 * EAB_SPAN_THREADS + 4 * t;
        const int i = n0 + i0;
        if (i >= cap) continue;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < le) {
            float ve[4];
            eab_load4(e, ae, i, le, ve);
            // s[i + q - k] is S[i0 + q - k + K]: the window of the four outputs at tap k, moved down one sample per tap
            double w0 = (double)S[i0 + K], w1 = (double)S[i0 + K + 1], w2 = (double)S[i0 + K + 2], w3 = (double)S[i0 + K + 3];
            double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
            for (int k = 0; k < K; ++k) {
                const double hk = H[k];
                p0 = fma(hk, w0, p0);
                p1 = fma(hk, w1, p1);
                p2 = fma(hk, w2, p2);
                p3 = fma(hk, w3, p3);
                w3 = w2;
                w2 = w1;
                w1 = w0;
                w0 = (double)S[i0 + K - 1 - k];
            }
            const double p[4] = {p0, p1, p2, p3};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q < le) v[q] = (float)(ca * (double)ve[q] + cc * p[q]);
        }
        if (ag && i + 4 <= cap) {
            *reinterpret_cast<f32x4*>(g + i) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q < cap) g[i + q] = v[q];
        }
    }
}

static inline bool sdr_finite_nonneg(double v) { return v >= 0.0 && v < 1e300; }   // (refuses NaN too)

extern "C" int eab_sdr_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride, int clean_cap,
                           const int32_t* lens, int B, int filter_length, double load_diag, double eps, double* partial,
                           int partial_spans, double* out, double* h, eab_stream_t stream) {
    const SdrRows rows = {{est, clean}, {est_stride, clean_stride}, {est_cap, clean_cap}};
    EAB_CHECK_ARG(lens && partial && out && eab_rows_ok(rows, B));
    EAB_CHECK_ARG(filter_length >= 1 && filter_length <= SDR_MAX_TAPS);
    EAB_CHECK_ARG(sdr_finite_nonneg(load_diag) && sdr_finite_nonneg(eps));
    const int spans = eab_rows_spans(rows);
    EAB_CHECK_ARG(partial_spans >= spans);
    hipLaunchKernelGGL(sdr_corr_kernel, dim3((unsigned)spans, (unsigned)B), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), rows, lens,
                       partial_spans, filter_length, partial);
    hipLaunchKernelGGL(sdr_solve_kernel, dim3((unsigned)B), dim3(SDR_WAVE), 0, eab_stream(stream), partial, lens, rows, partial_spans,
                       filter_length, load_diag, eps, out, h);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_sdr_loss_bwd_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride,
                                    int clean_cap, const int32_t* lens, int B, int filter_length, const double* coef, const double* h,
                                    const float* grad_out, int grad_out_stride, double scale, float* grad, long long grad_stride,
                                    eab_stream_t stream) {
    const SdrRows rows = {{est, clean}, {est_stride, clean_stride}, {est_cap, clean_cap}};
    EAB_CHECK_ARG(lens && coef && h && grad_out && grad && eab_rows_ok(rows, B));
    EAB_CHECK_ARG(filter_length >= 1 && filter_length <= SDR_MAX_TAPS);
    EAB_CHECK_ARG(grad_out_stride >= 0 && (B == 1 || grad_stride >= est_cap));
    const int spans = eab_spans(est_cap);
    hipLaunchKernelGGL(sdr_bwd_kernel, dim3((unsigned)spans, (unsigned)B), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), rows, lens,
                       filter_length, coef, h, grad_out, grad_out_stride, scale, grad, grad_stride);
    EAB_RETURN_LAUNCH_STATUS();
}
