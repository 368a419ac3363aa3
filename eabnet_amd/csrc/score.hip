// Evaluation scores per utterance of a padded batch, on the device (reference test.py:126-153 cal_single_metrics ->
// metrics.py:14-39 energy_ratios, metrics.py:71-75 si_sdr; train_distributed.py:98-156 evaluate -> com_mag_mse_loss per file).
//
// eab_energy_ratios_f32: with n = y - s (every signal zero from its own length up to the longest of the three) the six sums
//     A = s^.s^   S = s.s   N = n.n   P = s^.s   Q = s^.n   R = s.n          (fp64 products of the fp32 samples, fp64 sums)
// give, with a_s = P/S and a_n = Q/N,
//     |s_target|^2        = a_s^2 S                      |e_noise|^2 = a_n^2 N
//     |e_art|^2           = A + a_s^2 S + a_n^2 N - 2 a_s P - 2 a_n Q + 2 a_s a_n R
//     |e_noise + e_art|^2 = A - P^2/S                    (s^ minus its projection on s)
//     si_sdr(s, y)        = 10 log10( ((S+R)^2/S) / (N - R^2/S) )            (y = s + n)
// from ONE read of each signal.  The closed forms lose digits only where |e_art|^2 is ~1e-10 of A (SAR ~ 100 dB).
//
// eab_com_mag_mse_loss_lens_f32: the masked loss of loss.hip for every utterance alone; its valid bins are the first
// frames[b]*F floats of each of its two planes, i.e. two contiguous rows per spectrum.
//
// Determinism (both): the sample (bin) index is cut into SPANS of EAB_SPAN = 4096 (rows.h), workgroup (span, b) owns span `span` of
// utterance b whatever B, the row length, the row's alignment and the neighbours are.  Inside a span lane `tid` owns the indices
// j*1024 + 4*tid + {0..3}, j = 0..3, and adds them in that order; a row whose address is 16-byte aligned loads its four as one
// dwordx4, any other row (and the quad that straddles the row's length) loads them one by one AT THE SAME indices, so the bits do
// not depend on the load path.  Lanes are added by a fixed shuffle tree, the four waves in wave order through LDS, the spans in
// index order by the final kernel.  No atomics.  Samples at or past a signal's length are never read.
// Bound: launch latency and HBM (3 * L * 4 bytes per utterance; 4 * frames * F * 4 bytes for the loss).
#include "rows.h"

typedef EabRows<3> ScoreRows;       // estimate, clean, noisy

__global__ __launch_bounds__(EAB_SPAN_THREADS) void energy_partial_kernel(const ScoreRows rows, const int32_t* __restrict__ lens,
                                                                       int spans, double* __restrict__ partial) {
    const int b = blockIdx.y, span = blockIdx.x;
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1), ly = eab_len(lens, rows, b, 2);
    const int longest = max(le, max(ls, ly));
    if ((long long)span * EAB_SPAN >= longest) return;          // (workgroup-uniform) the final kernel does not read this row
    const float* e = rows.p[0] + (long long)b * rows.stride[0];
    const float* s = rows.p[1] + (long long)b * rows.stride[1];
    const float* y = rows.p[2] + (long long)b * rows.stride[2];
    const bool ae = eab_aligned16(e), as = eab_aligned16(s), ay = eab_aligned16(y);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < EAB_SPAN / (4 * EAB_SPAN_THREADS); ++j) {
        const int i = eab_span_quad(span, j, (int)threadIdx.x);
        if (i < longest) {
            float ve[4], vs[4], vy[4];
            eab_load4(e, ae, i, le, ve);
            eab_load4(s, as, i, ls, vs);
            eab_load4(y, ay, i, ly, vy);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double de = (double)ve[k], ds = (double)vs[k], dn = (double)vy[k] - (double)vs[k];
                acc[0] += de * de;
                acc[1] += ds * ds;
                acc[2] += dn * dn;
                acc[3] += de * ds;
                acc[4] += de * dn;
                acc[5] += ds * dn;
            }
        }
    }
    eab_span_reduce<6>(acc, partial + ((long long)b * spans + span) * 6);
}

__global__ void energy_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ lens, const ScoreRows rows,
                                    int B, int spans, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1), ly = eab_len(lens, rows, b, 2);
    const int longest = max(le, max(ls, ly));
    const int used = (int)(((long long)longest + EAB_SPAN - 1) / EAB_SPAN);
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < used; ++k)
        for (int q = 0; q < 6; ++q) a[q] += partial[((long long)b * spans + k) * 6 + q];
    const double A = a[0], S = a[1], N = a[2], P = a[3], Q = a[4], R = a[5];
    const double as = P / S, an = Q / N;                          // 0/0 = NaN for a silent clean or noise row, as in numpy
    const double target = as * as * S, noise = an * an * N;
    const double art = A + target + noise - 2.0 * as * P - 2.0 * an * Q + 2.0 * as * an * R;
    const double resid = A - as * P + 0.0 * an;                   // (the reference's e_noise + e_art is NaN with a_n)
    const double am = (S + R) / S;
    double* o = out + (long long)b * 8;
    o[0] = 10.0 * log10(target / resid);
    o[1] = 10.0 * log10(target / noise);
    o[2] = 10.0 * log10(target / art);
    o[3] = 10.0 * log10((am * am * S) / (N - R * R / S));
    o[4] = target;
    o[5] = noise;
    o[6] = art;
    o[7] = resid;
}

extern "C" int eab_energy_ratios_f32(const float* est, long long est_stride, int est_cap, const float* clean,
                                     long long clean_stride, int clean_cap, const float* noisy, long long noisy_stride,
                                     int noisy_cap, const int32_t* lens, int B, double* partial, int partial_spans, double* out,
                                     eab_stream_t stream) {
    const ScoreRows rows = {{est, clean, noisy}, {est_stride, clean_stride, noisy_stride}, {est_cap, clean_cap, noisy_cap}};
    EAB_CHECK_ARG(lens && partial && out && eab_rows_ok(rows, B));
    const int spans = eab_rows_spans(rows);
    EAB_CHECK_ARG(partial_spans >= spans);
    hipLaunchKernelGGL(energy_partial_kernel, dim3((unsigned)spans, (unsigned)B), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), rows,
                       lens, partial_spans, partial);
    hipLaunchKernelGGL(energy_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, eab_stream(stream), partial, lens, rows, B,
                       partial_spans, out);
    EAB_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// per-utterance loss: esti [B][2][T_esti][F], label [B][2][T_label][F]; the valid bins of utterance b are i < frames[b]*F of a plane
__global__ __launch_bounds__(EAB_SPAN_THREADS) void loss_lens_partial_kernel(const float* __restrict__ esti, const float* __restrict__ label,
                                                                          const int32_t* __restrict__ frames, int T_esti, int T_label,
                                                                          int T_max, int F, int spans, double* __restrict__ partial) {
    const int b = blockIdx.y, span = blockIdx.x;
    const int len = eab_clamp(frames[b], T_max) * F;
    if ((long long)span * EAB_SPAN >= len) return;
    const long long pe = (long long)T_esti * F, pl = (long long)T_label * F;
    const float* er = esti + (long long)b * 2 * pe;
    const float* lr = label + (long long)b * 2 * pl;
    const float* ei = er + pe;
    const float* li = lr + pl;
    const bool a0 = eab_aligned16(er), a1 = eab_aligned16(ei), a2 = eab_aligned16(lr), a3 = eab_aligned16(li);
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < EAB_SPAN / (4 * EAB_SPAN_THREADS); ++j) {
        const int i = eab_span_quad(span, j, (int)threadIdx.x);
        if (i < len) {
            float v0[4], v1[4], v2[4], v3[4];
            eab_load4(er, a0, i, len, v0);
            eab_load4(ei, a1, i, len, v1);
            eab_load4(lr, a2, i, len, v2);
            eab_load4(li, a3, i, len, v3);
#pragma unroll
            for (int k = 0; k < 4; ++k) {                         // (bins at and past len are zeros: they add +0.0)
                const float me = sqrtf(v0[k] * v0[k] + v1[k] * v1[k]), ml = sqrtf(v2[k] * v2[k] + v3[k] * v3[k]);
                const double dm = (double)(me - ml), dr = (double)(v0[k] - v2[k]), di = (double)(v1[k] - v3[k]);
                acc[0] += dm * dm;
                acc[1] += dr * dr + di * di;
            }
        }
    }
    eab_span_reduce<2>(acc, partial + ((long long)b * spans + span) * 2);
}

__global__ void loss_lens_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ frames, int B, int T_max, int F,
                                       int spans, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int len = eab_clamp(frames[b], T_max) * F;
    const int used = (len + EAB_SPAN - 1) / EAB_SPAN;
    double a = 0.0, c = 0.0;
    for (int k = 0; k < used; ++k) {
        a += partial[((long long)b * spans + k) * 2];
        c += partial[((long long)b * spans + k) * 2 + 1];
    }
    out[b] = 0.5 * (a + 0.5 * c) / (double)len;                   // no frames: 0/0 = NaN, as the reference's empty mask
}

extern "C" int eab_com_mag_mse_loss_lens_f32(const float* esti, const float* label, const int32_t* frames, int B, int T_esti,
                                             int T_label, int F, double* partial, int partial_spans, double* loss,
                                             eab_stream_t stream) {
    EAB_CHECK_ARG(esti && label && frames && partial && loss && B > 0 && B <= 65535 && T_esti > 0 && T_label > 0 && F > 0);
    const int T_max = T_esti < T_label ? T_esti : T_label;
    EAB_CHECK_ARG((long long)T_max * F <= EAB_ROWS_MAX_LEN);
    const int spans = eab_spans(T_max * F);
    EAB_CHECK_ARG(partial_spans >= spans);
    hipLaunchKernelGGL(loss_lens_partial_kernel, dim3((unsigned)spans, (unsigned)B), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), esti,
                       label, frames, T_esti, T_label, T_max, F, partial_spans, partial);
    hipLaunchKernelGGL(loss_lens_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, eab_stream(stream), partial, frames, B,
                       T_max, F, partial_spans, loss);
    EAB_RETURN_LAUNCH_STATUS();
}
