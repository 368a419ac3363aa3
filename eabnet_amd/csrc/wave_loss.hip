// Waveform training loss: negative SI-SDR per utterance of a padded batch, value and gradient (the quantity score.hip reports
// per file -- metrics.si_sdr of the reference -- as a loss the optimiser can follow).
//
// With e the estimate, s the clean wave (each zero from its own length up to the longer of the two, never read there) and
// k = 10 / ln 10:
//     es = <e,s>   ss = <s,s>   ee = <e,e>   alpha = es / ss   tgt = es^2 / ss   res = ee - tgt
//     loss_b = -k [ ln(tgt + eps) - ln(res + eps) ]
//     d loss_b / d e_i = a_b e_i + c_b s_i,    a_b = 2 k / (res + eps),   c_b = -2 k alpha [ 1 / (tgt + eps) + 1 / (res + eps) ]
// eab_si_sdr_loss_f32: the three sums by score.hip's scheme, with the helpers of rows.h (fp64 products of the fp32 samples, fixed
// spans of EAB_SPAN = 4096 samples, eab_span_reduce: lanes by a fixed shuffle tree, waves in order; spans in index order: the row of
// an utterance has the same bits alone and in any batch, whatever the strides and alignments), then ONE workgroup turns them into
// (loss_b, a_b, c_b) and the batch's sum and mean.
// eab_si_sdr_loss_bwd_f32: grad[b][i] = g_b (a_b e_i + c_b s_i) for i < Le_b, exactly 0 from there to the row's end; g_b is read
// from device memory (autograd's grad_output: nothing goes through the host).  Three launches for a loss and its gradient, no
// atomics.  Bound: launch latency and HBM (2 reads of each signal, one write of the gradient).
#include "rows.h"

typedef EabRows<2> WaveRows;        // estimate, clean

__global__ __launch_bounds__(EAB_SPAN_THREADS) void si_sdr_partial_kernel(const WaveRows rows, const int32_t* __restrict__ lens, int spans,
                                                                      double* __restrict__ partial) {
    const int b = blockIdx.y, span = blockIdx.x;
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1);
    const int longest = max(le, ls);
    if ((long long)span * EAB_SPAN >= longest) return;           // (workgroup-uniform) the final kernel does not read this row
    const float* e = rows.p[0] + (long long)b * rows.stride[0];
    const float* s = rows.p[1] + (long long)b * rows.stride[1];
    const bool ae = eab_aligned16(e), as = eab_aligned16(s);
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < EAB_SPAN / (4 * EAB_SPAN_THREADS); ++j) {
        const int i = eab_span_quad(span, j, (int)threadIdx.x);
        if (i < longest) {
            float ve[4], vs[4];
            eab_load4(e, ae, i, le, ve);
            eab_load4(s, as, i, ls, vs);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double de = (double)ve[k], ds = (double)vs[k];
                acc[0] += de * de;
                acc[1] += ds * ds;
                acc[2] += de * ds;
            }
        }
    }
    eab_span_reduce<3>(acc, partial + ((long long)b * spans + span) * 3);
}

// one workgroup: lane `tid` takes the utterances tid, tid + 256, ...; the batch's sum adds each lane's values in that order and
// the 256 lanes in lane order
__global__ __launch_bounds__(EAB_SPAN_THREADS) void si_sdr_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ lens,
                                                                    const WaveRows rows, int B, int spans, double eps,
                                                                    double* __restrict__ out, float* __restrict__ loss,
                                                                    float* __restrict__ total) {
    __shared__ double lane_sum[EAB_SPAN_THREADS];
    const double K = 4.342944819032518;                           // 10 / ln 10
    double mine = 0.0;
    for (int b = threadIdx.x; b < B; b += EAB_SPAN_THREADS) {
        const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1);
        const int longest = max(le, ls);
        const int used = (int)(((long long)longest + EAB_SPAN - 1) / EAB_SPAN);
        double a[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < used; ++k)
            for (int q = 0; q < 3; ++q) a[q] += partial[((long long)b * spans + k) * 3 + q];
        const double ee = a[0], ss = a[1], es = a[2];
        const double alpha = es / ss;                             // 0/0 = NaN for a silent clean row, as in energy_ratios
        const double tgt = es * es / ss, res = ee - tgt;
        const double v = -K * (log(tgt + eps) - log(res + eps));
        out[3 * b] = v;
        out[3 * b + 1] = 2.0 * K / (res + eps);
        out[3 * b + 2] = -2.0 * K * alpha * (1.0 / (tgt + eps) + 1.0 / (res + eps));
        loss[b] = (float)v;
        mine += v;
    }
    lane_sum[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int l = 0; l < EAB_SPAN_THREADS; ++l) s += lane_sum[l];
        total[0] = (float)s;
        total[1] = (float)(s / (double)B);
    }
}

// grad row b: cap[0] floats, `gstride` floats between two rows; workgroup (span, b) writes span `span` of it
__global__ __launch_bounds__(EAB_SPAN_THREADS) void si_sdr_bwd_kernel(const WaveRows rows, const int32_t* __restrict__ lens,
                                                                  const double* __restrict__ coef, const float* __restrict__ gout,
                                                                  int gout_stride, double scale, float* __restrict__ grad,
                                                                  long long gstride) {
    const int b = blockIdx.y, span = blockIdx.x;
    const int cap = rows.cap[0];
    const int le = eab_len(lens, rows, b, 0), ls = eab_len(lens, rows, b, 1);
    const float* e = rows.p[0] + (long long)b * rows.stride[0];
    const float* s = rows.p[1] + (long long)b * rows.stride[1];
    float* g = grad + (long long)b * gstride;
    const bool ae = eab_aligned16(e), as = eab_aligned16(s), ag = eab_aligned16(g);
    const double w = (double)gout[(long long)b * gout_stride] * scale;
    const double ca = w * coef[3 * b + 1], cc = w * coef[3 * b + 2];
#pragma unroll
    for (int j = 0; j < EAB_SPAN / (4 * EAB_SPAN_THREADS); ++j) {
        const int i = eab_span_quad(span, j, (int)threadIdx.x);
        if (i >= cap) continue;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < le) {
            float ve[4], vs[4];
            eab_load4(e, ae, i, le, ve);
            eab_load4(s, as, i, ls, vs);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < le) v[k] = (float)(ca * (double)ve[k] + cc * (double)vs[k]);
        }
        if (ag && i + 4 <= cap) {
            *reinterpret_cast<f32x4*>(g + i) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < cap) g[i + k] = v[k];
        }
    }
}

extern "C" int eab_si_sdr_loss_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride,
                                   int clean_cap, const int32_t* lens, int B, double eps, double* partial, int partial_spans,
                                   double* out, float* loss, float* total, eab_stream_t stream) {
    const WaveRows rows = {{est, clean}, {est_stride, clean_stride}, {est_cap, clean_cap}};
    EAB_CHECK_ARG(lens && partial && out && loss && total && eab_rows_ok(rows, B));
    EAB_CHECK_ARG(eps >= 0.0 && eps < 1e300);                     // (refuses NaN too)
    const int spans = eab_rows_spans(rows);
    EAB_CHECK_ARG(partial_spans >= spans);
    hipLaunchKernelGGL(si_sdr_partial_kernel, dim3((unsigned)spans, (unsigned)B), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), rows, lens,
                       partial_spans, partial);
    hipLaunchKernelGGL(si_sdr_final_kernel, dim3(1), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), partial, lens, rows, B, partial_spans,
                       eps, out, loss, total);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_si_sdr_loss_bwd_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride,
                                       int clean_cap, const int32_t* lens, int B, const double* coef, const float* grad_out,
                                       int grad_out_stride, double scale, float* grad, long long grad_stride, eab_stream_t stream) {
    const WaveRows rows = {{est, clean}, {est_stride, clean_stride}, {est_cap, clean_cap}};
    EAB_CHECK_ARG(lens && coef && grad_out && grad && eab_rows_ok(rows, B));
    EAB_CHECK_ARG(grad_out_stride >= 0 && (B == 1 || grad_stride >= est_cap));
    const int spans = eab_spans(est_cap);
    hipLaunchKernelGGL(si_sdr_bwd_kernel, dim3((unsigned)spans, (unsigned)B), dim3(EAB_SPAN_THREADS), 0, eab_stream(stream), rows, lens, coef,
                       grad_out, grad_out_stride, scale, grad, grad_stride);
    EAB_RETURN_LAUNCH_STATUS();
}
