// Gradient with respect to the network input X [B][T][F][M][2] of the training programs.  X has two readers:
// the first convolution of the encoder and the filter-and-sum Y = sum_m W_m X_m (EaBNet.py:114-117).  The convolution's data
// gradient arrives as a 64-column tile per bin (dconv, memory channel m*2+ri, written by eab_conv_f32 with the transposed
// weights padded with zero rows); the filter-and-sum's adjoint with respect to X is filter_sum_bwd_kernel (train.hip) with its
// operands exchanged: dX_m = conj(W_m) dY.  One launch forms both and stores every element of din once:
//   din[bin][m].re = dr w.re + di w.im + dconv[bin][2m]
//   din[bin][m].im = di w.re - dr w.im + dconv[bin][2m+1]        (dr, di) = dout[b][0|1][t][f],  w = bw[bin][2m .. 2m+1]
// Four lanes per bin, lane p takes microphones p, p+4, ..: a wave reads 16 consecutive rows of both tiles and writes one
// contiguous block of din.  Traffic: two `ld`-float rows read and 2M floats written per bin; measured times: DESIGN.md 4.28.
// lens != NULL: frames t >= lens[b] are stored as exact zeros by selection, whatever the operands hold there (the masked
// convolutions leave the rows of padding frames of dconv unwritten, and dout may carry anything behind a length).
#include "common.h"

#define IG_THREADS 256

__global__ __launch_bounds__(IG_THREADS) void input_grad_kernel(const float* __restrict__ dout, const float* __restrict__ bw,
                                                                const float* __restrict__ dconv, float* __restrict__ din,
                                                                unsigned TF, unsigned F, int M, int ld, unsigned bins,
                                                                const int* __restrict__ lens) {
    const unsigned p = threadIdx.x & 3;
    for (unsigned bin = blockIdx.x * (IG_THREADS / 4) + (threadIdx.x >> 2); bin < bins; bin += gridDim.x * (IG_THREADS / 4)) {
        const unsigned b = bin / TF, pos = bin - b * TF;
        const bool pad = lens && (long long)pos >= (long long)lens[b] * F;
        const float dr = dout[(size_t)(2 * b) * TF + pos], di = dout[(size_t)(2 * b + 1) * TF + pos];
        const float2* wp = reinterpret_cast<const float2*>(bw + (size_t)bin * ld);
        const float2* cp = reinterpret_cast<const float2*>(dconv + (size_t)bin * ld);
        float2* op = reinterpret_cast<float2*>(din) + (size_t)bin * M;
        for (int m = p; m < M; m += 4) {
            const float2 w = wp[m], c = cp[m];
            const float re = dr * w.x + di * w.y + c.x, im = di * w.x - dr * w.y + c.y;
            op[m] = make_float2(pad ? 0.0f : re, pad ? 0.0f : im);
        }
    }
}

extern "C" int eab_input_grad_f32(const float* dout, const float* bw, const float* dconv, float* din, int B, int T, int F, int M,
                                  int ld, const int32_t* lens, eab_stream_t stream) {
    EAB_CHECK_ARG(dout && bw && dconv && din && B > 0 && T > 0 && F > 0 && M > 0 && ld >= 2 * M && (ld % 2) == 0);
    const long long bins = (long long)B * T * F;
    EAB_CHECK_ARG(bins < (1ll << 30));                     // 32-bit bin arithmetic in the kernel
    const long long tiles = (bins + IG_THREADS / 4 - 1) / (IG_THREADS / 4);
    const unsigned grid = (unsigned)(tiles < 256 * 8 ? tiles : 256 * 8);
    hipLaunchKernelGGL(input_grad_kernel, dim3(grid), dim3(IG_THREADS), 0, eab_stream(stream), dout, bw, dconv, din,
                       (unsigned)((long long)T * F), (unsigned)F, M, ld, (unsigned)bins, lens);
    EAB_RETURN_LAUNCH_STATUS();
}
