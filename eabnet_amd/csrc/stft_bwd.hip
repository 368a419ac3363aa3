// Adjoint of the STFT front end (eab_stft_compress_f32, stft.hip): dspec, the gradient with respect to the
// compressed spectrogram, -> dwav [B][M][L], the gradient with respect to the waves.
//
// Compression.  The forward stores s = X |X|^-1/2 per bin.  With rho = |s| and g = dL/ds the gradient with respect to X is
//   gX = g / rho - s (s . g) / (2 rho^3)            (s . g the real dot product: the Jacobian of X |X|^-1/2 written in s),
// formed here as (g - n (n . g) / 2) / rho with n = s / rho -- no cancellation (the component along s is halved, the one across
// it kept) and no cube.  At rho = 0 the result is exactly (0, 0), with no division: the true derivative is unbounded there, and a
// silent microphone must give a finite zero gradient.
// Transform.  The plain transpose of the one-sided windowed DFT, theta = 2 pi k n / n_fft:
//   u_t[n] = w[n] sum_{k = 0 .. n_fft/2} (gXr[k] cos theta - gXi[k] sin theta)
// (interior bins not doubled; the imaginary parts at DC and Nyquist do not reach the wave).  That is n_fft/2 times the C2R
// inverse transform of (2 gXr[0], gX[1], .., gX[n_fft/2 - 1], 2 gXr[n_fft/2]), which runs as in istft_body.inc: even/odd split,
// conj(FFT(conj .)) on the forward Stockham passes of fft_lds.h.
// Overlap and reflection.  dpad[p] = sum_t u_t[p - t hop] over the at most R = ceil(n_fft / hop) frames t < T_b = 1 + L_b / hop
// that cover the padded position p, highest frame first; with H = n_fft / 2
//   dwav[j] = dpad[j + H]  (+ dpad[H - j], 1 <= j <= H)  (+ dpad[2 (L_b - 1) - j + H], L_b - 1 - H <= j <= L_b - 2),
// the three terms added in that order; samples j >= L_b are zeros; frames >= T_b of dspec and spec are never read.
//
// One workgroup owns one signal (b, m) and the padded positions [chunk span, (chunk + 1) span), span = (FFT_SIGS - (R - 1)) hop:
// the FFT_SIGS frames from chunk (FFT_SIGS - (R - 1)) - (R - 1) on cover them completely (consecutive workgroups re-invert the
// R - 1 frames they share: no inter-workgroup dependency).  A workgroup whose samples have a mirror image in the reflected
// head or tail of the padded wave inverts those frames too (the first ones, or the last FFT_SIGS of the utterance: at most
// ceil(H / hop) + 1 <= 5 frames cover either margin) and takes the mirrored positions from them.  No atomics, every output is
// stored once, and nothing depends on the grid: the bits are the same alone and in any batch.
// Traffic: 4 F floats read per frame and signal, hop floats written.  Layout (B,T,F,M,2) is read with a stride of M bins per
// lane, so the M workgroups of a frame each touch the same cache lines; measured times: DESIGN.md 4.28.
#include "common.h"
#include "fft_lds.h"

#define SB_THREADS 256
#define SB_MAX_NFFT 512
#define SB_MAXE (FFT_SIGS * SB_MAX_NFFT / SB_THREADS)      // positions per thread: span <= FFT_SIGS * hop, hop <= n_fft

// the forward's clamp of a per-utterance sample count (stft_utt_len, stft.hip)
__device__ __forceinline__ int sb_utt_len(const int* __restrict__ lens, int b, int n_fft, int L) {
    const int n = lens[b];
    return n > L ? L : (n <= n_fft / 2 ? n_fft / 2 + 1 : n);
}

__device__ __forceinline__ float2 sb_decompress_grad(float2 s, float2 g) {
    const float rho = sqrtf(s.x * s.x + s.y * s.y);
    if (!(rho > 0.0f)) return make_float2(0.0f, 0.0f);
    const float nx = s.x / rho, ny = s.y / rho;
    const float h = 0.5f * (nx * g.x + ny * g.y);
    return make_float2((g.x - nx * h) / rho, (g.y - ny * h) / rho);
}

template <bool VARLEN>
__global__ __launch_bounds__(SB_THREADS) void stft_compress_bwd_kernel(
    const float* __restrict__ dspec, const float* __restrict__ spec, const float* __restrict__ window,
    const float* __restrict__ twiddle, float* __restrict__ dwav, int M, int L, int T, int n_fft, int hop, int chunks, int layout,
    FftPlan plan, const int* __restrict__ lens) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int NH = n_fft / 2, F = NH + 1;
    const int R = (n_fft + hop - 1) / hop;
    float2* tw = reinterpret_cast<float2*>(smem);                 // [n_fft] exp(-2 pi i j / n_fft)
    float2* buf0 = tw + n_fft;                                    // [FFT_SIGS][NH]
    float2* buf1 = buf0 + FFT_SIGS * NH;
    float* win = reinterpret_cast<float*>(buf1 + FFT_SIGS * NH);  // [n_fft]
    float* xs = win + n_fft;                                      // [FFT_SIGS][2][F] gX of the staged frames
    const int tid = threadIdx.x;
    const int sig = blockIdx.x / chunks, chunk = blockIdx.x - sig * chunks;
    const int b = sig / M, m = sig - b * M;
    const int Lb = VARLEN ? sb_utt_len(lens, b, n_fft, L) : L;    // samples of this utterance
    const int Tb = 1 + Lb / hop;                                  // ... and its frames (<= T)
    const int per = FFT_SIGS - (R - 1), span = per * hop;
    const int j_lo = chunk * span - NH, j_hi = j_lo + span;       // this workgroup's samples [j_lo, j_hi) (clipped to [0, L))
    float* out = dwav + ((size_t)b * M + m) * L;
    if (j_lo >= Lb) {                                             // workgroup-uniform, before any barrier: padding only
        for (int j = j_lo + tid; j < j_hi && j < L; j += SB_THREADS) out[j] = 0.0f;
        return;
    }
    for (int k = tid; k < n_fft; k += SB_THREADS) {
        const float2 cs = reinterpret_cast<const float2*>(twiddle)[k];     // (cos, sin)(+theta)
        tw[k] = make_float2(cs.x, -cs.y);
        win[k] = window[k];
    }
    float tot[SB_MAXE];
#pragma unroll
    for (int i = 0; i < SB_MAXE; ++i) tot[i] = 0.0f;
    for (int term = 0; term < 3; ++term) {
        // term 0: the sample's own position; 1: its mirror image in the reflected head; 2: in the reflected tail
        int ts;                                                   // first of the FFT_SIGS frames inverted for this term
        if (term == 0) {
            ts = chunk * per - (R - 1);
        } else if (term == 1) {
            if (!(j_lo <= NH && j_hi > 1)) continue;              // (workgroup-uniform)
            ts = 0;
        } else {
            if (!(j_lo <= Lb - 2 && j_hi > Lb - 1 - NH)) continue;
            ts = Tb > FFT_SIGS ? Tb - FFT_SIGS : 0;
        }
        __syncthreads();                                          // (tw, win staged; the previous term's reads of xs are over)
        for (int e = tid; e < FFT_SIGS * F; e += SB_THREADS) {
            const int c = e / F, f = e - c * F;
            const int t = ts + c;
            float2 gx = make_float2(0.0f, 0.0f);
            if (t >= 0 && t < Tb) {
                float2 s, g;
                if (layout == EAB_STFT_LAYOUT_BTFM2) {
                    const size_t o = (((size_t)b * T + t) * F + f) * M + m;
                    s = reinterpret_cast<const float2*>(spec)[o];
                    g = reinterpret_cast<const float2*>(dspec)[o];
                } else {                                          // (B,2,T,F), M == 1
                    const size_t o0 = (((size_t)b * 2 + 0) * T + t) * F + f, o1 = (((size_t)b * 2 + 1) * T + t) * F + f;
                    s = make_float2(spec[o0], spec[o1]);
                    g = make_float2(dspec[o0], dspec[o1]);
                }
                gx = sb_decompress_grad(s, g);
            }
            xs[c * 2 * F + f] = gx.x;
            xs[c * 2 * F + F + f] = gx.y;
        }
        __syncthreads();
        // conj(Z[k]),  Z = E + iO  of the spectrum (2 gXr[0], gX[1], .., 2 gXr[NH])
        for (int e = tid; e < FFT_SIGS * NH; e += SB_THREADS) {
            const int c = e / NH, k = e - c * NH;
            const float* re = xs + c * 2 * F;
            const float* im = re + F;
            float2 xk = make_float2(re[k], im[k]);
            float2 xm = make_float2(re[NH - k], im[NH - k]);
            if (k == 0) {                                         // DC and Nyquist: real, and counted once
                xk = make_float2(2.0f * xk.x, 0.0f);
                xm = make_float2(2.0f * xm.x, 0.0f);
            }
            const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
            const float2 D = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
            const float2 O = cmul(D, make_float2(tw[k].x, -tw[k].y)); // * e^{+i theta_k}
            buf0[e] = make_float2(E.x - O.y, -(E.y + O.x));
        }
        __syncthreads();
        const float2* y = fft_run(buf0, buf1, tw, NH, n_fft, plan, tid, SB_THREADS);
        // sample idx of frame c: float idx of y_c, the odd ones negated (x[2j] = Re y[j], x[2j+1] = -Im y[j])
        const float* yf = reinterpret_cast<const float*>(y);
#pragma unroll
        for (int i = 0; i < SB_MAXE; ++i) {
            const int e = tid + i * SB_THREADS;
            const int j = j_lo + e;
            if (e >= span || j < 0 || j >= Lb) continue;
            int q;                                                // padded position this term reads for sample j
            if (term == 0) {
                q = j + NH;
            } else if (term == 1) {
                if (j < 1 || j > NH) continue;
                q = NH - j;
            } else {
                if (j < Lb - 1 - NH || j > Lb - 2) continue;
                q = 2 * (Lb - 1) - j + NH;
            }
            const int th = q / hop;
            float acc = 0.0f;
            for (int r = 0; r < R; ++r) {
                const int t = th - r;
                const int idx = q - t * hop;
                if (t < 0 || idx >= n_fft) break;
                const int c = t - ts;
                if (t >= Tb || c < 0 || c >= FFT_SIGS) continue;  // (c: always inside by the choice of ts)
                float a = yf[c * n_fft + idx];
                if (idx & 1) a = -a;
                acc = fmaf(win[idx], a, acc);
            }
            tot[i] = term == 0 ? acc : tot[i] + acc;
        }
    }
#pragma unroll
    for (int i = 0; i < SB_MAXE; ++i) {
        const int e = tid + i * SB_THREADS;
        const int j = j_lo + e;
        if (e >= span || j < 0 || j >= L) continue;
        out[j] = j < Lb ? tot[i] : 0.0f;
    }
}

extern "C" int eab_stft_compress_bwd_f32(const float* dspec, const float* spec, const float* window, const float* twiddle,
                                         float* dwav, const int32_t* lens, int B, int M, int L, int n_fft, int hop, int layout,
                                         eab_stream_t stream) {
    EAB_CHECK_ARG(dspec && spec && window && twiddle && dwav);
    EAB_CHECK_ARG(B > 0 && M > 0 && hop > 0);
    EAB_CHECK_ARG(n_fft >= 4 && n_fft <= SB_MAX_NFFT && (n_fft % 2) == 0);
    EAB_CHECK_ARG(L > n_fft / 2);                           // reflect padding needs pad < L (as the forward)
    EAB_CHECK_ARG(layout == EAB_STFT_LAYOUT_BTFM2 || (layout == EAB_STFT_LAYOUT_B2TF && M == 1));
    // at most FFT_SIGS frames may cover a sample (as eab_istft_f32), and the half-length transform must factor
    if (hop > n_fft || (n_fft + hop - 1) / hop > FFT_SIGS) return EAB_EUNSUPPORTED;
    FftPlan plan;
    if (!fft_plan(n_fft / 2, &plan)) return EAB_EUNSUPPORTED;
    const int T = 1 + L / hop;
    const int R = (n_fft + hop - 1) / hop, per = FFT_SIGS - (R - 1);
    const long long span = (long long)per * hop;
    const long long chunks = ((long long)n_fft / 2 + L + span - 1) / span;   // padded positions [0, n_fft/2 + L)
    EAB_CHECK_ARG((long long)B * M * chunks < (1ll << 31) && 2ll * L + 2ll * n_fft + span < (1ll << 31));   // 32-bit positions
    const size_t sh = (size_t)(2 * n_fft + 2 * FFT_SIGS * n_fft + n_fft + FFT_SIGS * 2 * (n_fft / 2 + 1)) * sizeof(float);
    if (lens)
        hipLaunchKernelGGL(stft_compress_bwd_kernel<true>, dim3((unsigned)(B * M * chunks)), dim3(SB_THREADS), sh, eab_stream(stream),
                           dspec, spec, window, twiddle, dwav, M, L, T, n_fft, hop, (int)chunks, layout, plan, lens);
    else
        hipLaunchKernelGGL(stft_compress_bwd_kernel<false>, dim3((unsigned)(B * M * chunks)), dim3(SB_THREADS), sh, eab_stream(stream),
                           dspec, spec, window, twiddle, dwav, M, L, T, n_fft, hop, (int)chunks, layout, plan, lens);
    EAB_RETURN_LAUNCH_STATUS();
}
