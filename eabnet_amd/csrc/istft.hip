// ISTFT back end: (B,2,T,F) estimate -> (B, hop*(T-1)) wave.
// Reference: enhance.py:59-62 / test.py:189-191 / train_distributed.py:128-130
//   esti.permute(0,3,2,1) -> view_as_complex -> torch.istft(n_fft=320, hop=160, win=320, hann)
// i.e. (torch.istft defaults: center, onesided, not normalized, length=None)
//   frame_t = irfft(X[:, t]) * w;   y = overlap_add(frame) / overlap_add(w^2);   trim n_fft/2 per side.
// Any hop with R = ceil(n_fft/hop) <= 8 frames per sample (the reference: 320/160, R = 2; the hop need not divide n_fft): the
// padded position p is covered by the frames t = floor(p/hop), floor(p/hop)-1, ... while t hop + n_fft > p, so there is no
// scatter and no envelope buffer --
//   y[p] = sum_t w[p - t hop] x_t[p - t hop] / sum_t w[p - t hop]^2,   frames outside [0, T) skipped.
//
// One workgroup inverts FFT_SIGS consecutive frames t0 .. t0+7 of one utterance in LDS and emits the positions whose
// covering frames it holds completely: [(t0-1) hop + n_fft, (t0+8) hop); consecutive workgroups start per = FFT_SIGS-(R-1)
// frames apart, so their ranges tile the wave (the next workgroup re-inverts the R-1 shared frames: no inter-workgroup
// dependency).  Real inverse FFT by the even/odd split: with
// E = (X[k] + conj X[N/2-k])/2 and O = (X[k] - conj X[N/2-k])/2 * e^{+2 pi i k/N},
// z = IDFT_{N/2}(E + iO) holds x[2n] + i x[2n+1]; the inverse transform runs as
// conj(FFT(conj .)) on the forward Stockham passes of fft_lds.h.  As in a C2R transform the
// imaginary parts of the DC and Nyquist bins are ignored.
// Bound: HBM (reads 2*F*4 B, writes hop*4 B per frame); at the reference sizes it is launch/latency
// sized (13 MB per 16-utterance batch).
#include "common.h"
#include "fft_lds.h"

#define ISTFT_THREADS 256
#define ISTFT_MAX_NFFT 512

// VARLEN (eab_istft_lens_f32): `lens` holds B frame counts; T is the capacity (row strides of spec and wav).  Utterance b is
// inverted as by a launch with T = lens[b] -- frames t >= lens[b] are neither read nor added nor counted in the envelope --
// and its samples from hop (lens[b] - 1) on are written as zeros.  The count is clamped to [1, T].
template <bool VARLEN>
__global__ __launch_bounds__(ISTFT_THREADS) void istft_kernel(const float* __restrict__ spec, const float* __restrict__ window,
                                                              const float* __restrict__ twiddle, float* __restrict__ wav,
                                                              int T, int n_fft, int hop, int chunks, FftPlan plan,
                                                              const int* __restrict__ lens) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int NH = n_fft / 2, F = NH + 1;
    const int R = (n_fft + hop - 1) / hop;                        // most frames that cover one output sample (2 for the reference)
    float2* tw = reinterpret_cast<float2*>(smem);                 // [n_fft] exp(-2 pi i j / n_fft)
    float2* buf0 = tw + n_fft;                                    // [FFT_SIGS][NH]
    float2* buf1 = buf0 + FFT_SIGS * NH;
    float* win = reinterpret_cast<float*>(buf1 + FFT_SIGS * NH);  // [n_fft]
    float* xs = win + n_fft;                                      // [FFT_SIGS][2][F] staged spectrum rows
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int t0 = chunk * (FFT_SIGS - (R - 1));                  // consecutive workgroups share R-1 frames
    const int Tb = VARLEN ? (lens[b] > T ? T : (lens[b] < 1 ? 1 : lens[b])) : T;   // frames of this utterance
    if (VARLEN && t0 >= Tb) {
        // every frame of this workgroup lies past the utterance (workgroup-uniform, before any barrier): its positions
        // start at t0 hop + n_fft - hop - n_fft/2 >= hop (Tb - 1), all of them padding -- zeros, no transform
        const int p0 = t0 * hop + n_fft - hop, p1 = p0 + (FFT_SIGS - (R - 1)) * hop, cap_len = hop * (T - 1);
        for (int p = p0 + tid; p < p1; p += ISTFT_THREADS) {
            const int j = p - NH;
            if (j >= 0 && j < cap_len) wav[(size_t)b * cap_len + j] = 0.0f;
        }
        return;
    }

    for (int k = tid; k < n_fft; k += ISTFT_THREADS) {
        const float2 cs = reinterpret_cast<const float2*>(twiddle)[k];     // (cos, sin)(+theta)
        tw[k] = make_float2(cs.x, -cs.y);
        win[k] = window[k];
    }
    // stage re/im rows of the frames (coalesced; the split below reads them mirrored)
    for (int e = tid; e < FFT_SIGS * 2 * F; e += ISTFT_THREADS) {
        const int c = e / (2 * F), r = e - c * 2 * F;
        const int ri = r / F, f = r - ri * F;
        const int t = t0 + c;
        xs[e] = t < Tb ? spec[(((size_t)b * 2 + ri) * T + t) * F + f] : 0.0f;
    }
    __syncthreads();
    // conj(Z[k]),  Z = E + iO
    for (int e = tid; e < FFT_SIGS * NH; e += ISTFT_THREADS) {
        const int c = e / NH, k = e - c * NH;
        const float* re = xs + c * 2 * F;
        const float* im = re + F;
        float2 xk = make_float2(re[k], im[k]);
        float2 xm = make_float2(re[NH - k], im[NH - k]);
        if (k == 0) xk.y = xm.y = 0.0f;                            // C2R: DC and Nyquist are real
        const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 D = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
        const float2 O = cmul(D, make_float2(tw[k].x, -tw[k].y)); // * e^{+i theta_k}
        buf0[e] = make_float2(E.x - O.y, -(E.y + O.x));
    }
    __syncthreads();
    const float2* y = fft_run(buf0, buf1, tw, NH, n_fft, plan, tid, ISTFT_THREADS);
    // x_c[2j] = Re y_c[j] / NH,  x_c[2j+1] = -Im y_c[j] / NH
    const float inv = 1.0f / (float)NH;
    const float* yf = reinterpret_cast<const float*>(y);
    // Overlap-add over the frames that cover a sample, divided by the squared-window envelope of the frames that exist
    // (torch.istft), then the centre trim.  This workgroup holds frames t0 .. t0+7 and emits the padded positions
    // [p_lo, p_hi) whose covering frames it holds completely (the first workgroup: from 0); highest frame first.
    const int per = FFT_SIGS - (R - 1);
    const int p_lo = chunk == 0 ? 0 : t0 * hop + n_fft - hop;
    const int p_hi = (t0 + per) * hop + n_fft - hop;
    const int out_len = hop * (T - 1), len_b = hop * (Tb - 1);     // row stride of wav; samples of this utterance
    for (int e = tid; e < p_hi - p_lo; e += ISTFT_THREADS) {
        const int p = p_lo + e;
        const int j = p - NH;                                      // output sample (centre trim of n_fft/2)
        if (j < 0 || j >= out_len) continue;
        if (VARLEN && j >= len_b) {                                // past the utterance's trim: zero
            wav[(size_t)b * out_len + j] = 0.0f;
            continue;
        }
        const int th = p / hop;
        float acc = 0.0f, env = 0.0f;
        for (int r = 0; r < R; ++r) {
            const int t = th - r;
            const int idx = p - t * hop;                           // sample of frame t; float index = idx (re/im interleave)
            if (t < 0 || idx >= n_fft) break;
            if (t >= Tb) continue;
            float a = yf[(t - t0) * n_fft + idx];
            if (idx & 1) a = -a;
            const float w = win[idx];
            acc = fmaf(w, a * inv, acc);
            env = fmaf(w, w, env);
        }
        wav[(size_t)b * out_len + j] = acc / env;
    }
}

// lens == NULL: every utterance is T frames long (eab_istft_f32); else per-utterance frame counts in a batch of capacity T
static int istft_launch(const float* spec, const float* window, const float* twiddle, float* wav, const int* lens, int B, int T,
                        int n_fft, int hop, eab_stream_t stream) {
    EAB_CHECK_ARG(spec && window && twiddle && wav);
    EAB_CHECK_ARG(B > 0 && T >= 2 && hop > 0);
    EAB_CHECK_ARG(n_fft >= 4 && n_fft <= ISTFT_MAX_NFFT && (n_fft % 2) == 0);
    // at most FFT_SIGS frames may cover a sample (R = ceil(n_fft / hop) <= 8: 87.5 % overlap); torch.istft wants hop <= win
    if (hop > n_fft || (n_fft + hop - 1) / hop > FFT_SIGS) return EAB_EUNSUPPORTED;
    FftPlan plan;
    if (!fft_plan(n_fft / 2, &plan)) return EAB_EUNSUPPORTED;
    const int R = (n_fft + hop - 1) / hop, per = FFT_SIGS - (R - 1);
    // padded positions [0, n_fft/2 + hop (T-1)) carry the trimmed output; the workgroup of chunk c ends at
    // (c+1) per hop + n_fft - hop
    const long long need = (long long)n_fft / 2 + (long long)hop * (T - 1) - (n_fft - hop);
    const int chunks = need <= 0 ? 1 : (int)((need + (long long)per * hop - 1) / ((long long)per * hop));
    EAB_CHECK_ARG((long long)B * chunks < (1ll << 31));
    const size_t sh = (size_t)(2 * n_fft + 2 * FFT_SIGS * n_fft + n_fft + FFT_SIGS * 2 * (n_fft / 2 + 1)) * sizeof(float);
    if (lens)
        hipLaunchKernelGGL(istft_kernel<true>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), spec, window, twiddle,
                           wav, T, n_fft, hop, chunks, plan, lens);
    else
        hipLaunchKernelGGL(istft_kernel<false>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), spec, window, twiddle,
                           wav, T, n_fft, hop, chunks, plan, lens);
    EAB_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Adjoint (eab_istft_bwd_f32): dwav [B][hop (T-1)] -> dspec [B][2][T][F].  The forward is linear in the spectrum, and a frame's
// bins enter the wave only through that frame's own samples, so the frames do not interact: with p = t hop + idx, j = p - n_fft/2,
//   u_t[idx] = w[idx] dwav[j] / env(p)  for 0 <= j < hop (Tb - 1), else 0          (env: the forward's envelope, in its order)
//   dspec[.][t][k] = c_k / n_fft * rfft(u_t)[k],   c_k = 1 at k = 0 and n_fft/2, else 2;   Im = 0 at those two bins (C2R).
// One workgroup owns FFT_SIGS consecutive frames of one utterance (no frame is shared between workgroups): it builds the u_t in LDS
// (consecutive lanes -> consecutive samples of dwav; the float index of sample idx IS the packed z[idx/2].(re|im)), runs the
// half-length transform once and splits it into the F bins as stft.hip does, one lane per pair (k, n_fft/2 - k), consecutive lanes
// -> consecutive k of one frame: LDS reads and the stores of both rows are unit-stride (the mirrored bins descending).
// Every output element is stored once, no atomics: the bits do not depend on scheduling.  Frames t >= Tb: zeros; dwav is never read
// at j >= hop (Tb - 1).  Bound: HBM and launch latency (reads hop*4 B, writes 2*F*4 B per frame).
template <bool VARLEN>
__global__ __launch_bounds__(ISTFT_THREADS) void istft_bwd_kernel(const float* __restrict__ dwav, const float* __restrict__ window,
                                                                  const float* __restrict__ twiddle, float* __restrict__ dspec,
                                                                  int T, int n_fft, int hop, int chunks, FftPlan plan,
                                                                  const int* __restrict__ lens) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int NH = n_fft / 2, F = NH + 1;
    const int R = (n_fft + hop - 1) / hop;
    float2* tw = reinterpret_cast<float2*>(smem);                 // [n_fft] exp(-2 pi i j / n_fft)
    float2* buf0 = tw + n_fft;                                    // [FFT_SIGS][NH]
    float2* buf1 = buf0 + FFT_SIGS * NH;
    float* win = reinterpret_cast<float*>(buf1 + FFT_SIGS * NH);  // [n_fft]
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int t0 = chunk * FFT_SIGS;
    const int nfr = T - t0 < FFT_SIGS ? T - t0 : FFT_SIGS;        // frames of this workgroup that exist in dspec
    const int Tb = VARLEN ? (lens[b] > T ? T : (lens[b] < 1 ? 1 : lens[b])) : T;
    float* d0 = dspec + ((size_t)b * 2 * T + t0) * F;             // real rows of frames t0 .., contiguous; imaginary rows T*F on
    float* d1 = d0 + (size_t)T * F;
    if (VARLEN && t0 >= Tb) {                                     // (workgroup-uniform, before any barrier) all frames past the utterance
        for (int e = tid; e < nfr * F; e += ISTFT_THREADS) d0[e] = d1[e] = 0.0f;
        return;
    }
    for (int k = tid; k < n_fft; k += ISTFT_THREADS) {
        const float2 cs = reinterpret_cast<const float2*>(twiddle)[k];
        tw[k] = make_float2(cs.x, -cs.y);
        win[k] = window[k];
    }
    __syncthreads();
    const int out_len = hop * (T - 1), len_b = hop * (Tb - 1);
    float* u = reinterpret_cast<float*>(buf0);
    for (int e = tid; e < FFT_SIGS * n_fft; e += ISTFT_THREADS) {
        const int c = e / n_fft, idx = e - c * n_fft;
        const int t = t0 + c;
        const int p = t * hop + idx, j = p - NH;
        float v = 0.0f;
        if (t < Tb && j >= 0 && j < len_b) {
            const int th = p / hop;
            float env = 0.0f;
            for (int r = 0; r < R; ++r) {                         // the forward's envelope: highest frame first
                const int tt = th - r;
                const int ii = p - tt * hop;
                if (tt < 0 || ii >= n_fft) break;
                if (tt >= Tb) continue;
                env = fmaf(win[ii], win[ii], env);
            }
            v = win[idx] * dwav[(size_t)b * out_len + j] / env;
        }
        u[e] = v;
    }
    __syncthreads();
    const float2* z = fft_run(buf0, buf1, tw, NH, n_fft, plan, tid, ISTFT_THREADS);
    // X[k] = E[k] + W^k O[k] and X[NH-k] = conj(E[k] - W^k O[k]) from the same two values (stft.hip)
    const int NP = NH / 2 + 1;
    const float inv = 1.0f / (float)n_fft;
    for (int e = tid; e < nfr * NP; e += ISTFT_THREADS) {
        const int c = e / NP, k = e - c * NP;
        float* o0 = d0 + (size_t)c * F;
        float* o1 = d1 + (size_t)c * F;
        const bool twice = 2 * k != NH;
        if (VARLEN && t0 + c >= Tb) {
            o0[k] = o1[k] = 0.0f;
            if (twice) o0[NH - k] = o1[NH - k] = 0.0f;
            continue;
        }
        const float2 a = z[c * NH + k];
        const float2 ac = z[c * NH + (k == 0 ? 0 : NH - k)];
        const float2 E = make_float2(0.5f * (a.x + ac.x), 0.5f * (a.y - ac.y));
        const float2 O = make_float2(0.5f * (a.y + ac.y), 0.5f * (ac.x - a.x));
        const float2 wo = cmul(tw[k], O);
        const float sc = k == 0 ? inv : 2.0f * inv;               // c_k / n_fft; k = 0 pairs DC with Nyquist
        o0[k] = (E.x + wo.x) * sc;
        o1[k] = k == 0 ? 0.0f : (E.y + wo.y) * sc;
        if (twice) {
            o0[NH - k] = (E.x - wo.x) * sc;
            o1[NH - k] = k == 0 ? 0.0f : (wo.y - E.y) * sc;
        }
    }
}

extern "C" int eab_istft_bwd_f32(const float* dwav, const float* window, const float* twiddle, float* dspec, const int32_t* lens,
                                 int B, int T, int n_fft, int hop, eab_stream_t stream) {
    EAB_CHECK_ARG(dwav && window && twiddle && dspec);
    EAB_CHECK_ARG(B > 0 && T >= 2 && hop > 0);
    EAB_CHECK_ARG(n_fft >= 4 && n_fft <= ISTFT_MAX_NFFT && (n_fft % 2) == 0);
    if (hop > n_fft || (n_fft + hop - 1) / hop > FFT_SIGS) return EAB_EUNSUPPORTED;
    FftPlan plan;
    if (!fft_plan(n_fft / 2, &plan)) return EAB_EUNSUPPORTED;
    const int chunks = (T + FFT_SIGS - 1) / FFT_SIGS;
    EAB_CHECK_ARG((long long)B * chunks < (1ll << 31) && (long long)hop * (T + FFT_SIGS) + n_fft < (1ll << 31));   // 32-bit positions
    const size_t sh = (size_t)(2 * n_fft + 2 * FFT_SIGS * n_fft + n_fft) * sizeof(float);
    if (lens)
        hipLaunchKernelGGL(istft_bwd_kernel<true>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), dwav, window, twiddle,
                           dspec, T, n_fft, hop, chunks, plan, lens);
    else
        hipLaunchKernelGGL(istft_bwd_kernel<false>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), dwav, window, twiddle,
                           dspec, T, n_fft, hop, chunks, plan, lens);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_istft_f32(const float* spec, const float* window, const float* twiddle, float* wav, int B, int T,
                             int n_fft, int hop, eab_stream_t stream) {
    return istft_launch(spec, window, twiddle, wav, nullptr, B, T, n_fft, hop, stream);
}

extern "C" int eab_istft_lens_f32(const float* spec, const float* window, const float* twiddle, float* wav, const int32_t* lens,
                                  int B, int T_cap, int n_fft, int hop, eab_stream_t stream) {
    return istft_launch(spec, window, twiddle, wav, lens, B, T_cap, n_fft, hop, stream);
}
