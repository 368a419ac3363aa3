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
// The reference applies this to the sqrt-compressed estimate as it is; eab_istft_lin_f32 / eab_istft_lin_bwd_f32 are the same
// kernels on y = s |s| per bin (the compression undone), from the same bodies (istft_body.inc, istft_bwd_body.inc).
#include "common.h"
#include "fft_lds.h"

#define ISTFT_THREADS 256
#define ISTFT_MAX_NFFT 512

// The linear-domain entry points (eab_istft_lin_f32, eab_istft_lin_bwd_f32) undo the front end's X |X|^-1/2 on the way in:
// y = s |s| per bin, one fp32 formula wherever a bin is decompressed (products and sum rounded one by one: -ffp-contract=off).
__device__ __forceinline__ float istft_modulus(float2 s) { return sqrtf(s.x * s.x + s.y * s.y); }
__device__ __forceinline__ float2 istft_decompress(float2 s) {
    const float r = istft_modulus(s);
    return make_float2(s.x * r, s.y * r);
}
// The adjoint of that step: y = s |s| has the symmetric Jacobian r I + s s^T / r, so dL/ds = r g + s (s . g) / r for g = dL/dy; at
// r = 0 the map is C1 with derivative 0 (|y| = |s|^2), and the result is exactly 0 there -- no division.
__device__ __forceinline__ float2 istft_decompress_bwd(float2 s, float2 g) {
    const float r = istft_modulus(s);
    if (r == 0.0f) return make_float2(0.0f, 0.0f);
    const float q = (s.x * g.x + s.y * g.y) / r;
    return make_float2(r * g.x + s.x * q, r * g.y + s.y * q);
}

// VARLEN (eab_istft_lens_f32): `lens` holds B frame counts; T is the capacity (row strides of spec and wav).  Utterance b is
// inverted as by a launch with T = lens[b] -- frames t >= lens[b] are neither read nor added nor counted in the envelope --
// and its samples from hop (lens[b] - 1) on are written as zeros.  The count is clamped to [1, T].
//
// LIN (eab_istft_lin_f32): the transform of y = s |s|, s = (re, im) the staged bin -- the sqrt compression of the front end undone.
// The modulus is taken where the split reads the bin from LDS (both lanes that read a bin form the same product), with the
// imaginary parts of the DC and Nyquist bins still in it; only then are those two parts dropped.  y never reaches memory.
// Both kernels are the one body of istft_body.inc, which reads LIN as a constant of its kernel (conv_st.hip's pattern): the
// reference kernel's code is what it was before LIN existed (tools/isa_diff.py).
template <bool VARLEN>
__global__ __launch_bounds__(ISTFT_THREADS) void istft_kernel(const float* __restrict__ spec, const float* __restrict__ window,
                                                              const float* __restrict__ twiddle, float* __restrict__ wav,
                                                              int T, int n_fft, int hop, int chunks, FftPlan plan,
                                                              const int* __restrict__ lens) {
    constexpr bool LIN = false;
#include "istft_body.inc"
}

template <bool VARLEN>
__global__ __launch_bounds__(ISTFT_THREADS) void istft_lin_kernel(const float* __restrict__ spec, const float* __restrict__ window,
                                                                  const float* __restrict__ twiddle, float* __restrict__ wav,
                                                                  int T, int n_fft, int hop, int chunks, FftPlan plan,
                                                                  const int* __restrict__ lens) {
    constexpr bool LIN = true;
#include "istft_body.inc"
}

// lens == NULL: every utterance is T frames long (eab_istft_f32); else per-utterance frame counts in a batch of capacity T
// lin: the linear-domain kernels (eab_istft_lin_f32), same grid and LDS
static int istft_launch(const float* spec, const float* window, const float* twiddle, float* wav, const int* lens, int B, int T,
                        int n_fft, int hop, eab_stream_t stream, bool lin = false) {
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
    if (lin && lens)
        hipLaunchKernelGGL(istft_lin_kernel<true>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), spec, window,
                           twiddle, wav, T, n_fft, hop, chunks, plan, lens);
    else if (lin)
        hipLaunchKernelGGL(istft_lin_kernel<false>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), spec, window,
                           twiddle, wav, T, n_fft, hop, chunks, plan, lens);
    else if (lens)
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
//
// LIN (eab_istft_lin_bwd_f32): the adjoint of the linear-domain forward.  The values above are g = dL/dy of the frame; the lane that
// holds the pair (k, n_fft/2 - k) loads the two bins of `spec` (row layout of dspec, so the same unit-stride pattern as its
// stores) and stores istft_decompress_bwd(s, g) instead -- g stays in registers.  g_im = 0 at DC and Nyquist, so the imaginary
// gradient there is im re g_re / r: those parts of `spec` act through the modulus.  `spec` is not read at frames t >= Tb.
template <bool VARLEN>
__global__ __launch_bounds__(ISTFT_THREADS) void istft_bwd_kernel(const float* __restrict__ dwav, const float* __restrict__ window,
                                                                  const float* __restrict__ twiddle, float* __restrict__ dspec,
                                                                  int T, int n_fft, int hop, int chunks, FftPlan plan,
                                                                  const int* __restrict__ lens) {
    constexpr bool LIN = false;
    constexpr const float* spec = nullptr;                        // (named by the body's LIN branch only)
#include "istft_bwd_body.inc"
}

template <bool VARLEN>
__global__ __launch_bounds__(ISTFT_THREADS) void istft_lin_bwd_kernel(const float* __restrict__ dwav, const float* __restrict__ spec,
                                                                      const float* __restrict__ window,
                                                                      const float* __restrict__ twiddle, float* __restrict__ dspec,
                                                                      int T, int n_fft, int hop, int chunks, FftPlan plan,
                                                                      const int* __restrict__ lens) {
    constexpr bool LIN = true;
#include "istft_bwd_body.inc"
}

// spec == NULL: eab_istft_bwd_f32; else the linear-domain adjoint at that spectrum
static int istft_bwd_launch(const float* dwav, const float* spec, const float* window, const float* twiddle, float* dspec,
                            const int* lens, int B, int T, int n_fft, int hop, eab_stream_t stream) {
    EAB_CHECK_ARG(dwav && window && twiddle && dspec);
    EAB_CHECK_ARG(B > 0 && T >= 2 && hop > 0);
    EAB_CHECK_ARG(n_fft >= 4 && n_fft <= ISTFT_MAX_NFFT && (n_fft % 2) == 0);
    if (hop > n_fft || (n_fft + hop - 1) / hop > FFT_SIGS) return EAB_EUNSUPPORTED;
    FftPlan plan;
    if (!fft_plan(n_fft / 2, &plan)) return EAB_EUNSUPPORTED;
    const int chunks = (T + FFT_SIGS - 1) / FFT_SIGS;
    EAB_CHECK_ARG((long long)B * chunks < (1ll << 31) && (long long)hop * (T + FFT_SIGS) + n_fft < (1ll << 31));   // 32-bit positions
    const size_t sh = (size_t)(2 * n_fft + 2 * FFT_SIGS * n_fft + n_fft) * sizeof(float);
    if (spec && lens)
        hipLaunchKernelGGL(istft_lin_bwd_kernel<true>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), dwav, spec,
                           window, twiddle, dspec, T, n_fft, hop, chunks, plan, lens);
    else if (spec)
        hipLaunchKernelGGL(istft_lin_bwd_kernel<false>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), dwav, spec,
                           window, twiddle, dspec, T, n_fft, hop, chunks, plan, lens);
    else if (lens)
        hipLaunchKernelGGL(istft_bwd_kernel<true>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), dwav, window, twiddle,
                           dspec, T, n_fft, hop, chunks, plan, lens);
    else
        hipLaunchKernelGGL(istft_bwd_kernel<false>, dim3(B * chunks), dim3(ISTFT_THREADS), sh, eab_stream(stream), dwav, window, twiddle,
                           dspec, T, n_fft, hop, chunks, plan, lens);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_istft_bwd_f32(const float* dwav, const float* window, const float* twiddle, float* dspec, const int32_t* lens,
                                 int B, int T, int n_fft, int hop, eab_stream_t stream) {
    return istft_bwd_launch(dwav, nullptr, window, twiddle, dspec, lens, B, T, n_fft, hop, stream);
}

extern "C" int eab_istft_f32(const float* spec, const float* window, const float* twiddle, float* wav, int B, int T,
                             int n_fft, int hop, eab_stream_t stream) {
    return istft_launch(spec, window, twiddle, wav, nullptr, B, T, n_fft, hop, stream);
}

extern "C" int eab_istft_lens_f32(const float* spec, const float* window, const float* twiddle, float* wav, const int32_t* lens,
                                  int B, int T_cap, int n_fft, int hop, eab_stream_t stream) {
    return istft_launch(spec, window, twiddle, wav, lens, B, T_cap, n_fft, hop, stream);
}

extern "C" int eab_istft_lin_f32(const float* spec, const float* window, const float* twiddle, float* wav, const int32_t* lens,
                                 int B, int T, int n_fft, int hop, eab_stream_t stream) {
    return istft_launch(spec, window, twiddle, wav, lens, B, T, n_fft, hop, stream, true);
}

extern "C" int eab_istft_lin_bwd_f32(const float* dwav, const float* spec, const float* window, const float* twiddle, float* dspec,
                                     const int32_t* lens, int B, int T, int n_fft, int hop, eab_stream_t stream) {
    EAB_CHECK_ARG(spec);
    return istft_bwd_launch(dwav, spec, window, twiddle, dspec, lens, B, T, n_fft, hop, stream);
}

