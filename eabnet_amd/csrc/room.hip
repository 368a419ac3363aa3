// Training mixtures of a padded batch on the device: shoebox image-source rooms (what McseDatasetOnline does per sample on
// the host: mcse_dataset.py:262-289 -> audio_util.py:6-88 make_audio with rir_method == "ism").  DESIGN.md 4.18 is the definition.
//
// eab_room_gains_f32      the dry gains of mix_scaler: per utterance the peaks, the S x S Gram matrix of the sources and the
//                         window sums of every source from ONE read (workgroup (window, b) owns window `window` of utterance b,
//                         fp64 products, lanes by a fixed shuffle tree, waves in wave order, windows in index order by the final
//                         kernel: no atomics), then the active rms, the scales q_j, the mixture's energy q^T G q and the gains.
// eab_room_rirs_f32       h [B][S][M+1][K]: workgroup (segment, m, (b, s)) owns ROOM_SEG consecutive samples of one response in
//                         LDS as 64-bit integers.  It walks the images |nx|+|ny|+|nz| <= O as columns (nx, ny) with the lanes
//                         along nz, image position, distance and delay in fp64, keeps those whose 81-tap pulse reaches the
//                         segment, and adds rint(tap * 2^40) with integer LDS atomics: integer addition is associative, so the
//                         bits do not depend on which wave meets which image when.  One conversion to fp32, ordinary stores.
//                         The 81 taps of an image are 81 lanes (tap i: lane i, and lanes 0..16 again for i >= 64): consecutive
//                         LDS addresses.  sinc(i - 40 - f) = -(-1)^i sin(pi f) / (pi (i - 40 - f)): one sinf per image.
// eab_room_rirs_tail_f32  the same table by the model "ism_tail" (DESIGN.md 4.23): of the images only those closer than
//                         r_mix = c tail_start to the centre of the array, and from tail_start on a train of virtual images that
//                         nothing stores: image j of source s is recomputed from four counter-based uniforms (arrival time at the
//                         centre, direction, sign).  Their arrival times rise with j, so a segment's images are an index range,
//                         computed from its bounds and the microphone's distance from the centre; the lanes run along j.  Both
//                         parts add into the same integers: the bits do not depend on the schedule here either.
// eab_room_convolve_f32   uniformly partitioned overlap-save, partition P = 512, 1024-point complex FFTs in LDS (fft_lds.h), three
//                         launches: spectra of the source blocks x[(i-1)P, (i+1)P), spectra of the response partitions with TWO
//                         channels per transform (h_c + i h_c', x is real: the product's real and imaginary parts are the two
//                         channels' outputs), and the multiply-accumulate: workgroup (group, pair, b) owns eight output blocks of
//                         two channels, sums sources in index order and partitions in index order with explicit fmaf, one inverse
//                         transform per block.  Channel M is the clean target (source 0 through the free-field row).  What is
//                         summed for an output sample depends on L_b, K_b and S_b only: same bits alone and in any batch.
//                         Rows at and past S_b and samples at and past L_b are never read; the output past L_b is zero, and so
//                         is the output before the first arrival (exactly, not to the transform's rounding).
#include "common.h"
#include "fft_lds.h"

#define ROOM_THREADS 256
#define ROOM_MAX_SRC 8
#define ROOM_MAX_MIC 32
#define ROOM_MAX_ORDER 255
#define ROOM_MAX_K (1 << 22)
#define ROOM_MAX_L (1 << 28)
#define ROOM_SCENE 144                        /* doubles of one scene record (eabnet_amd/simulate.py _scene_record) */
#define ROOM_TAPS 81
#define ROOM_SEG 4096                         /* samples of a response one workgroup holds: 32 KB of int64, four workgroups per CU */
#define ROOM_PART 512                         /* partition of the convolution */
#define ROOM_NFFT 1024
#define ROOM_GRAM 36                          /* upper triangle of 8 x 8 */
#define ROOM_NQ (ROOM_GRAM + ROOM_MAX_SRC)    /* + 8 peaks */
#define ROOM_EPS 2.220446049250313e-16
#define ROOM_C 343.0

// scene record: [0..2] room, [3] absorption, [4] order, [5] sources, [6] reference microphone, [7] dBFS, [8 + j] snr_j,
// [16 + 3 s + axis] source s, [40 + 3 m + axis] microphone m; read by room_rir_tail_kernel alone: [136] tail_seed,
// [137] tail_start, [138] tail_density, [139] the scene's own K (it fixes the tail's images), [140] the sample its responses are cut at
#define ROOM_TAIL_SEED 136
#define ROOM_TAIL_START 137
#define ROOM_TAIL_DENSITY 138
#define ROOM_TAIL_K 139
#define ROOM_TAIL_CUT 140
#define ROOM_MAX_DENSITY 64
__device__ __forceinline__ int room_int(double v, int lo, int hi) {
    const double c = fmin(fmax(v, (double)lo), (double)hi);        // (NaN -> lo)
    return (int)c;
}

extern __shared__ __attribute__((aligned(16))) unsigned char room_lds[];

// more than 64 KB of dynamic LDS needs the function attribute: set once per device and entry point, not on every call
static hipError_t room_large_lds(const void* const* fns, int n, int entry) {
    static bool done[3][64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && done[entry][dev]) return hipSuccess;
    for (int k = 0; k < n; ++k) {
        e = hipFuncSetAttribute(fns[k], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    if (dev >= 0 && dev < 64) done[entry][dev] = true;
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gains
__device__ __forceinline__ int room_tri(int i, int j) { return i * ROOM_MAX_SRC - (i * (i - 1)) / 2 + (j - i); }   // i <= j

__global__ __launch_bounds__(ROOM_THREADS) void room_gain_partial_kernel(const float* __restrict__ x, long long L, int S_max, int W,
                                                                         const int32_t* __restrict__ lens, const double* __restrict__ scenes,
                                                                         int nwin, double* __restrict__ partial) {
    __shared__ double red[ROOM_THREADS / 64][ROOM_NQ];
    const int b = blockIdx.y, w = blockIdx.x, tid = threadIdx.x;
    const int Lb = max(0, min(lens[b], (int)L));
    const int t0 = w * W, t1 = min(t0 + W, Lb);
    if (t0 >= Lb) return;                                              // (workgroup-uniform) the final kernel does not read it
    const int S = room_int(scenes[(long long)b * ROOM_SCENE + 5], 1, S_max);
    const float* xb = x + (long long)b * S_max * L;
    double acc[ROOM_NQ];
#pragma unroll
    for (int q = 0; q < ROOM_NQ; ++q) acc[q] = 0.0;
    for (int t = t0 + tid; t < t1; t += ROOM_THREADS) {
        double v[ROOM_MAX_SRC];
#pragma unroll
        for (int s = 0; s < ROOM_MAX_SRC; ++s) v[s] = s < S ? (double)xb[(long long)s * L + t] : 0.0;
#pragma unroll
        for (int i = 0; i < ROOM_MAX_SRC; ++i) {
#pragma unroll
            for (int j = i; j < ROOM_MAX_SRC; ++j) acc[room_tri(i, j)] += v[i] * v[j];
            acc[ROOM_GRAM + i] = fmax(acc[ROOM_GRAM + i], fabs(v[i]));
        }
    }
#pragma unroll
    for (int q = 0; q < ROOM_NQ; ++q)
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_down(acc[q], off, 64);
            acc[q] = q < ROOM_GRAM ? acc[q] + o : fmax(acc[q], o);
        }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0)
        for (int q = 0; q < ROOM_NQ; ++q) red[wave][q] = acc[q];
    __syncthreads();
    if (tid < ROOM_NQ) {
        double s = red[0][tid];
        for (int k = 1; k < ROOM_THREADS / 64; ++k) s = tid < ROOM_GRAM ? s + red[k][tid] : fmax(s, red[k][tid]);
        partial[((long long)b * nwin + w) * ROOM_NQ + tid] = s;
    }
}

__global__ void room_gain_final_kernel(const double* __restrict__ partial, long long L, int S_max, int W, const int32_t* __restrict__ lens,
                                       const double* __restrict__ scenes, int B, int nwin, double* __restrict__ gains) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* sc = scenes + (long long)b * ROOM_SCENE;
    const int Lb = max(0, min(lens[b], (int)L));
    const int S = room_int(sc[5], 1, S_max);
    const int used = (int)(((long long)Lb + W - 1) / W);
    const double* pb = partial + (long long)b * nwin * ROOM_NQ;
    double peak[ROOM_MAX_SRC], q[ROOM_MAX_SRC];
    for (int s = 0; s < S; ++s) {
        double p = 0.0;
        for (int w = 0; w < used; ++w) p = fmax(p, pb[(long long)w * ROOM_NQ + ROOM_GRAM + s]);
        peak[s] = p + ROOM_EPS;
    }
    double e00 = 0.0;
    for (int w = 0; w < used; ++w) e00 += pb[(long long)w * ROOM_NQ + room_tri(0, 0)];
    const double rms_clean = sqrt(e00 / (peak[0] * peak[0]) / (double)Lb);
    q[0] = 1.0;
    for (int s = 1; s < S; ++s) {
        double asum = 0.0;
        long long acnt = 0;
        for (int w = 0; w < used; ++w) {
            const int n = min(W, Lb - w * W);
            const double ws = pb[(long long)w * ROOM_NQ + room_tri(s, s)];
            if (sqrt(ws / (peak[s] * peak[s]) / (double)n) > 0.0031622776601683794) {      // 10^(-50/20)
                asum += ws;
                acnt += n;
            }
        }
        const double rms = acnt ? sqrt(asum / (peak[s] * peak[s]) / (double)acnt) : ROOM_EPS;
        q[s] = rms_clean / pow(10.0, sc[8 + s] / 20.0) / (rms + ROOM_EPS);
    }
    double energy = 0.0;
    for (int i = 0; i < S; ++i)
        for (int j = i; j < S; ++j) {
            double g = 0.0;
            for (int w = 0; w < used; ++w) g += pb[(long long)w * ROOM_NQ + room_tri(i, j)];
            g = g / (peak[i] * peak[j]) * (q[i] * q[j]);
            energy += i == j ? g : 2.0 * g;
        }
    const double G = pow(10.0, sc[7] / 20.0) / (sqrt(fmax(energy, 0.0) / (double)Lb) + ROOM_EPS);
    for (int s = 0; s < S_max; ++s) gains[(long long)b * S_max + s] = s < S ? G * q[s] / peak[s] : 0.0;
}

extern "C" int eab_room_gains_f32(const float* x, int B, int S_max, int L, const int32_t* lens, const double* scenes, double fs,
                                  double* partial, int partial_windows, double* gains, eab_stream_t stream) {
    EAB_CHECK_ARG(x && lens && scenes && partial && gains);
    EAB_CHECK_ARG(B >= 1 && B <= 4096 && S_max >= 1 && S_max <= ROOM_MAX_SRC && L >= 1 && L <= ROOM_MAX_L);
    EAB_CHECK_ARG(fs >= 10.0 && fs <= 1.0e7);
    const int W = (int)(fs / 10.0);
    const int nwin = (L + W - 1) / W;
    EAB_CHECK_ARG(partial_windows >= nwin && nwin <= 65535 * 64);
    hipLaunchKernelGGL(room_gain_partial_kernel, dim3((unsigned)nwin, (unsigned)B), dim3(ROOM_THREADS), 0, eab_stream(stream), x,
                       (long long)L, S_max, W, lens, scenes, partial_windows, partial);
    hipLaunchKernelGGL(room_gain_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, eab_stream(stream), partial, (long long)L,
                       S_max, W, lens, scenes, B, partial_windows, gains);
    EAB_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// impulse responses
__device__ __forceinline__ double room_image(int n, double L, double s) { return (n & 1) ? (double)(n + 1) * L - s : (double)n * L + s; }

__global__ __launch_bounds__(ROOM_THREADS) void room_rir_kernel(const double* __restrict__ scenes, double fs, int S_max, int M, int K,
                                                                float* __restrict__ h) {
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(room_lds);          // [ROOM_SEG]
    float* beta = reinterpret_cast<float*>(room_lds + sizeof(unsigned long long) * ROOM_SEG);   // [ROOM_MAX_ORDER + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg0 = blockIdx.x * ROOM_SEG, m = blockIdx.y, bs = blockIdx.z, b = bs / S_max, s = bs - b * S_max;
    const int seglen = min(ROOM_SEG, K - seg0);
    const double* sc = scenes + (long long)b * ROOM_SCENE;
    float* hr = h + ((long long)bs * (M + 1) + m) * K + seg0;
    const int S = room_int(sc[5], 1, S_max);
    if (s >= S) {                                                      // (workgroup-uniform) a row nobody reads: zeros
        for (int t = tid; t < seglen; t += ROOM_THREADS) hr[t] = 0.0f;
        return;
    }
    const int O = m == M ? 0 : room_int(sc[4], 0, ROOM_MAX_ORDER);     // row M: the free-field response, the image n = 0 alone
    const int mic = m == M ? room_int(sc[6], 0, M - 1) : m;
    const double Lx = sc[0], Ly = sc[1], Lz = sc[2];
    const double sx = sc[16 + 3 * s], sy = sc[17 + 3 * s], sz = sc[18 + 3 * s];
    const double rx = sc[40 + 3 * mic], ry = sc[41 + 3 * mic], rz = sc[42 + 3 * mic];
    for (int t = tid; t < seglen; t += ROOM_THREADS) acc[t] = 0ull;
    for (int k = tid; k <= O; k += ROOM_THREADS) beta[k] = (float)pow(1.0 - sc[3], 0.5 * (double)k);
    __syncthreads();

    // the window of the fractional-delay filter and the sign of sin(pi (i - 40 - f)) for this lane's taps i = lane, lane + 64
    const float hann0 = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)lane / 80.0));
    const float hann1 = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)(lane + 64) / 80.0));
    const float sgn = (lane & 1) ? 1.0f : -1.0f;                       // -(-1)^i, the same for i and i + 64
    const float x0 = (float)(lane - 40), x1 = (float)(lane + 24);
    const float pi_f = 3.14159265358979323846f;
    const int D = 2 * O + 1;

    for (int col = wave; col < D * D; col += ROOM_THREADS / 64) {      // (everything but the lanes' nz is wave-uniform)
        const int nx = col / D - O, ny = col % D - O;
        const int rem = O - abs(nx) - abs(ny);
        if (rem < 0) continue;
        const double dx = room_image(nx, Lx, sx) - rx, dy = room_image(ny, Ly, sy) - ry;
        const double dxy2 = dx * dx + dy * dy;
        if (fmin(sqrt(dxy2) * fs / ROOM_C, 2.0e9) >= (double)(seg0 + seglen)) continue;   // the whole column arrives later
        for (int nz0 = -rem; nz0 <= rem; nz0 += 64) {
            const int nz = nz0 + lane;
            const double dz = room_image(nz, Lz, sz) - rz;
            const double d = sqrt(dxy2 + dz * dz);
            const double tau = fmin(d * fs / ROOM_C, 2.0e9);
            const double fl = floor(tau);
            const int k0 = (int)fl;
            const bool keep = nz <= rem && k0 + (ROOM_TAPS - 1) >= seg0 && k0 < seg0 + seglen && d > 0.0;
            unsigned long long mask = __ballot(keep);
            if (!mask) continue;
            const float ff = (float)(tau - fl);
            const float g = beta[min(abs(nx) + abs(ny) + abs(nz), O)] / (4.0f * pi_f * (float)d);
            const float a = g * sinf(pi_f * (ff > 0.5f ? 1.0f - ff : ff)) / pi_f;      // g sin(pi f) / pi
            const int krel = k0 - seg0;
            while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int kk = __shfl(krel, src, 64);
                const float gg = __shfl(g, src, 64), aa = __shfl(a, src, 64), fr = __shfl(ff, src, 64);
                {
                    const float xx = x0 - fr;
                    const float v = hann0 * (xx == 0.0f ? gg : sgn * aa / xx);
                    const int t = kk + lane;
                    if (t >= 0 && t < seglen) atomicAdd(&acc[t], (unsigned long long)llrintf(v * 1099511627776.0f));
                }
                if (lane < ROOM_TAPS - 64) {
                    const float xx = x1 - fr;
                    const float v = hann1 * (sgn * aa / xx);
                    const int t = kk + lane + 64;
                    if (t >= 0 && t < seglen) atomicAdd(&acc[t], (unsigned long long)llrintf(v * 1099511627776.0f));
                }
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < seglen; t += ROOM_THREADS) hr[t] = (float)((double)(long long)acc[t] * 9.094947017729282e-13);   // 2^-40
}

extern "C" int eab_room_rirs_f32(const double* scenes, int B, int S_max, int M, int K, double fs, float* h, eab_stream_t stream) {
    EAB_CHECK_ARG(scenes && h);
    EAB_CHECK_ARG(B >= 1 && B <= 4096 && S_max >= 1 && S_max <= ROOM_MAX_SRC && M >= 1 && M <= ROOM_MAX_MIC);
    EAB_CHECK_ARG(K >= 1 && K <= ROOM_MAX_K && fs >= 10.0 && fs <= 1.0e7);
    const size_t lds = sizeof(unsigned long long) * ROOM_SEG + sizeof(float) * (ROOM_MAX_ORDER + 1);
    const void* fn = reinterpret_cast<const void*>(&room_rir_kernel);
    hipError_t e = room_large_lds(&fn, 1, 0);
    if (e != hipSuccess) return eab_hip_status(e);
    hipLaunchKernelGGL(room_rir_kernel, dim3((unsigned)((K + ROOM_SEG - 1) / ROOM_SEG), (unsigned)(M + 1), (unsigned)(B * S_max)),
                       dim3(ROOM_THREADS), lds, eab_stream(stream), scenes, fs, S_max, M, K, h);
    EAB_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// impulse responses, "ism_tail": the images near the array and a sampled tail
struct RoomTaps {                             // what a lane knows of its taps i = lane and lane + 64 (room_rir_kernel has the same values)
    float hann0, hann1, sgn, x0, x1;
    int lane;
};

// the pulses of the lanes that `keep`, one after the other (the whole wave calls this): gain g, delay krel + f against the
// segment's first sample; taps at and past `cut` are dropped.  The arithmetic of a tap is room_rir_kernel's.
__device__ __forceinline__ void room_add_pulses(unsigned long long* acc, int cut, bool keep, int krel, float g, float ff,
                                                const RoomTaps& tp) {
    unsigned long long mask = __ballot(keep);
    if (!mask) return;
    const float pi_f = 3.14159265358979323846f;
    const float a = g * sinf(pi_f * (ff > 0.5f ? 1.0f - ff : ff)) / pi_f;              // g sin(pi f) / pi
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int kk = __shfl(krel, src, 64);
        const float gg = __shfl(g, src, 64), aa = __shfl(a, src, 64), fr = __shfl(ff, src, 64);
        {
            const float xx = tp.x0 - fr;
            const float v = tp.hann0 * (xx == 0.0f ? gg : tp.sgn * aa / xx);
            const int t = kk + tp.lane;
            if (t >= 0 && t < cut) atomicAdd(&acc[t], (unsigned long long)llrintf(v * 1099511627776.0f));
        }
        if (tp.lane < ROOM_TAPS - 64) {
            const float xx = tp.x1 - fr;
            const float v = tp.hann1 * (tp.sgn * aa / xx);
            const int t = kk + tp.lane + 64;
            if (t >= 0 && t < cut) atomicAdd(&acc[t], (unsigned long long)llrintf(v * 1099511627776.0f));
        }
    }
}

__device__ __forceinline__ unsigned long long room_mix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// uniform d (0..3) of image j of source s, in [0, 1)
__device__ __forceinline__ double room_uniform(unsigned long long seed, int s, int d, int j) {
    const unsigned long long counter = ((unsigned long long)(4 * s + d) << 32) | (unsigned long long)(unsigned int)j;
    return (double)(room_mix64(seed + 0x9E3779B97F4A7C15ull * (1ull + counter)) >> 11) * 1.1102230246251565e-16;   // 2^-53
}

// the orders n whose image can lie closer than r to the coordinate c: the image of n lies in [n L, (n + 1) L] for a source
// inside the room.  One order of slack either side; every image is tested exactly afterwards.
__device__ __forceinline__ void room_orders(double c, double r, double L, int O, int* lo, int* hi) {
    *lo = room_int(floor((c - r) / L) - 1.0, -O, O);
    *hi = room_int(floor((c + r) / L) + 1.0, -O, O);
}

__global__ __launch_bounds__(ROOM_THREADS) void room_rir_tail_kernel(const double* __restrict__ scenes, double fs, int S_max, int M,
                                                                     int K, float* __restrict__ h) {
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(room_lds);          // [ROOM_SEG]
    float* beta = reinterpret_cast<float*>(room_lds + sizeof(unsigned long long) * ROOM_SEG);   // [ROOM_MAX_ORDER + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg0 = blockIdx.x * ROOM_SEG, m = blockIdx.y, bs = blockIdx.z, b = bs / S_max, s = bs - b * S_max;
    const int seglen = min(ROOM_SEG, K - seg0);
    const double* sc = scenes + (long long)b * ROOM_SCENE;
    float* hr = h + ((long long)bs * (M + 1) + m) * K + seg0;
    const int S = room_int(sc[5], 1, S_max);
    const int cut = max(0, min(seglen, room_int(sc[ROOM_TAIL_CUT], 1, K) - seg0));     // the scene's responses end inside this segment
    if (s >= S || cut == 0) {                                          // (workgroup-uniform) a row nobody reads, or past the end: zeros
        for (int t = tid; t < seglen; t += ROOM_THREADS) hr[t] = 0.0f;
        return;
    }
    const bool free_row = m == M;                                      // row M: the free-field response, the image n = 0 alone
    const int O = free_row ? 0 : room_int(sc[4], 0, ROOM_MAX_ORDER);
    const int mic = free_row ? room_int(sc[6], 0, M - 1) : m;
    const double Lx = sc[0], Ly = sc[1], Lz = sc[2];
    const double sx = sc[16 + 3 * s], sy = sc[17 + 3 * s], sz = sc[18 + 3 * s];
    const double rx = sc[40 + 3 * mic], ry = sc[41 + 3 * mic], rz = sc[42 + 3 * mic];
    double cx = 0.0, cy = 0.0, cz = 0.0;                               // the centre of the array: the microphones in index order
    for (int q = 0; q < M; ++q) {
        cx += sc[40 + 3 * q];
        cy += sc[41 + 3 * q];
        cz += sc[42 + 3 * q];
    }
    cx /= (double)M, cy /= (double)M, cz /= (double)M;
    const double t_start = fmin(fmax(sc[ROOM_TAIL_START], 0.0), 1.0e6);                // (NaN -> 0)
    const double r_mix = ROOM_C * t_start;
    for (int t = tid; t < seglen; t += ROOM_THREADS) acc[t] = 0ull;
    for (int k = tid; k <= O; k += ROOM_THREADS) beta[k] = (float)pow(1.0 - sc[3], 0.5 * (double)k);
    __syncthreads();

    RoomTaps tp;
    tp.hann0 = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)lane / 80.0));
    tp.hann1 = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)(lane + 64) / 80.0));
    tp.sgn = (lane & 1) ? 1.0f : -1.0f;                                // -(-1)^i, the same for i and i + 64
    tp.x0 = (float)(lane - 40), tp.x1 = (float)(lane + 24);
    tp.lane = lane;
    const float pi_f = 3.14159265358979323846f;

    // the early part: the lattice walk of room_rir_kernel over the orders that can lie inside the sphere of r_mix about the centre
    int nxl, nxh, nyl, nyh, nzl, nzh;
    room_orders(cx, r_mix, Lx, O, &nxl, &nxh);
    room_orders(cy, r_mix, Ly, O, &nyl, &nyh);
    room_orders(cz, r_mix, Lz, O, &nzl, &nzh);
    const int W = max(0, nxh - nxl + 1), H = max(0, nyh - nyl + 1);
    for (int col = wave; col < W * H; col += ROOM_THREADS / 64) {        // (everything but the lanes' nz is wave-uniform)
        const int nx = nxl + col / H, ny = nyl + col % H;
        const int rem = O - abs(nx) - abs(ny);
        if (rem < 0) continue;
        const double px = room_image(nx, Lx, sx), py = room_image(ny, Ly, sy);
        const double ex = px - cx, ey = py - cy;
        const double exy2 = ex * ex + ey * ey;
        if (!free_row && !(sqrt(exy2) < r_mix)) continue;              // the column's nearest image lies beyond r_mix
        const double dx = px - rx, dy = py - ry;
        const double dxy2 = dx * dx + dy * dy;
        if (fmin(sqrt(dxy2) * fs / ROOM_C, 2.0e9) >= (double)(seg0 + cut)) continue;    // the whole column arrives later
        const int zl = max(-rem, nzl), zh = min(rem, nzh);
        for (int nz0 = zl; nz0 <= zh; nz0 += 64) {
            const int nz = nz0 + lane;
            const double pz = room_image(nz, Lz, sz);
            const double dz = pz - rz, ez = pz - cz;
            const double d = sqrt(dxy2 + dz * dz);
            const double tau = fmin(d * fs / ROOM_C, 2.0e9);
            const double fl = floor(tau);
            const int k0 = (int)fl;
            const bool inside = free_row || sqrt(exy2 + ez * ez) < r_mix;                // the test on the centre: one image set for all microphones
            const bool keep = nz <= zh && inside && k0 + (ROOM_TAPS - 1) >= seg0 && k0 < seg0 + cut && d > 0.0;
            const float g = beta[min(abs(nx) + abs(ny) + abs(nz), O)] / (4.0f * pi_f * (float)d);
            room_add_pulses(acc, cut, keep, k0 - seg0, g, (float)(tau - fl), tp);
        }
    }

    // the tail: J virtual images spread over the n_slots samples from tail_start to the scene's own K - ROOM_TAPS
    const double k_mix = fmin(floor(t_start * fs), 2.0e9);
    const double n_slots = (double)room_int(sc[ROOM_TAIL_K], 1, ROOM_MAX_K) - (double)ROOM_TAPS - k_mix;
    const double density = fmin(fmax(sc[ROOM_TAIL_DENSITY], 0.0), (double)ROOM_MAX_DENSITY);
    const double absorb = fmax(sc[3], 0.0);
    if (!free_row && n_slots > 0.0 && absorb < 1.0 && density > 0.0) { // (workgroup-uniform)
        const int J = (int)ceil(density * n_slots);                    // <= 64 * 2^22
        const double nu = (double)J / n_slots;
        const double ex = rx - cx, ey = ry - cy, ez = rz - cz;
        const double rho = sqrt(ex * ex + ey * ey + ez * ez) * fs / ROOM_C;            // |tau - fs t_j| <= rho: the triangle inequality
        // image j reaches the centre (j + U0) / nu samples after tail_start: those that can reach [seg0 - 80, seg0 + cut), one
        // sample and one image of slack either side; each is tested exactly below
        const double first = ((double)seg0 - (double)(ROOM_TAPS - 1) - rho - t_start * fs - 1.0) * nu;
        const double last = ((double)(seg0 + cut) + rho - t_start * fs + 1.0) * nu;
        const int jlo = room_int(floor(first) - 1.0, 0, J), jhi = room_int(floor(last) + 1.0, -1, J - 1);
        const unsigned long long seed = (unsigned long long)fmin(fmax(sc[ROOM_TAIL_SEED], 0.0), 9007199254740991.0);
        const double half_ln = 0.5 * log(1.0 - absorb);
        const double V = Lx * Ly * Lz;
        for (int j0 = jlo + wave * 64; j0 <= jhi; j0 += ROOM_THREADS) {                // (wave-uniform) the lanes along j
            const int j = j0 + lane;
            const double u0 = room_uniform(seed, s, 0, j), u1 = room_uniform(seed, s, 1, j);
            const double u2 = room_uniform(seed, s, 2, j), u3 = room_uniform(seed, s, 3, j);
            const double t = t_start + ((double)j + u0) / (nu * fs);
            const double z = 2.0 * u1 - 1.0;
            const double r = sqrt(fmax(1.0 - z * z, 0.0));
            double sn, cs;
            sincospi(2.0 * u2, &sn, &cs);
            const double ux = r * cs, uy = r * sn, ct = ROOM_C * t;
            const double dx = (cx + ct * ux) - rx, dy = (cy + ct * uy) - ry, dz = (cz + ct * z) - rz;
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            const double tau = fmin(d * fs / ROOM_C, 2.0e9);
            const double fl = floor(tau);
            const int k0 = (int)fl;
            const bool keep = j <= jhi && k0 + (ROOM_TAPS - 1) >= seg0 && k0 < seg0 + cut && d > 0.0;
            if (!__ballot(keep)) continue;
            const double walls = ct * (fabs(ux) / Lx + fabs(uy) / Ly + fabs(z) / Lz);  // this image's own reflection count
            const double g = sqrt(4.0 * M_PI * ROOM_C * ROOM_C * ROOM_C * t * t / (V * fs * nu)) * exp(walls * half_ln) / (4.0 * M_PI * d);
            room_add_pulses(acc, cut, keep, k0 - seg0, (float)(u3 < 0.5 ? -g : g), (float)(tau - fl), tp);
        }
    }
    __syncthreads();
    for (int t = tid; t < seglen; t += ROOM_THREADS)
        hr[t] = t < cut ? (float)((double)(long long)acc[t] * 9.094947017729282e-13) : 0.0f;   // 2^-40
}

extern "C" int eab_room_rirs_tail_f32(const double* scenes, int B, int S_max, int M, int K, double fs, float* h, eab_stream_t stream) {
    EAB_CHECK_ARG(scenes && h);
    EAB_CHECK_ARG(B >= 1 && B <= 4096 && S_max >= 1 && S_max <= ROOM_MAX_SRC && M >= 1 && M <= ROOM_MAX_MIC);
    EAB_CHECK_ARG(K >= 1 && K <= ROOM_MAX_K && fs >= 10.0 && fs <= 1.0e7);
    const size_t lds = sizeof(unsigned long long) * ROOM_SEG + sizeof(float) * (ROOM_MAX_ORDER + 1);
    const void* fn = reinterpret_cast<const void*>(&room_rir_tail_kernel);
    hipError_t e = room_large_lds(&fn, 1, 2);
    if (e != hipSuccess) return eab_hip_status(e);
    hipLaunchKernelGGL(room_rir_tail_kernel, dim3((unsigned)((K + ROOM_SEG - 1) / ROOM_SEG), (unsigned)(M + 1), (unsigned)(B * S_max)),
                       dim3(ROOM_THREADS), lds, eab_stream(stream), scenes, fs, S_max, M, K, h);
    EAB_RETURN_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// convolution
struct RoomConvArgs {
    const float* x; int L; int S_max; int M; int K; int nblk, npart, npairs;
    const int32_t* lens; const int32_t* klen; const double* scenes; const double* gains; const float* h; const float2* tw;
    float2* xs;                               // [B][S_max][nblk][ROOM_NFFT]
    float2* hs;                               // [B][S_max][npairs][npart][ROOM_NFFT]
    float* noisy; float* clean;
    FftPlan plan;
};

// the spectra: HS false: eight source blocks of (b, s); HS true: eight response partitions of (b, s, channel pair)
template <bool HS>
__global__ __launch_bounds__(ROOM_THREADS) void room_spectra_kernel(const RoomConvArgs a) {
    float2* tw = reinterpret_cast<float2*>(room_lds);                  // [ROOM_NFFT]
    float2* buf0 = tw + ROOM_NFFT;                                     // [FFT_SIGS][ROOM_NFFT]
    float2* buf1 = buf0 + FFT_SIGS * ROOM_NFFT;
    const int tid = threadIdx.x;
    const int bs = blockIdx.z, b = bs / a.S_max, s = bs - b * a.S_max;
    const int S = room_int(a.scenes[(long long)b * ROOM_SCENE + 5], 1, a.S_max);
    if (s >= S) return;                                                // (workgroup-uniform) never read
    const int Lb = max(0, min(a.lens[b], a.L));
    const int Kb = max(0, min(a.klen[2 * b], a.K));
    const int first = blockIdx.x * FFT_SIGS;
    const int count = HS ? (Kb + ROOM_PART - 1) / ROOM_PART : min(a.nblk, (Lb + ROOM_PART - 1) / ROOM_PART + 1);
    if (first >= count) return;
    for (int k = tid; k < ROOM_NFFT; k += ROOM_THREADS) tw[k] = a.tw[k];
    if (HS) {
        const int c0 = 2 * blockIdx.y, c1 = c0 + 1;
        // channel M is the clean target: the free-field row of source 0, nothing of the others
        const bool on0 = c0 < a.M || (c0 == a.M && s == 0), on1 = c1 < a.M || (c1 == a.M && s == 0);
        const float* h0 = a.h + ((long long)bs * (a.M + 1) + min(c0, a.M)) * a.K;
        const float* h1 = a.h + ((long long)bs * (a.M + 1) + min(c1, a.M)) * a.K;
        for (int e = tid; e < FFT_SIGS * ROOM_NFFT; e += ROOM_THREADS) {
            const int k = e / ROOM_NFFT, n = e - k * ROOM_NFFT;
            const int t = (first + k) * ROOM_PART + n;
            const bool in = n < ROOM_PART && t < Kb;
            buf0[e] = make_float2(in && on0 ? h0[t] : 0.0f, in && on1 ? h1[t] : 0.0f);
        }
    } else {
        const float* xr = a.x + (long long)bs * a.L;
        for (int e = tid; e < FFT_SIGS * ROOM_NFFT; e += ROOM_THREADS) {
            const int k = e / ROOM_NFFT, n = e - k * ROOM_NFFT;
            const int t = (first + k - 1) * ROOM_PART + n;
            buf0[e] = make_float2(t >= 0 && t < Lb ? xr[t] : 0.0f, 0.0f);
        }
    }
    __syncthreads();
    const float2* z = fft_run(buf0, buf1, tw, ROOM_NFFT, ROOM_NFFT, a.plan, tid, ROOM_THREADS);
    float2* dst = HS ? a.hs + (((long long)bs * a.npairs + blockIdx.y) * a.npart + first) * ROOM_NFFT
                     : a.xs + ((long long)bs * a.nblk + first) * ROOM_NFFT;
    const int keep = min(FFT_SIGS, count - first);
    for (int e = tid; e < keep * ROOM_NFFT; e += ROOM_THREADS) dst[e] = z[e];
}

__global__ __launch_bounds__(ROOM_THREADS) void room_mix_kernel(const RoomConvArgs a) {
    float2* tw = reinterpret_cast<float2*>(room_lds);
    float2* buf0 = tw + ROOM_NFFT;
    float2* buf1 = buf0 + FFT_SIGS * ROOM_NFFT;
    const int tid = threadIdx.x, b = blockIdx.z, pair = blockIdx.y, j0 = blockIdx.x * FFT_SIGS;
    const int Lb = max(0, min(a.lens[b], a.L));
    const int Kb = max(0, min(a.klen[2 * b], a.K));
    const int arrive = a.klen[2 * b + 1];                              // nothing reaches a microphone before this sample
    const int S = room_int(a.scenes[(long long)b * ROOM_SCENE + 5], 1, a.S_max);
    const int c0 = 2 * pair, c1 = c0 + 1;
    float* y0 = c0 < a.M ? a.noisy + ((long long)b * a.M + c0) * a.L : (c0 == a.M ? a.clean + (long long)b * a.L : nullptr);
    float* y1 = c1 < a.M ? a.noisy + ((long long)b * a.M + c1) * a.L : (c1 == a.M ? a.clean + (long long)b * a.L : nullptr);
    const int t_lo = j0 * ROOM_PART, t_hi = min(t_lo + FFT_SIGS * ROOM_PART, a.L);
    if (t_lo >= Lb) {                                                  // (workgroup-uniform) past the utterance: zeros
        for (int t = t_lo + tid; t < t_hi; t += ROOM_THREADS) {
            if (y0) y0[t] = 0.0f;
            if (y1) y1[t] = 0.0f;
        }
        return;
    }
    for (int k = tid; k < ROOM_NFFT; k += ROOM_THREADS) tw[k] = a.tw[k];
    const int npb = (Kb + ROOM_PART - 1) / ROOM_PART;                  // partitions of this utterance's responses
    const int nxb = min(a.nblk, (Lb + ROOM_PART - 1) / ROOM_PART + 1); // source blocks that hold samples
    float2 acc[FFT_SIGS][ROOM_NFFT / ROOM_THREADS];
#pragma unroll
    for (int k = 0; k < FFT_SIGS; ++k)
#pragma unroll
        for (int r = 0; r < ROOM_NFFT / ROOM_THREADS; ++r) acc[k][r] = make_float2(0.0f, 0.0f);
    for (int s = 0; s < S; ++s) {
        const float g = (float)fmin(fmax(a.gains[(long long)b * a.S_max + s], -3.0e38), 3.0e38);
        const float2* hsp = a.hs + (((long long)(b * a.S_max + s)) * a.npairs + pair) * a.npart * ROOM_NFFT;
        const float2* xsp = a.xs + ((long long)(b * a.S_max + s)) * a.nblk * ROOM_NFFT;
        for (int p = 0; p < npb; ++p) {
            float2 hg[ROOM_NFFT / ROOM_THREADS];
#pragma unroll
            for (int r = 0; r < ROOM_NFFT / ROOM_THREADS; ++r) {
                const float2 v = hsp[(long long)p * ROOM_NFFT + tid + r * ROOM_THREADS];
                hg[r] = make_float2(g * v.x, g * v.y);
            }
#pragma unroll
            for (int k = 0; k < FFT_SIGS; ++k) {
                const int i = j0 + k - p;
                if (i < 0 || i >= nxb || (j0 + k) * ROOM_PART >= Lb) continue;         // (workgroup-uniform)
#pragma unroll
                for (int r = 0; r < ROOM_NFFT / ROOM_THREADS; ++r) {
                    const float2 xv = xsp[(long long)i * ROOM_NFFT + tid + r * ROOM_THREADS];
                    acc[k][r].x = fmaf(xv.x, hg[r].x, acc[k][r].x);
                    acc[k][r].x = fmaf(-xv.y, hg[r].y, acc[k][r].x);
                    acc[k][r].y = fmaf(xv.x, hg[r].y, acc[k][r].y);
                    acc[k][r].y = fmaf(xv.y, hg[r].x, acc[k][r].y);
                }
            }
        }
    }
    // inverse transform as conj(FFT(conj(Y))) / N
#pragma unroll
    for (int k = 0; k < FFT_SIGS; ++k)
#pragma unroll
        for (int r = 0; r < ROOM_NFFT / ROOM_THREADS; ++r)
            buf0[k * ROOM_NFFT + tid + r * ROOM_THREADS] = make_float2(acc[k][r].x, -acc[k][r].y);
    __syncthreads();
    const float2* z = fft_run(buf0, buf1, tw, ROOM_NFFT, ROOM_NFFT, a.plan, tid, ROOM_THREADS);
    const float inv = 1.0f / (float)ROOM_NFFT;
    for (int e = tid; e < FFT_SIGS * ROOM_PART; e += ROOM_THREADS) {
        const int k = e / ROOM_PART, n = e - k * ROOM_PART;
        const int t = t_lo + e;
        if (t >= t_hi) continue;
        const float2 v = z[k * ROOM_NFFT + ROOM_PART + n];
        const bool in = t < Lb && t >= arrive;
        if (y0) y0[t] = in ? v.x * inv : 0.0f;
        if (y1) y1[t] = in ? -v.y * inv : 0.0f;
    }
}

static inline bool room_conv_shape(int B, int S_max, int M, int L, int K, int* nblk, int* npart, int* npairs) {
    if (B < 1 || B > 4096 || S_max < 1 || S_max > ROOM_MAX_SRC || M < 1 || M > ROOM_MAX_MIC) return false;
    if (L < 1 || L > ROOM_MAX_L || K < 1 || K > ROOM_MAX_K) return false;
    *nblk = (L + ROOM_PART - 1) / ROOM_PART;
    *npart = (K + ROOM_PART - 1) / ROOM_PART;
    *npairs = (M + 2) / 2;                                             // M + 1 channels
    return true;
}

extern "C" long long eab_room_workspace_bytes(int B, int S_max, int M, int L, int K) {
    int nblk, npart, npairs;
    if (!room_conv_shape(B, S_max, M, L, K, &nblk, &npart, &npairs)) return -1;
    return (long long)sizeof(float2) * ROOM_NFFT * B * S_max * ((long long)nblk + (long long)npairs * npart);
}

extern "C" int eab_room_convolve_f32(const float* x, int B, int S_max, int L, const int32_t* lens, const double* scenes,
                                     const int32_t* klen, const double* gains, const float* h, int M, int K, const float* twiddle,
                                     void* work, long long work_bytes, float* noisy, float* clean, eab_stream_t stream) {
    EAB_CHECK_ARG(x && lens && scenes && klen && gains && h && twiddle && work && noisy && clean);
    RoomConvArgs a;
    EAB_CHECK_ARG(room_conv_shape(B, S_max, M, L, K, &a.nblk, &a.npart, &a.npairs));
    EAB_CHECK_ARG(work_bytes >= eab_room_workspace_bytes(B, S_max, M, L, K) && (reinterpret_cast<uintptr_t>(work) & 15u) == 0);
    EAB_CHECK_ARG(fft_plan(ROOM_NFFT, &a.plan));
    a.x = x; a.L = L; a.S_max = S_max; a.M = M; a.K = K;
    a.lens = lens; a.klen = klen; a.scenes = scenes; a.gains = gains; a.h = h; a.tw = reinterpret_cast<const float2*>(twiddle);
    a.xs = reinterpret_cast<float2*>(work);
    a.hs = a.xs + (long long)B * S_max * a.nblk * ROOM_NFFT;
    a.noisy = noisy; a.clean = clean;
    const size_t lds = sizeof(float2) * ROOM_NFFT * (1 + 2 * FFT_SIGS);
    const void* fns[3] = {reinterpret_cast<const void*>(&room_spectra_kernel<false>), reinterpret_cast<const void*>(&room_spectra_kernel<true>),
                          reinterpret_cast<const void*>(&room_mix_kernel)};
    hipError_t e = room_large_lds(fns, 3, 1);
    if (e != hipSuccess) return eab_hip_status(e);
    const unsigned groups = (unsigned)((a.nblk + FFT_SIGS - 1) / FFT_SIGS);
    hipLaunchKernelGGL(room_spectra_kernel<false>, dim3(groups, 1u, (unsigned)(B * S_max)), dim3(ROOM_THREADS), lds, eab_stream(stream), a);
    hipLaunchKernelGGL(room_spectra_kernel<true>, dim3((unsigned)((a.npart + FFT_SIGS - 1) / FFT_SIGS), (unsigned)a.npairs, (unsigned)(B * S_max)),
                       dim3(ROOM_THREADS), lds, eab_stream(stream), a);
    hipLaunchKernelGGL(room_mix_kernel, dim3(groups, (unsigned)a.npairs, (unsigned)B), dim3(ROOM_THREADS), lds, eab_stream(stream), a);
    EAB_RETURN_LAUNCH_STATUS();
}
