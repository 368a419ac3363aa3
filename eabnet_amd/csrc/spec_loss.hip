// Multi-resolution STFT loss on the waveform, value and gradient: spectral convergence plus log-magnitude distance of an estimate
// to a clean wave at R time-frequency resolutions (Parallel WaveGAN; DESIGN.md §4.21 has the definition and the deviations).
//
// For a resolution (N, H, W) -- torch.stft(x[:n_b], N, H, W, hann(W), center=True, pad_mode="reflect") -- utterance b has
// T = 1 + n_b / H frames of F = N/2 + 1 bins.  With P = max(re^2 + im^2, floor), E = sqrt(P_est), S = sqrt(P_clean):
//     A = sum (S - E)^2    Q = sum S^2    C = sum |ln S - ln E|            (over the utterance's own frames and bins)
//     loss_b = 1/R sum_r [ factor_sc sqrt(A_r) / sqrt(Q_r) + factor_mag C_r / (T_r F_r) ]
//     d loss_b / d E = -1/R [ factor_sc (S - E) / (sqrt A sqrt Q) + factor_mag sign(S - E) / (T F E) ],  through a bin of the estimate
//     that is not clamped: d E / d (re, im) = (re, im) / E; zero through a clamped one; the sc part is zero where A = 0.
//
// eab_mrstft_loss_f32: one launch per resolution -- a workgroup owns MR_FRAMES = 4 consecutive frames of one utterance, gathers
// the reflected, windowed frames of BOTH waves straight from the rows (scalar loads at the same indices whatever the alignment)
// into the FFT_SIGS = 8 slots of the half-length LDS transform of fft_lds.h (est frames in slots 0..3, clean frames in 4..7: no
// two signals share a transform), splits the packed transforms into bins as stft.hip does, forms the three terms per bin in
// fp32 and adds them in fp64: a lane's bins in index order, lanes by a fixed shuffle tree, waves in order -> one partial triple
// per workgroup.  Then ONE finalize workgroup adds an utterance's partials (a wave per utterance: a lane's groups in index order,
// the same tree) resolution by resolution and writes loss_b, the two coefficients per (utterance, resolution) that the gradient
// needs, and the batch's sum and mean.
// eab_mrstft_loss_bwd_f32: one launch per resolution recomputes the spectra of the same four frames, forms d L / d X per bin scaled
// by grad_output (read on the device), runs the adjoint of the real transform through the same forward passes
// (conj(FFT(conj .)) as istft.hip), applies the window and stores every frame's W samples to a workspace.  One gather launch then
// adds, per sample, the frames that cover it in ONE fixed order: resolutions ascending; within one the direct position's frames
// ascending, then those of the left reflection, then those of the right one; fp64 accumulator, one rounding.  Exactly zero from
// n_b to the row's end.  No atomics anywhere: an utterance has the same bits alone, in any batch, at any alignment and in a
// second call.
// Bound: LDS transforms (72 N bytes of LDS per workgroup: 144 KB at N = 2048, one workgroup of 1024 lanes per CU) and launch
// latency.
#include "rows.h"
#include "fft_lds.h"

#define MR_THREADS 256               /* finalize and gather; the frames kernel: mr_frames_threads(N) lanes */
#define MR_MAX_THREADS 1024
#define MR_FRAMES (FFT_SIGS / 2)      /* frames of a workgroup: est and clean of each fill the FFT_SIGS slots */
#define MR_MAX_RES 8
#define MR_MIN_NFFT 8
#define MR_MAX_NFFT 2048
#define MR_MAX_COVER 8                /* frames whose window support covers one sample: ceil(win / hop) */

typedef EabRows<2> MrRows;            // estimate, clean

struct MrGeom {
    int N, hop, off, W;               // frame, hop, first sample of the window's support in the frame, support
    int Tcap, groups, goff;           // frames and workgroups of a row of `cap` samples; first partial of this resolution in a row
    FftPlan plan;
    long long toff, soff;             // floats: this resolution's (window[N], twiddle[N][2]) in `tables`; its frames in the workspace
};
struct MrSet {
    int R, nmin, cap, sum_groups;     // nmin = max N / 2 + 1: the shortest utterance reflect padding allows
    long long seg_floats;
    MrGeom g[MR_MAX_RES];
};

// one dynamic LDS array for every kernel of this file (the host emulation defines it)
extern __shared__ __attribute__((aligned(16))) float mr_smem[];

// resolutions (n_fft, hop, win) as HOST int32 triples -> the launch geometry of B rows of `cap` readable samples; false: refused
static bool mr_build(const int32_t* res, int R, int B, int cap, MrSet* s) {
    if (!res || R < 1 || R > MR_MAX_RES || B < 1 || B > 65535 || cap < 1 || cap > EAB_ROWS_MAX_LEN) return false;
    long long toff = 0, goff = 0, soff = 0;
    int maxN = 0;
    for (int r = 0; r < R; ++r) {
        MrGeom& g = s->g[r];
        const int N = res[3 * r], hop = res[3 * r + 1], W = res[3 * r + 2];
        if (N < MR_MIN_NFFT || N > MR_MAX_NFFT || (N & 1)) return false;
        if (hop < 1 || hop > N || W < 1 || W > N || (W + hop - 1) / hop > MR_MAX_COVER) return false;
        if (!fft_plan(N / 2, &g.plan)) return false;
        g.N = N; g.hop = hop; g.W = W; g.off = (N - W) / 2;
        g.Tcap = 1 + cap / hop;
        g.groups = (g.Tcap + MR_FRAMES - 1) / MR_FRAMES;
        g.goff = (int)goff; g.toff = toff; g.soff = soff;
        toff += 3ll * N;
        goff += g.groups;
        soff += (long long)B * g.Tcap * W;
        if (goff >= (1ll << 30)) return false;
        maxN = N > maxN ? N : maxN;
    }
    s->R = R; s->nmin = maxN / 2 + 1; s->cap = cap; s->sum_groups = (int)goff; s->seg_floats = soff;
    return cap >= s->nmin;
}

// samples of utterance b: device content clamped into [nmin, cap], so every reflected index stays inside the row
__device__ __forceinline__ int mr_len(const int32_t* __restrict__ lens, int b, int nmin, int cap) {
    const int n = lens[b];
    return n < nmin ? nmin : (n > cap ? cap : n);
}

// bins k and NH - k of one real frame from its packed half-length transform (stft.hip): X[k] = E + W^k O, X[NH-k] = conj(E - W^k O)
__device__ __forceinline__ void mr_split(const float2* __restrict__ z, const float2* __restrict__ tw, int NH, int k, float2 x[2]) {
    const float2 a = z[k], ac = z[k == 0 ? 0 : NH - k];
    const float2 E = make_float2(0.5f * (a.x + ac.x), 0.5f * (a.y - ac.y));
    const float2 O = make_float2(0.5f * (a.y + ac.y), 0.5f * (ac.x - a.x));
    const float2 wo = cmul(tw[k], O);
    x[0] = make_float2(E.x + wo.x, E.y + wo.y);
    x[1] = make_float2(E.x - wo.x, wo.y - E.y);
}

// BWD = false: partial[(b sum_groups + goff + group) * 3 ..] = (A, Q, C) of the workgroup's frames.
// BWD = true: seg[soff + ((b Tcap + t) W + i)] = w[off + i] * (d L / d frame_t)[off + i], scaled by grad_out[b] * scale.
template <bool BWD>
__global__ __launch_bounds__(MR_MAX_THREADS) void mrstft_frames_kernel(const MrRows rows, const int32_t* __restrict__ lens, int nmin, int cap,
                                                                   const MrGeom g, const float* __restrict__ tables, float floor_p,
                                                                   double* __restrict__ partial, int sum_groups,
                                                                   const double* __restrict__ coef, int R, int r,
                                                                   const float* __restrict__ gout, int gout_stride, double scale,
                                                                   float* __restrict__ seg) {
    const int N = g.N, NH = N / 2, hop = g.hop;
    float2* tw = reinterpret_cast<float2*>(mr_smem);              // [N] exp(-2 pi i j / N)
    float2* buf0 = tw + N;                                        // [FFT_SIGS][NH]
    float2* buf1 = buf0 + FFT_SIGS * NH;
    double* red = reinterpret_cast<double*>(buf1 + FFT_SIGS * NH);   // [waves][3]
    const int tid = threadIdx.x, nthr = blockDim.x, b = blockIdx.y, t0 = (int)blockIdx.x * MR_FRAMES;
    const int n = mr_len(lens, b, nmin, cap);
    const int T = 1 + n / hop;
    if (t0 >= T) return;                                          // (workgroup-uniform, before any barrier) nobody reads its output
    const float* win = tables + g.toff;
    const float2* twg = reinterpret_cast<const float2*>(win + N); // (cos, sin)(+theta)
    for (int k = tid; k < N; k += nthr) {
        const float2 cs = twg[k];
        tw[k] = make_float2(cs.x, -cs.y);
    }
    const float* pe = rows.p[0] + (long long)b * rows.stride[0];
    const float* ps = rows.p[1] + (long long)b * rows.stride[1];
    // gather + window: slot sig holds frame t0 + (sig & 3) of est (sig < 4) or clean; the float index of sample idx IS the packed
    // z[idx / 2].(re | im); consecutive lanes -> consecutive samples, a lane's eight loads of one idx in flight together
    float* fr = reinterpret_cast<float*>(buf0);
    for (int idx = tid; idx < N; idx += nthr) {
        const bool under = idx >= g.off && idx < g.off + g.W;
        const float w = under ? win[idx] : 0.0f;
        float v[FFT_SIGS];
#pragma unroll
        for (int sig = 0; sig < FFT_SIGS; ++sig) {
            const int t = t0 + (sig & (MR_FRAMES - 1));
            v[sig] = under && t < T ? (sig < MR_FRAMES ? pe : ps)[eab_reflect(t * hop + idx, NH, n)] : 0.0f;
        }
#pragma unroll
        for (int sig = 0; sig < FFT_SIGS; ++sig) fr[sig * N + idx] = w * v[sig];
    }
    __syncthreads();
    float2* z = fft_run(buf0, buf1, tw, NH, N, g.plan, tid, nthr);
    float2* other = z == buf0 ? buf1 : buf0;

    const int NP = NH / 2 + 1;                                    // pairs (k, NH - k); k = 0 pairs DC with Nyquist
    double acc[3] = {0.0, 0.0, 0.0};
    float c_sc = 0.0f, c_lm = 0.0f;
    if (BWD) {
        const double w = (double)gout[(long long)b * gout_stride] * scale;
        c_sc = (float)(w * coef[((long long)b * R + r) * 2]);
        c_lm = (float)(w * coef[((long long)b * R + r) * 2 + 1]);
        for (int e = tid; e < MR_FRAMES * NH; e += nthr) other[MR_FRAMES * NH + e] = make_float2(0.0f, 0.0f);   // idle slots
    }
    for (int e = tid; e < MR_FRAMES * NP; e += nthr) {
        const int f = e / NP, k = e - f * NP;
        const bool twice = 2 * k != NH;                           // NH even: k = NH / 2 is its own partner
        if (t0 + f >= T) {
            if (BWD) {
                other[f * NH + k] = make_float2(0.0f, 0.0f);
                if (k > 0 && twice) other[f * NH + NH - k] = make_float2(0.0f, 0.0f);
            }
            continue;
        }
        float2 xe[2], xc[2], G[2];
        mr_split(z + f * NH, tw, NH, k, xe);
        mr_split(z + (MR_FRAMES + f) * NH, tw, NH, k, xc);
        G[0] = G[1] = make_float2(0.0f, 0.0f);
        for (int q = 0; q < (twice ? 2 : 1); ++q) {
            const float raw = xe[q].x * xe[q].x + xe[q].y * xe[q].y, rawc = xc[q].x * xc[q].x + xc[q].y * xc[q].y;
            const float Pe = raw > floor_p ? raw : floor_p, Pc = rawc > floor_p ? rawc : floor_p;
            const float E = sqrtf(Pe), d = sqrtf(Pc) - E;
            if (!BWD) {
                acc[0] += (double)(d * d);
                acc[1] += (double)Pc;
                acc[2] += (double)(0.5f * fabsf(logf(Pc / Pe)));
            } else if (raw >= floor_p) {                          // (torch.clamp: the gradient passes at the bound itself)
                const float sg = Pc > Pe ? 1.0f : (Pc < Pe ? -1.0f : 0.0f);
                const float gE = -(c_sc * d + c_lm * sg / E) / E;
                G[q] = make_float2(gE * xe[q].x, gE * xe[q].y);
            }
        }
        if (BWD) {
            // adjoint of the real transform: d frame[n] = Re sum_k G_k e^{+i theta k n} = (N/2) irfft(Y)[n] with Y = G inside and
            // 2 Re G at DC and Nyquist; packed as istft.hip packs a spectrum: other[k] = conj(E + i O), other[NH-k] = E - i O
            float2 y0 = G[0], y1 = twice ? G[1] : G[0];
            if (k == 0) {
                y0 = make_float2(2.0f * y0.x, 0.0f);
                y1 = make_float2(2.0f * y1.x, 0.0f);
            }
            const float2 Ev = make_float2(0.5f * (y0.x + y1.x), 0.5f * (y0.y - y1.y));
            const float2 Dv = make_float2(0.5f * (y0.x - y1.x), 0.5f * (y0.y + y1.y));
            const float2 Ov = cmul(Dv, make_float2(tw[k].x, -tw[k].y));
            other[f * NH + k] = make_float2(Ev.x - Ov.y, -(Ev.y + Ov.x));
            if (k > 0 && twice) other[f * NH + NH - k] = make_float2(Ev.x + Ov.y, Ev.y - Ov.x);
        }
    }
    if (!BWD) {
        // lanes by the fixed shuffle tree, waves in index order (as eab_span_reduce of rows.h, for nthr lanes)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
        if ((tid & 63) == 0)
            for (int q = 0; q < 3; ++q) red[(tid >> 6) * 3 + q] = acc[q];
        __syncthreads();
        if (tid < 3) {
            double s = red[tid];
            for (int w = 1; w < nthr / 64; ++w) s += red[w * 3 + tid];
            partial[((long long)b * sum_groups + g.goff + (int)blockIdx.x) * 3 + tid] = s;
        }
        return;
    }
    __syncthreads();
    const float* yf = reinterpret_cast<const float*>(fft_run(other, z, tw, NH, N, g.plan, tid, nthr));
    // d frame[2j] = Re y[j], d frame[2j+1] = -Im y[j]; then the window; only its support leaves the workgroup
    float* out = seg + g.soff + ((long long)b * g.Tcap + t0) * g.W;
    const int nf = T - t0 < MR_FRAMES ? T - t0 : MR_FRAMES;
    for (int f = 0; f < nf; ++f)
        for (int i = tid; i < g.W; i += nthr) {
            const int idx = g.off + i;
            const float a = yf[f * N + idx];
            out[f * g.W + i] = win[idx] * ((idx & 1) ? -a : a);
        }
}

// ONE workgroup; wave w takes the utterances w, w + 4, ...: lane l adds the partials l, l + 64, ... of a resolution, the lanes by
// the shuffle tree.  The batch's sum adds a wave's utterances in that order and the four waves in order.
__global__ __launch_bounds__(MR_THREADS) void mrstft_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ lens,
                                                                  const MrSet set, int B, double f_sc, double f_mag,
                                                                  double* __restrict__ coef, float* __restrict__ loss,
                                                                  float* __restrict__ total) {
    double* wave_sum = reinterpret_cast<double*>(mr_smem);        // [MR_THREADS / 64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = set.R < 1 ? 1 : (set.R > MR_MAX_RES ? MR_MAX_RES : set.R);
    double mine = 0.0;
    for (int b = wave; b < B; b += MR_THREADS / 64) {
        const int n = mr_len(lens, b, set.nmin, set.cap);
        double v = 0.0;
        for (int r = 0; r < R; ++r) {
            const MrGeom& g = set.g[r];
            const int T = 1 + n / g.hop, groups = (T + MR_FRAMES - 1) / MR_FRAMES;
            const double* p = partial + ((long long)b * set.sum_groups + g.goff) * 3;
            double a[3] = {0.0, 0.0, 0.0};
            for (int k = lane; k < groups; k += 64)
                for (int q = 0; q < 3; ++q) a[q] += p[3ll * k + q];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_down(a[q], o, 64);
            if (lane == 0) {
                const double sA = sqrt(a[0]), sQ = sqrt(a[1]), TF = (double)T * (double)(g.N / 2 + 1);
                v += f_sc * (sA / sQ) + f_mag * (a[2] / TF);
                coef[((long long)b * R + r) * 2] = a[0] > 0.0 ? f_sc / ((double)R * sA * sQ) : 0.0;
                coef[((long long)b * R + r) * 2 + 1] = f_mag / ((double)R * TF);
            }
        }
        if (lane == 0) {
            v /= (double)R;
            loss[b] = (float)v;
            mine += v;
        }
    }
    if (lane == 0) wave_sum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < MR_THREADS / 64; ++w) s += wave_sum[w];
        total[0] = (float)s;
        total[1] = (float)(s / (double)B);
    }
}

// the frames t < T whose window support [t hop + off, t hop + off + W) holds the padded position p, ascending
__device__ __forceinline__ double mr_add_frames(double acc, const float* __restrict__ segb, const MrGeom& g, int T, int p) {
    const int q = p - g.off;
    if (q < 0) return acc;
    int t_hi = q / g.hop;
    if (t_hi > T - 1) t_hi = T - 1;
    const int lo = q - g.W + 1;
    const int t_lo = lo <= 0 ? 0 : (lo + g.hop - 1) / g.hop;
    for (int t = t_lo; t <= t_hi; ++t) acc += (double)segb[(long long)t * g.W + (q - t * g.hop)];
    return acc;
}

// grad row b: est_cap floats, `gstride` apart; one lane per sample
__global__ __launch_bounds__(MR_THREADS) void mrstft_gather_kernel(const float* __restrict__ seg, const int32_t* __restrict__ lens,
                                                                   const MrSet set, int est_cap, float* __restrict__ grad,
                                                                   long long gstride) {
    const int b = blockIdx.y;
    const long long j0 = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (j0 >= est_cap) return;
    const int j = (int)j0;
    const int n = mr_len(lens, b, set.nmin, set.cap);
    float v = 0.0f;
    if (j < n) {
        const int R = set.R < 1 ? 1 : (set.R > MR_MAX_RES ? MR_MAX_RES : set.R);
        double acc = 0.0;
        for (int r = 0; r < R; ++r) {
            const MrGeom& g = set.g[r];
            const int NH = g.N / 2, T = 1 + n / g.hop;
            const float* segb = seg + g.soff + (long long)b * g.Tcap * g.W;
            acc = mr_add_frames(acc, segb, g, T, j + NH);                                   // direct
            if (j >= 1 && j <= NH) acc = mr_add_frames(acc, segb, g, T, NH - j);            // left reflection: padded NH - j
            const int m = 2 * (n - 1) - j;                                                  // right reflection: sample index m >= n
            if (m >= n && m <= n - 1 + NH) acc = mr_add_frames(acc, segb, g, T, m + NH);
        }
        v = (float)acc;
    }
    grad[(long long)b * gstride + j] = v;
}

#ifdef __HIPCC__
// more than 64 KB of dynamic LDS needs the function attribute: set once per device
static hipError_t mr_large_lds() {
    static bool done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
    const void* fns[2] = {reinterpret_cast<const void*>(&mrstft_frames_kernel<false>),
                          reinterpret_cast<const void*>(&mrstft_frames_kernel<true>)};
    for (int k = 0; k < 2; ++k) {
        e = hipFuncSetAttribute(fns[k], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    if (dev >= 0 && dev < 64) done[dev] = true;
    return hipSuccess;
}
#else
static hipError_t mr_large_lds() { return hipSuccess; }
#endif

static size_t mr_frames_lds(int N) { return (size_t)72 * N + (MR_MAX_THREADS / 64) * 3 * sizeof(double); }
// lanes of a frames workgroup: the 144 KB of N = 2048 leave one workgroup per CU, which then needs its sixteen waves itself
static unsigned mr_frames_threads(int N) { return N >= 2048 ? 1024u : (N >= 1024 ? 512u : 256u); }

extern "C" long long eab_mrstft_workspace_bytes(const int32_t* res, int R, int B, int cap, int backward) {
    MrSet set;
    if (!mr_build(res, R, B, cap, &set)) return -1;
    return backward ? set.seg_floats * (long long)sizeof(float) : (long long)B * set.sum_groups * 3 * (long long)sizeof(double);
}

extern "C" int eab_mrstft_loss_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride,
                                   int clean_cap, const int32_t* lens, int B, const int32_t* res, int R, const float* tables,
                                   double factor_sc, double factor_mag, double floor, void* work, long long work_bytes, double* coef,
                                   float* loss, float* total, eab_stream_t stream) {
    const MrRows rows = {{est, clean}, {est_stride, clean_stride}, {est_cap, clean_cap}};
    EAB_CHECK_ARG(lens && res && tables && work && coef && loss && total && eab_rows_ok(rows, B));
    EAB_CHECK_ARG(factor_sc >= 0.0 && factor_sc < 1e300 && factor_mag >= 0.0 && factor_mag < 1e300 && floor > 0.0 && floor < 1e30);
    MrSet set;
    EAB_CHECK_ARG(mr_build(res, R, B, est_cap < clean_cap ? est_cap : clean_cap, &set));
    EAB_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7u) == 0 && work_bytes >= (long long)B * set.sum_groups * 3 * (long long)sizeof(double));
    const hipError_t le = mr_large_lds();
    if (le != hipSuccess) return eab_hip_status(le);
    double* partial = static_cast<double*>(work);
    for (int r = 0; r < R; ++r)
        hipLaunchKernelGGL(mrstft_frames_kernel<false>, dim3((unsigned)set.g[r].groups, (unsigned)B), dim3(mr_frames_threads(set.g[r].N)),
                           mr_frames_lds(set.g[r].N), eab_stream(stream), rows, lens, set.nmin, set.cap, set.g[r], tables, (float)floor,
                           partial, set.sum_groups, (const double*)nullptr, R, r, (const float*)nullptr, 0, 0.0, (float*)nullptr);
    hipLaunchKernelGGL(mrstft_final_kernel, dim3(1), dim3(MR_THREADS), (MR_THREADS / 64) * sizeof(double), eab_stream(stream),
                       (const double*)partial, lens, set, B, factor_sc, factor_mag, coef, loss, total);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_mrstft_loss_bwd_f32(const float* est, long long est_stride, int est_cap, const float* clean, long long clean_stride,
                                       int clean_cap, const int32_t* lens, int B, const int32_t* res, int R, const float* tables,
                                       double floor, const double* coef, const float* grad_out, int grad_out_stride, double scale,
                                       void* work, long long work_bytes, float* grad, long long grad_stride, eab_stream_t stream) {
    const MrRows rows = {{est, clean}, {est_stride, clean_stride}, {est_cap, clean_cap}};
    EAB_CHECK_ARG(lens && res && tables && work && coef && grad_out && grad && eab_rows_ok(rows, B));
    EAB_CHECK_ARG(floor > 0.0 && floor < 1e30 && scale == scale && grad_out_stride >= 0 && (B == 1 || grad_stride >= est_cap));
    MrSet set;
    EAB_CHECK_ARG(mr_build(res, R, B, est_cap < clean_cap ? est_cap : clean_cap, &set));
    EAB_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 3u) == 0 && work_bytes >= set.seg_floats * (long long)sizeof(float));
    const hipError_t le = mr_large_lds();
    if (le != hipSuccess) return eab_hip_status(le);
    float* seg = static_cast<float*>(work);
    for (int r = 0; r < R; ++r)
        hipLaunchKernelGGL(mrstft_frames_kernel<true>, dim3((unsigned)set.g[r].groups, (unsigned)B), dim3(mr_frames_threads(set.g[r].N)),
                           mr_frames_lds(set.g[r].N), eab_stream(stream), rows, lens, set.nmin, set.cap, set.g[r], tables, (float)floor,
                           (double*)nullptr, set.sum_groups, coef, R, r, grad_out, grad_out_stride, scale, seg);
    hipLaunchKernelGGL(mrstft_gather_kernel, dim3((unsigned)((est_cap + MR_THREADS - 1) / MR_THREADS), (unsigned)B), dim3(MR_THREADS), 0,
                       eab_stream(stream), (const float*)seg, lens, set, est_cap, grad, grad_stride);
    EAB_RETURN_LAUNCH_STATUS();
}
