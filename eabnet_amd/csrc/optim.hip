// The end of the training step on flat buffers: clip_grad_norm_(max_norm) and torch.optim.Adam (no amsgrad, maximize False) of
// train_distributed.py:222-230 in two launches (include/eabnet_hip.h has the argument contract).
//
// A segment table describes ONE run of elements, the segments laid end to end; chunk k is the elements [k, k + 1) * 4096 of the run,
// whichever segments they lie in.  One workgroup of 256 per chunk in both kernels:
//   1  opt_sumsq_kernel  partial[k] = sum of squares of chunk k, fp64: lane t owns the elements 4t + 1024 j + {0..3} in that order
//                        (the square of an fp32 value is exact in fp64), lanes by a fixed shuffle tree, the four waves in index order
//                        through LDS.  A chunk that lies in one segment at a 16-byte aligned address loads four values at once, any
//                        other one by one AT THE SAME indices.
//   2  opt_adam_kernel   every workgroup adds ALL partials in one fixed order (lane t the entries t + 256 j ascending, the same tree):
//                        norm = sqrt(total), c = min(1, max_norm / (norm + 1e-6)) in fp64, then the element-wise recurrence with
//                        the host's scalars; workgroup 0 writes the norm.
// Determinism: no atomics; every sum has one order that depends on an element's position in the run alone, so the norm has the same
// bits in every run and for every way of cutting the same values into segments.
// Non-finite gradients behave as in torch: a NaN norm makes c NaN and with it every updated value; an Inf norm makes c zero, and
// 0 * Inf is NaN for the infinite elements.  Without clipping (max_norm <= 0) c is exactly 1 and only the affected elements are lost.
// Bound: launch latency and HBM (7 passes of 4 bytes per element); both kernels also compile as host C++ against tests/hip_host_shim.
#include "rows.h"

#define OPT_THREADS 256
#define OPT_CHUNK EAB_OPTIM_CHUNK
#define OPT_QUADS (OPT_CHUNK / (4 * OPT_THREADS))       /* quads of four elements per lane */
#define OPT_MAX_CHUNKS (1 << 24)
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a chunk is a whole number of quads per lane");

struct OptTable {
    eab_optim_segment seg[EAB_OPTIM_MAX_SEGMENTS];
    long long start[EAB_OPTIM_MAX_SEGMENTS + 1];        // first run element of segment s; start[s] = total from nseg on
    long long total;
};

struct OptScalars {                                     // the host's doubles, rounded once
    float step_size, w1, beta2, w2, bias2_sqrt, eps;
    double weight_decay, max_norm;
};

struct OptPointers {
    float* p;
    const float* g;
    float* m;
    float* v;
};

// the segment that holds run elements [e, e + len), its pointers moved to e; all null when the span straddles two segments.
// Static indices only: the table stays in the kernel's argument registers.
__device__ __forceinline__ OptPointers opt_span(const OptTable& t, long long e, int len) {
    OptPointers r = {nullptr, nullptr, nullptr, nullptr};
#pragma unroll
    for (int s = 0; s < EAB_OPTIM_MAX_SEGMENTS; ++s)
        if (e >= t.start[s] && e + len <= t.start[s + 1]) {
            const long long o = e - t.start[s];
            r.g = t.seg[s].grad + o;
            r.p = t.seg[s].param ? t.seg[s].param + o : nullptr;
            r.m = t.seg[s].exp_avg ? t.seg[s].exp_avg + o : nullptr;
            r.v = t.seg[s].exp_avg_sq ? t.seg[s].exp_avg_sq + o : nullptr;
        }
    return r;
}

// the sum of the four waves' values in index order, in every lane; acc is one value per lane
__device__ __forceinline__ double opt_block_sum(double acc, double* wsum, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    double s = wsum[0];
    for (int w = 1; w < OPT_THREADS / 64; ++w) s += wsum[w];
    return s;
}

__global__ __launch_bounds__(OPT_THREADS) void opt_sumsq_kernel(const OptTable t, double* __restrict__ partial) {
    __shared__ double wsum[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * OPT_CHUNK;
    const long long left = t.total - e0;                               // >= 1: the grid is the number of chunks
    const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const OptPointers c = opt_span(t, e0, len);
    double acc = 0.0;
    if (c.g) {                                                          // (workgroup-uniform)
        const bool al = eab_aligned16(c.g);
        for (int j = 0; j < OPT_QUADS; ++j) {
            float v[4];
            eab_load4(c.g, al, 4 * tid + 4 * OPT_THREADS * j, len, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += (double)v[k] * (double)v[k];
        }
    } else {                                                            // the chunk straddles segments: element by element
        for (int j = 0; j < OPT_QUADS; ++j)
            for (int k = 0; k < 4; ++k) {
                const int i = 4 * tid + 4 * OPT_THREADS * j + k;
                const float x = i < len ? *opt_span(t, e0 + i, 1).g : 0.0f;
                acc += (double)x * (double)x;
            }
    }
    const double s = opt_block_sum(acc, wsum, tid);
    if (tid == 0) partial[blockIdx.x] = s;
}

// With weight decay, g = c g0 + wd p is formed in fp64 and rounded once: where the two terms cancel, fp32 products would leave an
// error of eps (|c g0| + |wd p|), far above the contract's eps |g| (torch's own step is 6.5 units off there at 2.8 M elements).
__device__ __forceinline__ void opt_adam(float& p, float g0, float& m, float& v, double cd, const OptScalars& h) {
    float g = (float)cd * g0;                                           // c = 1 leaves g0 as it is
    if (h.weight_decay != 0.0) g = (float)(cd * (double)g0 + h.weight_decay * (double)p);
    m = m + (g - m) * h.w1;
    v = h.beta2 * v + h.w2 * g * g;
    const float denom = sqrtf(v) / h.bias2_sqrt + h.eps;
    p = p - h.step_size * (m / denom);
}

__global__ __launch_bounds__(OPT_THREADS) void opt_adam_kernel(const OptTable t, const OptScalars h, const double* __restrict__ partial,
                                                               long long npartial, double* __restrict__ norm_out) {
    __shared__ double wsum[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long k = tid; k < npartial; k += OPT_THREADS) acc += partial[k];
    const double norm = sqrt(opt_block_sum(acc, wsum, tid));
    if (blockIdx.x == 0 && tid == 0 && norm_out) *norm_out = norm;
    double cd = 1.0;
    if (h.max_norm > 0.0) {
        const double r = h.max_norm / (norm + 1e-6);
        cd = r < 1.0 ? r : (r != r ? r : 1.0);                          // min(1, r) that keeps a NaN
    }
    const long long e0 = (long long)blockIdx.x * OPT_CHUNK;
    const long long left = t.total - e0;
    if (left <= 0) return;                                              // (a table without elements: one workgroup, for the norm)
    const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const OptPointers q = opt_span(t, e0, len);
    if (q.g && eab_aligned16(q.g) && eab_aligned16(q.p) && eab_aligned16(q.m) && eab_aligned16(q.v)) {
        for (int j = 0; j < OPT_QUADS; ++j) {
            const int i = 4 * tid + 4 * OPT_THREADS * j;
            if (i + 4 <= len) {
                f32x4 p = *reinterpret_cast<const f32x4*>(q.p + i), m = *reinterpret_cast<const f32x4*>(q.m + i);
                f32x4 v = *reinterpret_cast<const f32x4*>(q.v + i);
                const f32x4 g = *reinterpret_cast<const f32x4*>(q.g + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pk = p[k], mk = m[k], vk = v[k];
                    opt_adam(pk, g[k], mk, vk, cd, h);
                    p[k] = pk; m[k] = mk; v[k] = vk;
                }
                *reinterpret_cast<f32x4*>(q.p + i) = p;
                *reinterpret_cast<f32x4*>(q.m + i) = m;
                *reinterpret_cast<f32x4*>(q.v + i) = v;
            } else {
                for (int k = i; k < len; ++k) opt_adam(q.p[k], q.g[k], q.m[k], q.v[k], cd, h);
            }
        }
    } else {                                                            // unaligned or straddling: lane after lane, coalesced
        for (int i = tid; i < len; i += OPT_THREADS) {
            const OptPointers r = q.g ? OptPointers{q.p + i, q.g + i, q.m + i, q.v + i} : opt_span(t, e0 + i, 1);
            opt_adam(*r.p, *r.g, *r.m, *r.v, cd, h);
        }
    }
}

// the checks of both entry points; fills the device table
static int opt_table(const eab_optim_segment* segs, int nseg, bool adam, OptTable& t) {
    EAB_CHECK_ARG(segs && nseg >= 1 && nseg <= EAB_OPTIM_MAX_SEGMENTS);
    long long total = 0;
    for (int s = 0; s < EAB_OPTIM_MAX_SEGMENTS; ++s) {
        t.start[s] = total;
        t.seg[s] = eab_optim_segment{nullptr, nullptr, nullptr, nullptr, 0};
        if (s >= nseg) continue;
        const eab_optim_segment& g = segs[s];
        EAB_CHECK_ARG(g.n >= 0 && g.n <= (long long)OPT_MAX_CHUNKS * OPT_CHUNK);
        if (g.n == 0) continue;
        EAB_CHECK_ARG(g.grad && (!adam || (g.param && g.exp_avg && g.exp_avg_sq)));
        t.seg[s] = g;
        if (!adam) t.seg[s].param = t.seg[s].exp_avg = t.seg[s].exp_avg_sq = nullptr;
        total += g.n;
    }
    t.start[EAB_OPTIM_MAX_SEGMENTS] = t.total = total;
    EAB_CHECK_ARG((total + OPT_CHUNK - 1) / OPT_CHUNK <= OPT_MAX_CHUNKS);
    return EAB_OK;
}

extern "C" int eab_grad_sumsq_f64(const eab_optim_segment* segs, int nseg, double* partial, long long partial_cap,
                                  eab_stream_t stream) {
    OptTable t;
    if (int rc = opt_table(segs, nseg, false, t)) return rc;
    const long long chunks = (t.total + OPT_CHUNK - 1) / OPT_CHUNK;
    EAB_CHECK_ARG(partial && partial_cap >= chunks);
    if (chunks == 0) return EAB_OK;
    hipLaunchKernelGGL(opt_sumsq_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, eab_stream(stream), t, partial);
    EAB_RETURN_LAUNCH_STATUS();
}

extern "C" int eab_adam_clip_f32(const eab_optim_segment* segs, int nseg, const double* partial, long long npartial,
                                 double max_norm, double step_size, double beta1, double beta2, double bias2_sqrt, double eps,
                                 double weight_decay, double* norm_out, eab_stream_t stream) {
    OptTable t;
    if (int rc = opt_table(segs, nseg, true, t)) return rc;
    EAB_CHECK_ARG(npartial >= 0 && npartial <= 4LL * OPT_MAX_CHUNKS && (partial || npartial == 0));
    const OptScalars h = {(float)step_size, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)bias2_sqrt, (float)eps,
                          weight_decay, max_norm};
    const long long chunks = (t.total + OPT_CHUNK - 1) / OPT_CHUNK;
    if (chunks == 0 && !norm_out) return EAB_OK;
    hipLaunchKernelGGL(opt_adam_kernel, dim3((unsigned)(chunks ? chunks : 1)), dim3(OPT_THREADS), 0, eab_stream(stream), t, h, partial,
                       npartial, norm_out);
    EAB_RETURN_LAUNCH_STATUS();
}
