// Host stand-in for <hip/hip_runtime.h>, enough to run csrc/stoi.hip and csrc/score.hip on the CPU (tests/test_*_host_emulation.py): one
// std::thread per lane of a workgroup, workgroups one after the other, __syncthreads and the wave operations through pthread
// barriers.  Valid for kernels whose returns are workgroup-uniform and whose wave operations sit in wave-uniform control flow.
// __shared__ becomes a function-local static: correct because only one workgroup runs at a time.
#pragma once
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)

struct float2 { float x, y; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
typedef void* hipStream_t;
typedef int hipError_t;
#define hipSuccess 0
static inline hipError_t hipGetLastError() { return hipSuccess; }

struct ShimWorkgroup {
    pthread_barrier_t all, wave[16];
    double slot[1024];
    int pred[1024];
};
extern thread_local dim3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;
extern ShimWorkgroup shim;
void shim_launch(dim3 grid, dim3 block, std::function<void()> fn);
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) shim_launch(grid, block, [=] { kernel(__VA_ARGS__); })

static inline void __syncthreads() { pthread_barrier_wait(&shim.all); }
static inline double __shfl_down(double v, int off, int) {
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    shim.slot[t] = v;
    pthread_barrier_wait(&shim.wave[w]);
    const double r = l + off < 64 ? shim.slot[t + off] : v;
    pthread_barrier_wait(&shim.wave[w]);
    return r;
}
static inline unsigned long long __ballot(int p) {
    const int t = threadIdx.x, w = t >> 6;
    shim.pred[t] = p != 0;
    pthread_barrier_wait(&shim.wave[w]);
    unsigned long long r = 0;
    for (int l = 0; l < 64; ++l) r |= (unsigned long long)shim.pred[64 * w + l] << l;
    pthread_barrier_wait(&shim.wave[w]);
    return r;
}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline double cospi(double x) { return std::cos(M_PI * x); }
static inline double sinpi(double x) { return std::sin(M_PI * x); }
using std::max;
using std::min;
