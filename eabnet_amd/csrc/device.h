// Device-only helpers shared by the kernels: vector types and the few functions built on gfx950 builtins.  Kept apart from
// common.h because the files that also compile as host C++ (stoi.hip, score.hip; tests/hip_host_shim) cannot parse the builtins.
// eab_sigmoid / eab_tanh of common.h are the IEEE-division forms and are NOT these.
#pragma once
#include "common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 h16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// Byte offset outside every legal tensor: the host side of every entry point checks that a tensor (one batch element of it, where
// the resource is rebased per element) is shorter than 2^31 bytes, so a raw buffer load at this offset gives 0 and a store is dropped.
#define EAB_OOB 0x80000000u

// sigmoid / tanh on the hardware exp and rcp (1 ulp class): abs error ~2e-7, three orders of magnitude inside the 1e-4 parity bar,
// and short enough to hide under MFMAs.
__device__ __forceinline__ float eab_fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float eab_fast_tanh(float x) { return fmaf(2.0f, eab_fast_sigmoid(2.0f * x), -1.0f); }

// sum over the 16 lanes of a DPP row; every lane ends with the total
__device__ __forceinline__ float eab_row_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    return v;
}

// two fp32 -> packed bf16, round to nearest even (v_cvt_pk_bf16_f32): the rounding the bf16 contractions apply to their operands
__device__ __forceinline__ unsigned eab_bf2(float x0, float x1) {
    const bf16x2 v = {(__bf16)x0, (__bf16)x1};
    return __builtin_bit_cast(unsigned, v);
}

// x = hi + lo with hi = x truncated to fp16 and lo = fp16(x - hi), two elements at a time
// (v_cvt_pkrtz_f16_f32; fp16 subnormals are honoured by the f16 MFMA, probed on gfx950).
__device__ __forceinline__ void eab_split2(float x0, float x1, unsigned& hi, unsigned& lo) {
    const h16x2 h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
    const h16x2 l = __builtin_amdgcn_cvt_pkrtz(x0 - (float)h[0], x1 - (float)h[1]);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}

// fused source transform of four channels: InstanceNorm affine and PReLU in the order XF names
template <int XF>
__device__ __forceinline__ f32x4 eab_xform(f32x4 v, f32x4 sh01, f32x4 sh23, f32x4 sl) {
    // sh01 = (scale0, shift0, scale1, shift1), sh23 likewise for channels 2,3
    const float sc[4] = {sh01[0], sh01[2], sh23[0], sh23[2]};
    const float sf[4] = {sh01[1], sh01[3], sh23[1], sh23[3]};
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (XF == EAB_XF_NORM_PRELU)
            r[j] = eab_prelu(fmaf(v[j], sc[j], sf[j]), sl[j]);
        else
            r[j] = fmaf(eab_prelu(v[j], sl[j]), sc[j], sf[j]);
    }
    return r;
}

// q / n for 0 <= q < 2^22 via the fp32 reciprocal, exact after one correction
__device__ __forceinline__ int eab_div(int q, int n, float inv_n) {
    int t = (int)((float)q * inv_n);
    if (t * n > q) --t;
    if ((t + 1) * n <= q) ++t;
    return t;
}
