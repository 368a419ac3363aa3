// Stand-alone driver of the host emulation of csrc/gag.hip: eab_gag_pack_f32, eab_gag_crm_f32 and eab_gag_crm_bwd_lens_f32 under
// per-utterance lengths, every array allocated at EXACTLY its size (16-byte aligned, as the arenas are), so that AddressSanitizer
// sees any access outside one; the outputs start from a sentinel, so a write to a padding frame shows in the file.
//   gag_emulation IN OUT
// IN:  int32 [7] B T F ld lin_ld act use_lens, int32 [B] lens, then the fp32 arrays
//      inpt [B][2][T][F], pre_x [B][2][T][F]                                        (pack)
//      pre [B][T][ld], g, r, i [B][T][lin_ld]                                       (crm)
//      dplanar [B][2][T][F], dpre_out [B][T][ld], acc_in [B][T][ld]                 (crm backward, on the same pre and g)
// OUT: the fp32 arrays enc_in [B][T][F][4], pre (pack) [B][T][ld], pre_out [B][T][ld], planar [B][2][T][F],
//      dg, dr, di [B][T][lin_ld], dpre [B][T][ld]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eabnet_hip.h"

#define SENTINEL 7.25f

// the device's fast exponential (gag_act): glibc declares the name and does not export it
extern "C" float __expf(float x) noexcept { return expf(x); }

static float* exact(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, n * sizeof(float))) exit(2);
    return static_cast<float*>(p);
}

static float* read_array(FILE* f, size_t n) {
    float* p = exact(n);
    if (fread(p, 4, n, f) != n) exit(2);
    return p;
}

static float* fresh(size_t n) {
    float* p = exact(n);
    for (size_t k = 0; k < n; ++k) p[k] = SENTINEL;
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h[7];
    if (fread(h, 4, 7, f) != 7) return 2;
    const int B = h[0], T = h[1], F = h[2], ld = h[3], lin = h[4], act = h[5], use_lens = h[6];
    if (B < 1 || B > 64 || T < 1 || F < 1) return 2;
    int32_t* lens = static_cast<int32_t*>(malloc(sizeof(int32_t) * B));           // exactly B counts
    if (fread(lens, 4, B, f) != (size_t)B) return 2;
    const size_t planar = (size_t)B * 2 * T * F, rows = (size_t)B * T;
    float* inpt = read_array(f, planar);
    float* pre_x = read_array(f, planar);
    float* pre = read_array(f, rows * ld);
    float* g = read_array(f, rows * lin);
    float* r = read_array(f, rows * lin);
    float* im = read_array(f, rows * lin);
    float* dplanar = read_array(f, planar);
    float* dpre_out = read_array(f, rows * ld);
    float* acc_in = read_array(f, rows * ld);
    fclose(f);
    float* enc_in = fresh(rows * F * 4);
    float* pre_p = fresh(rows * ld);
    float* pre_out = fresh(rows * ld);
    float* pl = fresh(planar);
    float* dg = fresh(rows * lin);
    float* dr = fresh(rows * lin);
    float* di = fresh(rows * lin);
    float* dpre = fresh(rows * ld);
    const eab_time_window win{nullptr, 0, use_lens ? lens : nullptr};
    int rc = eab_gag_pack_f32(inpt, pre_x, enc_in, pre_p, B, T, F, ld, win, nullptr);
    if (!rc) rc = eab_gag_crm_f32(pre, g, r, im, pre_out, pl, B, T, F, ld, lin, act, win, nullptr);
    if (!rc) rc = eab_gag_crm_bwd_lens_f32(pre, g, dplanar, dpre_out, acc_in, dg, dr, di, dpre, B, T, F, ld, lin, act,
                                           use_lens ? lens : nullptr, nullptr);
    if (rc) {
        printf("gag entry point returned %d\n", rc);
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(enc_in, 4, rows * F * 4, o);
    fwrite(pre_p, 4, rows * ld, o);
    fwrite(pre_out, 4, rows * ld, o);
    fwrite(pl, 4, planar, o);
    fwrite(dg, 4, rows * lin, o);
    fwrite(dr, 4, rows * lin, o);
    fwrite(di, 4, rows * lin, o);
    fwrite(dpre, 4, rows * ld, o);
    fclose(o);
    float* all[] = {inpt, pre_x, pre, g, r, im, dplanar, dpre_out, acc_in, enc_in, pre_p, pre_out, pl, dg, dr, di, dpre};
    for (float* p : all) free(p);
    free(lens);
    return 0;
}
