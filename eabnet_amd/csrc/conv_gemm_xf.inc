// conv_gemm_kernel: the (scale, shift, slope) tables of a fused transform -> LDS.  Included as text where the kernel fills them:
// at its start, or -- PATCH and LEAN gather pipelines -- behind the first loads of the tile.
    if (XF != EAB_XF_NONE) {
        // (scale, shift, slope) tables of this batch element -> LDS.  Either the host ran
        // eab_in_finalize_f32 (xf0/xf1) or the producer left few enough tiles that every
        // consumer workgroup reduces them itself (fin_stats; fp64, fixed order, so all
        // workgroups and the stand-alone kernel agree bit for bit).
        const int k = tid >> 7, c = tid & (CG_XFC - 1);
        const int Ck = (k == 0 || DUAL) ? d.C0 : d.C1;
        const float* xfk = k == 0 ? d.xf0 : d.xf1;
        const float* slk = k == 0 ? d.slope0 : d.slope1;
        float sc = 1.0f, sh = 0.0f, sl = 1.0f;
        if (c < Ck) {
            if (d.fin_stats && k < d.fin_nsets) {
                const float* gm = k == 0 ? d.fin_gamma0 : d.fin_gamma1;
                const float* bt = k == 0 ? d.fin_beta0 : d.fin_beta1;
                double sn = 0.0, sm = 0.0, sq = 0.0;            // same exact merge as in_finalize_kernel
                for (int t = 0; t < d.fin_tiles; ++t) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(
                        &d.fin_stats[((((size_t)b * d.fin_tiles + t) * d.fin_nsets + k) * d.C0 + c) * 4]);
                    const double n = (double)v[0], mu = (double)v[1];
                    sn += n;
                    sm = fma(n, mu, sm);
                    sq += fma(n * mu, mu, (double)v[2]);
                }
                const double mean = sn > 0.0 ? sm / sn : 0.0;
                double var = sn > 0.0 ? sq / sn - mean * mean : 0.0;
                if (var < 0.0) var = 0.0;
                const double scale = (double)gm[c] / sqrt(var + (double)d.fin_eps);
                sc = (float)scale;
                sh = (float)((double)bt[c] - mean * scale);
                sl = slk[c];
            } else if (xfk) {
                const float2 v = *reinterpret_cast<const float2*>(&xfk[((size_t)b * Ck + c) * 2]);
                sc = v.x;
                sh = v.y;
                sl = slk[c];
            }
        }
        sm.xft[k][c][0] = sc;
        sm.xft[k][c][1] = sh;
        sm.xsl[k][c] = sl;
    }
