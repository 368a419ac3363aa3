    // The body of istft_bwd_kernel<VARLEN> (LIN = false) and istft_lin_bwd_kernel<VARLEN> (LIN = true; reads `spec`), included by
    // istft.hip inside each kernel: see the comment above them.
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
        if (!LIN) {
            o0[k] = (E.x + wo.x) * sc;
            o1[k] = k == 0 ? 0.0f : (E.y + wo.y) * sc;
            if (twice) {
                o0[NH - k] = (E.x - wo.x) * sc;
                o1[NH - k] = k == 0 ? 0.0f : (wo.y - E.y) * sc;
            }
        } else {
            const float* s0 = spec + ((size_t)b * 2 * T + t0 + c) * F;   // the frame's row of `spec`: real parts, imaginary T*F on
            const float* s1 = s0 + (size_t)T * F;
            const float2 dk = istft_decompress_bwd(make_float2(s0[k], s1[k]),
                                                   make_float2((E.x + wo.x) * sc, k == 0 ? 0.0f : (E.y + wo.y) * sc));
            o0[k] = dk.x;
            o1[k] = dk.y;
            if (twice) {
                const float2 dm = istft_decompress_bwd(make_float2(s0[NH - k], s1[NH - k]),
                                                       make_float2((E.x - wo.x) * sc, k == 0 ? 0.0f : (wo.y - E.y) * sc));
                o0[NH - k] = dm.x;
                o1[NH - k] = dm.y;
            }
        }
    }
