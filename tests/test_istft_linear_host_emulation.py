"""The linear-domain back end of csrc/istft.hip (eab_istft_lin_f32, eab_istft_lin_bwd_f32), compiled for the HOST against
tests/hip_host_shim (one thread per lane, pthread barriers) into a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer, and run as a child process: the same source the GPU runs, checked for accesses past a row (the arrays
are allocated at their exact sizes), for reads behind a length (NaN there, in the spectrum and in the wave gradient), and against
the float64 restatement of tests/istft_lin_ref.py.  No GPU needed; the compiler is the one that builds the library.

Bound: 1e-5 of max |ref| on the wave and on the gradient (tests/test_istft_linear_gpu.py)."""
import struct

import numpy as np
import pytest

import host_emulation
import istft_lin_ref as R

TOL = 1e-5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_emulation.build(tmp_path_factory, "istft_lin")


@pytest.mark.parametrize("n_fft,hop,win,T,lens", [(320, 160, 320, 9, [9, 4]), (256, 64, 200, 5, [5, 3])])
def test_linear_istft_and_adjoint_on_the_host_match_the_restatement_and_stay_in_bounds(program, tmp_path, n_fft, hop, win, T, lens):
    B, F = len(lens), n_fft // 2 + 1
    spec, dwav, window, zero = R.make_case(n_fft, hop, win, T, B)
    assert zero[1] < lens[zero[0]], "the zero bin lies inside its utterance"
    for with_lens in (False, True):
        s, d = spec.copy(), dwav.copy()
        if with_lens:
            for b, n in enumerate(lens):
                s[b, :, n:] = np.nan                              # never read
                d[b, hop * (n - 1):] = np.nan
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("5i", B, T, n_fft, hop, int(with_lens)))
            f.write(struct.pack(f"{B}i", *lens))
            f.write(window.tobytes())
            f.write(s.tobytes())
            f.write(d.tobytes())
        host_emulation.run(program, src, dst)                     # a sanitizer report is a non-zero exit status
        raw = np.fromfile(dst, np.float32)
        wav, grad = raw[:dwav.size].reshape(dwav.shape), raw[dwav.size:].reshape(B, 2, T, F)
        use = lens if with_lens else None
        want_wav, want_grad = R.istft(s, window, n_fft, hop, use), R.istft_bwd(d, s, window, n_fft, hop, use)
        assert np.isfinite(wav).all() and np.isfinite(grad).all(), "an element was not written, or a NaN behind a length was read"
        ew = np.abs(wav - want_wav).max() / np.abs(want_wav).max()
        eg = np.abs(grad - want_grad).max() / np.abs(want_grad).max()
        print(f"({n_fft},{hop},{win},{T}) lens={with_lens}: wave {ew:.2e}, gradient {eg:.2e} of max |ref| (bound {TOL:.0e})")
        assert ew <= TOL and eg <= TOL
        assert (grad[zero[0], :, zero[1], zero[2]] == 0).all(), "the gradient at a zero bin is exactly zero"
        if with_lens:
            for b, n in enumerate(lens):
                assert (wav[b, hop * (n - 1):] == 0).all() and (grad[b, :, n:] == 0).all(), b
