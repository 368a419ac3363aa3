"""The refusals of ``si_sdr_loss``, ``mr_stft_loss`` and ``stoi_loss`` -- exception type, full message and which one fires first for
a call that is wrong in two ways -- as they were before the argument front of the three moved into ``eabnet_amd/_rows.py``.  Every
check up to the CUDA one runs on CPU tensors: no GPU needed.  The expected strings are what the commit before that move raised for
the same table; they are literals here, never taken from the code under test."""
import pytest
import torch

from eabnet_amd import wave
from eabnet_amd._lib import EabError

B, L = 2, 40
CALLS = {"si_sdr_loss": (wave.si_sdr_loss, {}),
         "mr_stft_loss": (wave.mr_stft_loss, {"resolutions": ((16, 4, 16),)}),        # max n_fft / 2 + 1 = 9 <= L
         "stoi_loss": (wave.stoi_loss, {})}


def _w(*shape, dtype=torch.float32):
    return torch.zeros(shape or (B, L), dtype=dtype)


# row -> (est, clean, keywords); a fresh call's arguments every time
ROWS = {
    "reduction": lambda: (_w(), _w(), {"reduction": "avg"}),
    "est_1d": lambda: (_w(L), _w(), {}),
    "clean_rows": lambda: (_w(), _w(B + 1, L), {}),
    "est_fp64": lambda: (_w(dtype=torch.float64), _w(), {}),
    "clean_requires_grad": lambda: (_w(), _w().requires_grad_(), {}),
    "lengths_count": lambda: (_w(), _w(), {"lengths": [10, 20, 30]}),
    "lengths_b3": lambda: (_w(), _w(), {"lengths": torch.full((B, 3), 10, dtype=torch.int64)}),
    "lengths_float": lambda: (_w(), _w(), {"lengths": torch.tensor([10.0, 20.0])}),
    "length_above_row": lambda: (_w(), _w(), {"lengths": [10, L + 1]}),
    "mixed_pairs": lambda: (_w(), _w(), {"lengths": [(10, 10), 20]}),
    "cpu": lambda: (_w(), _w(), {"lengths": [10, L]}),
    "reduction_and_shape": lambda: (_w(L), _w(), {"reduction": "avg"}),
    "dtype_and_lengths": lambda: (_w(dtype=torch.float64), _w(), {"lengths": [10, L + 1]}),
}
NOT_FOR = {"mr_stft_loss": ("lengths_b3", "mixed_pairs")}         # it takes (B,) counts only: no (B, 2) spelling to get wrong

EXPECTED = {
    ('si_sdr_loss', 'reduction'): (ValueError,
        "reduction must be one of ('mean', 'sum', 'none'), got 'avg'"),
    ('si_sdr_loss', 'est_1d'): (ValueError,
        'est must be a (B, L) tensor (clean may be (B, 1, L)), got (40,)'),
    ('si_sdr_loss', 'clean_rows'): (ValueError,
        'est and clean must hold the same number of rows, got 2 and 3'),
    ('si_sdr_loss', 'est_fp64'): (TypeError,
        'si_sdr_loss takes fp32 waves, got torch.float64 and torch.float32 (there is no operator fallback)'),
    ('si_sdr_loss', 'clean_requires_grad'): (NotImplementedError,
        'si_sdr_loss is differentiable with respect to est only: clean requires grad (detach it; there is no operator fallback)'),
    ('si_sdr_loss', 'lengths_count'): (ValueError,
        'lengths must hold 2 values (one per utterance), got 3'),
    ('si_sdr_loss', 'lengths_b3'): (ValueError,
        'lengths must have shape (2,) or (2, 2), got (2, 3)'),
    ('si_sdr_loss', 'lengths_float'): (ValueError,
        'lengths must be integers, got torch.float32'),
    ('si_sdr_loss', 'length_above_row'): (ValueError,
        "lengths must lie in [1, 40] (the signal's row length), got [41]"),
    ('si_sdr_loss', 'mixed_pairs'): (ValueError,
        'lengths must be integers, got [(10, 10), 20]'),
    ('si_sdr_loss', 'cpu'): (EabError,
        'si_sdr_loss needs CUDA (ROCm) tensors; there is no CPU fallback by design.'),
    ('si_sdr_loss', 'reduction_and_shape'): (ValueError,
        "reduction must be one of ('mean', 'sum', 'none'), got 'avg'"),
    ('si_sdr_loss', 'dtype_and_lengths'): (TypeError,
        'si_sdr_loss takes fp32 waves, got torch.float64 and torch.float32 (there is no operator fallback)'),
    ('mr_stft_loss', 'reduction'): (ValueError,
        "reduction must be one of ('mean', 'sum', 'none'), got 'avg'"),
    ('mr_stft_loss', 'est_1d'): (ValueError,
        'est must be a (B, L) tensor (clean may be (B, 1, L)), got (40,)'),
    ('mr_stft_loss', 'clean_rows'): (ValueError,
        'est and clean must hold the same number of rows, got 2 and 3'),
    ('mr_stft_loss', 'est_fp64'): (TypeError,
        'mr_stft_loss takes fp32 waves, got torch.float64 and torch.float32 (there is no operator fallback)'),
    ('mr_stft_loss', 'clean_requires_grad'): (NotImplementedError,
        'mr_stft_loss is differentiable with respect to est only: clean requires grad (detach it; there is no operator fallback)'),
    ('mr_stft_loss', 'lengths_count'): (ValueError,
        'lengths must hold 2 values (one per utterance), got 3'),
    ('mr_stft_loss', 'lengths_float'): (ValueError,
        'lengths must be integers, got torch.float32'),
    ('mr_stft_loss', 'length_above_row'): (ValueError,
        'lengths must lie in [9, 40] (max n_fft / 2 < samples <= min(Le, Ls)), got [41]'),
    ('mr_stft_loss', 'cpu'): (EabError,
        'mr_stft_loss needs CUDA (ROCm) tensors; there is no CPU fallback by design.'),
    ('mr_stft_loss', 'reduction_and_shape'): (ValueError,
        "reduction must be one of ('mean', 'sum', 'none'), got 'avg'"),
    ('mr_stft_loss', 'dtype_and_lengths'): (TypeError,
        'mr_stft_loss takes fp32 waves, got torch.float64 and torch.float32 (there is no operator fallback)'),
    ('stoi_loss', 'reduction'): (ValueError,
        "reduction must be one of ('mean', 'sum', 'none'), got 'avg'"),
    ('stoi_loss', 'est_1d'): (ValueError,
        'est must be a (B, L) tensor (clean may be (B, 1, L)), got (40,)'),
    ('stoi_loss', 'clean_rows'): (ValueError,
        'est and clean must hold the same number of rows, got 2 and 3'),
    ('stoi_loss', 'est_fp64'): (TypeError,
        'stoi_loss takes fp32 waves, got torch.float64 and torch.float32 (there is no operator fallback)'),
    ('stoi_loss', 'clean_requires_grad'): (NotImplementedError,
        'stoi_loss is differentiable with respect to est only: clean requires grad (detach it; there is no operator fallback)'),
    ('stoi_loss', 'lengths_count'): (ValueError,
        'lengths must hold 2 values (one per utterance), got 3'),
    ('stoi_loss', 'lengths_b3'): (ValueError,
        'lengths must have shape (2,) or (2, 2), got (2, 3)'),
    ('stoi_loss', 'lengths_float'): (ValueError,
        'lengths must be integers, got torch.float32'),
    ('stoi_loss', 'length_above_row'): (ValueError,
        "lengths must lie in [1, 40] (the signal's row length), got [41]"),
    ('stoi_loss', 'mixed_pairs'): (ValueError,
        'lengths must be integers, got [(10, 10), 20]'),
    ('stoi_loss', 'cpu'): (EabError,
        'stoi_loss needs CUDA (ROCm) tensors; there is no CPU fallback by design.'),
    ('stoi_loss', 'reduction_and_shape'): (ValueError,
        "reduction must be one of ('mean', 'sum', 'none'), got 'avg'"),
    ('stoi_loss', 'dtype_and_lengths'): (TypeError,
        'stoi_loss takes fp32 waves, got torch.float64 and torch.float32 (there is no operator fallback)'),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_the_refusals_of_the_wave_losses_did_not_move(name):
    fn, kw = CALLS[name]
    rows = [r for r in ROWS if r not in NOT_FOR.get(name, ())]
    assert sorted(r for n, r in EXPECTED if n == name) == sorted(rows)
    for row in rows:
        est, clean, more = ROWS[row]()
        kind, message = EXPECTED[name, row]
        with pytest.raises(Exception) as info:
            fn(est, clean, **kw, **more)
        assert (type(info.value), str(info.value)) == (kind, message), (name, row)
