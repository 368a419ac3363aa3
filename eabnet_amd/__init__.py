"""eabnet_amd -- MI355X (gfx950) implementation of EaBNet's per-frame causal
beamforming hot path behind the reference's Python call surface.

    from eabnet_amd import EaBNet, prepare_data, numParams, com_mag_mse_loss

Importing the package does not touch the GPU; the HIP library
(eabnet_amd/lib/libeabnet_hip.so) is loaded on first use and its absence is an
error, never a fallback.
"""
from .spec import GagConfig, NetConfig, gag_param_specs, param_specs  # noqa: F401
from .model import (EaBNet, GaGNet, EaBNetWithPostNet, make_gag_net, make_eabnet_with_postnet,  # noqa: F401
                    StreamingEnhancer, Pipeline, prepare_data, stft_compress, istft, filter_and_sum, numParams, com_mag_mse_loss,
                    stagewise_com_mag_mse_loss, eabnet_with_postnet_loss)
from .enhance import Enhancer, plan_batches  # noqa: F401
from .score import Scorer, energy_ratios, com_mag_mse_loss_per_utterance, intelligibility, stoi, sdr  # noqa: F401
from .resample import resample, resampled_length, filter_bank, StreamResampler  # noqa: F401
from .simulate import (Scene, RoomSimulator, inverse_sabine, rir_length, sample_scene, image_source_rirs, mix_gains,  # noqa: F401
                       simulate_rooms)
from .optim import FlatAdam  # noqa: F401
from .wave import mr_stft_loss, sdr_loss, si_sdr_loss, stoi_loss  # noqa: F401

__all__ = ["EaBNet", "GaGNet", "EaBNetWithPostNet", "make_gag_net", "make_eabnet_with_postnet", "StreamingEnhancer", "Pipeline", "Enhancer", "plan_batches", "Scorer", "energy_ratios",
           "com_mag_mse_loss_per_utterance", "intelligibility", "stoi", "sdr", "resample", "resampled_length", "filter_bank", "StreamResampler",
           "Scene", "RoomSimulator", "inverse_sabine", "rir_length", "sample_scene", "image_source_rirs", "mix_gains", "simulate_rooms",
           "FlatAdam", "si_sdr_loss", "mr_stft_loss", "stoi_loss", "sdr_loss", "prepare_data",
           "stft_compress", "istft", "filter_and_sum", "numParams", "com_mag_mse_loss", "stagewise_com_mag_mse_loss",
           "eabnet_with_postnet_loss",
           "NetConfig", "GagConfig", "param_specs", "gag_param_specs"]
