"""videogpa_amd.vae on clips without a GPU: the frame batches of diffusers' `_encode`, which clip lengths are taken and which are refused, and the
C-ABI entries of the two new kernels (tests/test_cabi.py checks every prototype against the ctypes table and the library's exports)."""
import os
import re

import pytest
import torch

import vae_video_oracle as vv
from videogpa_amd.vae import AutoencoderKLCogVideoX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)

BATCHES = {
    1: [(0, 1)],
    5: [(0, 5)],
    9: [(0, 9)],
    13: [(0, 13)],
    17: [(0, 9), (9, 17)],
    21: [(0, 13), (13, 21)],
    49: [(0, 9), (9, 17), (17, 25), (25, 33), (33, 41), (41, 49)],
    81: [(0, 9)] + [(8 * i + 1, 8 * i + 9) for i in range(1, 10)],
}


@pytest.mark.parametrize("frames", sorted(BATCHES))
def test_frame_batches(frames):
    vae = AutoencoderKLCogVideoX(**NARROW)
    assert vae.num_sample_frames_batch_size == 8
    got = vae.frame_batches(frames)
    assert got == BATCHES[frames]
    assert got[0][0] == 0 and got[-1][1] == frames and all(a[1] == b[0] for a, b in zip(got, got[1:]))       # every frame once, in order
    # the oracle's loop, written as upstream's (ends past the clip are cut by the slice), covers the same frames
    assert [(s, min(e, frames)) for s, e in vv.frame_batches(frames)] == got
    # latent frames: the first batch keeps its first frame aside at both temporal poolings, the others halve twice
    pool = lambda t: (t + 1) // 2
    assert sum(pool(pool(e - s)) for s, e in got) == (frames - 1) // 4 + 1


def test_frame_batch_size_is_a_plain_attribute():
    vae = AutoencoderKLCogVideoX(**NARROW)
    vae.num_sample_frames_batch_size = 4
    assert vae.frame_batches(9) == [(0, 5), (5, 9)]


@pytest.mark.parametrize("frames", [2, 3, 4, 8, 50])
def test_other_clip_lengths_are_refused_by_name(frames):
    vae = AutoencoderKLCogVideoX(**NARROW).requires_grad_(False)
    with pytest.raises(NotImplementedError, match=rf"encode of {frames} frames"):
        vae.encode(torch.zeros(1, 3, frames, 16, 16))


def test_a_clip_on_the_cpu_is_refused():
    vae = AutoencoderKLCogVideoX(**NARROW).requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vae.encode(torch.zeros(1, 3, 5, 16, 16))


def test_new_entry_points_are_declared_bound_and_refuse_bad_arguments():
    from videogpa_amd import _lib
    header = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    for name in ("vgpa_conv3x3x3_causal_f32", "vgpa_vae_downsample_f32"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    lib = _lib.load()
    # VGPA_ERR_INVALID before any launch (no device is touched): null pointers, channels that are no multiple of 16, a misaligned cache, in place
    assert lib.vgpa_conv3x3x3_causal_f32(None, None, None, None, None, None, 1, 1, 4, 4, 16, 16, None) == -1
    assert lib.vgpa_conv3x3x3_causal_f32(4096, None, 8192, None, None, 16384, 1, 2, 4, 4, 24, 16, None) == -1
    assert lib.vgpa_conv3x3x3_causal_f32(4096, 4100, 8192, None, None, 16384, 1, 2, 4, 4, 16, 16, None) == -1
    assert lib.vgpa_conv3x3x3_causal_f32(4096, None, 8192, None, None, 4096, 1, 2, 4, 4, 16, 16, None) == -1
    assert lib.vgpa_conv3x3x3_causal_f32(4096, None, 8192, None, None, 16384, 1, 0, 4, 4, 16, 16, None) == -1
    assert lib.vgpa_vae_downsample_f32(None, None, None, None, 1, 1, 4, 4, 16, 16, 1, None) == -1
    assert lib.vgpa_vae_downsample_f32(4096, 8192, None, 16384, 1, 3, 1, 4, 16, 16, 1, None) == -1           # a one-row map
    assert lib.vgpa_vae_downsample_f32(4096, 8192, None, 16384, 1, 3, 4, 4, 16, 16, 2, None) == -1           # compress_time is 0 | 1
    assert lib.vgpa_vae_downsample_f32(4096, 8192, None, 16384, 1, 3, 4, 4, 16, 40, 1, None) == -1


def test_one_frame_does_not_build_the_three_dimensional_weights():
    """packed() (what the one-frame path and the trainer use) is not grown by the clip path: the 3-D weights are a cache entry of their own"""
    vae = AutoencoderKLCogVideoX(**NARROW)
    folded = vae.packed()
    assert tuple(folded["conv_in"][0].shape) == (3, 3, 16, 32) and "video" not in vae._packed._c
    video = vae.packed_video()
    assert tuple(video["conv_in"].shape) == (3, 3, 3, 16, 32) and not video["conv_in"][:, :, :, 3:].any()
    assert tuple(video["conv_out"].shape) == (3, 3, 3, 64, 32) and len(video["resnets"]) == 10
    assert torch.allclose(video["conv_out"].sum(dim=0), folded["conv_out"][0], rtol=1e-6, atol=1e-7)          # the fold is the sum over the temporal taps
