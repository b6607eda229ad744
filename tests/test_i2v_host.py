"""The image-to-video path without a GPU: the DDIM scheduler and both schedulers' step_coefficients in fp64, and the resize restatement
(tests/resize_ref.py) against PIL itself.  The C ABI side (header, ctypes table and exports extended together) is tests/test_cabi.py, unchanged."""
import numpy as np
import pytest
import torch

import i2v_ref
import resize_ref
from oracle import scheduler as osch
from videogpa_amd.scheduler import CogVideoXDDIMScheduler, CogVideoXDPMScheduler


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("steps", [6, 50])
def test_ddim_trailing_timesteps_match_the_oracle(steps):
    sch = CogVideoXDDIMScheduler(timestep_spacing="trailing")
    sch.set_timesteps(steps)
    assert sch.timesteps.tolist() == osch.trailing_timesteps(steps).tolist() == sch.timesteps_host
    assert torch.equal(sch.alphas_cumprod, osch.alphas_cumprod())
    assert torch.equal(sch.alphas_cumprod, CogVideoXDPMScheduler().alphas_cumprod)
    x = _rand((2, 3), 0)
    assert sch.scale_model_input(x, 5) is x and sch.init_noise_sigma == 1.0


def test_ddim_leading_and_linspace_spacings():
    sch = CogVideoXDDIMScheduler(timestep_spacing="leading")
    sch.set_timesteps(5)
    assert sch.timesteps.tolist() == [800, 600, 400, 200, 0]
    sch = CogVideoXDDIMScheduler(timestep_spacing="linspace")
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == [999, 666, 333, 0]
    sch = CogVideoXDDIMScheduler.from_config(dict(CogVideoXDPMScheduler().config), timestep_spacing="trailing")
    assert sch.config.timestep_spacing == "trailing" and sch.config.set_alpha_to_one is True


@pytest.mark.parametrize("steps", [6, 50])
def test_ddim_step_matches_the_textbook_form(steps):
    sch = CogVideoXDDIMScheduler()
    sch.set_timesteps(steps)
    abar = osch.alphas_cumprod()
    for i, t in enumerate(sch.timesteps_host):
        x, v = _rand((2, 3, 4), 10 + i), _rand((2, 3, 4), 100 + i)
        prev, x0 = sch.step(v, t, x)
        ref_prev, ref_x0 = i2v_ref.ddim_textbook_step(abar, v, t, x, steps)
        assert prev.dtype == torch.float64 and torch.isfinite(prev).all()
        assert (prev - ref_prev).abs().max().item() < 1e-12 and (x0 - ref_x0).abs().max().item() < 1e-12, (steps, i)


def test_ddim_step_edges():
    sch = CogVideoXDDIMScheduler()
    sch.set_timesteps(50)
    # zero terminal SNR: a_999 = 0 exactly, and the first step stays finite (x0 = -v, the sample only enters through sqrt(1 - a_prev))
    assert sch.timesteps_host[0] == 999 and float(sch.alphas_cumprod[999]) == 0.0
    x, v = _rand((1, 2, 4, 4, 4), 1), _rand((1, 2, 4, 4, 4), 2)
    prev, x0 = sch.step(v, 999, x)
    assert torch.isfinite(prev).all() and torch.equal(x0, -v)
    # a perfect denoiser is a fixed point of the last step (prev_t < 0: a_prev = 1)
    assert sch.timesteps_host[-1] == 19
    x0t, e = _rand((1, 2, 4, 4, 4), 3), _rand((1, 2, 4, 4, 4), 4)
    a = sch.alphas_cumprod[19]
    xt, vv = a.sqrt() * x0t + (1 - a).sqrt() * e, a.sqrt() * e - (1 - a).sqrt() * x0t
    prev, px0 = sch.step(vv, 19, xt)
    assert torch.allclose(px0, x0t, atol=1e-9) and torch.allclose(prev, x0t, atol=1e-9)
    # set_alpha_to_one=False ends on a_0 instead
    other = CogVideoXDDIMScheduler(set_alpha_to_one=False)
    other.set_timesteps(50)
    assert float(other.final_alpha_cumprod) == float(other.alphas_cumprod[0]) < 1.0
    assert not torch.allclose(other.step(vv, 19, xt)[0], prev, atol=1e-9)
    with pytest.raises(NotImplementedError, match="eta"):
        sch.step(vv, 19, xt, eta=0.5)
    # the sample dtype comes back
    assert sch.step(vv.float(), 19, xt.float())[0].dtype == torch.float32


def _apply(coef, x, v, old, noise):
    x0 = coef["sa"] * x - coef["sb"] * v
    out = coef["k_x"] * x + coef["k_0"] * x0
    if coef["k_old"] is not None:
        out = out + coef["k_old"] * old
    if coef["k_n"] is not None:
        out = out + coef["k_n"] * noise
    return out, x0


@pytest.mark.parametrize("steps", [6, 50])
def test_step_coefficients_reproduce_step_at_every_index(steps):
    """both schedulers, every index: the first step (no history, a_t = 0), the step behind it (history from the zero-SNR step: r = inf) and the last one
    (prev_t < 0 at 50 steps: first order again)"""
    ddim, dpm = CogVideoXDDIMScheduler(), CogVideoXDPMScheduler()
    ddim.set_timesteps(steps)
    dpm.set_timesteps(steps)
    ts = dpm.timesteps_host
    old = None
    saw_first_order_last = False
    for i, t in enumerate(ts):
        x, v, noise = _rand((2, 5), 20 + i), _rand((2, 5), 200 + i), _rand((2, 2, 5), 2000 + i)
        c = ddim.step_coefficients(i)
        assert c["k_old"] is None and c["k_n"] is None
        got, got0 = _apply(c, x, v, None, None)
        want, want0 = ddim.step(v, t, x)
        assert (got - want).abs().max().item() < 1e-12 and (got0 - want0).abs().max().item() < 1e-12, ("ddim", i)
        c = dpm.step_coefficients(i)
        second = c["k_old"] is not None
        assert second == (i > 0 and t - 1000 // steps >= 0)
        saw_first_order_last |= (i == len(ts) - 1 and not second)
        got, got0 = _apply(c, x, v, old, noise[1 if second else 0])
        want, want0 = dpm.step(v, old, t, ts[i - 1] if i > 0 else None, x, noise=noise)
        assert torch.isfinite(got).all()
        assert (got - want).abs().max().item() < 1e-12 and (got0 - want0).abs().max().item() < 1e-12, ("dpm", i)
        old = want0
    assert saw_first_order_last == (steps == 50)


@pytest.mark.parametrize("filter", ["bicubic", "lanczos"])
@pytest.mark.parametrize("src,dst", resize_ref.SIZES)
def test_resize_restatement_equals_pil(filter, src, dst):
    Image = pytest.importorskip("PIL.Image")
    img = resize_ref.test_image(*src)
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), getattr(Image.Resampling, filter.upper())))
    got = resize_ref.resize(img, dst[0], dst[1], filter)
    assert got.shape == want.shape == (dst[0], dst[1], 3) and np.array_equal(got, want), int((got.astype(int) - want).__abs__().max())


def test_resize_restatement_is_pil_default_and_identity():
    Image = pytest.importorskip("PIL.Image")
    img = resize_ref.test_image(37, 53)
    # PIL's default filter of Image.resize is bicubic (replicate.py:201 relies on it); an unchanged size is a copy
    assert np.array_equal(np.asarray(Image.fromarray(img).resize((64, 48))), resize_ref.resize(img, 48, 64, "bicubic"))
    assert np.array_equal(resize_ref.resize(img, 37, 53, "lanczos"), img)
    assert not np.array_equal(resize_ref.resize(img, 48, 64, "bicubic"), resize_ref.resize(img, 48, 64, "lanczos"))
