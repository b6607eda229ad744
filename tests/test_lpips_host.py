"""videogpa_amd.lpips.LPIPS without a GPU: the constructor's contract, upstream's state-dict forms, the restatement's own sanity (tests/lpips_ref.py)
and the C ABI table.

The restatement's fp32 evaluation gives d32 of tests/test_gpu_lpips.py.  Its bounds here come from the number format, not from a run: a scalar output is
one fp32 number whose terms were summed in fp32, so it sits within 8 * 2^-24 of the fp64 answer (half an ulp is 2^-24 relative; the sums over <= 512 channels
and <= 4270 pixels are random walks of a few ulps); a feature map is thirteen fp32 convolutions deep with K <= 9 * 512 products each, a random walk of
sqrt(4608) * 2^-24 = 4e-6 at the very most relative to the map's maximum, observed an order below."""
import pytest
import torch

import lpips_ref as R


def fresh(**kw):
    from videogpa_amd.lpips import LPIPS
    return LPIPS(pretrained=False, pnet_rand=True, **kw)


def packed_equal(a, b):
    ca, la, fa = a.packed()
    cb, lb, fb = b.packed()
    assert fa == fb
    assert all(torch.equal(x, y) for x, y in zip(la, lb)) and len(la) == len(lb) == 5
    for ra, rb in zip(ca, cb):
        for (wa, ba), (wb, bb) in zip(ra, rb):
            assert torch.equal(wa, wb) and torch.equal(ba, bb)


def test_constructor_rejects_what_is_not_built():
    from videogpa_amd import lpips
    with pytest.raises(NotImplementedError, match="net"):
        lpips.LPIPS(net="alex", pretrained=False, pnet_rand=True)
    with pytest.raises(NotImplementedError, match="spatial"):
        lpips.LPIPS(net="vgg", spatial=True, pretrained=False, pnet_rand=True)
    with pytest.raises(NotImplementedError, match="version"):
        lpips.LPIPS(version="0.0", pretrained=False, pnet_rand=True)
    with pytest.raises(NotImplementedError, match="lpips"):
        lpips.LPIPS(lpips=False, pretrained=False, pnet_rand=True)
    with pytest.raises(RuntimeError, match=r"vgg\.pth.*vgg16"):
        lpips.LPIPS(net="vgg")                                        # pretrained=True without paths: names both files, never a silent random init
    with pytest.raises(RuntimeError, match="vgg16"):
        lpips.LPIPS(pretrained=False)                                 # upstream keeps the trained backbone here: it needs the file too
    m = lpips.LPIPS(net="vgg16", pretrained=False, pnet_rand=True)
    assert not any(p.requires_grad for p in m.parameters()) and not m.training


def test_seeded_random_init_is_reproducible_and_packs_conv1_1_to_16_channels():
    a, b = fresh(), fresh(frames_chunk=1)
    packed_equal(a, b)
    convs, lins, (shift, scale) = a.packed()
    assert [len(r) for r in convs] == [2, 2, 3, 3, 3]
    assert tuple(convs[0][0][0].shape) == (3, 3, 16, 64) and float(convs[0][0][0][:, :, 3:].abs().max()) == 0.0
    assert tuple(convs[4][2][0].shape) == (3, 3, 512, 512) and [l.numel() for l in lins] == list(R.CHNS)
    assert shift == pytest.approx((-.030, -.088, -.188)) and scale == pytest.approx((.458, .448, .450))
    assert a.packed() is a.packed()                                   # packed once ...
    old = a.packed()
    want = 2 * lins[0]
    with torch.no_grad():
        a.lins[0].model[1].weight.mul_(2.0)
    assert a.packed() is not old and torch.equal(a.packed()[1][0], want)                 # ... and again when a parameter changes


def test_state_dict_keys_are_upstreams_and_both_forms_round_trip(tmp_path):
    sd = R.make_state_dict(3)
    want = fresh()
    assert set(want.state_dict()) == set(sd)                          # the module's own names are upstream's full form, duplicates included
    assert all(want.state_dict()[k].shape == v.shape for k, v in sd.items())
    want.load_state_dict(sd)
    assert torch.equal(want.packed()[0][2][1][0], sd["net.slice3.12.weight"].permute(2, 3, 1, 0))

    torch.save(sd, tmp_path / "full.pth")
    full = fresh()
    full.load_state_dict(torch.load(tmp_path / "full.pth", weights_only=True))
    packed_equal(full, want)

    lin, tv = R.two_files(sd)
    assert any(k.startswith("classifier.") for k in tv) and all(k.startswith("lin") for k in lin)
    torch.save(lin, tmp_path / "vgg.pth")
    torch.save(tv, tmp_path / "vgg16-features.pth")
    two = fresh()
    two.load_state_dict(torch.load(tmp_path / "vgg16-features.pth", weights_only=True))
    two.load_state_dict(torch.load(tmp_path / "vgg.pth", weights_only=True))
    packed_equal(two, want)
    assert not any(p.requires_grad for p in two.parameters())

    with pytest.raises(RuntimeError):
        fresh().load_state_dict({"features.0.weight": torch.zeros(64, 3, 5, 5)})          # a wrong shape is an error, not a skip
    with pytest.raises(RuntimeError):
        fresh().load_state_dict({"encoder.weight": torch.zeros(3)})


def test_from_pretrained_reads_both_files_from_one_directory(tmp_path):
    from safetensors.torch import save_file
    from videogpa_amd.lpips import LPIPS
    sd = R.make_state_dict(4)
    want = fresh()
    want.load_state_dict(sd)
    lin, tv = R.two_files(sd)
    with pytest.raises(FileNotFoundError, match="local"):
        LPIPS.from_pretrained(str(tmp_path))
    d1 = tmp_path / "pth"
    (d1 / "weights" / "v0.1").mkdir(parents=True)
    torch.save(lin, d1 / "weights" / "v0.1" / "vgg.pth")
    torch.save(tv, d1 / "vgg16-397923af.pth")
    packed_equal(LPIPS.from_pretrained(str(d1)), want)
    d2 = tmp_path / "st"
    d2.mkdir()
    save_file({k: v.contiguous() for k, v in lin.items()}, str(d2 / "vgg.safetensors"))
    save_file({k: v.contiguous() for k, v in tv.items()}, str(d2 / "vgg16.safetensors"))
    got = LPIPS.from_pretrained(str(d2), frames_chunk=2)
    packed_equal(got, want)
    assert got.frames_chunk == 2
    # the constructor's own two paths
    packed_equal(LPIPS(net="vgg", model_path=str(d1 / "weights" / "v0.1" / "vgg.pth"), vgg_path=str(d1 / "vgg16-397923af.pth")), want)


def test_forward_fails_loudly():
    m = fresh()
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.features(x)
    with pytest.raises(ValueError):
        m(x, torch.zeros(2, 3, 16, 17))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 3, 15, 16), torch.zeros(2, 3, 15, 16))
    with pytest.raises(ValueError):
        m(x.double(), x.double())
    with pytest.raises(ValueError):
        m(torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16))


def test_scorer_message_points_at_the_native_network():
    from videogpa_amd import scorer
    with pytest.raises(RuntimeError, match="third-party") as e:
        scorer.LPIPSMetric().compute(gt=None, rep=None)
    assert "videogpa_amd.lpips.LPIPS" in str(e.value)


def test_restatement_sanity():
    sd = R.state()
    for shape in R.NET_CASES:
        c = R.net_case(shape)
        with torch.no_grad():
            same, _ = R.lpips(sd, c["gt"], c["gt"], torch.float64)
            back, _ = R.lpips(sd, c["rep"], c["gt"], torch.float64)
            norm, _ = R.lpips(sd, (c["gt"].double() + 1) / 2, (c["rep"].double() + 1) / 2, torch.float64, normalize=True)
        assert float(same.abs().max()) == 0.0
        assert torch.equal(back, c["val64"])                          # (a - b)^2 = (b - a)^2 exactly
        assert R.rel_err(norm, c["val64"]) < 1e-13
        assert float(c["val64"].min()) > 0 and all(float(p.min()) >= 0 for p in c["per64"])
        d_val = R.rel_err(c["val32"], c["val64"])
        d_per = R.rel_err(torch.stack(c["per32"]), torch.stack(c["per64"]))
        d_feat = [R.rel_err(a, b) for a, b in zip(c["feat32"], c["feat64"])]
        print(f"restatement {shape}: d32 total {d_val:.2e} per-layer {d_per:.2e} features {' '.join(f'{d:.2e}' for d in d_feat)}")
        assert d_val <= 8 * 2.0 ** -24 and d_per <= 8 * 2.0 ** -24
        assert max(d_feat) <= 4e-6 and min(d_feat) > 0


def test_new_symbols_are_in_the_ctypes_table():
    from videogpa_amd import _lib
    for name in ("vgpa_lpips_input_f32", "vgpa_maxpool2x2_f32", "vgpa_lpips_layer_f32", "vgpa_lpips_layer_workspace_bytes"):
        assert name in _lib.SIGNATURES
    # pure host arithmetic: one fp64 partial per workgroup, a workgroup owns (256 / G) * 8 pixels with G = C / 8 lanes per pixel
    q = lambda *a: _lib.query("vgpa_lpips_layer_workspace_bytes", *a)
    assert q(1, 300, 301, 64) == 8 * -(-300 * 301 // 256)
    assert q(3, 9, 7, 512) == 8 * 3 * -(-63 // 32)
    assert q(2, 1, 1, 64) == 16
    assert q(1, 4, 4, 516) == 0 and q(1, 4, 4, 6) == 0 and q(0, 4, 4, 64) == 0
