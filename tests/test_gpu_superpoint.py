"""SuperPoint on the device: the kernels of csrc/superpoint.hip, videogpa_amd.superpoint.SuperPoint and LightGlueMatcher's front half.  -m gpu only.

Continuous outputs follow tests/test_gpu_lpips.py's convention: error = max-abs difference over max-abs of the float64 answer (tests/superpoint_ref.py,
a torch restatement of upstream), bound 8 x d32 with d32 that same distance for the fp32 evaluation on the CPU; every check prints `name err d32 ratio`
before it asserts.  Discrete outputs are exact: torch's NMS + borders + threshold + selection run on the DEVICE's score image must give the device's
keypoints and scores, order included.  End to end against the float64 oracle the keypoint sets may differ in 1 % of the oracle's count per frame; the
test first asserts on the CPU that the fp32 and fp64 oracles agree and that an active cut has a gap of 1e-4 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import superpoint_ref as R

pytestmark = pytest.mark.gpu
MARGIN = 8.0
SEED = 1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from videogpa_amd import ops
    return ops


@pytest.fixture(scope="module")
def sd():
    return R.state(SEED)


_NETS = {}


def make_net(sd, **conf):
    from videogpa_amd.superpoint import SuperPoint
    key = tuple(sorted(conf.items()))
    if key not in _NETS:
        net = SuperPoint(pretrained=False, **conf)
        net.load_state_dict(sd)
        _NETS[key] = net.cuda()
    return _NETS[key]


def check(name, got, want64, ref32):
    err, d32 = R.rel_err(got, want64), R.rel_err(ref32, want64)
    print(f"{name}: err {err:.3e} d32 {d32:.3e} ratio {err / d32 if d32 > 0 else float('nan'):.2f}")
    assert np.isfinite(err) and err <= MARGIN * d32, (name, err, d32)


def conv1a_packed(ops, sd):
    return ops.pack_conv_weight(sd["conv1a.weight"]).cuda(), sd["conv1a.bias"].cuda()


# ---------------------------------------------------------------------------------------------------------------- input stage
def test_gray_bytes_and_the_255_table_are_exact(ops, sd):
    frames = R.noise_frames(2, 37, 41, 5)
    frames[0, 0, :6] = torch.tensor([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]], dtype=torch.uint8)
    _, gray = ops.sp_input_conv1a(frames.cuda(), *conv1a_packed(ops, sd), return_gray=True)
    want_bytes = R.gray_bytes(frames.numpy())                                             # integer numpy evaluation
    assert np.array_equal((gray.cpu().double() * 255).round().numpy().astype(np.uint8), want_bytes)
    assert torch.equal(gray.cpu(), torch.from_numpy(want_bytes / 255.0).float())            # g / 255.0 in float64, then .float()
    assert torch.equal(gray.cpu(), R.frame2tensor(frames)[:, 0])


@pytest.mark.parametrize("shape,size", [((48, 72), (64, 96)), ((53, 75), (70, 99)), ((20, 31), (20, 31))])
def test_resize_against_interpolate_and_conv1a(ops, sd, shape, size):
    frames = R.smooth_frames(2, *shape, seed=shape[0])
    img = R.frame2tensor(frames)
    w, b = conv1a_packed(ops, sd)
    out, gray = ops.sp_input_conv1a(frames.cuda(), w, b, size=size, return_gray=True)
    want64, ref32 = R.resize(img.double(), size), R.resize(img, size)
    if size == shape:
        assert torch.equal(gray.cpu(), img[:, 0])
    else:
        check(f"resized gray {shape}->{size}", gray[:, None], want64, ref32)
    c64 = F.conv2d(want64, sd["conv1a.weight"].double(), sd["conv1a.bias"].double(), padding=1)
    c32 = F.conv2d(ref32, sd["conv1a.weight"], sd["conv1a.bias"], padding=1)
    check(f"conv1a {shape}->{size}", out.permute(0, 3, 1, 2), c64, c32)
    # the float inputs of forward / extract: one channel as it is, three reduced with (0.299, 0.587, 0.114)
    out_f, gray_f = ops.sp_input_conv1a(img.cuda(), w, b, size=size, return_gray=True)
    assert torch.equal(out_f, out) and torch.equal(gray_f, gray)
    rgb = frames.permute(0, 3, 1, 2).float() / 255
    scale = torch.tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)
    _, gray3 = ops.sp_input_conv1a(rgb.cuda().contiguous(), w, b, size=size, return_gray=True)
    check(f"rgb float gray {shape}->{size}", gray3[:, None], R.resize((rgb.double() * scale.double()).sum(1, keepdim=True), size),
          R.resize((rgb * scale).sum(1, keepdim=True), size))


# ---------------------------------------------------------------------------------------------------------------- maps
@pytest.mark.parametrize("shape", [(64, 96), (53, 75)])
def test_score_image_and_descriptor_map(sd, ops, shape):
    img = R.frame2tensor(R.noise_frames(2, *shape, seed=shape[1]))
    m64, m32 = R.backbone({k: v.double() for k, v in sd.items()}, img.double()), R.backbone(sd, img)
    net = make_net(sd)
    taps = {}
    with torch.no_grad():
        net._detect(img.cuda(), taps=taps)
    assert taps["scores"].shape == (2, shape[0] // 8 * 8, shape[1] // 8 * 8)
    check(f"conv1a {shape}", taps["conv1a"].permute(0, 3, 1, 2), m64["conv1a"], m32["conv1a"])
    check(f"score image {shape}", taps["scores"], m64["scores"], m32["scores"])
    check(f"descriptor map {shape}", taps["dmap"].permute(0, 3, 1, 2), m64["dmap"], m32["dmap"])


def test_sampled_descriptors(sd, ops):
    img = R.frame2tensor(R.noise_frames(2, 53, 75, seed=9))
    taps = {}
    with torch.no_grad():
        make_net(sd)._detect(img.cuda(), taps=taps)
    dmap = taps["dmap"]                                                              # [2,6,9,256]
    g = torch.Generator().manual_seed(3)
    kp = torch.stack([torch.randint(0, 72, (2, 40), generator=g), torch.randint(0, 48, (2, 40), generator=g)], -1).float()
    kp[:, 0], kp[:, 1], kp[:, 2], kp[:, 3] = torch.tensor([0., 0.]), torch.tensor([71., 47.]), torch.tensor([0., 47.]), torch.tensor([71., 0.])
    counts = torch.tensor([40, 17], dtype=torch.int32)
    got = ops.sp_sample_desc_f32(dmap, kp.cuda(), counts.cuda())
    for t in range(2):
        n = int(counts[t])
        d = dmap[t].permute(2, 0, 1).cpu()
        check(f"sampled descriptors frame {t}", got[t, :n], R.sample_descriptors(kp[t, :n].double(), d.double()), R.sample_descriptors(kp[t, :n], d))


# ---------------------------------------------------------------------------------------------------------------- discrete, exact
def device_detect(net, src, size=None):
    taps = {}
    with torch.no_grad():
        kp, sc, desc, counts = net._detect(src, size=size, taps=taps)
    return kp.cpu(), sc.cpu(), desc.cpu(), counts.cpu().tolist(), taps


def exact_case(sd, frames, thr_mode="default", **conf):
    """torch on the device's own score image must select the device's keypoints, in its order.  Returns the per-frame counts before the cut."""
    img = R.frame2tensor(frames).cuda()
    probe = make_net(sd)
    score = device_detect(probe, img)[4]["scores"].cpu()
    radius, border = conf.get("nms_radius", 4), conf.get("remove_borders", 4)
    nms_ref = R.nms_borders(score, radius, border)
    thr = 0.0005
    if thr_mode == "median":
        thr = float(nms_ref[nms_ref > thr].median())
        conf["detection_threshold"] = thr
    cand = [int((nms_ref[t] > thr).sum()) for t in range(len(frames))]
    k = conf.get("max_num_keypoints")
    if k == "equal":
        k = conf["max_num_keypoints"] = cand[0]
    net = make_net(sd, **conf)
    kp, sc, desc, counts, taps = device_detect(net, img)
    assert torch.equal(taps["scores"].cpu(), score)                                   # run to run, net to net
    assert torch.equal(taps["nms"].cpu(), nms_ref)
    for t in range(len(frames)):
        kp_ref, sc_ref = R.select(nms_ref[t], thr, k)
        print(f"frame {t}: candidates {cand[t]} kept {counts[t]} (k = {k}, threshold {thr:.3e}, radius {radius}, borders {border})")
        assert counts[t] == len(sc_ref)
        assert torch.equal(kp[t, :counts[t]], kp_ref) and torch.equal(sc[t, :counts[t]], sc_ref)
    exact_case.nms = nms_ref
    return cand, counts


def test_exact_constant_frame_plateaus_and_mass_ties(sd, ops):
    """a cell further than the network's receptive field (84 pixels) from every edge sees the same input as its neighbours: 6 x 14 identical cells"""
    frames = torch.full((1, 144, 208, 3), 128, dtype=torch.uint8)
    cand, _ = exact_case(sd, frames)
    top = torch.sort(exact_case.nms[0].flatten(), descending=True).values[:cand[0]]
    vals, runs = torch.unique_consecutive(top, return_counts=True)
    i = int(runs.argmax())
    start, run = int(runs[:i].sum()), int(runs[i])
    print(f"constant frame: {cand[0]} candidates, the longest run of equal scores holds {run}, from rank {start}")
    assert run >= 20                                                                   # mass ties
    _, counts = exact_case(sd, frames, max_num_keypoints=start + run // 2)             # the cut falls inside that run
    assert counts == [start + run // 2]


@pytest.mark.parametrize("k", [32, "equal", 2048, None])
def test_exact_cut_below_equal_and_above_the_count(sd, ops, k):
    cand, counts = exact_case(sd, R.noise_frames(2, 64, 96, seed=11), max_num_keypoints=k)
    assert counts == ([32, 32] if k == 32 else [cand[0], min(cand)] if k == "equal" else cand)


@pytest.mark.parametrize("border,radius", [(0, 4), (4, 2), (0, 2)])
def test_exact_borders_and_radius(sd, ops, border, radius):
    exact_case(sd, R.noise_frames(2, 53, 75, seed=12), remove_borders=border, nms_radius=radius)


def test_exact_threshold_at_the_median_candidate(sd, ops):
    cand, counts = exact_case(sd, R.noise_frames(2, 64, 96, seed=13), thr_mode="median")
    assert counts == cand and min(counts) > 0                                          # `cand` is counted at the raised threshold already
    base, _ = exact_case(sd, R.noise_frames(2, 64, 96, seed=13))
    assert counts[0] + counts[1] < base[0] + base[1]                                   # the threshold bit


def test_nms_kernel_on_plateaus_across_tiles(ops):
    """the NMS kernel alone on a quantised map larger than one tile: plateaus, ties and tile seams, every radius, borders from the map's edge"""
    g = torch.Generator().manual_seed(0)
    s = (torch.rand(2, 75, 101, generator=g) * 6).floor() / 8 + 0.125
    s[0, 20:50, 28:36] = 1.0                                                           # a plateau over a tile seam
    for radius in (1, 2, 3, 4):
        for border in (0, 4):
            assert torch.equal(ops.sp_nms_f32(s.cuda(), radius, border).cpu(), R.nms_borders(s, radius, border)), (radius, border)


@pytest.mark.parametrize("k", [1, 100, 1000, 4096, None])
def test_select_kernel_on_many_tied_candidates(ops, k):
    """the selection alone on a synthetic map: thousands of candidates on 64 score levels (more than one pass of the block scan, every radix
    digit shared by many, ties across the cut), negative values, several compaction chunks; k not a power of two and at the sort's capacity"""
    g = torch.Generator().manual_seed(4)
    img = (torch.rand(2, 96, 136, generator=g) * 64).floor() / 64 * torch.rand(2, 1, 1, generator=g) - 0.25
    img[1, :, 100:] = -1.0
    kp, sc, counts = ops.sp_select(img.cuda(), 0.05, k)
    for t in range(2):
        kp_ref, sc_ref = R.select(img[t], 0.05, k)
        n = int(counts[t])
        print(f"select k={k} frame {t}: candidates {int((img[t] > 0.05).sum())} kept {n}")
        assert n == len(sc_ref) and (k is None or int((img[t] > 0.05).sum()) > 4096)
        assert torch.equal(kp[t, :n].cpu(), kp_ref) and torch.equal(sc[t, :n].cpu(), sc_ref)


# ---------------------------------------------------------------------------------------------------------------- end to end
E2E = {"noise k=32": ("noise", 2, 64, 96, 21, 32), "noise k=2048": ("noise", 2, 64, 96, 21, 2048), "odd 53x75": ("noise", 2, 53, 75, 22, 2048),
       "smooth 120x160": ("smooth", 3, 120, 160, 23, 64)}
_ORACLE = {}


def oracle(sd, name):
    if name not in _ORACLE:
        kind, T, H, W, seed, k = E2E[name]
        frames = (R.noise_frames if kind == "noise" else R.smooth_frames)(T, H, W, seed)
        img = R.frame2tensor(frames)
        f64, _ = R.detect({n: v.double() for n, v in sd.items()}, img.double(), k=k)
        f32, _ = R.detect(sd, img, k=k)
        full, _ = R.detect({n: v.double() for n, v in sd.items()}, img.double(), k=None)
        _ORACLE[name] = (frames, f64, f32, full, k)
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(E2E))
def test_end_to_end_against_float64(sd, ops, name):
    frames, f64, f32, full, k = oracle(sd, name)
    for t in range(len(frames)):                                                        # the test's own preconditions, on the CPU
        assert R.keyset(f64[t][0]) == R.keyset(f32[t][0]), f"{name} frame {t}: the fp32 and fp64 oracles keep different sets"
        s = torch.sort(full[t][1], descending=True).values
        if k < len(s):
            gap = float((s[k - 1] - s[k]) / s[k - 1])
            print(f"{name} frame {t}: cut at {k} of {len(s)}, gap {gap:.3e}")
            assert gap >= 1e-4, f"{name} frame {t}: the cut has no gap ({gap:.2e}): pick another seed"
    feats = make_net(sd, max_num_keypoints=k).extract_clip(frames, resize=None)
    assert len(feats) == len(frames)
    for t, f in enumerate(feats):
        kp, sc, desc = f["keypoints"][0].cpu(), f["keypoint_scores"][0].cpu(), f["descriptors"][0].cpu()
        want = {p: i for i, p in enumerate(map(tuple, f64[t][0].long().tolist()))}
        got = {p: i for i, p in enumerate(map(tuple, kp.long().tolist()))}
        diff = set(want) ^ set(got)
        print(f"{name} frame {t}: oracle {len(want)} device {len(got)} symmetric difference {len(diff)}")
        assert len(diff) <= 0.01 * len(want)
        common = sorted(set(want) & set(got))
        wi, gi = [want[p] for p in common], [got[p] for p in common]
        r32 = {p: i for i, p in enumerate(map(tuple, f32[t][0].long().tolist()))}
        ri = [r32[p] for p in common]
        check(f"{name} frame {t} descriptors", desc[gi], f64[t][2][wi], f32[t][2][ri])
        check(f"{name} frame {t} scores", sc[gi], f64[t][1][wi], f32[t][1][ri])
        assert tuple(f["image_size"][0].tolist()) == (frames.shape[2], frames.shape[1])


def test_chunkings_and_runs_are_bit_equal(sd, ops):
    frames = oracle(sd, "smooth 120x160")[0]
    net = make_net(sd, max_num_keypoints=64)
    ref = net.extract_clip(frames.cuda(), resize=None, frames_chunk=3)
    for chunk in (1, 2, 3):
        got = net.extract_clip(frames, resize=None, frames_chunk=chunk)
        for a, b in zip(ref, got):
            assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), chunk


# ---------------------------------------------------------------------------------------------------------------- extract
def test_extract_resizes_and_rescales(sd, ops):
    frames = R.smooth_frames(1, 48, 72, seed=31)
    img = R.frame2tensor(frames)
    net = make_net(sd, max_num_keypoints=2048)
    f = net.extract(img[0].cuda(), resize=96)
    assert f["image_size"].tolist() == [[72.0, 48.0]] and f["keypoints"].shape[0] == 1 and f["descriptors"].shape[-1] == 256
    big64 = R.resize(img.double(), (64, 96))
    (kp64, sc64, d64), = R.detect({n: v.double() for n, v in sd.items()}, big64, k=2048)[0]
    raw = ((f["keypoints"][0].cpu() + 0.5) * torch.tensor([96 / 72, 64 / 48]) - 0.5).round().long()
    want = R.keyset(kp64)
    got = {tuple(p) for p in raw.tolist()}
    print(f"extract 48x72 -> 64x96: oracle {len(want)} device {len(got)} symmetric difference {len(want ^ got)}")
    assert len(want ^ got) <= 0.01 * len(want) and len(got) == f["keypoints"].shape[1]
    kp_dev, *_ = device_detect(net, img.cuda(), size=(64, 96))
    scales = torch.tensor([96 / 72, 64 / 48], dtype=torch.float32)
    assert torch.equal(f["keypoints"][0].cpu(), (kp_dev[0, :f["keypoints"].shape[1]] + 0.5) / scales[None] - 0.5)
    same = net.extract(img.cuda(), resize=None)
    fwd = net({"image": img.cuda()})
    assert all(torch.equal(same[k], fwd[k]) for k in fwd) and same["image_size"].tolist() == [[72.0, 48.0]]
    with pytest.raises(NotImplementedError, match="48 x 72 to 40 x 60"):
        net.extract(img.cuda(), resize=60)
    two = torch.cat([img, R.frame2tensor(R.smooth_frames(1, 48, 72, seed=32))]).cuda()
    with pytest.raises(RuntimeError, match="different numbers of keypoints"):
        net({"image": two})


# ---------------------------------------------------------------------------------------------------------------- matcher front
def test_lightglue_matcher_front(sd, ops):
    from videogpa_amd import scorer as S
    frames, f64, _, _, k = oracle(sd, "smooth 120x160")
    net = make_net(sd, max_num_keypoints=k)
    m = S.LightGlueMatcher(min_matches=8, extractor=net, matcher=R.mutual_nn)
    net_conf, net.preprocess_conf["resize"] = net.preprocess_conf["resize"], None       # the oracle above ran at the frames' own size
    try:
        feat = lambda t: {"keypoints": f64[t][0][None].float(), "descriptors": f64[t][2][None].float()}
        pairs = m.match_clip(frames.numpy())
        assert len(pairs) == len(frames) - 1
        for i, (p1, p2) in enumerate(pairs):
            mm = R.mutual_nn({"image0": feat(i), "image1": feat(i + 1)})["matches"][0]
            want = {(*f64[i][0][a].tolist(), *f64[i + 1][0][b].tolist()) for a, b in mm.tolist()}
            got = {(*a, *b) for a, b in zip(p1.tolist(), p2.tolist())}
            print(f"pair {i}: {len(got)} matches, oracle {len(want)}")
            assert got == want and p1.dtype == np.float32 and len(got) >= 8
            q1, q2, n, meta = m.get_matched_points(frames[i].numpy(), frames[i + 1].numpy())
            assert np.array_equal(q1, p1) and np.array_equal(q2, p2) and n == len(p1) and meta == {"descriptor_type": "lightglue", "total_matches": n}
            c1, c2 = m(frames[i].numpy(), frames[i + 1].numpy())
            assert np.array_equal(c1, p1) and np.array_equal(c2, p2)
        em = S.EpipolarMetric(descriptor_type="lightglue", min_matches=8, matcher=m)
        val = em.compute(gt=frames.numpy())
        assert val == em.compute_from_matches([a for a, _ in pairs], [b for _, b in pairs]) and val >= 0
        assert val == em.compute(gt=frames.permute(0, 3, 1, 2).contiguous().numpy())        # [T,3,H,W] bytes
        few = S.LightGlueMatcher(min_matches=10 ** 6, extractor=net, matcher=R.mutual_nn).get_matched_points(frames[0], frames[1])
        assert few[0] is None and few[1] is None and "Too few matches" in few[3]["error"]
    finally:
        net.preprocess_conf["resize"] = net_conf
