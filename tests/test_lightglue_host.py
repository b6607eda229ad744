"""LightGlue without a GPU: the module's names, configuration and errors, and the oracle tests/lightglue_ref.py itself: its builders meet the conditions
the GPU tests rely on, its three modes agree on every decision, and the same comparisons reject five wrong restatements."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightglue_ref as R  # noqa: E402

PRUNE_CONF = {"pruning_threshold": 64}


@functools.lru_cache(maxsize=None)
def matching(mode, variant=None):
    return R.forward(R.matching_state(0), R.pair(330, 300, 1), mode, variant=variant)


@functools.lru_cache(maxsize=None)
def pruning(mode, variant=None):
    return R.forward(R.prune_state(1), R.pair(200, 150, 11, extra=40), mode, conf=PRUNE_CONF, variant=variant)


@functools.lru_cache(maxsize=None)
def stopping(layer, mode):
    return R.forward(R.stop_state(0, layer), R.pair(130, 130, 3, extra=127), mode)


def margin():
    """16 x the ref16 oracle's measured log-score distance from fp64 on the matching pair"""
    return 16.0 * float((matching("ref16")["scores"] - matching("f64")["scores"]).abs().max())


# ---- the module ------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_both_spellings_load():
    from videogpa_amd.lightglue import LightGlue
    net = LightGlue()
    want = R.names()
    own = net.state_dict()
    assert set(own) == set(want) and all(tuple(own[k].shape) == tuple(want[k]) for k in want)
    sd = R.state(3)
    for spelled in (sd, R.checkpoint_spelling(sd)):
        other = LightGlue(seed=7)
        other.load_state_dict(spelled)
        assert all(torch.equal(other.state_dict()[k], sd[k]) for k in sd)
    assert "self_attn.4.Wqkv.weight" in R.checkpoint_spelling(sd) and "cross_attn.0.to_qk.bias" in R.checkpoint_spelling(sd)
    with pytest.raises(RuntimeError):
        LightGlue().load_state_dict({k: v for k, v in sd.items() if "to_v" not in k})
    assert not any(p.requires_grad for p in net.parameters()) and not net.training


def test_conf_errors_and_unbuilt_arms(tmp_path):
    from videogpa_amd.lightglue import DEFAULT_CONF, LightGlue
    assert LightGlue().conf == DEFAULT_CONF and DEFAULT_CONF["n_layers"] == 9 and DEFAULT_CONF["num_heads"] == 4 and DEFAULT_CONF["flash"] is True
    assert (DEFAULT_CONF["depth_confidence"], DEFAULT_CONF["width_confidence"], DEFAULT_CONF["filter_threshold"]) == (0.95, 0.99, 0.1)
    assert LightGlue.pruning_keypoint_thresholds == {"cpu": -1, "mps": -1, "cuda": 1024, "flash": 1536} and LightGlue().pruning_min_kpts() == 1536
    net = LightGlue(depth_confidence=-1)
    net.pruning_keypoint_thresholds = {**LightGlue.pruning_keypoint_thresholds, "flash": 64}          # per instance
    assert net.pruning_min_kpts() == 64 and LightGlue().pruning_min_kpts() == 1536
    with pytest.raises(TypeError, match="unknown configuration"):
        LightGlue(depth_confidense=0.9)
    for kw in ({"features": "disk"}, {"features": "aliked"}, {"features": "sift"}, {"add_scale_ori": True}, {"mp": True}, {"flash": False},
               {"input_dim": 128}, {"descriptor_dim": 128}, {"num_heads": 8}):
        with pytest.raises(NotImplementedError):
            LightGlue(**kw)
    with pytest.raises(NotImplementedError):
        LightGlue().compile()
    with pytest.raises(RuntimeError, match="never downloads"):
        LightGlue(pretrained=True)
    with pytest.raises(FileNotFoundError, match="local files only"):
        LightGlue.from_pretrained(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="local files only"):
        LightGlue.from_pretrained(str(tmp_path / "nothing.pth"))
    torch.save(R.checkpoint_spelling(R.state(5)), tmp_path / "superpoint_lightglue.pth")
    got = LightGlue.from_pretrained(str(tmp_path)).state_dict()
    assert all(torch.equal(got[k], v) for k, v in R.state(5).items())


def test_loud_errors():
    from videogpa_amd.lightglue import LightGlue
    net = LightGlue()
    f = lambda n, **kw: {"keypoints": torch.zeros(1, n, 2, **kw), "descriptors": torch.zeros(1, n, 256, **kw)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net({"image0": f(5), "image1": f(6)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.match_batch([f(5), f(6)])
    with pytest.raises(ValueError, match="fp32 inputs only"):
        net({"image0": f(5, dtype=torch.float16), "image1": f(6)})
    g = f(5)
    g["descriptors"].requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        net({"image0": g, "image1": f(6)})
    from videogpa_amd.scorer import LightGlueMatcher
    with pytest.raises(FileNotFoundError, match="local files only"):
        LightGlueMatcher.from_pretrained(os.path.join(os.path.dirname(__file__), "no_such_dir"))


def test_confidence_thresholds_equal_the_formula():
    import math
    from videogpa_amd.lightglue import LightGlue, confidence_threshold
    net = LightGlue()
    want = [min(max(0.8 + 0.1 * math.exp(-4.0 * i / 9), 0.0), 1.0) for i in range(9)]
    assert [confidence_threshold(i, 9) for i in range(9)] == want == [R.confidence_threshold(i) for i in range(9)]
    assert torch.equal(net.confidence_thresholds, torch.tensor(want, dtype=torch.float32)) and net.confidence_thresholds.dtype == torch.float32
    assert abs(want[0] - 0.9) < 1e-15 and want == sorted(want, reverse=True)


def test_interleaved_qkv_index_map():
    """feature f = h * 192 + d * 3 + {q, k, v}: checked against unflatten(-1, (4, 64, 3)) on a tensor that holds its own index"""
    from videogpa_amd.lightglue import qkv_feature_index
    lab = torch.arange(768.0)[None]
    t = lab.unflatten(-1, (4, 64, 3)).transpose(0, 1)                  # upstream's [heads, tokens, 64, 3]
    for h in range(4):
        for d in range(64):
            for w in range(3):
                assert int(t[h, 0, d, w]) == qkv_feature_index(h, d, w)
    q, k, v = R.split_qkv(lab)
    assert int(q[1, 0, 2]) == 192 + 6 and int(k[1, 0, 2]) == 192 + 7 and int(v[3, 0, 63]) == 767
    qb, _, vb = R.split_qkv(lab, "qkv_blocks")
    assert int(qb[1, 0, 2]) == 66 and int(vb[0, 0, 0]) == 512        # the wrong reading: three contiguous blocks


def test_oracle_rotate_half_acts_on_adjacent_pairs():
    x = torch.arange(1.0, 9.0)
    assert R.rotate_half(x).tolist() == [-2, 1, -4, 3, -6, 5, -8, 7]
    assert R.rotate_half(x, "rotate_halves").tolist() == [-5, -6, -7, -8, 1, 2, 3, 4]
    enc = R.posenc(torch.tensor([[1.0, 0.0]] * 32), torch.tensor([[0.5, 0.0]]))
    assert enc.shape == (2, 1, 1, 64) and torch.equal(enc[0, 0, 0, 0::2], enc[0, 0, 0, 1::2])
    r = R.rope(enc, torch.tensor([1.0, 0.0] * 32)[None, None])
    assert torch.allclose(r[0, 0, 0::2], torch.cos(torch.tensor(0.5)).expand(32)) and torch.allclose(r[0, 0, 1::2], torch.sin(torch.tensor(0.5)).expand(32))


# ---- the builders meet their conditions on the oracle ---------------------------------------------------------------------------------------------
def test_matching_builder_returns_the_planted_matches():
    d, o = R.pair(330, 300, 1), matching("f64")
    assert o["stop"] == 9 and len(o["matches"]) == 300
    assert torch.equal(d["gt"][o["matches"][:, 1]], o["matches"][:, 0])
    x0 = o["desc"][-1][0]
    assert float((x0 - d["descriptors0"].double()).norm(dim=-1).mean()) > 0.5          # the transformer matters
    assert float((o["matching_scores0"] - 0.1).abs().min()) > 0.02
    plain = R.forward(R.state(0), R.pair(330, 300, 1), "f32")
    assert len(plain["matches"]) == 0                                                  # why matching_state exists


def test_f32_and_ref16_oracles_decide_as_fp64():
    for run in (matching, pruning, functools.partial(stopping, 1), functools.partial(stopping, 4)):
        ref = run("f64")
        for mode in ("f32", "ref16"):
            o = run(mode)
            assert o["stop"] == ref["stop"] and torch.equal(o["matches"], ref["matches"]), (run, mode)
            assert torch.equal(o["prune0"].double(), ref["prune0"].double()) and torch.equal(o["prune1"].double(), ref["prune1"].double())
            assert len(o["keep"]) == len(ref["keep"])
            for a, b in zip(o["keep"], ref["keep"]):
                for s in range(2):
                    assert (a[s] is None) == (b[s] is None) and (a[s] is None or torch.equal(a[s], b[s]))


def test_stop_builder_stops_where_asked():
    assert stopping(1, "f64")["stop"] == 2 and stopping(4, "f64")["stop"] == 5
    assert len(stopping(1, "f64")["matches"]) >= 100 and len(stopping(4, "f64")["matches"]) >= 100
    assert not torch.equal(stopping(1, "f64")["scores"], stopping(4, "f64")["scores"])


def test_prune_builder_prunes_without_stopping_early():
    o = pruning("f64")
    assert o["stop"] >= 5
    for side in range(2):
        removed = [1.0 - float(k[side].float().mean()) for k in o["keep"] if k[side] is not None]
        assert sum(0.10 <= r <= 0.60 for r in removed) >= 2, removed
    assert len(o["matches"]) >= 8 and int((o["prune0"] > 1).sum()) > 0 and int((o["prune0"] == 1).sum()) > 0
    assert len(o["ind0"]) < 200 and len(o["ind1"]) < 190


def test_no_decision_sits_on_its_threshold():
    thr = R.state(0)["confidence_thresholds"]
    for o in (matching("f64"), pruning("f64"), stopping(1, "f64"), stopping(4, "f64")):
        for i, c in enumerate(o["conf"]):
            assert float((torch.cat(c) - thr[i]).abs().min()) > 1e-3
        for sig in o["msig"]:
            for s in sig:
                assert s is None or float((s - 0.01).abs().min()) > 1e-3
        ms = o["matching_scores0"]
        assert float((ms[ms > 0] - 0.1).abs().min()) > 0.02 if o is not pruning("f64") else True
    # the prune builder's scores: nearest 0.07 from the threshold (measured); the GPU test takes its matches from rows clear of it
    ms = pruning("f64")["matching_scores0"]
    assert float((ms[ms > 0] - 0.1).abs().min()) > 0.02


def test_few_rows_have_a_small_top_two_gap():
    m = margin()
    assert 0 < m < 0.1, m
    for o in (matching("f64"), stopping(1, "f64"), stopping(4, "f64"), pruning("f64")):
        gap = R.top2_gap(o["scores"])
        assert float((gap < m).float().mean()) <= 0.05


# ---- the same comparisons reject wrong restatements -------------------------------------------------------------------------------------------------
def test_wrong_restatements_are_rejected():
    """each variant against the fp64 oracle, by the measures the GPU tests use: the last layer's descriptors within 2 x d16, the log score within the
    margin, the stop layer and the keep masks exact"""
    sd, d, free = R.state(0), R.pair(130, 130, 3, extra=127), {"depth_confidence": -1, "width_confidence": -1}
    ref, r16 = R.forward(sd, d, "f64", free), R.forward(sd, d, "ref16", free)
    assert len(ref["desc"]) == 9
    for v in ("qkv_blocks", "rotate_halves", "cross_scale_twice"):
        o = R.forward(sd, d, "f32", free, variant=v)
        for layer in (0, 8):                                           # plain random weights, as the GPU test of the per-layer descriptors
            assert R.err(o["desc"][layer][0], ref["desc"][layer][0]) > 2 * R.err(r16["desc"][layer][0], ref["desc"][layer][0]), (v, layer)
    assert float((matching("f32", "no_col_softmax")["scores"] - matching("f64")["scores"]).abs().max()) > margin()
    # the original-count quirk: a pair steered so that, after pruning, the points still below the threshold are few against the ORIGINAL count
    sp = R.prune_state(1)
    quirk = R.steer(R.pair(200, 150, 11, extra=40), sp, 3, 0.12)
    pr, wrong = R.forward(sp, quirk, "f64", PRUNE_CONF), R.forward(sp, quirk, "f64", PRUNE_CONF, variant="num_points_after_prune")
    assert pr["stop"] == 4 and wrong["stop"] != pr["stop"]
