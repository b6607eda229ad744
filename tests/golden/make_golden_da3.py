"""Writes tests/golden/da3_*.pt and da3_names.json: Depth Anything 3's DINOv2 backbone (depth_anything_3/model/dinov2/vision_transformer.py), its
reference-view selection (reference_view_selector.py), CameraDec (cam_dec.py) and the pose decoding (model/utils/transform.py; the inverse of utils/geometry.py:55-59 is da3_ref.invert_rigid), imported
from the reference and evaluated on the CPU.

    python tests/golden/make_golden_da3.py /path/to/reference

Tensors, numbers and names only, every file below 1 MiB.  The reduced configurations, the cases and the seeded recipe are tests/da3_ref.py's:
  da3_a_state.pt, da3_a_cam_dec_state.pt   configuration (a), dim 64: the state dicts of the backbone and of CameraDec themselves
  da3_{a,b,c}.pt        per configuration: cfg, shapes and per-tensor float64 sums of both states (the tests regenerate the states from the recipe and
                        check the sums), the input seed of every case, the seeds the selection search rejected, and the camera decoder's goldens
  da3_{a,b,c}_CASE.pt   per case (its outputs in da3_{a,b,c}_CASE_L<i>.pt, one file per out layer, where one file would pass 1 MiB): per out layer features and camera token in float64 and fp32, the reference's own CPU bf16-autocast distance from float64
                        (d16) per output tensor, and for the cases that select: the view chosen by the float64, fp32 and bf16-autocast runs and the
                        float64 balance scores
A "saddle_balanced" case is kept only if the three runs choose the same view and the float64 gap between the best and the second-best balance score is
at least 0.15: the min-max normalisation behind the score amplifies rounding, and a case the reference's own precisions disagree on pins nothing."""
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import da3_ref as D  # noqa: E402
import dinov2_ref  # noqa: E402

MIN_GAP, SEARCH = 0.15, range(100, 112)


def save(name, obj):
    path = os.path.join(HERE, name)
    torch.save(obj, path)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20), "fixtures stay below 1 MiB each"


def import_reference(ref_root):
    """the package __init__ chain needs addict / omegaconf: the parent packages are registered as plain namespaces (make_golden.py::golden_da3_attention)"""
    sys.path.insert(0, ref_root)
    for pkg in ("depth_anything_3", "depth_anything_3.model", "depth_anything_3.model.dinov2", "depth_anything_3.model.utils", "depth_anything_3.utils"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(ref_root, *pkg.split("."))]
            sys.modules[pkg] = m
    from depth_anything_3.model import cam_dec, reference_view_selector
    from depth_anything_3.model.dinov2 import dinov2, vision_transformer
    from depth_anything_3.model.utils import transform
    return vision_transformer, dinov2, reference_view_selector, cam_dec, transform


def save_case(tag, name, c):
    """one file per case; a case whose outputs pass the limit keeps them in one file per out layer (da3_ref.load_case puts them back)"""
    total = sum(t.numel() * t.element_size() for key in ("out64", "out32") for pair in c[key] for t in pair)
    if total < (1 << 20) - 8192:
        return save(f"da3_{tag}_{name}.pt", c)
    for i, (o64, o32) in enumerate(zip(c["out64"], c["out32"])):
        save(f"da3_{tag}_{name}_L{i}.pt", (o64, o32))
    save(f"da3_{tag}_{name}.pt", dict({k: v for k, v in c.items() if k not in ("out64", "out32")}, layer_files=len(c["out64"])))


def main(ref_root):
    vt, dinov2_mod, _, cam_dec_mod, transform = import_reference(ref_root)
    picked = []                                           # what the reference's selection returned, per call
    inner = vt.select_reference_view

    def recording(x, strategy="saddle_balanced"):
        idx = inner(x, strategy=strategy)
        picked.append((idx.clone(), x[:, :, 0].detach().clone()))
        return idx
    vt.select_reference_view = recording

    def build(cfg):
        return vt.DinoVisionTransformer(img_size=D.IMG_SIZE, patch_size=D.PATCH, embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"],
                                        mlp_ratio=4, alt_start=cfg["alt_start"], qknorm_start=cfg["qknorm_start"], rope_start=cfg["rope_start"],
                                        cat_token=True).eval()

    def run(m, x, cfg, cam, strategy, dtype=None, autocast=False):
        """-> (per out layer (features, camera token), the selected views or None, the class tokens the selection saw)"""
        picked.clear()
        kw = dict(cam_token=None if cam is None else cam.to(dtype or torch.float32), ref_view_strategy=strategy)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            out, aux = m.get_intermediate_layers(x.to(dtype or torch.float32), cfg["out_layers"], **kw)
        assert aux == [] and len(picked) <= 1
        return [(f.clone(), c.clone()) for f, c in out], (picked[0][0] if picked else None), (picked[0][1] if picked else None)

    for tag, cfg in D.CONFIGS.items():
        m = build(cfg)
        state = D.seeded_state({k: v.shape for k, v in m.state_dict().items()}, cfg["seed"])
        m.load_state_dict(state, strict=True)
        m64 = build(cfg).double()
        m64.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
        C = cfg["embed_dim"]
        dec = cam_dec_mod.CameraDec(2 * C).eval()
        dec_state = D.cam_dec_state({k: v.shape for k, v in dec.state_dict().items()}, cfg["seed"])
        dec.load_state_dict(dec_state, strict=True)

        def dec64(feat):          # CameraDec.forward casts to fp32 inside (cam_dec.py:37-40): its float64 evaluation is the same layers restated
            w = {k: v.double() for k, v in dec_state.items()}
            f = feat.reshape(-1, feat.shape[-1])
            for i in (0, 2):
                f = torch.relu(F.linear(f, w[f"backbone.{i}.weight"], w[f"backbone.{i}.bias"]))
            parts = [F.linear(f, w["fc_t.weight"], w["fc_t.bias"]), F.linear(f, w["fc_qvec.weight"], w["fc_qvec.bias"]),
                     torch.relu(F.linear(f, w["fc_fov.0.weight"], w["fc_fov.0.bias"]))]
            return torch.cat(parts, dim=-1).reshape(*feat.shape[:2], 9)

        def evaluate(x, cam, strategy):
            o64, p64, cls64 = run(m64, x, cfg, cam, strategy, torch.float64)
            o32, p32, _ = run(m, x, cfg, cam, strategy)
            o16, p16, _ = run(m, x, cfg, cam, strategy, autocast=True)
            c = {"out64": o64, "out32": o32, "d16": [(D.rel(f16, f64), D.rel(c16, c64)) for (f16, c16), (f64, c64) in zip(o16, o64)],
                 "d32": [(D.rel(f32, f64), D.rel(c32, c64)) for (f32, c32), (f64, c64) in zip(o32, o64)]}
            if p64 is not None:
                balance = D.select_metrics(cls64)[3]
                if strategy == "saddle_balanced":
                    assert torch.equal(balance.argmin(dim=1), p64), "the restated balance score disagrees with the reference's choice"
                # the restated similarity range against the reference's own "saddle_sim_range" choice on the same class tokens
                assert torch.equal(inner(cls64[:, :, None], strategy="saddle_sim_range"), D.select(cls64, "saddle_sim_range"))
                top2 = balance.sort(dim=1).values[:, :2]
                c.update(ref64=p64, ref32=p32, ref16=p16, balance64=balance, gap64=float((top2[:, 1] - top2[:, 0]).min()))
            return c

        meta = {"cfg": dict(cfg, img_size=D.IMG_SIZE, patch_size=D.PATCH), "shapes": {k: list(v.shape) for k, v in state.items()},
                "sums": dinov2_ref.state_sums(state), "cam_dec_shapes": {k: list(v.shape) for k, v in dec_state.items()},
                "cam_dec_sums": dinov2_ref.state_sums(dec_state), "input_seed": {}, "rejected": [], "cases": list(D.CASES_OF[tag])}
        # the selection search: B = 1, S = 4 inputs on which float64, fp32 and bf16 autocast agree, with a float64 gap of at least MIN_GAP
        B, S, hw, strategy, _ = D.CASES["saddle0"]
        kept = []
        for seed in SEARCH:
            c = evaluate(D.images(seed, B, S, hw), None, strategy)
            agree = torch.equal(c["ref64"], c["ref32"]) and torch.equal(c["ref64"], c["ref16"])
            print(tag, "seed", seed, "ref", c["ref64"].tolist(), c["ref32"].tolist(), c["ref16"].tolist(), "gap", round(c["gap64"], 4))
            if agree and c["gap64"] >= MIN_GAP:
                kept.append((seed, c))
                if len(kept) == 2:
                    break
            else:
                meta["rejected"].append({"seed": seed, "ref64": c["ref64"].tolist(), "ref32": c["ref32"].tolist(), "ref16": c["ref16"].tolist(),
                                         "gap64": c["gap64"]})
        assert len(kept) == 2, "fewer than two saddle_balanced inputs qualified"
        assert len({int(c["ref64"][0]) for _, c in kept} | {0}) > 1, "every kept input selects view 0: the reordering would go untested"
        last_cam = None
        for name in D.CASES_OF[tag]:
            B, S, hw, strategy, own_cam = D.CASES[name]
            if name in ("saddle0", "saddle1"):
                seed, c = kept[int(name[-1])]
            else:
                seed = {"s1": 1, "s2": 2, "first": 3, "middle": 4, "camtok": 5, "saddle_b2": -1}[name]
                x = torch.cat([D.images(s, 1, S, hw) for s, _ in kept]) if name == "saddle_b2" else D.images(seed, B, S, hw)
                c = evaluate(x, D.cam_tokens(seed, B, S, C) if own_cam else None, strategy)
            if name == "saddle_b2":
                assert c["ref64"].tolist() == [int(k["ref64"][0]) for _, k in kept] and torch.equal(c["ref64"], c["ref32"]) and torch.equal(c["ref64"], c["ref16"])
                meta["input_seed"][name] = [s for s, _ in kept]
            else:
                meta["input_seed"][name] = seed
            assert ("ref64" in c) == (S >= 3 and not own_cam)
            print(tag, name, "d16", [(round(a, 5), round(b, 5)) for a, b in c["d16"]], "d32", [(float(f"{a:.2e}"), float(f"{b:.2e}")) for a, b in c["d32"]],
                  "ref", c.get("ref64"))
            save_case(tag, name, c)
            last_cam = c["out64"][-1][1]
        # the camera decoder on the last case's camera token (rounded to fp32: the input of both evaluations)
        cam_in = last_cam.float()
        H, W = D.CASES[D.CASES_OF[tag][-1]][2]
        cams = {"cam_in": cam_in, "hw": (H, W)}
        for key, d, dt in (("64", dec64, torch.float64), ("32", dec, torch.float32)):
            with torch.no_grad():
                pose = d(cam_in.to(dt))
                c2w, intr = transform.pose_encoding_to_extri_intri(pose, (H, W))
                cams.update({"pose_enc" + key: pose, "c2w" + key: c2w, "extrinsics" + key: D.invert_rigid(c2w), "intrinsics" + key: intr})
        # upstream builds the intrinsics in an fp32 tensor whatever the encoding's dtype: the float64 golden is da3_ref.pinhole in
        # float64, and the reference's tensor must be its rounding
        assert cams["intrinsics64"].dtype == torch.float32
        ref_k, k64 = cams["intrinsics64"], D.pinhole(cams["pose_enc64"][..., 7:], (H, W))
        assert torch.equal(k64.float(), ref_k), (k64.float() - ref_k).abs().max()
        cams["intrinsics64"] = k64
        assert D.rel(dec64(cam_in.double()).float(), cams["pose_enc32"]) < 1e-5
        cams["d32"] = {k: D.rel(cams[k + "32"], cams[k + "64"]) for k in ("pose_enc", "extrinsics", "intrinsics")}
        print(tag, "cameras d32", cams["d32"], "fov", cams["pose_enc64"][..., 7:].flatten().tolist())
        meta["cameras"] = cams
        if tag == "a":
            save("da3_a_state.pt", state)
            save("da3_a_cam_dec_state.pt", dec_state)
        save(f"da3_{tag}.pt", meta)

    full = dinov2_mod.DinoV2("vitl", [11, 15, 19, 23], 8, 8, 8, True)          # DA3-Large (configs/da3-large.yaml); its constructor reads tensor values,
    with torch.device("meta"):                                                  # so it is built for real
        dec = cam_dec_mod.CameraDec(2048)
    names = {"backbone": {k: list(v.shape) for k, v in full.state_dict().items()}, "cam_dec": {k: list(v.shape) for k, v in dec.state_dict().items()}}
    path = os.path.join(HERE, "da3_names.json")
    with open(path, "w") as f:
        json.dump(names, f, indent=0, sort_keys=True)
    print(path, len(names["backbone"]), len(names["cam_dec"]), os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
