"""The C-ABI library loads on CPU and exports exactly what include/videogpa_hip.h declares (no compute calls)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "videogpa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"#ifdef VGPA_VARIANTS.*?#endif", "", src, flags=re.S)      # entry points of variant builds (tools/build_variant.sh) only
    return set(re.findall(r"\b(vgpa_[a-z0-9_]+)\s*\(", src))


_CTYPE = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "vgpa_stream_t": ctypes.c_void_p}


def _header_signatures(variants):
    """name -> (restype, [argtypes]) of every prototype of the header (variants: of its VGPA_VARIANTS block instead), pointers as c_void_p"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "videogpa_hip.h")).read(), flags=re.S)
    blocks = re.findall(r"#ifdef VGPA_VARIANTS(.*?)#endif", src, flags=re.S)
    src = "".join(blocks) if variants else re.sub(r"#ifdef VGPA_VARIANTS.*?#endif", "", src, flags=re.S)
    ctype = lambda decl: ctypes.c_void_p if "*" in decl else _CTYPE[decl.replace("const", "").split()[0]]
    return {name: (ctype(ret), [ctype(a) for a in args.split(",") if a.strip() != "void"])
            for ret, name, args in re.findall(r"\b(\w+)\s+(vgpa_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_ctypes_table_matches_every_prototype_of_the_header():
    """_lib.SIGNATURES is written by hand: a wrong width there corrupts arguments on the device and nothing on the CPU would notice"""
    from videogpa_amd import _lib
    declared = _header_signatures(variants=False)
    assert set(declared) == _header_symbols() and len(declared) >= 20
    wrong = {n: (sig, _lib.SIGNATURES.get(n)) for n, sig in declared.items() if _lib.SIGNATURES.get(n) != sig}
    assert not wrong and set(_lib.SIGNATURES) == set(declared), wrong
    optional = _header_signatures(variants=True)
    assert optional == _lib.OPTIONAL_SIGNATURES, (optional, _lib.OPTIONAL_SIGNATURES)


def test_library_exports_every_declared_symbol():
    from videogpa_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _header_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in videogpa_hip.h but not exported"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vgpa_[a-z0-9_]+)", out))
    assert exported == declared, f"undeclared exports: {exported - declared}; missing: {declared - exported}"
    assert set(_lib.SIGNATURES) == declared, f"ctypes table drift: {set(_lib.SIGNATURES) ^ declared}"


def test_library_reads_no_environment_and_product_sources_hold_no_variant_code():
    """include/videogpa_hip.h promises "no global state": the product library imports neither getenv nor setenv (round 5 had seven getenv knobs inside it; they
    are compile-time constants of variant builds now), the product sources carry no kernel that only a variant build compiles (those live in tools/variants/),
    and the dispatch constants of ops.py are not read from the environment."""
    from videogpa_amd import _lib, build
    build.build(verbose=False)
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\b(secure_)?getenv\b|\bsetenv\b|\bputenv\b", und), [ln for ln in und.splitlines() if "env" in ln]
    csrc = os.path.join(ROOT, "videogpa_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h", ".inc")):
            continue
        src = open(os.path.join(csrc, f)).read()
        assert "getenv" not in src, f
        for m in re.finditer(r"#ifdef VGPA_VARIANTS(.*?)#e(ndif|lse)", src, flags=re.S):       # only #include lines of tools/variants/ may sit inside
            body = [ln for ln in m.group(1).splitlines()[1:] if ln.strip()]
            assert all(ln.strip().startswith("#include") for ln in body), (f, body[:3])
    assert not os.path.exists(os.path.join(csrc, "gemm_w1.hip"))
    ops_src = open(os.path.join(ROOT, "videogpa_amd", "ops.py")).read()
    env_reads = set(re.findall(r"environ\.get\(\"([A-Z_0-9]+)\"", ops_src))
    assert env_reads <= {"VGPA_PRECISE_DELTA", "PYTORCH_TUNABLEOP_ENABLED"}, env_reads


def test_pure_host_queries():
    from videogpa_amd import _lib
    assert _lib.query("vgpa_dpo_loss_workspace_bytes", 3) == 3 * 256 * 4 * 8
    # kmax word per (batch, head) + one redo flag per 256-row strip, at the cfg5 self-attention shape (2 x 24 heads, 18 480 tokens -> 73 strips)
    assert _lib.query("vgpa_attn128_fwd_workspace_bytes", 2, 24, 18480) == 4 * 2 * 24 + 4 * 2 * 24 * 73
    assert _lib.query("vgpa_attn128_fwd_workspace_bytes", 0, 24, -1) == 0
    assert _lib.query("vgpa_grad_norm_workspace_bytes") == 1024 * 8
    # the split backward at the headline shape (2 x 48 heads, 17 776 tokens -> 70 tasks of 256 rows per head): the (task, chunk) pairs saturate at one per
    # compute unit (256, also the fallback without a device), each with the dK/dV part = 2 x [256 x 64] fp32
    assert _lib.query("vgpa_attn_bwd_split_workspace_bytes", 2, 48, 17776) == 256 * (2 * 256 * 64 * 4)
    assert _lib.query("vgpa_attn_bwd_split_workspace_bytes", 0, 48, 17776) == 0
    assert _lib.query("vgpa_attn_bwd_split_workspace_bytes", 2, 48, -1) == 0


def test_ops_fail_loudly_without_gpu():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from videogpa_amd import ops
    from videogpa_amd.transformer import CogVideoXTransformer3DModel
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gelu_tanh(torch.zeros(8, dtype=torch.bfloat16))
    m = CogVideoXTransformer3DModel(num_attention_heads=2, num_layers=1, time_embed_dim=32, text_embed_dim=48,
                                    use_rotary_positional_embeddings=True).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 16, 4, 4, dtype=torch.bfloat16), torch.zeros(1, 2, 48, dtype=torch.bfloat16), torch.tensor([1]))


def test_preprocess_shape_host_arithmetic_matches_the_reference_sizing():
    """vgpa_preprocess_shape is host code (no GPU): utils/model_utils.py:36-48,54-71 -- Python's round-half-to-even included -- over a sweep of
    frame sizes, against the oracle's restatement of those lines."""
    import ctypes
    from oracle import preprocess as pp
    from videogpa_amd import _lib
    lib = _lib.load()
    for H in list(range(20, 1200, 37)) + [175, 189, 518, 720, 1080]:
        for W in list(range(24, 2000, 53)) + [518, 1280, 1920]:
            for mode, mi in (("crop", 0), ("pad", 1)):
                nw, nh = pp.output_size(H, W, mode)
                h, w = ctypes.c_int32(), ctypes.c_int32()
                rc = lib.vgpa_preprocess_shape(H, W, mi, ctypes.byref(h), ctypes.byref(w))
                if nw <= 0 or nh <= 0:
                    assert rc != 0
                    continue
                assert rc == 0
                want = (518, 518) if mode == "pad" else (min(nh, 518), nw)
                assert (h.value, w.value) == want, (H, W, mode, (h.value, w.value), want)
