"""Structure rules: the product never touches the oracle; required files exist."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_does_not_import_oracle_or_reference():
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|/root/reference", re.M)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "videogpa_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not pat.search(src), f"{f} references the oracle / reference tree"
    for f in ("bench.py", "__graft_entry__.py"):
        assert "/root/reference" not in open(os.path.join(ROOT, f)).read()


def test_required_layout():
    for p in ("include/videogpa_hip.h", "oracle/__init__.py", "tests/golden/make_golden.py", "bench.py", "__graft_entry__.py",
              "DESIGN.md", "INTEGRATION.md", "profiles"):
        assert os.path.exists(os.path.join(ROOT, p)), p


def test_generated_attention_loops_are_in_sync_with_their_generator():
    """csrc/w1_*_loop.inc / *_clobbers.inc are the checked-in output of tools/gen_w1_asm.py (default knobs)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("W1_ABLATE", "W1_KNOBS")}
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_w1_asm.py"), "--check"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr


GENERATED = [os.path.join(ROOT, d, f) for d in ("videogpa_amd/csrc", "tools/variants")
             for f in sorted(os.listdir(os.path.join(ROOT, d))) if f.startswith("w1_") and f.endswith(".inc")]
ATTENTION_LOOPS = {f"w1_{n}_loop.inc" for n in ("dq", "dkv", "fwd", "fwd128", "fwd128f8", "dkv128", "dq128x2")}


def _check_generator(knobs=None, ablate=None):
    """`gen_w1_asm.py --check` (writes nothing) under W1_KNOBS / W1_ABLATE: (exit status, names reported out of date, stderr); the
    checked-in files must be what they were"""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("W1_ABLATE", "W1_KNOBS")}
    if knobs is not None:
        env["W1_KNOBS"] = knobs
    if ablate is not None:
        env["W1_ABLATE"] = ablate
    before = [open(p, "rb").read() for p in GENERATED]
    assert before
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_w1_asm.py"), "--check"], capture_output=True, text=True, env=env)
    assert [open(p, "rb").read() for p in GENERATED] == before
    assert "Traceback" not in r.stderr, r.stderr
    stale = {ln.split(":")[0] for ln in r.stdout.splitlines() if ln.endswith(": out of date")}
    return r.returncode, stale, r.stderr


REMOVED_KNOBS = ("noexp", "nomul", "nocvt", "nop7", "pad", "pkmul", "ringv", "cinit", "vorder")


@pytest.mark.parametrize("knobs, ablate, offender", [("laed=4", None, "laed"), ("lead=4,laed=4", None, "laed"), (None, "nolsd", "nolsd"),
                                                     (None, "novalu,lead", "lead"), ("novalu=1", None, "novalu"), (None, "novalu=1", "novalu"),
                                                     ("lead", None, "lead")]
                         + [(f"{k}=1", None, k) for k in REMOVED_KNOBS])
def test_generator_rejects_an_undeclared_knob_or_ablation(knobs, ablate, offender):
    """a mistyped or retired name must not silently build the product loops: exit status non-zero, the name in the message, nothing generated"""
    rc, stale, err = _check_generator(knobs, ablate)
    assert rc != 0 and not stale
    assert ("W1_KNOBS" if knobs else "W1_ABLATE") in err and re.search(rf"\b{offender}\b", err.split(";")[0]), err


def test_generator_kept_switches_still_generate():
    """the kept knobs and ablations are outside the product path: each must still run to the end and change exactly the files it reaches"""
    # lead: the six bf16 attention loops' fragment lead; not the e4m3 forward (lead8), not the GEMM probe, no clobber list
    rc, stale, _ = _check_generator(knobs="lead=4")
    assert rc == 1 and stale == ATTENTION_LOOPS - {"w1_fwd128f8_loop.inc"}
    # nolds reaches every loop's LDS reads (the GEMM probe's too); mfsum=0 also frees a[128:131] and tells the C++ shell
    rc, stale, _ = _check_generator(knobs="mfsum=0", ablate="novalu,nolds")
    assert rc == 1 and stale == ATTENTION_LOOPS | {"w1_gemm_loop.inc", "w1_fwd_clobbers.inc", "w1_fwd_knobs.inc"}
