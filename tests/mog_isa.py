"""The gfx950 assembly of the MoG labeller's kernel files (cova_amd/csrc/mog_update.hip, mog_post.hip), for the host tests
that assert on it: each file is compiled once per test run, with the library's flags for these files."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMA = re.compile(r"^\s+v_(fma|fmac|mac)_f32", re.M)
SCRATCH = re.compile(r"^\s+scratch_", re.M)


@functools.lru_cache(maxsize=None)
def _compiled(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        return None
    csrc = os.path.join(ROOT, "cova_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src + ".s")
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                            "-I", csrc, "--cuda-device-only", "-S", "-o", out, os.path.join(csrc, src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(out) as f:
            s = f.read()
    bodies = dict(re.findall(r"^(_Z\w*k_mog_\w*):[^\n]*\n(.*?)^\.Lfunc_end", s, re.S | re.M))
    scratch = dict(re.findall(r"\.name:\s+(\S*k_mog_\w*)\n(?:.*\n)*?.*\.private_segment_fixed_size:\s+(\d+)", s))
    vgprs = dict(re.findall(r"\.name:\s+(\S*k_mog_\w*)\n(?:.*\n)*?.*\.vgpr_count:\s+(\d+)", s))
    assert bodies.keys() == scratch.keys() == vgprs.keys()
    return {name: {"body": bodies[name], "scratch": int(scratch[name]), "vgprs": int(vgprs[name])} for name in bodies}


def kernels(src, family):
    """{mangled name: {"body", "scratch", "vgprs"}} of the kernels of csrc/`src` whose name has a match of `family`"""
    all_ = _compiled(src)
    if all_ is None:
        pytest.skip("hipcc not available")
    return {name: k for name, k in all_.items() if re.search(family, name)}


def assert_update_family(family, count):
    """`count` update kernels of the family, none with an f32 fused multiply-add, none with scratch; returns them"""
    ks = kernels("mog_update.hip", family)
    assert len(ks) == count, sorted(ks)
    for name, k in ks.items():
        assert not FMA.search(k["body"]), name
        assert not SCRATCH.search(k["body"]), name
        assert k["scratch"] == 0, name
    return ks


def assert_post_family(family, count):
    """`count` post kernels of the family, none with scratch"""
    ks = kernels("mog_post.hip", family)
    assert len(ks) == count, sorted(ks)
    for name, k in ks.items():
        assert not SCRATCH.search(k["body"]) and k["scratch"] == 0, name
