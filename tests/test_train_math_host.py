"""The training arithmetic's interface without a GPU (include/covahip.h, "Training arithmetic"): the header declares the two
functions and the two constants, cova_amd/_lib.py binds them, the Python names agree with the constants, and the command line
lists --math.  The GPU side is tests/test_gpu_train_math.py."""
import ctypes as C
import os
import re
import subprocess
import sys

from cova_amd import _lib as L, train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "covahip.h")) as f:
        return f.read()


def test_header_declares_the_mode():
    h = _header()
    assert re.search(r"\bCOVAHIP_TRAIN_MATH_EXACT\s*=\s*0\b", h)
    assert re.search(r"\bCOVAHIP_TRAIN_MATH_MATRIX\s*=\s*1\b", h)
    assert re.search(r"\bint\s+covahip_train_set_math\s*\(\s*covahip_train\s*\*\s*tr\s*,\s*int\s+math\s*\)\s*;", h)
    assert re.search(r"\bint\s+covahip_train_get_math\s*\(\s*covahip_train\s*\*\s*tr\s*,\s*int\s*\*\s*math\s*\)\s*;", h)


def test_lib_binds_the_functions():
    assert L.PROTOTYPES["covahip_train_set_math"] == (C.c_int, [C.c_void_p, C.c_int])
    assert L.PROTOTYPES["covahip_train_get_math"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])


def test_python_names_follow_the_constants():
    h = _header()
    for name, const in zip(T.MATH_MODES, ("COVAHIP_TRAIN_MATH_EXACT", "COVAHIP_TRAIN_MATH_MATRIX")):
        assert int(re.search(const + r"\s*=\s*(\d+)", h).group(1)) == T.MATH_MODES.index(name)
    assert T.MATH_MODES == ("exact", "matrix")
    for cls in (T.Trainer, T.TrainerSet):
        assert callable(cls.set_math) and isinstance(cls.math, property)


def test_command_line_lists_math(tmp_path):
    post = tmp_path / "p.json"
    post.write_text("{}")
    r = subprocess.run([sys.executable, "-m", "cova_amd.train", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert re.search(r"--math \{exact,matrix\}", r.stdout), r.stdout
    a = T.parse_args(["x.tfrecord", "-o", "out.cvhw"])
    assert a.math == "exact"
    out = ["-o", "out"]
    for extra in (["--set"] + out, ["--resume", "s.state"] + out, ["--eval-only", "w.cvhw"], ["--freeze", "encoder"] + out,
                  ["--freeze-bn"] + out, ["--post", str(post)] + out, ["--windows", "overlap"] + out):
        assert T.parse_args(["x.tfrecord", "--math", "matrix"] + extra).math == "matrix", extra
