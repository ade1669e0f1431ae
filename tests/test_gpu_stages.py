"""Every kernel stage of the HIP BlobNet path against its float64 reference (tests/blobnet_stages.py), on the kernel's own input.

The oracle test of the whole network (tests/test_gpu_blobnet.py) spends most of its tolerance on legitimate fp16 noise and lets
a kernel that drops a 3x3 tap of a level-2 channel pass; a check per stage is about 30x more sensitive.  After each forward the
workspace is read back (include/covahip_dev.h, covahip_dev_blobnet_buffer) and every stage output is checked with
|hip - ref| <= K * u * (rms(ref) + |ref|), u = 2^-11, 2K for the stages that span two levels (blobnet_stages.K).

K = 16 (2K = 32 for E1 / E23 / D012).  Worst ratio |hip - ref| / (u * (rms(ref) + |ref|)) per stage over this module's cases on
MI355X: E0 4.69, E1 9.87, E2 3.98, E3 4.08, E23 8.38, D0 3.75, D1 3.03, D2 2.30, D012 8.18, T 1.59 -- at least 3.2x below the
bound; the fp16 emulation of tests/test_stage_bounds.py reaches 2.3 - 4.4 (9.8 fused), its planted bugs 148 and more.
"""
import os
import re

import pytest

from tests import stage_check
from tests.stage_check import ALWAYS, DEC012, DEC0_2, ENC23, ENC2_3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w, batch, impl, weights, entry, kernels that must launch, kernels that must not).  entry "stack": the stacked tensor through
# covahip_blobnet_forward (unfused tail); "frames": carrier frames with a shuffled stack table through covahip_filter_forward_frames
# (fused tail where it fits).  Every stage is checked at every shape; the sets pin the path of each case.
CASES = [
    (68, 120, 20, "mfma", "seed", "stack", ENC2_3 | DEC012 | {"dec3_final_mfma"}, ENC23),
    (68, 120, 256, "mfma", "seed", "frames", ENC23 | DEC012 | {"dec3_bboxcc_fused"}, ENC2_3),
    (68, 120, 256, "mfma", "smallvar", "stack", ENC23, ENC2_3),
    (67, 120, 16, "mfma", "seed", "stack", {"dec3_final_mfma"}, set()),
    (67, 120, 16, "mfma", "mixed", "frames", {"dec3_bboxcc_fused"}, set()),
    (45, 80, 8, "mfma", "seed", "frames", {"dec3_bboxcc_fused"}, set()),
    (35, 60, 8, "mfma", "mixed", "stack", set(), set()),
    (61, 100, 8, "mfma", "seed", "frames", set(), set()),
    (66, 116, 8, "mfma", "smallvar", "frames", set(), set()),
    (36, 64, 8, "mfma", "seed", "stack", set(), set()),
    (24, 32, 8, "mfma", "seed", "frames", set(), set()),
    (128, 120, 4, "mfma", "seed", "frames", set(), set()),
    (124, 124, 4, "mfma", "mixed", "stack", set(), set()),
    (128, 128, 4, "mfma", "seed", "frames", set(), set()),
    (135, 240, 2, "mfma", "seed", "frames", DEC0_2 | {"dec3_final_mfma"}, DEC012 | {"dec3_bboxcc_fused"}),
    (68, 120, 20, "dec_separate", "mixed", "frames", DEC0_2, DEC012),
    (35, 60, 8, "dec_separate", "smallvar", "stack", DEC0_2, DEC012),
    (67, 120, 16, "enc1_legacy", "seed", "frames", set(), set()),
    (35, 60, 8, "enc1_legacy", "mixed", "stack", set(), set()),
    (68, 120, 20, "enc_general_tiles", "mixed", "stack", ENC2_3, ENC23),
    (45, 80, 8, "enc_general_tiles", "seed", "frames", ENC2_3, ENC23),
    (68, 120, 20, "enc23_force", "mixed", "frames", ENC23, ENC2_3),
    (67, 120, 16, "enc23_force", "smallvar", "stack", ENC23, ENC2_3),
    (68, 120, 256, "enc23_separate", "seed", "frames", ENC2_3, ENC23),
    (68, 120, 20, "tail_skip_tensor", "mixed", "frames", {"dec3_bboxcc_fused"}, set()),
    (67, 120, 16, "tail_skip_tensor", "seed", "stack", {"dec3_final_mfma"}, set()),
    (68, 120, 20, "tail_band_tiles", "seed", "frames", {"dec3_bboxcc_fused"}, set()),
]

_RATIOS = {}   # stage -> worst ratio over the module (printed at the end for the record in the docstring)


PROF_SCOPES = {"enc0p_mfma", "enc1_mfma", "enc2_mfma", "enc3_mfma", "enc23_mfma", "dec012_mfma", "dec0_mfma", "dec1_mfma", "dec2_mfma",
               "dec3_final_mfma", "dec3_bboxcc_fused"}


def _prof_scopes():
    """The profile names blobnet_mfma.hip launches under: the second argument of its launch helper."""
    src = open(os.path.join(ROOT, "cova_amd", "csrc", "blobnet_mfma.hip")).read()
    return set(re.findall(r'\blaunch\(f, "([a-z0-9_]+)"', src))


def test_cases_cover_every_profile_scope():
    """Across the module every kernel of blobnet_mfma.hip's ProfScopes is REQUIRED to launch by some case."""
    assert _prof_scopes() == PROF_SCOPES, sorted(_prof_scopes() ^ PROF_SCOPES)   # (an extraction that finds nothing proves nothing)
    must = ALWAYS.union(*(c[6] for c in CASES))
    assert _prof_scopes() <= must, sorted(_prof_scopes() - must)


@pytest.mark.parametrize("h,w,b,impl,wname,entry,must,mustnot", CASES,
                         ids=[f"{c[0]}x{c[1]}-b{c[2]}-{c[3]}-{c[4]}-{c[5]}" for c in CASES])
def test_stages_against_float64(ctx, h, w, b, impl, wname, entry, must, mustnot):
    stage_check.run(ctx, h, w, b, impl, wname, entry, must, mustnot, _RATIOS)
