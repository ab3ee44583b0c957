"""The masks of tests/test_gpu_finalize_one.py for the multi-element rule (cmatrices.c:524-534), on the CPU: the checker
leaves exactly the intended length-1 columns of the GLRLM zero, so the GPU cases test what they claim to test."""
import numpy as np

from test_gpu_finalize_one import AXIS_X, MULTI, SHAPE
from test_gpu_fw import _levels


def test_multi_masks_mean_what_they_say(checker):
    """the reference on the CPU: the masks leave exactly the intended length-1 columns zero"""
    img = _levels(13, SHAPE, 32, "uniform")
    for name, (mk, keeps) in MULTI.items():
        mask = mk()
        er, ang = checker.calculate_glrlm(img, mask, 32, 130, False, 0)
        for n, a in enumerate(ang):
            a = tuple(int(c) for c in a)
            want = True if keeps is None else bool(keeps(a))
            assert bool(er[0][:, 0, n].any()) == want, (name, a)
            if name in ("checkerboard", "two-on-a-row") and a == AXIS_X:
                assert er[0][:, 1:, n].sum() == 0     # kept although the angle has no run longer than 1
