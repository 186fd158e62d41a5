"""The host-compilable part of tap-net_amd/csrc/tap_step_seam.h, compiled with g++ (tests/host/step_seam_host.cpp): the
strided feature writer every container-per-thread, -wave and -workgroup kernel calls, against numpy on random
height-maps -- all three forms, 2D and 3D with L not dividing the stride, strides 1, 64 and 256 emulated by one call per
member -- and the admission function on a table.  No GPU needed; the kernels that call the header are compared with the
oracle in tests/test_step_seam_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, ZERO, DIFF = 0, 1, 2                                        # TAP_FEAT_* (tapenv.h)


@pytest.fixture(scope="module")
def seam(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("seam") / "libseam.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(ROOT, "tap-net_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "step_seam_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.seam_feature.restype = None
    lib.seam_feature.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p] + [C.c_int] * 3
    lib.seam_admit.restype = C.c_int
    lib.seam_admit.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)]
    return lib


def _want(feature, D, W, L, hm):
    g = hm.reshape(W, L).astype(np.int64)
    if feature == DIFF:
        if D == 2:
            return np.diff(g[:, 0])
        dx, dy = np.zeros_like(g), np.zeros_like(g)
        dx[1:] = g[1:] - g[:-1]
        dy[:, 1:] = g[:, 1:] - g[:, :-1]
        return np.concatenate([dx.reshape(-1), dy.reshape(-1)])
    return g.reshape(-1) - (g.min() if feature == ZERO else 0)


@pytest.mark.parametrize("stride", [1, 64, 256])
@pytest.mark.parametrize("feature", [FULL, ZERO, DIFF], ids=["full", "zero", "diff"])
def test_feature_writer_against_numpy(seam, feature, stride):
    rng = np.random.RandomState(11 + stride)
    shapes = [(2, W, 1) for W in (1, 2, 63, 64, 65, 300)] + [(3, 9, 8), (3, 9, 9), (3, 10, 10), (3, 65, 65), (3, 3, 100), (3, 20, 1),
                                                             (3, 1, 7), (3, 17, 300)]
    for D, W, L in shapes:
        hm = rng.randint(0, 40, size=W * L).astype(np.int32)
        want = _want(feature, D, W, L, hm)
        out = np.full(max(len(want), 1) + 2, -7.0, np.float32)                    # two guard values behind the feature
        for first in range(stride):                                               # one call per member of the unit
            seam.seam_feature(feature, D, W, L, hm.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), first, stride,
                              int(hm.min()))
        assert np.array_equal(out[:len(want)], want.astype(np.float32)), (D, W, L)
        assert (out[len(want):] == -7.0).all(), (D, W, L)


# (act, count, n_max, (bx, by, bz), family_rejects) -> (do_step, err)
ADMIT = [((1, 0, 4, (1, 1, 1), 0), (1, 0)), ((1, 3, 4, (5, 1, 2), 0), (1, 0)),
         ((1, 4, 4, (1, 1, 1), 0), (0, 2)), ((1, 9, 4, (1, 1, 1), 0), (0, 2)),          # full
         ((1, 0, 4, (0, 1, 1), 0), (0, 4)), ((1, 0, 4, (1, 0, 1), 0), (0, 4)), ((1, 0, 4, (1, 1, -3), 0), (0, 4)),   # a side < 1
         ((1, 0, 4, (17, 2, 1), 1), (0, 4)), ((1, 0, 4, (17, 2, 1), 0), (1, 0)),        # the family's own limit, passed in
         ((1, 4, 4, (0, 1, 1), 0), (0, 6)), ((1, 4, 4, (2, 2, 1), 1), (0, 6)),          # full and bad: both bits
         ((0, 0, 4, (1, 1, 1), 0), (0, 0)), ((0, 4, 4, (0, 0, 0), 1), (0, 0))]          # idle: neither stepped nor flagged


def test_admission_table(seam):
    for (act, count, n_max, (bx, by, bz), fam), want in ADMIT:
        err = C.c_int(-1)
        go = seam.seam_admit(act, count, n_max, bx, by, bz, fam, C.byref(err))
        assert (go, err.value) == want, (act, count, n_max, bx, by, bz, fam)
