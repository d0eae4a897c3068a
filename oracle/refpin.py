"""ctypes loader for oracle/_ref/libstevi_refpin.so: the reference's own correlation templates (oracle/ref_pin.cpp).

TEST INFRASTRUCTURE ONLY, like the oracle: loaded by tests/test_reference_pins.py and tests/test_gpu_reference_pins.py.  The library
exists only where build() found a reference tree (`make -C oracle ref`); available() says whether it is there.

Functions take and return dense numpy arrays with the oracle's conventions (oracle/__init__.py): images [H][W] or [H][W][C], volumes
[H][W][D], census words [H][W][nW] uint32, index / disparity maps [H][W] int32; the enum values are the oracle's.
"""
import ctypes as C
import os

import numpy as np

from . import granted_cpus
from . import CC, NCC, SSD, SAD, ZCC, ZNCC, ZSSD, ZSAD, HAMMING, CENSUS  # noqa: F401  (re-exported enum values)
from . import COST, SCORE, LEFT_TO_RIGHT, RIGHT_TO_LEFT, TCV_SAME, TCV_REVERSED, TCV_BOTH, EQUIANGULAR, PARABOLA, GAUSSIAN  # noqa: F401

MEDAD, ZMEDAD = 8, 9  # correlation/matching_costs.h:48-49

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref", "libstevi_refpin.so")
DEPS_PATH = os.path.join(os.path.dirname(LIB_PATH), "libstevi_refpin.d")

# T_CV of the volumes sgm() takes (ref_pin.cpp: RP_FLOAT32 ...)
_CV_TYPES = {np.dtype(np.float32): 0, np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3, np.dtype(np.int32): 4, np.dtype(np.uint32): 5}
_IMG_TYPES = {np.dtype(np.float32): 0, np.dtype(np.uint8): 1}

_lib = None


class RefPinError(RuntimeError):
    pass


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RefPinError(f"{LIB_PATH} was not built: build() found no reference tree")
        _lib = C.CDLL(LIB_PATH)
        if "OMP_NUM_THREADS" not in os.environ:  # (an explicit request stands)
            _lib.rp_set_num_threads(min(int(_lib.rp_num_threads()), granted_cpus()))
    return _lib


def _check(rc, what):
    if rc:
        raise RefPinError(f"{what}: " + {1: "the reference threw", 2: "argument not dispatched", 3: "unexpected result shape"}.get(rc, f"rc={rc}"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _img(img):
    img = np.ascontiguousarray(img)
    if img.dtype not in _IMG_TYPES:
        img = img.astype(np.float32)
    return img


def _channels(img):
    return 0 if img.ndim == 2 else img.shape[2]


def census_words(F):
    return (F - 1) // 32 + 1


def census_transform(img, h_r, v_r):
    """censusTransform2D<T_I, 2 | 3>(img, h_r, v_r) with the automatic padding: float32 or uint8 images."""
    img = _img(img)
    H, W = img.shape[:2]
    F = (2 * h_r + 1) * (2 * v_r + 1) * max(_channels(img), 1)
    out = np.empty((H, W, census_words(F)), np.uint32)
    _check(lib().rp_census_transform(_IMG_TYPES[img.dtype], _p(img), H, W, _channels(img), int(h_r), int(v_r), _p(out), *out.shape),
           "censusTransform2D")
    return out


def census_features(feat):
    feat = np.ascontiguousarray(feat, np.float32)
    H, W, F = feat.shape
    out = np.empty((H, W, census_words(F)), np.uint32)
    _check(lib().rp_census_features(_p(feat), H, W, F, _p(out), out.shape[2]), "censusFeatures")
    return out


def unfold_cost_volume(func, img_l, img_r, h_r, v_r, D, ddir=RIGHT_TO_LEFT):
    """unfoldBasedCostVolume<func, T, T, 2 | 3, ddir, float>; float32 images for every function, uint8 for HAMMING / CENSUS."""
    img_l, img_r = _img(img_l), _img(img_r)
    assert img_l.dtype == img_r.dtype and img_l.ndim == img_r.ndim
    H, Wl = img_l.shape[:2]
    Wr = img_r.shape[1]
    Ws = Wr if ddir == RIGHT_TO_LEFT else Wl
    cv = np.empty((H, Ws, D), np.float32)
    _check(lib().rp_unfold_cost_volume(int(func), int(ddir), _IMG_TYPES[img_l.dtype], _p(img_l), _p(img_r), H, Wl, Wr, _channels(img_l),
                                       int(h_r), int(v_r), int(D), _p(cv), Ws), "unfoldBasedCostVolume")
    return cv


def _margins(margins):
    return (C.c_int * 4)(*[int(x) for x in margins])


def sgm(cv, n_dir, strategy, P1, P2, margins=(0, 0, 0, 0), Pout=100.0):
    """sgmCostVolume<n_dir, strategy, T_CV>; T_CV = cv.dtype (float32, uint8, uint16, int16, int32, uint32); margins = (left, top, right, bottom)."""
    cv = np.ascontiguousarray(cv)
    H, W, D = cv.shape
    out = np.empty((H, W, D), np.float32)
    _check(lib().rp_sgm(int(n_dir), int(strategy), _CV_TYPES[cv.dtype], _p(cv), H, W, D, C.c_float(P1), C.c_float(P2), _margins(margins),
                        C.c_float(Pout), _p(out)), "sgmCostVolume")
    return out


def sgm_add_direction(sgm_cv, cv, direction, strategy, P1, P2, margins=(0, 0, 0, 0), Pout=100.0):
    """Internal::addDirectionalCost<direction, strategy> into sgm_cv (float32, C-contiguous, updated in place)."""
    cv = np.ascontiguousarray(cv, np.float32)
    assert sgm_cv.dtype == np.float32 and sgm_cv.flags.c_contiguous and sgm_cv.shape == cv.shape
    H, W, D = cv.shape
    _check(lib().rp_sgm_add_direction(int(direction), int(strategy), 0, _p(cv), H, W, D, C.c_float(P1), C.c_float(P2), _margins(margins),
                                      C.c_float(Pout), _p(sgm_cv)), "addDirectionalCost")
    return sgm_cv


def extract_index(cv, strategy):
    cv = np.ascontiguousarray(cv, np.float32)
    H, W, D = cv.shape
    idx = np.empty((H, W), np.int32)
    _check(lib().rp_extract_index(int(strategy), _p(cv), H, W, D, _p(idx)), "extractSelectedIndex")
    return idx


def index_to_disp(idx, ddir=RIGHT_TO_LEFT, offset=0):
    idx = np.ascontiguousarray(idx, np.int32)
    H, W = idx.shape
    out = np.empty_like(idx)
    _check(lib().rp_index_to_disp(int(ddir), _p(idx), H, W, C.c_int32(int(offset)), _p(out)), "selectedIndexToDisp")
    return out


def truncated_cost_volume(cv, idx, h_r, v_r, r, sdir=TCV_SAME, ddir=RIGHT_TO_LEFT):
    cv, idx = np.ascontiguousarray(cv, np.float32), np.ascontiguousarray(idx, np.int32)
    H, W, D = cv.shape
    T = 4 * r + 1 if sdir == TCV_BOTH else 2 * r + 1
    out = np.empty((H, W, T), np.float32)
    _check(lib().rp_truncated_cost_volume(int(sdir), int(ddir), _p(cv), _p(idx), H, W, D, int(h_r), int(v_r), int(r), _p(out), T),
           "truncatedCostVolume")
    return out


def refine_disp(tcv, raw, kernel=PARABOLA):
    tcv, raw = np.ascontiguousarray(tcv, np.float32), np.ascontiguousarray(raw, np.int32)
    H, W, T = tcv.shape
    out = np.empty((H, W), np.float32)
    _check(lib().rp_refine_disp(int(kernel), _p(tcv), _p(raw), H, W, T, _p(out)), "refineDispCostInterpolation")
    return out


def deps():
    """The headers the build of the library read, from its make dependency file (absolute paths, normalised)."""
    with open(DEPS_PATH) as f:
        text = f.read().replace("\\\n", " ")
    first = text.split("\n\n")[0] if "\n\n" in text else text.splitlines()[0]
    return [os.path.normpath(t) for t in first.split(":", 1)[1].split()]
