"""The HIP kernels against the reference's own code, with no oracle in between: the library through the C ABI against
oracle/_ref/libstevi_refpin.so (oracle/ref_pin.cpp, the reference's census, Hamming, matching-function, SGM, winner and truncation
templates compiled by build()).  The library travels with the tree; the reference tree itself is never read here.

Integer, index and bit-pattern outputs must match exactly, float volumes within 1e-4 (the north-star tolerance) with identical NaN masks.
The reference build converts target census words the x86-64 way (rule E2, mode 1: 2^32 -> 0, DESIGN.md section 2;
tests/test_reference_pins.py::test_e2_mode_of_the_reference_build), so census volumes are compared with census_float_overflow = 1.
"""
import numpy as np
import pytest

from oracle import refpin as rp
from helpers import parallax_pair

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)
if not rp.available():
    pytest.skip("oracle/_ref/libstevi_refpin.so was not built: build() found no reference tree", allow_module_level=True)

import libstevi_amd as sv  # noqa: E402
from libstevi_amd import matchingFunctions as MF  # noqa: E402

TOL = 1e-4
DEV = torch.device("cuda:0")
REF_BUILD_E2_MODE = 1
R2L, L2R = sv.dispDirection.RightToLeft, sv.dispDirection.LeftToRight


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def assert_bits(got, exp):
    got = host(got)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    a = got.view(np.uint32) if got.dtype == np.float32 else got.astype(exp.dtype)
    b = exp.view(np.uint32) if exp.dtype == np.float32 else exp
    nbad = int((a != b).sum())
    assert nbad == 0, f"{nbad} of {a.size} elements differ"


def assert_close(got, exp, tol=TOL):
    got = host(got)
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp)), "NaN masks differ"
    both_inf = np.isinf(got) & np.isinf(exp) & (np.sign(got) == np.sign(exp))
    ok = ~np.isnan(exp) & ~both_inf
    err = np.abs(got[ok].astype(np.float64) - exp[ok].astype(np.float64))
    lim = tol * np.maximum(1.0, np.abs(exp[ok].astype(np.float64)))
    assert np.all(err <= lim), f"max err {err.max() if err.size else 0} (tol {tol})"


def with_specials(rng, x, frac=0.03):
    x = x.copy()
    pick = rng.random(x.shape) < frac
    x[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(pick.sum()))
    return x


@pytest.fixture
def ref_e2_mode():
    probe = torch.zeros(1, device=DEV)
    sv.set_option(probe, "census_float_overflow", REF_BUILD_E2_MODE)
    yield
    sv.set_option(probe, "census_float_overflow", 0)


def gradient_pair(H, W, rng):
    """Smooth images falling towards the bottom right: whole census words of ones (>= 0xFFFFFF80, rule E2) with some noise."""
    i, j = np.mgrid[0:H, 0:W].astype(np.float32)
    left = -(i * 1.3 + j) + rng.uniform(0, 0.05, (H, W)).astype(np.float32)
    right = -(i * 1.3 + j * 0.9) + rng.uniform(0, 0.8, (H, W)).astype(np.float32)
    return left.astype(np.float32), right.astype(np.float32)


# ------------------------------------------------------------------------------------------------ census words, Hamming volumes
@pytest.mark.parametrize("h_r,v_r", [(1, 1), (2, 3), (4, 4), (5, 2), (7, 7), (3, 5)])
def test_census_words(rng, h_r, v_r):
    img = with_specials(rng, rng.uniform(-1, 1, (17, 23)).astype(np.float32))
    assert_bits(sv.censusTransform2D(dev(img), h_r, v_r), rp.census_transform(img, h_r, v_r))
    img8 = rng.integers(0, 256, (13, 19)).astype(np.uint8)
    assert_bits(sv.censusTransform2D(dev(img8), h_r, v_r), rp.census_transform(img8, h_r, v_r))
    small = rng.uniform(-1, 1, (3, 4)).astype(np.float32)  # smaller than the window
    assert_bits(sv.censusTransform2D(small, h_r, v_r), rp.census_transform(small, h_r, v_r))


@pytest.mark.parametrize("D", [1, 37, 70])
@pytest.mark.parametrize("ddir", [R2L, L2R])
def test_hamming_volumes(rng, ref_e2_mode, ddir, D):
    left, right = gradient_pair(11, 48, rng)
    noise_l = with_specials(rng, rng.uniform(-1, 1, (9, 29)).astype(np.float32))
    noise_r = with_specials(rng, rng.uniform(-1, 1, (9, 29)).astype(np.float32))
    for func in (MF.CENSUS, MF.HAMMING):
        for l, r in ((left, right), (noise_l, noise_r)):
            for h_r, v_r in ((4, 4), (2, 3)):
                exp = rp.unfold_cost_volume(int(func), l, r, h_r, v_r, D, int(ddir))
                assert_bits(sv.unfoldBasedCostVolume(func, dev(l), dev(r), h_r, v_r, D, ddir), exp)
        l8, r8 = rng.integers(0, 256, (7, 21)).astype(np.uint8), rng.integers(0, 256, (7, 21)).astype(np.uint8)
        assert_bits(sv.unfoldBasedCostVolume(func, dev(l8), dev(r8), 4, 4, D, ddir), rp.unfold_cost_volume(int(func), l8, r8, 4, 4, D, int(ddir)))


# ------------------------------------------------------------------------------------------------ float functions, MEDAD / ZMEDAD
@pytest.mark.parametrize("ddir", [R2L, L2R])
@pytest.mark.parametrize("func", [MF.CC, MF.NCC, MF.SSD, MF.SAD, MF.ZCC, MF.ZNCC, MF.ZSSD, MF.ZSAD])
def test_float_matching_functions(rng, func, ddir):
    for shape, (h_r, v_r), D in (((11, 19), (2, 2), 7), ((7, 13, 3), (1, 2), 16), ((21, 70), (3, 3), 40)):
        l = rng.uniform(0.1, 1, shape).astype(np.float32)
        r = rng.uniform(0.1, 1, shape).astype(np.float32)
        assert_close(sv.unfoldBasedCostVolume(func, dev(l), dev(r), h_r, v_r, D, ddir), rp.unfold_cost_volume(int(func), l, r, h_r, v_r, D, int(ddir)))


@pytest.mark.parametrize("ddir", [R2L, L2R])
@pytest.mark.parametrize("func", [MF.MEDAD, MF.ZMEDAD])
def test_medad_zmedad(rng, func, ddir):
    """Bit for bit on finite inputs (std::nth_element on NaN is undefined: NaN inputs stay with tests/test_gpu_medad.py)."""
    for shape, (h_r, v_r), D in (((9, 17), (1, 1), 6), ((7, 13), (2, 2), 15), ((6, 11, 3), (1, 1), 5), ((12, 40), (3, 3), 20)):
        l = rng.integers(0, 8, shape).astype(np.float32)
        m = rng.random(shape) < 0.5
        l[m] = rng.normal(0, 3, int(m.sum())).astype(np.float32)
        r = rng.normal(0, 3, shape).astype(np.float32)
        assert_bits(sv.unfoldBasedCostVolume(func, dev(l), dev(r), h_r, v_r, D, ddir), rp.unfold_cost_volume(int(func), l, r, h_r, v_r, D, int(ddir)))


# ------------------------------------------------------------------------------------------------ SGM, winner, truncation
SGM_CASES = [((0, 0, 0, 0), (0.001, 0.01, 100.0)), ((1, 2, 3, 1), (2.0, 7.0, 3.0)), ((0, 0, 0, 0), (5.0, 1.0, 0.5)),  # P1 > P2
             ((2, 0, 0, 1), (0.0, 0.0, 0.0)), ((0, 1, 2, 0), (0.3, 0.9, 7.0))]


@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("n_dir", [4, 8])  # the library refuses 16 directions (test_gpu_parity.py::test_sgm_rejects_16_directions)
@pytest.mark.parametrize("D", [1, 2, 5, 70, 256])
def test_sgm_volumes(rng, n_dir, strategy, D):
    for shape in ((9, 12, D), (1, 13, D), (11, 1, D)):
        for integer, specials in ((True, False), (False, True)):
            cv = (rng.integers(0, 65, shape) if integer else rng.uniform(-1, 1, shape)).astype(np.float32)
            if specials:
                cv = with_specials(rng, cv, 0.02)
            for margins, (P1, P2, Pout) in SGM_CASES:
                if margins[2] > shape[1] or margins[3] > shape[0]:  # the reference never returns there (ref_pin.cpp margins_of)
                    continue
                exp = rp.sgm(cv, n_dir, strategy, P1, P2, margins, Pout)
                got = sv.sgmCostVolume(n_dir, strategy, dev(cv), P1, P2, sv.Margins(*margins), Pout)
                assert_bits(got, exp)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_sgm_integer_volumes(rng, dtype):
    hi = {np.uint8: 255, np.int16: 3000, np.int32: 1 << 26}[dtype]
    lo = 0 if dtype == np.uint8 else -hi
    cv = rng.integers(lo, hi, (13, 21, 19)).astype(dtype)
    for strategy in (0, 1):
        assert_bits(sv.sgmCostVolume(8, strategy, dev(cv), 0.5, 2.0, None, 7.0), rp.sgm(cv, 8, strategy, 0.5, 2.0, (0, 0, 0, 0), 7.0))


@pytest.mark.parametrize("D", [1, 3, 8, 65, 300])
def test_winner_and_disparity(rng, D):
    cv = rng.integers(0, 4, (11, 14, D)).astype(np.float32)
    cv[0, 0, 0] = np.nan
    cv[1, :, :] = 2.0
    if D > 2:
        cv[2, 2, D // 2] = np.nan
        cv[3, 3, :] = 1.0
        cv[3, 3, 0] = 0.0
        cv[3, 4, :] = 1.0
        cv[3, 4, D - 1] = 0.0
        cv[4, 4, :] = np.inf
        cv[5, 5, 1:] = np.nan
        cv[6, 6, 0] = np.nan
        cv[6, 6, D - 1] = -np.inf
    for strategy in (0, 1):
        exp = rp.extract_index(cv, strategy)
        assert_bits(sv.extractSelectedIndex(strategy, dev(cv)), exp)
        for ddir in (R2L, L2R):
            assert_bits(sv.selectedIndexToDisp(dev(exp), 3, ddir), rp.index_to_disp(exp, int(ddir), 3))


@pytest.mark.parametrize("sdir", [0, 1, 2])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_truncated_cost_volume(rng, sdir, r):
    H, W, D = 9, 16, 7
    cv = rng.uniform(0, 1, (H, W, D)).astype(np.float32)
    idx = rng.integers(0, D, (H, W)).astype(np.int32)
    idx[:, 0], idx[:, -1], idx[0, :], idx[-1, :] = 0, D - 1, D - 1, 0
    for ddir in (R2L, L2R):
        for h_r, v_r in ((0, 0), (2, 1), (3, 2)):
            exp = rp.truncated_cost_volume(cv, idx, h_r, v_r, r, sdir, int(ddir))
            assert_bits(sv.truncatedCostVolume(dev(cv), dev(idx), h_r, v_r, r, ddir, sdir), exp)


# ------------------------------------------------------------------------------------------------ the call bench.py times
def reference_chain(tgt, src, D, P):
    """censusTransform2D -> unfoldBasedCostVolume<CENSUS> -> sgmCostVolume<8> -> extractSelectedIndex -> selectedIndexToDisp."""
    words_l, words_r = rp.census_transform(tgt, 4, 4), rp.census_transform(src, 4, 4)
    cv = rp.unfold_cost_volume(rp.CENSUS, tgt, src, 4, 4, D)
    vol = rp.sgm(cv, 8, rp.COST, P[0], P[1], (0, 0, 0, 0), P[2])
    return words_l, words_r, rp.index_to_disp(rp.extract_index(vol, rp.COST))


@pytest.mark.parametrize("H,W,D", [(48, 64, 32), (270, 480, 256)])
def test_stereo_match_volume_free(ref_e2_mode, H, W, D):
    """stereoMatch(CENSUS 9x9, SGM-8) with no volume requested: the fused census sweep / scan kernels (tiled and FP4 forms at the larger
    width) against the reference's own chain."""
    src, tgt, _ = parallax_pair(H, W, H // 3, H // 4, W // 3, 2, 9, seed=11)
    P = (0.001, 0.01, 100.0)
    words_l, words_r, disp = reference_chain(tgt, src, D, P)
    assert_bits(sv.censusTransform2D(dev(tgt), 4, 4), words_l)
    res = sv.stereoMatch(MF.CENSUS, dev(tgt), dev(src), 4, 4, D, sgmDirections=8, P1=P[0], P2=P[1], Pout=P[2])
    torch.cuda.synchronize()
    assert_bits(res["disp"], disp)
