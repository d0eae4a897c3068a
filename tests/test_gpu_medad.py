"""MEDAD / ZMEDAD on the GPU against the numpy restatement (tests/medad_ref.py), bit for bit (equal NaN masks): feature and image volumes,
1-D and 2-D, both directions, every compile-time F and several generic ones, the per-voxel form, the fused pipeline and its refusals."""
import numpy as np
import pytest

import oracle as so
import medad_ref as mr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import libstevi_amd as sv  # noqa: E402
from libstevi_amd import matchingFunctions as MF  # noqa: E402

DEV = torch.device("cuda:0")
R2L, L2R = sv.dispDirection.RightToLeft, sv.dispDirection.LeftToRight
FUNCS = [MF.MEDAD, MF.ZMEDAD]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def assert_same(got, exp):
    got = host(got)
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp)), "NaN masks differ"
    ok = ~np.isnan(exp)
    nbad = int((got[ok].view(np.uint32) != exp[ok].view(np.uint32)).sum())
    assert nbad == 0, f"{nbad} of {exp.size} voxels differ"


def image(rng, H, W, C=None, specials=False):
    shp = (H, W) if C is None else (H, W, C)
    x = rng.integers(0, 8, shp).astype(np.float32)  # small integers: ties
    m = rng.random(shp) < 0.5
    x[m] = rng.normal(0, 3, int(m.sum())).astype(np.float32)
    if specials:
        pick = rng.random(shp) < 0.04
        x[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), int(pick.sum()))
    return x


def set_form(value):
    sv.set_test_option(dev(np.zeros(1, np.float32)), "median_form", value)


@pytest.fixture(params=[0, 1, 2], ids=["auto", "select", "per_voxel"])
def form(request):
    set_form(request.param)
    yield request.param
    set_form(0)


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("C,h_r,v_r", [(None, 0, 0), (None, 1, 1), (None, 2, 2), (None, 3, 3), (None, 4, 4), (None, 3, 1), (3, 1, 1), (3, 2, 2),
                                       (2, 1, 1), (4, 1, 2), (None, 1, 2)])
@pytest.mark.parametrize("ddir", [R2L, L2R])
def test_unfold_volume_is_the_restatement(form, func, C, h_r, v_r, ddir):
    rng = np.random.default_rng(hash((int(func), C, h_r, v_r, int(ddir))) % 1000)
    l, r = image(rng, 13, 37, C, specials=True), image(rng, 13, 37, C, specials=True)
    D = 19
    got = sv.unfoldBasedCostVolume(func, dev(l), dev(r), h_r, v_r, D, ddir)
    assert_same(got, mr.image_volume(int(func), l, r, h_r, v_r, D, int(ddir)))


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("F", [1, 2, 9, 17, 25, 27, 33, 49, 75, 81, 150])
@pytest.mark.parametrize("D", [1, 7, 64, 100, 300])
def test_feature_volume_is_the_restatement(func, F, D):
    rng = np.random.default_rng(F * 1000 + D)
    W = 40 if D < 100 else 90  # narrower than D: the zero target vector
    fl, fr = image(rng, 5, W, F, specials=True), image(rng, 5, W + 3, F, specials=True)
    for ddir in (R2L, L2R):
        for lower in (0, -5, 3):
            exp = mr.feature_volume(int(func), fl, fr, D, int(ddir), lower)
            assert_same(sv.featureVolume2CostVolume(func, dev(fl), dev(fr), sv.searchOffset1(lower, lower + D - 1), ddir), exp)
    assert_same(sv.featureVolume2CostVolume(func, fl, fr, D), mr.feature_volume(int(func), fl, fr, D))  # host arrays


def test_network_and_bitwise_selection_agree_on_every_compile_time_f():
    rng = np.random.default_rng(5)
    for F in (9, 25, 27, 49, 75, 81):
        fl, fr = image(rng, 6, 70, F), image(rng, 6, 70, F)
        vols = []
        for form in (0, 1, 2):
            set_form(form)
            vols.append(host(sv.featureVolume2CostVolume(MF.MEDAD, dev(fl), dev(fr), 80)))
        set_form(0)
        exp = mr.feature_volume(mr.MEDAD, fl, fr, 80)
        for v in vols:
            assert_same(v, exp)


@pytest.mark.parametrize("func", FUNCS)
def test_2d_volumes_are_the_restatement(func):
    rng = np.random.default_rng(int(func))
    l, r = image(rng, 14, 22, specials=True), image(rng, 14, 22, specials=True)
    o = sv.searchOffset2(-2, 3, -1, 9)
    got = sv.unfoldBased2dDisparityCostVolume(func, dev(l), dev(r), 1, 1, o)
    assert_same(got, mr.image_volume_2d(int(func), l, r, 1, 1, (-2, 3), (-1, 9)))
    fl, fr = image(rng, 14, 22, 17), image(rng, 14, 25, 17)
    got = sv.featureVolume2CostVolume(func, dev(fl), dev(fr), o, L2R)
    assert_same(got, mr.feature_volume_2d(int(func), fl, fr, (-2, 3), (-1, 9), int(L2R)))


def test_medad_radius_zero_grey_is_sad():
    rng = np.random.default_rng(9)
    l, r = image(rng, 20, 50), image(rng, 20, 50)
    for ddir in (R2L, L2R):
        a = host(sv.unfoldBasedCostVolume(MF.MEDAD, dev(l), dev(r), 0, 0, 33, ddir))
        b = host(sv.unfoldBasedCostVolume(MF.SAD, dev(l), dev(r), 0, 0, 33, ddir))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_zmedad_of_an_offset_pair_is_medad_of_the_zero_meaned_pair():
    rng = np.random.default_rng(10)
    fs = rng.integers(0, 16, (6, 30, 25)).astype(np.float32)
    ft = fs + np.float32(4.0)  # exact
    z = host(sv.featureVolume2CostVolume(MF.ZMEDAD, dev(fs), dev(ft), 12))
    m = host(sv.featureVolume2CostVolume(MF.MEDAD, dev(mr.zero_mean(fs)), dev(mr.zero_mean(ft)), 12))
    assert np.array_equal(z.view(np.uint32), m.view(np.uint32))


def test_feature_volume_for_match_func():
    rng = np.random.default_rng(12)
    f = image(rng, 7, 9, 25)
    assert np.array_equal(host(sv.getFeatureVolumeForMatchFunc(MF.MEDAD, dev(f))).view(np.uint32), f.view(np.uint32))
    assert np.array_equal(host(sv.getFeatureVolumeForMatchFunc(MF.ZMEDAD, dev(f))).view(np.uint32), mr.zero_mean(f).view(np.uint32))


def test_full_hd_grey_5x5():
    rng = np.random.default_rng(13)
    l, r = image(rng, 1080, 1920), image(rng, 1080, 1920)
    got = host(sv.unfoldBasedCostVolume(MF.MEDAD, dev(l), dev(r), 2, 2, 64))
    rows = [0, 1, 537, 1078, 1079]
    exp = mr.feature_volume(mr.MEDAD, mr.unfold(l, 2, 2)[rows], mr.unfold(r, 2, 2)[rows], 64)
    assert_same(got[rows], exp)


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("n_dir", [0, 8])
@pytest.mark.parametrize("refine", [None, sv.InterpolationKernel.Parabola])
def test_stereo_match_is_the_chain_on_the_restated_volume(func, n_dir, refine):
    rng = np.random.default_rng(int(func) * 10 + n_dir)
    tgt, src = image(rng, 24, 40), image(rng, 24, 40)
    D, P = 20, (0.5, 2.0, 9.0)
    cv = mr.image_volume(int(func), tgt, src, 2, 2, D)
    vol = so.sgm(cv, n_dir, so.COST, P[0], P[1], (0, 0, 0, 0), P[2]) if n_dir else cv
    idx = so.extract_index(vol, so.COST)
    disp = so.index_to_disp(idx)
    for mk in (lambda x: x, dev):
        res = sv.stereoMatch(func, mk(tgt), mk(src), 2, 2, D, sgmDirections=n_dir, P1=P[0], P2=P[1], Pout=P[2], refineKernel=refine,
                             want_cv=True, want_sgm_cv=bool(n_dir))
        assert_same(res["cv"], cv)
        if n_dir:
            assert_same(res["sgm_cv"], vol)
        assert np.array_equal(host(res["disp"]), disp)
        if refine is not None:
            exp = so.refine_disp(so.truncated_cost_volume(vol, idx, 0, 0, 1), idx, so.PARABOLA)
            assert np.allclose(host(res["refined"]), exp, atol=1e-4, equal_nan=True)
        lean = sv.stereoMatch(func, mk(tgt), mk(src), 2, 2, D, sgmDirections=n_dir, P1=P[0], P2=P[1], Pout=P[2])
        assert np.array_equal(host(lean["disp"]), disp)


@pytest.mark.parametrize("func", FUNCS)
def test_keep_minima_and_keep_winner(func):
    rng = np.random.default_rng(21)
    l, r = image(rng, 20, 48), image(rng, 20, 48)
    exp = mr.image_volume(int(func), l, r, 1, 1, 24)
    for kw in ({"keep_minima": True}, {"keep_winner": True}):
        cv = sv.unfoldBasedCostVolume(func, dev(l), dev(r), 1, 1, 24, **kw)
        assert_same(cv, exp)
        assert np.array_equal(host(sv.extractSelectedIndex(sv.dispExtractionStartegy.Cost, cv)), so.extract_index(exp, so.COST))
        sg = sv.sgmCostVolume(8, sv.dispExtractionStartegy.Cost, cv, 0.5, 2.0, None, 9.0)
        assert_same(sg, so.sgm(exp, 8, so.COST, 0.5, 2.0, (0, 0, 0, 0), 9.0))


def test_uint8_medad_is_the_float_path():
    rng = np.random.default_rng(22)
    l8, r8 = rng.integers(0, 256, (16, 40), dtype=np.uint8), rng.integers(0, 256, (16, 40), dtype=np.uint8)
    a = host(sv.unfoldBasedCostVolume(MF.MEDAD, dev(l8), dev(r8), 2, 2, 16))
    b = host(sv.unfoldBasedCostVolume(MF.MEDAD, dev(l8.astype(np.float32)), dev(r8.astype(np.float32)), 2, 2, 16))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    d = sv.stereoMatch(MF.MEDAD, dev(l8), dev(r8), 2, 2, 16)["disp"]
    assert np.array_equal(host(d), so.index_to_disp(so.extract_index(b, so.COST)))


def refused(call):
    with pytest.raises(sv._capi.SvhError) as e:
        call()
    assert e.value.status == sv._capi.ERR_UNSUPPORTED
    return str(e.value)


def test_refusals():
    rng = np.random.default_rng(23)
    l8 = rng.integers(0, 256, (16, 40), dtype=np.uint8)
    refused(lambda: sv.unfoldBasedCostVolume(MF.ZMEDAD, dev(l8), dev(l8), 1, 1, 8))
    img = image(rng, 16, 40)
    f = image(rng, 16, 40, 9)
    guide = torch.zeros((16, 40), dtype=torch.int32, device=DEV)
    for func in FUNCS:
        msg = refused(lambda: sv.computeGuidedCV(func, dev(f), dev(f), guide, 2))
        assert func.name in msg
        refused(lambda: sv.hiearchicalTruncatedCostVolume(func, 1, dev(img), dev(img), [1, 1], [1, 1], 8))
        refused(lambda: sv.cachelessPatchMatch(func, dev(img), dev(img), 1, (0, 8)))
        refused(lambda: sv.stereoMatch(func, dev(img), dev(img), 1, 1, 16, shard=(0, 8)))
    refused(lambda: sv.censusShardKeys(dev(img), dev(img), 1, 1, 16, (0, 8), matchFunc=MF.MEDAD))
