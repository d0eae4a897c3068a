"""MEDAD / ZMEDAD without a GPU: the committed selection networks (0-1 principle), the drop-in headers' host MedianAbsDiff and traits
against the numpy restatement (tests/medad_ref.py) bit for bit, the compile-time refusals of hierarchical matching and PatchMatch, and the
Python enum values.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as so
import medad_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "libstevi_amd", "include")
NETWORKS = os.path.join(ROOT, "libstevi_amd", "csrc", "svh_median_networks.h")


def committed_networks():
    text = open(NETWORKS).read()
    nets = {}
    for m in re.finditer(r"#define SVH_MEDIAN_NETWORK_(\d+)\(k\) \\\n((?:    SVH_\w+\(k\[\d+\], k\[\d+\]\);(?: \\)?\n)+)", text):
        nets[int(m.group(1))] = [(op, int(i), int(j)) for op, i, j in re.findall(r"SVH_(\w+)\(k\[(\d+)\], k\[(\d+)\]\)", m.group(2))]
    return nets


def test_every_compile_time_size_has_a_committed_network():
    assert sorted(committed_networks()) == [9, 25, 27, 49, 75, 81]


def test_committed_header_is_what_the_generator_writes():
    import io
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_median_networks
    finally:
        sys.path.pop(0)
    buf = io.StringIO()
    gen_median_networks.main(buf)
    assert buf.getvalue() == open(NETWORKS).read()


def run_network(net, wires, lo, hi):
    """Apply a network to wires (list of arrays) with lo / hi the min / max of the element type (bitwise & / | for packed 0-1 inputs)."""
    w = list(wires)
    for op, i, j in net:
        a, b = w[i], w[j]
        if op in ("CE", "MIN"):
            w[i] = lo(a, b)
        if op in ("CE", "MAX"):
            w[j] = hi(a, b)
    return w


@pytest.mark.parametrize("F", [9, 25])
def test_networks_select_rank_f2_on_every_01_input(F):
    """0-1 principle, exhaustive: input x in [0, 2^F) puts bit c of x on wire c; 64 inputs per uint64 word."""
    net = committed_networks()[F]
    n_words = (1 << F) // 64
    word = np.arange(n_words, dtype=np.uint64)
    low = [np.uint64(sum(1 << b for b in range(64) if (b >> c) & 1)) for c in range(6)]
    wires = [np.full(n_words, low[c], np.uint64) for c in range(6)]
    wires += [np.where((word >> np.uint64(c - 6)) & np.uint64(1), np.uint64(~np.uint64(0)), np.uint64(0)) for c in range(6, F)]
    out = run_network(net, wires, np.bitwise_and, np.bitwise_or)[F // 2]
    # expected: rank F//2 of a 0-1 vector is 1 iff it has at least F - F//2 ones
    pc_hi = np.zeros(n_words, np.int64)
    for c in range(F - 6):
        pc_hi += ((word >> np.uint64(c)) & np.uint64(1)).astype(np.int64)
    pc_lo = np.array([bin(b).count("1") for b in range(64)])
    need = F - F // 2
    masks = np.array([np.uint64(sum(1 << b for b in range(64) if ph + pc_lo[b] >= need)) for ph in range(F - 5)], np.uint64)
    assert np.array_equal(out, masks[pc_hi])


@pytest.mark.parametrize("F", [27, 49, 75, 81])
def test_large_networks_on_random_and_ordered_inputs(F):
    net = committed_networks()[F]
    rng = np.random.default_rng(F)
    x = rng.integers(0, 1 << 20, (100000, F)).astype(np.uint32)
    x[:1000] = rng.integers(0, 3, (1000, F))  # many ties
    special = np.stack([np.full(F, 7), np.arange(F), np.arange(F)[::-1]]).astype(np.uint32)
    x = np.concatenate([special, x])
    got = run_network(net, [x[:, c] for c in range(F)], np.minimum, np.maximum)[F // 2]
    assert np.array_equal(got, np.sort(x, axis=1)[:, F // 2])


def test_restated_mean_is_the_librarys_channels_mean():
    rng = np.random.default_rng(3)
    feat = rng.normal(0, 100, (5, 7, 25)).astype(np.float32)
    exp = feat - so.channels_mean(feat)[..., None]
    assert np.array_equal(mr.zero_mean(feat).view(np.uint32), exp.astype(np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("medad_host") / "medad_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "tests", "cpp", "medad_host.cpp"),
                           "-o", out, "-L", os.path.join(ROOT, "libstevi_amd"), "-lstevi_hip", "-Wl,-rpath," + os.path.join(ROOT, "libstevi_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return out


def special_features(rng, H, W, F):
    f = rng.integers(-3, 4, (H, W, F)).astype(np.float32)  # small integers: many ties
    frac = rng.random(f.shape) < 0.3
    f[frac] = rng.normal(0, 2, int(frac.sum())).astype(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -3.4e38], np.float32)
    pick = rng.random(f.shape) < 0.08
    f[pick] = rng.choice(specials, int(pick.sum()))
    return f


@pytest.mark.parametrize("F", [1, 2, 4, 9, 17, 25, 49])
def test_host_median_abs_diff_is_the_restatement(host_exe, tmp_path, F):
    rng = np.random.default_rng(100 + F)
    H, W, D = 3, 11, 5
    fl, fr = special_features(rng, H, W, F), special_features(rng, H, W, F)
    fl[0, :, :] = rng.normal(0, 1, (W, F)).astype(np.float32)  # one row of distinct values
    fl.tofile(tmp_path / "fl.f32")
    fr.tofile(tmp_path / "fr.f32")
    out = subprocess.run([host_exe, str(H), str(W), str(F), str(D), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = np.fromfile(tmp_path / "cv_MEDAD.f32", np.float32).reshape(H, W, D)
    exp = mr.feature_volume(mr.MEDAD, fl, fr, D)
    assert mr.same_bits(got, exp)


@pytest.mark.parametrize("header,call,where", [
    ("correlation/hierarchical.h",
     "StereoVision::Correlation::hiearchicalTruncatedCostVolume<M, 1, float, float>(a, a, {1, 1}, {1, 1}, 8);", "hierarchical matching"),
    ("correlation/hierarchical.h",
     "StereoVision::Correlation::computeGuidedCV<M, float, float>(f, f, g, 2);", "hierarchical matching"),
    ("correlation/patchmatch.h",
     "StereoVision::Correlation::patchMatch<M, 1>(f, f, StereoVision::Correlation::searchOffset<1>(0, 8));", "PatchMatch"),
])
@pytest.mark.parametrize("func", ["MEDAD", "ZMEDAD"])
def test_partial_volume_paths_refuse_median_functions_at_compile_time(tmp_path, header, call, where, func):
    src = tmp_path / "refuse.cpp"
    src.write_text(f"""#include "{header}"
constexpr auto M = StereoVision::Correlation::matchingFunctions::{func};
void f_(Multidim::Array<float, 2> &a, Multidim::Array<float, 3> &f, Multidim::Array<StereoVision::Correlation::disp_t, 2> &g) {{
    (void)a; (void)f; (void)g;
    auto r = {call}
    (void)r;
}}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode != 0
    assert f"MEDAD / ZMEDAD are taken by the whole-volume cost functions only, not by {where}" in out.stderr, out.stderr[-2000:]


def test_the_same_translation_unit_compiles_for_sad(tmp_path):
    """(the refusal above is the new assertion, not a broken test program)"""
    src = tmp_path / "ok.cpp"
    src.write_text("""#include "correlation/hierarchical.h"
#include "correlation/patchmatch.h"
constexpr auto M = StereoVision::Correlation::matchingFunctions::SAD;
void f_(Multidim::Array<float, 2> &a, Multidim::Array<float, 3> &f, Multidim::Array<StereoVision::Correlation::disp_t, 2> &g) {
    auto r = StereoVision::Correlation::hiearchicalTruncatedCostVolume<M, 1, float, float>(a, a, {1, 1}, {1, 1}, 8);
    auto s = StereoVision::Correlation::computeGuidedCV<M, float, float>(f, f, g, 2);
    auto t = StereoVision::Correlation::patchMatch<M, 1>(f, f, StereoVision::Correlation::searchOffset<1>(0, 8));
    (void)r; (void)s; (void)t;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_python_enum_values():
    from libstevi_amd import correlation as corr
    MF = corr.matchingFunctions
    assert int(MF.MEDAD) == 8 and int(MF.ZMEDAD) == 9
    assert corr.matchFuncStrategy(MF.MEDAD) == corr.dispExtractionStartegy.Cost
    assert corr.matchFuncStrategy(MF.ZMEDAD) == corr.dispExtractionStartegy.Cost
    header = open(os.path.join(ROOT, "include", "stevi_hip.h")).read()
    assert "SVH_MEDAD = 8, SVH_ZMEDAD = 9" in header
