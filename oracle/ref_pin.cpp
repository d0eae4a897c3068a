// ref_pin.cpp -- the reference's own correlation templates behind a C ABI (test infrastructure only).
//
// `make -C oracle ref` compiles this file against the reference tree, read in place (never copied into this repository), into
// oracle/_ref/libstevi_refpin.so; oracle/refpin.py loads it.  The tests pin oracle/stevi_oracle.c and the HIP kernels to what the
// reference's census, Hamming, matching-function, SGM, winner, truncation and 1-D refinement code computes
// (tests/test_reference_pins.py, tests/test_gpu_reference_pins.py).
//
// Include path (oracle/Makefile): the reference first (-iquote, so "correlation/..." below resolves there), then oracle/ref_stubs
// (an Eigen stand-in: declarations only, every body throws), then libstevi_amd/include for MultidimArrays only.  The build's
// dependency file (_ref/libstevi_refpin.d) records which header came from where; the tests check it.
//
// Conventions follow oracle/stevi_oracle.c: dense row-major arrays, last index fastest; images [H][W] (C == 0) or [H][W][C],
// volumes [H][W][D], census words [H][W][nW], index / disparity maps [H][W].  The caller allocates every output with the shape the
// reference returns; a different shape is an error.  Every entry point returns 0 on success, 1 when the reference threw (nothing
// crosses the C boundary), 2 for an argument it does not dispatch and 3 when the reference's result has another shape.
#include "correlation/census.h"
#include "correlation/cost_based_refinement.h"
#include "correlation/cross_correlations.h"
#include "correlation/sgm.h"

#include <cstdint>
#include <cstring>
#include <exception>
#include <type_traits>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace SC = StereoVision::Correlation;
using SC::dispDirection;
using SC::dispExtractionStartegy;
using SC::matchingFunctions;

namespace {

enum { RP_OK = 0, RP_THREW = 1, RP_BAD_ARG = 2, RP_BAD_SHAPE = 3 };
enum { RP_FLOAT32 = 0, RP_UINT8 = 1, RP_UINT16 = 2, RP_INT16 = 3, RP_INT32 = 4, RP_UINT32 = 5 };

struct bad_arg {};
struct bad_shape {};

template <class F>
int guarded(F &&f) {
    try {
        f();
        return RP_OK;
    } catch (bad_arg const &) {
        return RP_BAD_ARG;
    } catch (bad_shape const &) {
        return RP_BAD_SHAPE;
    } catch (...) {
        return RP_THREW;
    }
}

// a dense read-only view over caller memory (the reference only reads its inputs)
template <class T, int nDim>
Multidim::Array<T, nDim> view(const void *data, std::array<int, nDim> shape) {
    typename Multidim::Array<T, nDim>::ShapeBlock sh(shape), st;
    int s = 1;
    for (int k = nDim - 1; k >= 0; k--) {
        st[k] = s;
        s *= shape[k];
    }
    return Multidim::Array<T, nDim>(static_cast<T *>(const_cast<void *>(data)), sh, st, false);
}

template <class T, int nDim>
void copy_out(Multidim::Array<T, nDim> const &a, std::array<int, nDim> shape, T *out) {
    for (int k = 0; k < nDim; k++)
        if (a.shape()[k] != shape[k]) throw bad_shape();
    std::size_t n = 1;
    for (int k = 0; k < nDim; k++) n *= static_cast<std::size_t>(shape[k]);
    if (n == 0) return;
    std::array<int, nDim> idx{};
    for (std::size_t e = 0; e < n; e++) {
        out[e] = a.template value<Multidim::AccessCheck::Check>(idx);
        for (int k = nDim - 1; k >= 0; k--) {
            if (++idx[k] < shape[k]) break;
            idx[k] = 0;
        }
    }
}

// calls f(std::integral_constant<...>) with the run-time value v among the listed compile-time values
template <class T, T... Vs, class F>
void dispatch(T v, F &&f) {
    bool hit = ((v == Vs ? (f(std::integral_constant<T, Vs>()), true) : false) || ...);
    if (!hit) throw bad_arg();
}

template <class F>
void with_ddir(int ddir, F &&f) {
    dispatch<dispDirection, dispDirection::LeftToRight, dispDirection::RightToLeft>(static_cast<dispDirection>(ddir), f);
}

template <class F>
void with_strategy(int strategy, F &&f) {
    dispatch<dispExtractionStartegy, dispExtractionStartegy::Cost, dispExtractionStartegy::Score>(
        static_cast<dispExtractionStartegy>(strategy), f);
}

template <class F>
void with_cv_type(int type, F &&f) {
    switch (type) {
    case RP_FLOAT32: f(float()); break;
    case RP_UINT8: f(uint8_t()); break;
    case RP_UINT16: f(uint16_t()); break;
    case RP_INT16: f(int16_t()); break;
    case RP_INT32: f(int32_t()); break;
    case RP_UINT32: f(uint32_t()); break;
    default: throw bad_arg();
    }
}

// addDirectionalCost computes `cv_shape[1] - margins.right()` and `cv_shape[0] - margins.bottom()` as int and loops up to them with a
// size_t (sgm.h:329-352): a right or bottom margin beyond the volume makes that bound ~2^64 and the call never ends.  Refused here.
StereoVision::Margins margins_of(const int m[4], int H, int W) {
    if (!m) return StereoVision::Margins();
    if (m[2] > W || m[3] > H) throw bad_arg();
    return StereoVision::Margins(m[0], m[1], m[2], m[3]);
}

// The 16-direction classes (sgm.h:41-44, UpLeft2Right ... DownLeft2Up) step {0, 1}: neighbouring start lines of one `omp parallel
// for` visit the same pixels, so with several threads the reference's `sgm_cv += ...` (sgm.h:299) is a data race and its sums depend on
// the schedule.  Their only defined result is the sequential one, the order oracle/stevi_oracle.c restates; those calls run on one
// thread.
struct sequential_scope {
    int saved = 0;
    bool active;
    explicit sequential_scope(bool on) : active(on) {
#ifdef _OPENMP
        if (active) {
            saved = omp_get_max_threads();
            omp_set_num_threads(1);
        }
#endif
    }
    ~sequential_scope() {
#ifdef _OPENMP
        if (active) omp_set_num_threads(saved);
#endif
    }
};

template <class T_I>
void census_transform(const void *img, int H, int W, int C, int h_r, int v_r, uint32_t *out, int Ho, int Wo, int nW) {
    Multidim::Array<SC::census_data_t, 3> words;
    if (C == 0)
        words = SC::censusTransform2D<T_I, 2>(view<T_I, 2>(img, {H, W}), h_r, v_r);
    else
        words = SC::censusTransform2D<T_I, 3>(view<T_I, 3>(img, {H, W, C}), h_r, v_r);
    static_assert(sizeof(SC::census_data_t) == sizeof(uint32_t), "census words are 32 bits");
    copy_out<SC::census_data_t, 3>(words, {Ho, Wo, nW}, reinterpret_cast<SC::census_data_t *>(out));
}

template <matchingFunctions func, class T_I, dispDirection dDir>
void cost_volume(const void *l, const void *r, int H, int Wl, int Wr, int C, int h_r, int v_r, int D, float *out, int Ws) {
    Multidim::Array<float, 3> cv;
    if (C == 0)
        cv = SC::unfoldBasedCostVolume<func, T_I, T_I, 2, dDir, float>(view<T_I, 2>(l, {H, Wl}), view<T_I, 2>(r, {H, Wr}), h_r, v_r, D);
    else
        cv = SC::unfoldBasedCostVolume<func, T_I, T_I, 3, dDir, float>(view<T_I, 3>(l, {H, Wl, C}), view<T_I, 3>(r, {H, Wr, C}), h_r,
                                                                        v_r, D);
    copy_out<float, 3>(cv, {H, Ws, D}, out);
}

template <SC::sgmDirections dir, dispExtractionStartegy S, class T_CV>
void add_direction(Multidim::Array<T_CV, 3> const &cv, Multidim::Array<float, 3> &sgm, float P1, float P2, StereoVision::Margins const &m,
                   float Pout) {
    SC::Internal::addDirectionalCost<dir, S>(cv, sgm, P1, P2, m, Pout);
}

} // namespace

extern "C" {

int rp_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

void rp_set_num_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

// censusTransform2D<T_I, 2 | 3> (census.h:117-130); dtype RP_FLOAT32 or RP_UINT8; C == 0: a 2-D image
int rp_census_transform(int dtype, const void *img, int H, int W, int C, int h_r, int v_r, uint32_t *out, int Ho, int Wo, int nW) {
    return guarded([&] {
        if (dtype == RP_FLOAT32)
            census_transform<float>(img, H, W, C, h_r, v_r, out, Ho, Wo, nW);
        else if (dtype == RP_UINT8)
            census_transform<uint8_t>(img, H, W, C, h_r, v_r, out, Ho, Wo, nW);
        else
            throw bad_arg();
    });
}

// censusFeatures on a [H][W][F] float feature volume (census.h:69-115)
int rp_census_features(const float *feat, int H, int W, int F, uint32_t *out, int nW) {
    return guarded([&] {
        auto words = SC::censusFeatures(view<float, 3>(feat, {H, W, F}));
        copy_out<SC::census_data_t, 3>(words, {H, W, nW}, reinterpret_cast<SC::census_data_t *>(out));
    });
}

// unfoldBasedCostVolume<func, T, T, 2 | 3, dDir, float> (cross_correlations.h:740-765); out has the shape [H][Ws][D]
int rp_unfold_cost_volume(int func, int ddir, int dtype, const void *l, const void *r, int H, int Wl, int Wr, int C, int h_r, int v_r,
                          int D, float *out, int Ws) {
    return guarded([&] {
        with_ddir(ddir, [&](auto dd) {
            constexpr dispDirection dDir = decltype(dd)::value;
            if (dtype == RP_FLOAT32) {
                dispatch<matchingFunctions, matchingFunctions::CC, matchingFunctions::NCC, matchingFunctions::SSD, matchingFunctions::SAD,
                         matchingFunctions::ZCC, matchingFunctions::ZNCC, matchingFunctions::ZSSD, matchingFunctions::ZSAD,
                         matchingFunctions::MEDAD, matchingFunctions::ZMEDAD, matchingFunctions::HAMMING, matchingFunctions::CENSUS>(
                    static_cast<matchingFunctions>(func), [&](auto f) {
                        cost_volume<decltype(f)::value, float, dDir>(l, r, H, Wl, Wr, C, h_r, v_r, D, out, Ws);
                    });
            } else if (dtype == RP_UINT8) { // the census functions only: the reference's uint8 normalised paths are broken
                dispatch<matchingFunctions, matchingFunctions::HAMMING, matchingFunctions::CENSUS>(
                    static_cast<matchingFunctions>(func), [&](auto f) {
                        cost_volume<decltype(f)::value, uint8_t, dDir>(l, r, H, Wl, Wr, C, h_r, v_r, D, out, Ws);
                    });
            } else {
                throw bad_arg();
            }
        });
    });
}

// sgmCostVolume<4 | 8 | 16, Cost | Score, T_CV> (sgm.h:360-407); margins = left, top, right, bottom
int rp_sgm(int n_dir, int strategy, int cv_type, const void *cv, int H, int W, int D, float P1, float P2, const int margins[4],
           float Pout, float *out) {
    return guarded([&] {
        with_cv_type(cv_type, [&](auto t) {
            using T_CV = decltype(t);
            auto base = view<T_CV, 3>(cv, {H, W, D});
            with_strategy(strategy, [&](auto s) {
                sequential_scope seq(n_dir == 16);
                dispatch<int, 4, 8, 16>(n_dir, [&](auto n) {
                    auto sgm = SC::sgmCostVolume<decltype(n)::value, decltype(s)::value, T_CV>(base, P1, P2, margins_of(margins, H, W), Pout);
                    copy_out<float, 3>(sgm, {H, W, D}, out);
                });
            });
        });
    });
}

// Internal::addDirectionalCost<direction, strategy> (sgm.h:313-356) on float volumes: adds one direction's path costs minus the
// base cost into sgm_inout, as sgmCostVolume does for each of its directions
int rp_sgm_add_direction(int direction, int strategy, int cv_type, const void *cv, int H, int W, int D, float P1, float P2,
                         const int margins[4], float Pout, float *sgm_inout) {
    return guarded([&] {
        if (cv_type != RP_FLOAT32) throw bad_arg();
        auto base = view<float, 3>(cv, {H, W, D});
        auto sgm = view<float, 3>(sgm_inout, {H, W, D});
        StereoVision::Margins m = margins_of(margins, H, W);
        using SD = SC::sgmDirections;
        sequential_scope seq(direction >= static_cast<int>(SD::UpLeft2Right));
        with_strategy(strategy, [&](auto s) {
            constexpr dispExtractionStartegy S = decltype(s)::value;
            dispatch<SD, SD::Up2Down, SD::Down2Up, SD::Left2Right, SD::Right2Left, SD::UpLeft2DownRight, SD::DownRight2UpLeft,
                     SD::UpRight2DownLeft, SD::DownLeft2UpRight, SD::UpLeft2Right, SD::DownRight2Left, SD::UpRight2Left,
                     SD::DownLeft2Right, SD::UpLeft2Down, SD::DownRight2Up, SD::UpRight2Down, SD::DownLeft2Up>(
                static_cast<SD>(direction), [&](auto d) { add_direction<decltype(d)::value, S, float>(base, sgm, P1, P2, m, Pout); });
        });
    });
}

// extractSelectedIndex<Cost | Score, float> (correlation_base.h:427-464)
int rp_extract_index(int strategy, const float *cv, int H, int W, int D, int32_t *idx) {
    return guarded([&] {
        with_strategy(strategy, [&](auto s) {
            auto sel = SC::extractSelectedIndex<decltype(s)::value, float>(view<float, 3>(cv, {H, W, D}));
            copy_out<SC::disp_t, 2>(sel, {H, W}, idx);
        });
    });
}

// selectedIndexToDisp<disp_t, dDir> (correlation_base.h:511-532)
int rp_index_to_disp(int ddir, const int32_t *idx, int H, int W, int32_t offset, int32_t *disp) {
    return guarded([&] {
        with_ddir(ddir, [&](auto dd) {
            auto d = SC::selectedIndexToDisp<SC::disp_t, decltype(dd)::value>(view<SC::disp_t, 2>(idx, {H, W}), offset);
            copy_out<SC::disp_t, 2>(d, {H, W}, disp);
        });
    });
}

// truncatedCostVolume<float, dDir, sdir> (correlation_base.h:579-671); out has the shape [H][W][T]
int rp_truncated_cost_volume(int sdir, int ddir, const float *cv, const int32_t *idx, int H, int W, int D, int h_r, int v_r, int r,
                             float *out, int T) {
    return guarded([&] {
        using TD = SC::truncatedCostVolumeDirection;
        with_ddir(ddir, [&](auto dd) {
            dispatch<TD, TD::Same, TD::Reversed, TD::Both>(static_cast<TD>(sdir), [&](auto sd) {
                auto tcv = SC::truncatedCostVolume<float, decltype(dd)::value, decltype(sd)::value>(
                    view<float, 3>(cv, {H, W, D}), view<SC::disp_t, 2>(idx, {H, W}), h_r, v_r, r);
                copy_out<float, 3>(tcv, {H, W, T}, out);
            });
        });
    });
}

// refineDispCostInterpolation<Equiangular | Parabola | Gaussian> (cost_based_refinement.h:128-163)
int rp_refine_disp(int kernel, const float *tcv, const int32_t *raw, int H, int W, int T, float *refined) {
    return guarded([&] {
        using IK = SC::InterpolationKernel;
        dispatch<IK, IK::Equiangular, IK::Parabola, IK::Gaussian>(static_cast<IK>(kernel), [&](auto k) {
            auto ref = SC::refineDispCostInterpolation<decltype(k)::value>(view<float, 3>(tcv, {H, W, T}), view<SC::disp_t, 2>(raw, {H, W}));
            copy_out<float, 2>(ref, {H, W}, refined);
        });
    });
}

} // extern "C"
