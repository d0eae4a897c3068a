// MEDAD / ZMEDAD in the drop-in headers, host side: MedianAbsDiff on both containers, MatchingFunctionTraits<MEDAD / ZMEDAD>, and a small
// volume built the way aggregateCost builds it -- featureComparison on 1-D views of the source vector and of the target vector of
// pixel (i, j + d), the zero vector past the right edge (RightToLeft).  No GPU call.
//
//   medad_host <H> <W> <F> <D> <dir>
// reads dir/{fl,fr}.f32 (H, W, F) feature volumes (already zero-meaned for ZMEDAD: featureComparison is the same function for both) and
// writes dir/cv_MEDAD.f32; tests/test_medad.py compares it with the numpy restatement.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "correlation/cross_correlations.h"
#include "correlation/matching_costs.h"

namespace SC = StereoVision::Correlation;
using SC::matchingFunctions;

// the traits constants of matching_costs.h:591-651
using TM = SC::MatchingFunctionTraits<matchingFunctions::MEDAD>;
using TZ = SC::MatchingFunctionTraits<matchingFunctions::ZMEDAD>;
static_assert(!TM::ZeroMean && !TM::Normalized && !TM::isCensusBased && TM::extractionStrategy == SC::dispExtractionStartegy::Cost);
static_assert(TZ::ZeroMean && !TZ::Normalized && !TZ::isCensusBased && TZ::extractionStrategy == SC::dispExtractionStartegy::Cost);
static_assert(SC::HipBridge::onGpuPath<matchingFunctions::MEDAD>() && SC::HipBridge::onGpuPath<matchingFunctions::ZMEDAD>());
static_assert(SC::HipBridge::wholeVolumeOnly<matchingFunctions::MEDAD>() && !SC::HipBridge::wholeVolumeOnly<matchingFunctions::SAD>());
static_assert(!SC::HipBridge::onGpuPath<matchingFunctions::KERMI>());
static_assert(SC::defaultCvValForMatchFunc<matchingFunctions::MEDAD>() == std::numeric_limits<float>::max());
static_assert(std::is_same_v<SC::MatchingFuncComputeTypeInfos<matchingFunctions::MEDAD, uint8_t>::FeatureType, uint8_t>);
static_assert(std::is_same_v<SC::MatchingFuncComputeTypeInfos<matchingFunctions::ZMEDAD, uint8_t>::FeatureType, int16_t>);

template <class T> static std::vector<T> slurp(std::string const &path, std::size_t n) {
    std::vector<T> v(n);
    std::ifstream in(path, std::ios::binary);
    in.read(reinterpret_cast<char *>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
    if (static_cast<std::size_t>(in.gcount()) != n * sizeof(T)) {
        fprintf(stderr, "short read: %s\n", path.c_str());
        exit(2);
    }
    return v;
}

static uint32_t bits(float x) {
    uint32_t w;
    std::memcpy(&w, &x, sizeof w);
    return w;
}

int main(int argc, char **argv) {
    if (argc != 6) return 1;
    const int H = atoi(argv[1]), W = atoi(argv[2]), F = atoi(argv[3]), D = atoi(argv[4]);
    const std::string dir = argv[5];
    if (std::string(TM::Name) != "MEDAD" || std::string(TZ::Name) != "ZMEDAD") {
        fprintf(stderr, "names\n");
        return 3;
    }
    auto fl = slurp<float>(dir + "/fl.f32", static_cast<std::size_t>(H) * W * F), fr = slurp<float>(dir + "/fr.f32", static_cast<std::size_t>(H) * W * F);
    std::vector<float> cv(static_cast<std::size_t>(H) * W * D), zeros(F, 0.0f);
    using View = Multidim::Array<float, 1, Multidim::ConstView>;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++)
            for (int d = 0; d < D; d++) { // source = right, target = left (RightToLeft)
                float *sp = &fr[(static_cast<std::size_t>(i) * W + j) * F];
                float *tp = j + d < W ? &fl[(static_cast<std::size_t>(i) * W + j + d) * F] : zeros.data();
                Multidim::Array<float, 1> s(sp, {F}, {1}), t(tp, {F}, {1});
                View sv(s), tv(t);
                const float a = TM::featureComparison<float, float, float>(sv, tv);
                const float b = TZ::featureComparison<float, float, float>(sv, tv);
                // the std::vector overload gives the same bits
                const float c = SC::MedianAbsDiff<float, float>(std::vector<float>(sp, sp + F), std::vector<float>(tp, tp + F));
                if (bits(a) != bits(b) || bits(a) != bits(c)) {
                    fprintf(stderr, "overloads disagree at (%d, %d, %d)\n", i, j, d);
                    return 3;
                }
                cv[(static_cast<std::size_t>(i) * W + j) * D + d] = a;
            }
    std::ofstream(dir + "/cv_MEDAD.f32", std::ios::binary).write(reinterpret_cast<const char *>(cv.data()), static_cast<std::streamsize>(cv.size() * sizeof(float)));
    // integer inputs: differences in the output type, exact
    std::vector<uint8_t> p{200, 100, 7, 9}, q{3, 250, 9, 9};
    if (SC::MedianAbsDiff<uint8_t, uint8_t, int32_t>(p, q) != 150 || SC::MedianAbsDiff<uint8_t, uint8_t, float>(p, q) != 150.0f) { // {197, 150, 2, 0}: rank 2
        fprintf(stderr, "integer inputs\n");
        return 3;
    }
    return 0;
}
