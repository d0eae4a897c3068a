// MEDAD / ZMEDAD cost volumes: the median absolute difference of two feature vectors (MedianAbsDiff, matching_costs.h:180-230).
//
// CV(i,j,d) = the element of rank F/2 (ascending; the upper median for even F) of |s_c - t_c|, c in [0, F), with s the source vector of
// pixel (i, j) and t the target vector of pixel (i + row_off, j + sign*(disp_lower+d)) -- the zero vector outside the image
// (cross_correlations.h:235).  ZMEDAD compares the zero-mean feature volumes (getFeatureVolumeForMatchFunc): (s - ms) - (t - mt), two
// rounded subtractions, and the target outside the image is zero AFTER zero-meaning.  Both sides are therefore processed once into
// scratch (dev_feature_volume_for_match_func: the same mean as ZSAD's) and the kernels below only ever see plain feature volumes.
//
// Order.  Each difference becomes the 31-bit key bits(s - t) & 0x7fffffff, which is bits(fabsf(s - t)).  Unsigned order on those keys is
// float order for every non-NaN value (-0 and +0 collapse, as fabs makes them), and every NaN key ranks above +inf -- NumPy's order for
// partition / sort.  The selection runs on the keys alone and returns one of them, so the result is exact: the bit pattern of one input's
// fabs, no rounding, no accumulation order.
//
// Work split: a block owns MD_TP consecutive source pixels of a row and stages their target records (MD_TP + D - 1 of them, mirrored for
// LeftToRight so that the record index grows with d) and source vectors in LDS; a wave takes one source pixel at a time with lane l on
// disparities l, l + 64, ...: the source feature is one broadcast LDS read, the stores are coalesced.  Then per lane:
//   - F in {9, 25, 27, 49, 75, 81} (3x3 / 5x5 / 7x7 / 9x9 grey windows, 3x3 / 5x5 RGB windows): the F keys in VGPRs through a selection
//     network -- Batcher's odd-even merge sort pruned to output F/2 (svh_median_networks.h, tools/gen_median_networks.py), every
//     comparator one v_min_u32 and / or one v_max_u32;
//   - any other F: an exact bitwise selection over the 31 key bits, most significant first, recomputing the keys from LDS on every pass
//     (31 passes over the vector; no per-lane array, so no scratch).
// Vectors whose records do not fit the LDS budget next to a chunk of at least 16 disparities, and grids of more than 65 535 rows, take a
// thread per voxel that reads both vectors from global memory with the same bitwise selection.
#include "svh_internal.h"

#include <algorithm>

#include "svh_median_networks.h"

namespace svh {

namespace {

constexpr int MD_TP = 64; // source pixels per block

__device__ __forceinline__ uint32_t abs_key(float s, float t) { return __float_as_uint(s - t) & 0x7fffffffu; }

#define SVH_CE(a, b)                   \
    do {                               \
        const uint32_t lo_ = min(a, b); \
        b = max(a, b);                 \
        a = lo_;                       \
    } while (0)
#define SVH_MIN(a, b) (a = min(a, b))
#define SVH_MAX(a, b) (b = max(a, b))

template <int F> __device__ __forceinline__ uint32_t network_select(uint32_t *k);
template <> __device__ __forceinline__ uint32_t network_select<9>(uint32_t *k) { SVH_MEDIAN_NETWORK_9(k); return k[4]; }
template <> __device__ __forceinline__ uint32_t network_select<25>(uint32_t *k) { SVH_MEDIAN_NETWORK_25(k); return k[12]; }
template <> __device__ __forceinline__ uint32_t network_select<27>(uint32_t *k) { SVH_MEDIAN_NETWORK_27(k); return k[13]; }
template <> __device__ __forceinline__ uint32_t network_select<49>(uint32_t *k) { SVH_MEDIAN_NETWORK_49(k); return k[24]; }
template <> __device__ __forceinline__ uint32_t network_select<75>(uint32_t *k) { SVH_MEDIAN_NETWORK_75(k); return k[37]; }
template <> __device__ __forceinline__ uint32_t network_select<81>(uint32_t *k) { SVH_MEDIAN_NETWORK_81(k); return k[40]; }

#undef SVH_CE
#undef SVH_MIN
#undef SVH_MAX

// rank F/2 of the keys abs_key(s[c], t[c]) (t_in false: the zero target vector), c < F: the answer's bits from the most significant down --
// at bit b, the keys that agree with the answer above b and have a 0 at b are counted; if the rank lies among them bit b is 0, otherwise it
// is 1 and they are skipped.  Exact for every F >= 1 (a key is 31 bits wide: bit 31 is always 0).
__device__ __forceinline__ uint32_t bitwise_select(const float *s, const float *t, bool t_in, int F) {
    uint32_t r = 0;
    int k = F / 2;
    for (int b = 30; b >= 0; b--) {
        const uint32_t hi = ~((2u << b) - 1u);
        int cnt = 0;
        for (int c = 0; c < F; c++) {
            const uint32_t key = abs_key(s[c], t_in ? t[c] : 0.0f);
            cnt += ((key & hi) == r) & !((key >> b) & 1u);
        }
        if (k >= cnt) {
            k -= cnt;
            r |= 1u << b;
        }
    }
    return r;
}

// NF > 0: F == NF at compile time, the network; NF == 0: the bitwise selection on the runtime F
template <int NF>
__global__ void __launch_bounds__(256) median_volume_tiled_kernel(const float *__restrict__ ps, const float *__restrict__ pt, int H, int Ws, int Wt,
                                                                  int F_arg, int D, int sign, int disp_lower, int row_off, int64_t px_stride,
                                                                  int64_t out_off, float *__restrict__ cv) {
    extern __shared__ __attribute__((aligned(16))) float mlds[];
    const int F = NF > 0 ? NF : F_arg;
    const int FS = F | 1; // record stride: odd, so that 64 lanes reading feature c of 64 consecutive records hit distinct banks
    const int i = blockIdx.y, j0 = blockIdx.x * MD_TP;
    const int n_rec = MD_TP + D - 1;
    const int it = i + row_off;
    const bool row_in = it >= 0 && it < H; // a target row outside the image is the zero vector
    const float *trow = pt + (int64_t)(row_in ? it : 0) * Wt * F;
    float *lsrc = mlds + (size_t)n_rec * FS;
    const int jt0 = sign > 0 ? j0 + disp_lower : j0 + (MD_TP - 1) - disp_lower, step = sign > 0 ? 1 : -1;
    for (int e = threadIdx.x; e < n_rec * F; e += blockDim.x) {
        const int y = e / F, c = e - y * F;
        const int jt = jt0 + step * y;
        mlds[y * FS + c] = (row_in && jt >= 0 && jt < Wt) ? trow[(int64_t)jt * F + c] : 0.0f;
    }
    const int n_px = min(MD_TP, Ws - j0);
    for (int e = threadIdx.x; e < n_px * F; e += blockDim.x) lsrc[e] = ps[((int64_t)i * Ws + j0) * F + e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int u = wave; u < n_px; u += 4) {
        const float *s = lsrc + u * F;
        const float *base = mlds + (sign > 0 ? u : MD_TP - 1 - u) * FS;
        float *out = cv + ((int64_t)i * Ws + j0 + u) * px_stride + out_off;
        for (int d = lane; d < D; d += 64) {
            const float *t = base + d * FS;
            uint32_t r;
            if constexpr (NF > 0) {
                uint32_t k[NF];
#pragma unroll
                for (int c = 0; c < NF; c++) k[c] = abs_key(s[c], t[c]);
                r = network_select<NF>(k);
            } else {
                r = bitwise_select(s, t, true, F);
            }
            out[d] = __uint_as_float(r);
        }
    }
}

// a thread per voxel, both vectors from global memory (long vectors, tall grids)
__global__ void median_volume_kernel(const float *__restrict__ ps, const float *__restrict__ pt, int H, int Ws, int Wt, int F, int D, int sign,
                                     int disp_lower, int row_off, int64_t px_stride, int64_t out_off, float *__restrict__ cv) {
    const int64_t n = (int64_t)H * Ws * D;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(e % D);
        const int64_t p = e / D;
        const int j = (int)(p % Ws), i = (int)(p / Ws);
        const int jt = j + sign * (disp_lower + d), it = i + row_off;
        const bool t_in = it >= 0 && it < H && jt >= 0 && jt < Wt;
        const uint32_t r = bitwise_select(ps + p * F, pt + (t_in ? ((int64_t)it * Wt + jt) * F : 0), t_in, F);
        cv[p * px_stride + out_off + d] = __uint_as_float(r);
    }
}

constexpr size_t MD_LDS_BUDGET = 60 * 1024;

// the volume of two (already processed) feature volumes
int median_volume(svh_context *ctx, const CostVolumeArgs &a, const float *ps, const float *pt, int F, float *cv) {
    if ((int64_t)a.H * a.Ws * a.D == 0) return SVH_OK;
    const int sign = a.sign();
    const size_t rec = (size_t)(F | 1) * sizeof(float), src_bytes = (size_t)MD_TP * F * sizeof(float);
    const int64_t max_rec = src_bytes < MD_LDS_BUDGET ? (int64_t)((MD_LDS_BUDGET - src_bytes) / rec) - (MD_TP - 1) : 0;
    const bool tiled = ctx->median_form != 2 && a.H <= 65535 && max_rec >= 16;
    if (!tiled) {
        const int64_t n = (int64_t)a.H * a.Ws * a.D;
        SVH_LAUNCH(ctx, "median_volume", median_volume_kernel, grid_for(n, 256, 65536), 256, 0, ps, pt, a.H, a.Ws, a.Wt, F, a.D, sign, a.disp_lower,
                   a.tgt_row_off, a.px_stride(), a.out_off, cv);
        SVH_CHECK_LAUNCH(ctx);
        return SVH_OK;
    }
    // the disparity range in chunks when the records of the whole range do not fit
    const int chunk = (int)std::min<int64_t>(a.D, max_rec >= 64 ? max_rec / 64 * 64 : max_rec);
    const bool network = ctx->median_form == 0;
    const dim3 grid(ceil_div(a.Ws, MD_TP), a.H);
    for (int d0 = 0; d0 < a.D; d0 += chunk) {
        const int Dc = std::min(chunk, a.D - d0), lower = a.disp_lower + d0;
        const int64_t off = a.out_off + d0;
        const size_t shmem = (size_t)(MD_TP + Dc - 1) * rec + src_bytes;
#define SVH_MD(NFV)                                                                                                                              \
    SVH_LAUNCH(ctx, NFV ? "median_volume_network" : "median_volume_select", median_volume_tiled_kernel<NFV>, grid, 256, shmem, ps, pt, a.H, a.Ws, \
               a.Wt, F, Dc, sign, lower, a.tgt_row_off, a.px_stride(), off, cv)
        if (network && F == 9) SVH_MD(9);
        else if (network && F == 25) SVH_MD(25);
        else if (network && F == 27) SVH_MD(27);
        else if (network && F == 49) SVH_MD(49);
        else if (network && F == 75) SVH_MD(75);
        else if (network && F == 81) SVH_MD(81);
        else SVH_MD(0);
#undef SVH_MD
    }
    SVH_CHECK_LAUNCH(ctx);
    return SVH_OK;
}

} // namespace

int dev_median_volume_from_features(svh_context *ctx, Scratch &scr, const CostVolumeArgs &a, const float *feat_src, const float *feat_tgt, int F,
                                    float *cv) {
    if (!func_median(a.func)) return fail(ctx, SVH_ERR_HIP, "internal: the median kernel got matching function %d", a.func);
    if (!cv) return fail(ctx, SVH_ERR_HIP, "internal: the median kernel writes the volume");
    if (a.n_dh != 1 || a.row_count != 0) return fail(ctx, SVH_ERR_HIP, "internal: the median kernel takes one vertical offset and the whole image");
    if ((int64_t)a.H * a.Ws * a.D == 0 || F < 1) return SVH_OK;
    if (!func_zero_mean(a.func)) return median_volume(ctx, a, feat_src, feat_tgt, F, cv);
    // ZMEDAD: both sides zero-meaned once (getFeatureVolumeForMatchFunc); the zero target vector is then inserted by the kernel
    float *zs = scr.get_n<float>((size_t)a.H * a.Ws * F), *zt = scr.get_n<float>((size_t)a.H * a.Wt * F);
    if (!zs || !zt) return SVH_ERR_OUT_OF_MEMORY;
    SVH_TRY(dev_feature_volume_for_match_func(ctx, scr, a.func, feat_src, a.H, a.Ws, F, zs));
    SVH_TRY(dev_feature_volume_for_match_func(ctx, scr, a.func, feat_tgt, a.H, a.Wt, F, zt));
    return median_volume(ctx, a, zs, zt, F, cv);
}

int dev_median_volume_from_images(svh_context *ctx, Scratch &scr, const CostVolumeArgs &a, ImageDesc src, ImageDesc tgt, int h_r, int v_r,
                                  float *cv) {
    if ((int64_t)a.H * a.Ws * a.D == 0) return SVH_OK;
    // unfoldBasedCostVolume = unfold (automatic zero padding: the output has the image's size) then featureVolume2CostVolume
    const int F = (2 * h_r + 1) * (2 * v_r + 1) * src.C;
    float *fs = scr.get_n<float>((size_t)src.H * src.W * F), *ft = scr.get_n<float>((size_t)tgt.H * tgt.W * F);
    if (!fs || !ft) return SVH_ERR_OUT_OF_MEMORY;
    SVH_TRY(dev_unfold(ctx, src, h_r, v_r, h_r, v_r, src.H, src.W, fs));
    SVH_TRY(dev_unfold(ctx, tgt, h_r, v_r, h_r, v_r, tgt.H, tgt.W, ft));
    return dev_median_volume_from_features(ctx, scr, a, fs, ft, F, cv);
}

} // namespace svh
