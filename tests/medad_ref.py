"""CPU restatement of MEDAD / ZMEDAD cost volumes (MedianAbsDiff over aggregateCost's feature vectors), written from the semantics:
the element of rank F // 2 of |s - t| in float32, the zero target vector outside the image, ZMEDAD on vectors that had their mean (a
sequential float32 sum times float32(1 / F)) subtracted first -- the zero target vector comes AFTER zero-meaning.  NaN ranks above +inf
(NumPy's partition order), so tests compare NaN masks and the bits of everything else."""
import numpy as np

MEDAD, ZMEDAD = 8, 9
RIGHT_TO_LEFT, LEFT_TO_RIGHT = 1, 0


def zero_mean(feat):
    feat = np.ascontiguousarray(feat, np.float32)
    F = feat.shape[-1]
    acc = np.zeros(feat.shape[:-1], np.float32)
    for c in range(F):  # sequential, never pairwise
        acc = (acc + feat[..., c]).astype(np.float32)
    mean = (acc * np.float32(1.0 / F)).astype(np.float32)
    return (feat - mean[..., None]).astype(np.float32)


def _features(func, feat):
    return zero_mean(feat) if func == ZMEDAD else np.ascontiguousarray(feat, np.float32)


def _slice_volume(fs, ft, dh, lower, D, sign):
    """(H, Ws, D) costs of source fs against target row i + dh, column j + sign * (lower + d)."""
    H, Ws, F = fs.shape
    Wt = ft.shape[1]
    out = np.empty((H, Ws, D), np.float32)
    j = np.arange(Ws)
    i = np.arange(H)
    it = i + dh
    row_ok = (it >= 0) & (it < H)
    for d in range(D):
        jt = j + sign * (lower + d)
        col_ok = (jt >= 0) & (jt < Wt)
        t = np.zeros((H, Ws, F), np.float32)
        t[np.ix_(row_ok, col_ok)] = ft[np.ix_(it[row_ok], jt[col_ok])]
        diff = np.abs(fs - t).astype(np.float32)
        out[..., d] = np.partition(diff, F // 2, axis=-1)[..., F // 2]
    return out


def feature_volume(func, feat_l, feat_r, D, ddir=RIGHT_TO_LEFT, disp_lower=0):
    """featureVolume2CostVolume<func>(feat_l, feat_r, D) restated."""
    src, tgt = (feat_r, feat_l) if ddir == RIGHT_TO_LEFT else (feat_l, feat_r)
    return _slice_volume(_features(func, src), _features(func, tgt), 0, disp_lower, D, 1 if ddir == RIGHT_TO_LEFT else -1)


def feature_volume_2d(func, feat_l, feat_r, range0, range1, ddir=RIGHT_TO_LEFT):
    """featureVolume2CostVolume<func>(..., searchOffset<2>): CV(i, j, dh, dw) against target (i + dh + lower0, j + dw + lower1)."""
    src, tgt = (feat_r, feat_l) if ddir == RIGHT_TO_LEFT else (feat_l, feat_r)
    fs, ft = _features(func, src), _features(func, tgt)
    (l0, u0), (l1, u1) = range0, range1
    return np.stack([_slice_volume(fs, ft, l0 + k, l1, u1 - l1 + 1, 1) for k in range(u0 - l0 + 1)], axis=2)


def unfold(img, h_r, v_r):
    """unfold with automatic zero padding: (H, W, (2v_r+1)(2h_r+1)C), window row, then column, then channel."""
    img = np.asarray(img, np.float32)
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    pad = np.zeros((H + 2 * v_r, W + 2 * h_r, C), np.float32)
    pad[v_r:v_r + H, h_r:h_r + W] = img
    parts = [pad[k:k + H, l:l + W, :] for k in range(2 * v_r + 1) for l in range(2 * h_r + 1)]
    return np.concatenate(parts, axis=2)


def image_volume(func, img_l, img_r, h_r, v_r, D, ddir=RIGHT_TO_LEFT, disp_lower=0):
    """unfoldBasedCostVolume<func> restated."""
    return feature_volume(func, unfold(img_l, h_r, v_r), unfold(img_r, h_r, v_r), D, ddir, disp_lower)


def image_volume_2d(func, img_l, img_r, h_r, v_r, range0, range1, ddir=RIGHT_TO_LEFT):
    return feature_volume_2d(func, unfold(img_l, h_r, v_r), unfold(img_r, h_r, v_r), range0, range1, ddir)


def same_bits(got, exp):
    """Equal NaN masks, equal bits elsewhere."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    if got.shape != exp.shape or not np.array_equal(np.isnan(got), np.isnan(exp)):
        return False
    ok = ~np.isnan(exp)
    return np.array_equal(got[ok].view(np.uint32), exp[ok].view(np.uint32))
