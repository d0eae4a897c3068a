#!/usr/bin/env python3
"""MEDAD / ZMEDAD cost volumes: time per call (device tensors in, device volume out) next to SAD / ZSAD on the same shape, the selection
network against the bitwise selection on the same F, and a check of a few rows of every volume against the CPU restatement
(tests/medad_ref.py).  One JSON line per row.

    python tools/bench_medad.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import libstevi_amd as sv  # noqa: E402
import medad_ref as mr  # noqa: E402

MF = sv.matchingFunctions
DEV = torch.device("cuda:0")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def set_form(x, form):
    sv.set_test_option(x, "median_form", form)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []

    def image(H, W, C=None):
        shp = (H, W) if C is None else (H, W, C)
        return rng.normal(0, 20, shp).astype(np.float32)

    def check(vol, func, l, r, h_r, v_r, D, feature=False):
        pick = [0, vol.shape[0] // 2, vol.shape[0] - 1]
        got = vol[pick].cpu().numpy()
        if feature:
            exp = mr.feature_volume(int(func), l[pick], r[pick], D)
        else:
            exp = mr.feature_volume(int(func), mr.unfold(l, h_r, v_r)[pick], mr.unfold(r, h_r, v_r)[pick], D)
        return bool(mr.same_bits(got, exp))

    shapes = [("grey 5x5", 1080, 1920, None, 2, 128), ("grey 7x7", 1080, 1920, None, 3, 128), ("RGB 5x5", 1080, 1920, 3, 2, 128),
              ("grey 7x7", 480, 640, None, 3, 160)]
    for name, H, W, C, rad, D in shapes:
        l, r = image(H, W, C), image(H, W, C)
        dl, dr = torch.from_numpy(l).to(DEV), torch.from_numpy(r).to(DEV)
        F = (2 * rad + 1) ** 2 * (C or 1)
        for func, base in ((MF.MEDAD, MF.SAD), (MF.ZMEDAD, MF.ZSAD)):
            res = {"shape": f"{H}x{W}x{D}", "window": name, "F": F, "func": func.name}
            for form, key in ((0, "network_ms"), (1, "bitwise_ms")):
                set_form(dl, form)
                vol = sv.unfoldBasedCostVolume(func, dl, dr, rad, rad, D)
                res[key] = round(timed(lambda: sv.unfoldBasedCostVolume(func, dl, dr, rad, rad, D), args.reps), 3)
                res["exact" if form == 0 else "exact_bitwise"] = check(vol, func, l, r, rad, rad, D)
                del vol
            set_form(dl, 0)
            res["gvox_s"] = round(H * W * D / res["network_ms"] / 1e6, 2)
            res[base.name + "_ms"] = round(timed(lambda: sv.unfoldBasedCostVolume(base, dl, dr, rad, rad, D), args.reps), 3)
            rows.append(res)
            print(json.dumps(res), flush=True)
        del dl, dr
        torch.cuda.empty_cache()
    # the generic path: F = 17 feature volumes (the compressors' length), 1080p x 128
    H, W, F, D = 1080, 1920, 17, 128
    fl, fr = image(H, W, F), image(H, W, F)
    dl, dr = torch.from_numpy(fl).to(DEV), torch.from_numpy(fr).to(DEV)
    for func, base in ((MF.MEDAD, MF.SAD), (MF.ZMEDAD, MF.ZSAD)):
        res = {"shape": f"{H}x{W}x{D}", "window": "feature volume", "F": F, "func": func.name}
        for form, key in ((1, "bitwise_ms"), (2, "per_voxel_ms")):
            set_form(dl, form)
            vol = sv.featureVolume2CostVolume(func, dl, dr, D)
            res[key] = round(timed(lambda: sv.featureVolume2CostVolume(func, dl, dr, D), args.reps), 3)
            res["exact" if form == 1 else "exact_per_voxel"] = check(vol, func, fl, fr, 0, 0, D, feature=True)
            del vol
        set_form(dl, 0)
        res["gvox_s"] = round(H * W * D / res["bitwise_ms"] / 1e6, 2)
        res[base.name + "_ms"] = round(timed(lambda: sv.featureVolume2CostVolume(base, dl, dr, D), args.reps), 3)
        rows.append(res)
        print(json.dumps(res), flush=True)
    ok = all(v for r in rows for k, v in r.items() if k.startswith("exact"))
    print(json.dumps({"all_exact": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
