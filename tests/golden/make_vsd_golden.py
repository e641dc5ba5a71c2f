"""Generate vsd_golden.npz by IMPORTING the reference's own numpy modules (build container only, like make_golden.py).

Run:  python tests/golden/make_vsd_golden.py        (needs /root/reference; never runs on the GPU box)

Modules imported from /root/reference by file path: lib/utils/visibility.py (estimate_visib_mask_gt / _est) and lib/utils/misc.py
(depth_im_to_dist_im).  The file holds arrays only: per case ("a": 48 x 64, "b": 50 x 63, two cameras) the three depth planes, K,
delta, the reference's three distance images and its two visibility masks; plus the list of taus the tests score.

The planes are smooth surfaces: the model at the ground truth and, shifted and pushed back by a ramp, at the estimate; the scene
shows the ground-truth surface in front of a far wall, an occluder in front of part of the object and a strip without depth.  The
generator asserts that every branch of the definition carries at least 50 pixels, and that no pixel sits near a threshold: no float32
difference within 4 float32 ulps of delta and no cost within 1e-9 of a tau, so the last bit of a square root cannot move a pixel
across one and exact counts are a fair thing to ask of another implementation."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/lib/utils"
TAUS = np.array([0.005, 0.01, 0.015, 0.02, 0.025, 0.03, 0.04, 0.05])
DELTA = 0.015


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def planes(H, W, K, phase):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    surf = 0.8 + 0.05 * np.sin(x / 9.0 + phase) * np.cos(y / 7.0) + 0.002 * x
    gt = np.where((y >= 8) & (y < 40) & (x >= 10) & (x < 50), surf, 0.0)
    # the estimate: the same surface four columns and two rows on, pushed back by a ramp from -1 cm to 7 cm
    ramp = -0.01 + 0.08 * (x - 14.0) / 40.0 + 0.003 * np.sin(y / 3.0 + phase)
    est = np.where((y >= 10) & (y < 42) & (x >= 14) & (x < 54), surf + ramp, 0.0)
    test = np.full((H, W), 1.5) + 0.01 * np.cos(x / 11.0)          # a far wall
    test = np.where(gt > 0, gt + 0.001 * np.sin(x * y / 50.0 + phase), test)   # the object where it is, with sensor noise
    test = np.where((x >= 10) & (x < 22), 0.5 + 0.001 * y, test)    # an occluder in front of the object's left part
    test = np.where((y >= 30) & (y < 34), 0.0, test)                # a strip without depth
    return test.astype(np.float32), gt.astype(np.float32), est.astype(np.float32)


def main():
    vis, misc = _load("visibility"), _load("misc")
    out = {"taus": TAUS}
    cams = {"a": np.array([[60.0, 0.0, 31.5], [0.0, 61.0, 23.5], [0.0, 0.0, 1.0]]),
            "b": np.array([[72.25, 0.0, 29.125], [0.0, 70.5, 26.75], [0.0, 0.0, 1.0]])}
    for name, (H, W), phase in (("a", (48, 64), 0.3), ("b", (50, 63), 1.1)):
        K = cams[name]
        d_test, d_gt, d_est = planes(H, W, K, phase)
        s_test, s_gt, s_est = (misc.depth_im_to_dist_im(d, K) for d in (d_test, d_gt, d_est))
        visib_gt = vis.estimate_visib_mask_gt(s_test, s_gt, DELTA)
        visib_est = vis.estimate_visib_mask_est(s_test, s_est, visib_gt, DELTA)
        assert s_test.dtype == np.float64 and visib_gt.dtype == bool
        # every branch carries weight
        diff_gt = s_gt.astype(np.float32) - s_test.astype(np.float32)
        diff_est = s_est.astype(np.float32) - s_test.astype(np.float32)
        own_est = (s_test > 0) & (s_est > 0) & (diff_est <= np.float32(DELTA))
        branches = {"gt hidden behind the scene": (s_test > 0) & (s_gt > 0) & (diff_gt > np.float32(DELTA)),
                    "est admitted through visib_gt": visib_gt & (s_est > 0) & ~own_est,
                    "est visible where gt is not": visib_est & ~visib_gt,
                    "no observed depth under a render": (s_test == 0) & ((s_gt > 0) | (s_est > 0)),
                    "both renders empty": (d_gt == 0) & (d_est == 0),
                    "intersection": visib_gt & visib_est}
        for what, m in branches.items():
            assert m.sum() >= 50, (name, what, int(m.sum()))
        # no pixel near a threshold
        d32 = np.float32(DELTA)
        lo, hi = d32, d32
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        for diff, s_m in ((diff_gt, s_gt), (diff_est, s_est)):
            both = (s_test > 0) & (s_m > 0)
            assert not np.any(both & (diff >= lo) & (diff <= hi)), name
        cost = np.abs(s_gt - s_est)[visib_gt & visib_est]
        assert np.abs(cost[:, None] - TAUS[None, :]).min() > 1e-9, name
        for tau in TAUS:   # every tau splits the intersection
            assert 0 < (cost >= tau).sum() < cost.size, (name, tau)
        for key, v in (("depth_test", d_test), ("depth_gt", d_gt), ("depth_est", d_est), ("K", K), ("delta", np.float64(DELTA)),
                       ("dist_test", s_test), ("dist_gt", s_gt), ("dist_est", s_est), ("visib_gt", visib_gt), ("visib_est", visib_est)):
            out["{}_{}".format(name, key)] = v
        print(name, {k: int(m.sum()) for k, m in branches.items()})
    path = os.path.join(HERE, "vsd_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
