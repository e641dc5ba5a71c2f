"""float64 restatement of the per-class pose regressors (network.REGRESSOR_NUM = K > 1: dim_pose_head_fwd_cls, dim_pose_head_bwd_cls,
dim_se3_dist_loss_grad_cls, dim_fc_wgrad_cls), built on tests/train_head_reference.py (R), the seeded inputs the CPU and GPU tests share
and named mutants.

Layout: rot_w (4K,256), rot_b (4K), trans_w (3K,256), trans_b (3K); class c owns rows 4c..4c+3 of rot and 3c..3c+2 of trans; sample b
reads the rows of class_index[b].  The backward and the distance loss call R's reference once per sample with that sample's class
slice, the weight gradient calls R.fc_wgrad once per class on the class's sub-batch: every bar is R's, worked out by R from the
actual inputs.  Only the forward has no counterpart in R; its bars follow R's stated rules (sums: 2 (n + p) U sum|term|; a first
stage's bar carried through the second stage's sum|w|):
  fc7 = LeakyReLU(fc6 W7^T + b7)       257-term sum, p = 2 (the slope product and the rounded 0.1)
  rot / trans = fc7 W_c^T + b_c        257-term sum, p = 1 (the zoom product of the two in-plane translations), fc7's bar carried
A class index outside [0, K) (K > 1): identity delta, zero gradients, no loss contribution, skipped by the weight gradient -- exact
values, bar 0.

`mutant=NAME` evaluates a plausible wrong kernel; tests/test_regressor_host.py shows that the shared inputs separate each one from the
reference by more than 10 bars on the outputs MUTANT_OUTPUTS names.
"""
import numpy as np

import train_head_reference as R

U = R.U
MUTANTS = ("class_of_sample_0_for_all", "rot_block_stride_3", "absent_class_rows_left_unwritten")
# where each mutant must show: (op, output)
MUTANT_OUTPUTS = {
    "class_of_sample_0_for_all": (("fwd", "se3"), ("bwd", "dz7"), ("dist", "d_zoom_trans"), ("wgrad", "dW")),
    "rot_block_stride_3": (("fwd", "se3"), ("bwd", "dz7")),
    "absent_class_rows_left_unwritten": (("wgrad", "dW"), ("wgrad", "db")),
}
# (B, K, classes): one sample; one class absent (1) and one non-contiguous (2, 0); 13 classes with 1, 4, 6, 8, 10 empty
CASES = (
    (1, 3, (1,)),
    (5, 3, (2, 0, 2, 2, 0)),
    (16, 13, (3, 7, 0, 12, 7, 5, 3, 9, 0, 11, 5, 7, 2, 12, 9, 3)),
)
BAD_CASE = (4, 3, (-1, 1, 3, 0))      # -1 and K: outside [0, K)
DIST_ARGS = dict(lw_rot=0.8, lw_trans=1.3, s=2.0)
PREFILL = 7.0                         # what the weight-gradient outputs hold before the call (the GPU test uses NaN)


def _check_mutant(mutant):
    assert mutant is None or mutant in MUTANTS, mutant


def _classes(class_index, B, K, mutant):
    cls = np.zeros(B, np.int64) if class_index is None else np.asarray(class_index, np.int64).reshape(B)
    assert class_index is not None or K == 1
    if mutant == "class_of_sample_0_for_all":
        cls = np.full(B, cls[0])
    return cls


def _ok(c, K):
    return K == 1 or 0 <= c < K


def _rot_rows(c, mutant):
    r0 = (3 if mutant == "rot_block_stride_3" else 4) * c
    return slice(r0, r0 + 4)


def _trans_rows(c):
    return slice(3 * c, 3 * c + 3)


# ------------------------------------------------------------------------------------------------ forward
def pose_head_fwd(fc6, fc7_w, fc7_b, rot_w, rot_b, trans_w, trans_b, class_index, K, zoom_factor, mutant=None):
    """-> se3 (B,7) = [rot (raw, 4), trans (3) with the two in-plane entries times zoom_factor[b, 0]], fc7 (B,256)"""
    _check_mutant(mutant)
    x, w7, b7, wr, br, wt, bt, zf = (R.f64(a) for a in (fc6, fc7_w, fc7_b, rot_w, rot_b, trans_w, trans_b, zoom_factor))
    B = x.shape[0]
    cls = _classes(class_index, B, K, mutant)
    z7 = x @ w7.T + b7[None]
    fc7 = np.where(z7 > 0.0, z7, R.SLOPE * z7)
    fc7_bar = 2.0 * (257 + 2) * U * (np.abs(x) @ np.abs(w7).T + np.abs(b7)[None])
    se3, bar = np.zeros((B, 7)), np.zeros((B, 7))
    for b in range(B):
        c = int(cls[b])
        if not _ok(c, K):
            se3[b, 0] = 1.0
            continue
        w = np.concatenate([wr[_rot_rows(c, mutant)], wt[_trans_rows(c)]])
        bias = np.concatenate([br[_rot_rows(c, mutant)], bt[_trans_rows(c)]])
        v = w @ fc7[b] + bias
        vb = np.abs(w) @ fc7_bar[b] + 2.0 * (257 + 1) * U * (np.abs(w) @ np.abs(fc7[b]) + np.abs(bias))
        scale = np.array([1.0, 1.0, 1.0, 1.0, zf[b, 0], zf[b, 0], 1.0])
        se3[b], bar[b] = v * scale, vb * np.abs(scale)
    return {"se3": (se3, bar), "fc7": (fc7, fc7_bar)}


# ------------------------------------------------------------------------------------------------ backward
def pose_head_bwd(fc6a, fc7, rot_raw, d_rot_norm, d_trans, fc7_w, rot_w, trans_w, class_index, K, mutant=None):
    """per sample R.pose_head_bwd with the rot / trans rows of the sample's class"""
    _check_mutant(mutant)
    B = np.shape(fc6a)[0]
    cls = _classes(class_index, B, K, mutant)
    out = {"d_rot": (np.zeros((B, 4)), np.zeros((B, 4))), "dz7": (np.zeros((B, 256)), np.zeros((B, 256))),
           "dz6": (np.zeros((B, 256)), np.zeros((B, 256)))}
    for b in range(B):
        c = int(cls[b])
        if not _ok(c, K):
            continue
        one = slice(b, b + 1)
        r = R.pose_head_bwd(fc6a[one], fc7[one], rot_raw[one], d_rot_norm[one], d_trans[one], fc7_w, rot_w[_rot_rows(c, mutant)],
                            trans_w[_trans_rows(c)])
        for k, (v, bar) in r.items():
            out[k][0][b], out[k][1][b] = v[0], bar[0]
    return out


# ------------------------------------------------------------------------------------------------ SE3_DIST_LOSS
def se3_dist_loss_grad(rot_norm, rot_gt, fc7, trans_w, trans_b, class_index, K, zt_gt, d_rot_prior, d_zt_prior, lw_rot, lw_trans,
                       trans_type="L2", s=3.0, sums_prior=(0.0, 0.0), mutant=None):
    """per sample R.se3_dist_loss_grad with the trans rows of the sample's class.  The two loss sums: every sample's own contribution
    and bar from its call (prior 0), then R's rule for a sum of n = B + 1 terms added in any order (the prior is one of them):
    2 n U sum|term| on top of the samples' bars"""
    _check_mutant(mutant)
    B = np.shape(rot_norm)[0]
    cls = _classes(class_index, B, K, mutant)
    d_rot, d_zt = R.f64(d_rot_prior).copy(), R.f64(d_zt_prior).copy()
    d_rot_bar, d_zt_bar = np.zeros((B, 4)), np.zeros((B, 3))
    prior = [R.sc(sums_prior[0]), R.sc(sums_prior[1])]
    sums, sums_bar, mags = list(prior), [0.0, 0.0], [abs(prior[0]), abs(prior[1])]
    for b in range(B):
        c = int(cls[b])
        if not _ok(c, K):
            continue
        one = slice(b, b + 1)
        r = R.se3_dist_loss_grad(rot_norm[one], rot_gt[one], fc7[one], trans_w[_trans_rows(c)], trans_b[_trans_rows(c)], zt_gt[one],
                                 d_rot_prior[one], d_zt_prior[one], lw_rot, lw_trans, trans_type=trans_type, s=s,
                                 sums_prior=(0.0, 0.0))
        d_rot[b], d_rot_bar[b] = r["d_rot_norm"][0][0], r["d_rot_norm"][1][0]
        d_zt[b], d_zt_bar[b] = r["d_zoom_trans"][0][0], r["d_zoom_trans"][1][0]
        for i, k in enumerate(("rot_loss_sum", "trans_loss_sum")):
            sums[i] += r[k][0]
            sums_bar[i] += r[k][1]
            mags[i] += abs(r[k][0])
    sums_bar = [sb + 2.0 * (B + 1) * U * m for sb, m in zip(sums_bar, mags)]
    return {"d_rot_norm": (d_rot, d_rot_bar), "d_zoom_trans": (d_zt, d_zt_bar), "rot_loss_sum": (sums[0], sums_bar[0]),
            "trans_loss_sum": (sums[1], sums_bar[1])}


# ------------------------------------------------------------------------------------------------ weight gradient
def fc_wgrad(dz, x, class_index, K, prefill=PREFILL, mutant=None):
    """dW (K Out, In), db (K Out): class c's rows = R.fc_wgrad over the samples of class c in their order; exact zeros for a class
    without samples"""
    _check_mutant(mutant)
    B, Out = np.shape(dz)
    In = np.shape(x)[1]
    cls = _classes(class_index, B, K, mutant)
    fill = prefill if mutant == "absent_class_rows_left_unwritten" else 0.0
    dW, dW_bar = np.full((K * Out, In), fill, np.float64), np.zeros((K * Out, In))
    db, db_bar = np.full((K * Out,), fill, np.float64), np.zeros((K * Out,))
    for c in range(K):
        idx = np.nonzero(cls == c)[0] if K > 1 else np.arange(B)
        if idx.size == 0:
            continue
        r = R.fc_wgrad(np.asarray(dz)[idx], np.asarray(x)[idx])
        rows = slice(c * Out, (c + 1) * Out)
        dW[rows], dW_bar[rows] = r["dW"]
        db[rows], db_bar[rows] = r["db"]
    return {"dW": (dW, dW_bar), "db": (db, db_bar)}


# ------------------------------------------------------------------------------------------------ shared seeded inputs
def inputs(B, K, classes):
    """every array the four ops read, float32.  The backward / distance-loss states are R's (pose_inputs, se3_inputs: exact zeros among
    the activations, a tiny quaternion, an antipodal rot_gt, non-zero priors) with K-fold heads whose classes differ as much as two
    trained heads do; the translation labels keep every residual R.GAP away from 0 and the smooth-L1 thresholds FOR THE SAMPLE'S CLASS
    (a class outside [0, K) takes class 0's rows for this)."""
    rng = np.random.default_rng(11000 + 131 * B + K)
    f = R._f32
    cls = np.asarray(classes, np.int32)
    assert cls.shape == (B,)
    pose, se3 = R.pose_inputs(B), R.se3_inputs(B)
    rot_w, rot_b = f(rng.normal(0, 0.05, (4 * K, 256))), f(rng.normal(0, 0.05, 4 * K))
    trans_w, trans_b = f(rng.normal(0, 0.02, (3 * K, 256))), f(rng.normal(0, 0.05, 3 * K))
    fc7_d = se3["fc7"]
    zt = np.zeros((B, 3))
    for b in range(B):
        c = int(cls[b]) if 0 <= int(cls[b]) < K else 0
        zt[b] = R.f64(trans_w[3 * c:3 * c + 3]) @ R.f64(fc7_d[b]) + R.f64(trans_b[3 * c:3 * c + 3])
    zt_gt = f(zt - R._residuals(rng, 3 * B).reshape(B, 3))
    return dict(
        class_index=cls, rot_w=rot_w, rot_b=rot_b, trans_w=trans_w, trans_b=trans_b, fc7_w=pose["fc7_w"], fc7_b=f(rng.normal(0, 0.05, 256)),
        # forward
        fc6=f(rng.normal(0, 0.5, (B, 256))), zoom_factor=f(np.stack([rng.uniform(1.5, 4.0, B), rng.uniform(1.5, 4.0, B),
                                                                     rng.normal(0, 0.1, B), rng.normal(0, 0.1, B)], axis=1)),
        # backward
        fc6a=pose["fc6a"], fc7=pose["fc7"], rot_raw=pose["rot_raw"], d_rot_norm=pose["d_rot_norm"], d_trans=pose["d_trans"],
        # distance loss
        rot_norm=se3["rot_norm"], rot_gt=se3["rot_gt"], fc7_dist=fc7_d, zt_gt=zt_gt, d_rot_prior=se3["d_rot_prior"],
        d_zt_prior=se3["d_zt_prior"], sums_prior=se3["sums_prior"])


def run_all(inp, K, class_index="own", trans_type="L2", mutant=None, prefill=PREFILL):
    """the four references on one input set -> {op: {output: (value, bar)}}; class_index "own" = the input set's"""
    cls = inp["class_index"] if isinstance(class_index, str) else class_index
    fwd = pose_head_fwd(inp["fc6"], inp["fc7_w"], inp["fc7_b"], inp["rot_w"], inp["rot_b"], inp["trans_w"], inp["trans_b"], cls, K,
                        inp["zoom_factor"], mutant=mutant)
    bwd = pose_head_bwd(inp["fc6a"], inp["fc7"], inp["rot_raw"], inp["d_rot_norm"], inp["d_trans"], inp["fc7_w"], inp["rot_w"], inp["trans_w"],
                        cls, K, mutant=mutant)
    dist = se3_dist_loss_grad(inp["rot_norm"], inp["rot_gt"], inp["fc7_dist"], inp["trans_w"], inp["trans_b"], cls, K, inp["zt_gt"],
                              inp["d_rot_prior"], inp["d_zt_prior"], DIST_ARGS["lw_rot"], DIST_ARGS["lw_trans"], trans_type=trans_type,
                              s=DIST_ARGS["s"], sums_prior=inp["sums_prior"], mutant=mutant)
    # the two weight gradients of the executor: rot from a (B,4) gradient, trans from a (B,3) one, both against fc7
    wgrad = fc_wgrad(inp["d_rot_norm"], inp["fc7"], cls, K, prefill=prefill, mutant=mutant)
    wgrad_t = fc_wgrad(inp["d_trans"], inp["fc7"], cls, K, prefill=prefill, mutant=mutant)
    return {"fwd": fwd, "bwd": bwd, "dist": dist, "wgrad": wgrad, "wgrad_trans": wgrad_t}
