"""Pose evaluation of the refinement results, as lib/dataset/LM6D_REFINE.py:329-830 computes it for the README tables:
rotation / translation / joint accuracies at (k deg, k cm), ADD(-S) at 0.02 / 0.05 / 0.10 of the diameter plus the AUC over
[0, 0.1 d] (Simpson), and the 2-D re-projection accuracy at 2 / 5 / 10 / 20 px plus its AUC over [0, 50 px].

Inputs have the reference's layout: all_poses_est[cls][iter] and all_poses_gt[cls][0] are lists of 3x4 poses.  Every method
returns its numbers as a dict and logs the reference's lines through `logger` / print.  Thresholding is vectorised (the
reference loops over 1000 thresholds per pose); pose errors come from lib/utils/pose_error.py, or -- `errors=` -- from the caller:
{"re", "te", "add", "arp_2d"} -> errors[key][cls][iter] = one number per pose of all_poses_est[cls][iter], as host_pose_errors
computes them (pred_eval with TEST.DEVICE_EVAL passes the device's, lib/hip/ops.py pose_errors)."""
from __future__ import print_function, division

import os
import pickle

import numpy as np

from lib.utils.pose_error import add, adi, arp_2d, calc_rt_dist_m, re

try:
    from scipy.integrate import simpson as _simps
except ImportError:  # older scipy
    from scipy.integrate import simps as _simps

SYM_CLASSES = ("eggbox", "glue", "bowl", "cup")            # ADI instead of ADD (:516)
RT_Z = np.array([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)  # eggbox: 180 deg about z (:357-362)


def se3_mul(RT1, RT2):
    """lib/utils/projection.py: [R1 R2 | R1 t2 + t1]"""
    R = RT1[:, :3].dot(RT2[:, :3])
    t = RT1[:, :3].dot(RT2[:, 3]) + RT1[:, 3]
    return np.concatenate([R, t.reshape(3, 1)], axis=1)


def print_and_log(s, logger=None):
    print(s)
    if logger:
        logger.info(s)


class PoseEvaluator(object):
    def __init__(self, classes, points, diameters, symmetries=None):
        """points: dict class -> (N,3) model points; diameters: dict class -> metres (LM6D_REFINE._points / ._diameters);
        symmetries: dict class -> a BOP model_info ({"symmetries_discrete": ..., "symmetries_continuous": ...}, lib/utils/symmetry.py)
        or a ready (S,3,4) set, read by the symmetry-aware errors (MSSD, MSPD).  A class without an entry has the identity only,
        except eggbox: {I, RT_Z}, the rule stated above."""
        self.classes = list(classes)
        self.num_classes = len(self.classes)
        self._points = points
        self._diameters = diameters
        self._symmetries = dict(symmetries or {})

    def symmetry_sets(self, max_sym_disc_step=0.01):
        """-> one (S,3,4) float64 set per class, in class order, the identity first"""
        from lib.utils.symmetry import as_symmetry_set

        cache = self.__dict__.setdefault("_symmetry_sets", {})
        key = float(max_sym_disc_step)
        if key not in cache:
            sets = []
            for c in self.classes:
                if c in self._symmetries:
                    sets.append(as_symmetry_set(self._symmetries[c], key))
                elif c == "eggbox":
                    sets.append(np.stack([np.eye(4)[:3], RT_Z]))
                else:
                    sets.append(np.eye(4)[None, :3].copy())
            cache[key] = sets
        return cache[key]

    def max_sym(self, max_sym_disc_step=0.01):
        """the size of the largest symmetry set (dim_bop_errors' max_sym)"""
        return max([len(s) for s in self.symmetry_sets(max_sym_disc_step)] or [1])

    def device_sym_tables(self, device, max_sym_disc_step=0.01):
        """-> (sym (Stot,3,4) float64, sym_off (n_classes+1,) int32) resident on `device`: the symmetry sets of all classes
        concatenated, as dim_bop_errors reads them next to device_tables.  Built once per device (and discretisation step)."""
        import torch

        key = (str(torch.device(device)), float(max_sym_disc_step))
        cache = self.__dict__.setdefault("_device_sym_tables", {})
        if key not in cache:
            sets = self.symmetry_sets(max_sym_disc_step)
            off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
            alls = np.ascontiguousarray(np.concatenate(sets, axis=0)) if sets else np.zeros((0, 3, 4))
            cache[key] = (torch.from_numpy(alls).to(device), torch.from_numpy(off).to(device))
        return cache[key]

    def device_tables(self, device):
        """-> (points (Ntot,3) float64, table_off (n_classes+1,) int32, class_flags (n_classes,) int32) resident on `device`, the model
        tables dim_pose_errors reads: ADD-S for SYM_CLASSES, the 180-degree rule for eggbox.  Built once per device."""
        import torch

        from lib.hip import ops

        key = str(torch.device(device))
        cache = self.__dict__.setdefault("_device_tables", {})
        if key not in cache:
            pts = [np.asarray(self._points[c], dtype=np.float64).reshape(-1, 3) for c in self.classes]
            off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
            flags = np.array([(ops.POSE_ERR_ADI if c in SYM_CLASSES else 0) | (ops.POSE_ERR_FLIP_Z180 if c == "eggbox" else 0)
                              for c in self.classes], dtype=np.int32)
            allp = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts else np.zeros((0, 3))
            cache[key] = (torch.from_numpy(allp).to(device), torch.from_numpy(off).to(device), torch.from_numpy(flags).to(device))
        return cache[key]

    def vsd_tau_table(self, fracs):
        """-> (n_classes, n_tau) float64, entry [c][k] = float(fracs[k]) * float(diameter of class c), in class order: the
        misalignment tolerances of BOP's VSD (fractions of the object diameter) in the unit of the depth planes.  The one rounding of
        each product is made here; dim_vsd_grid_errors only compares against the table."""
        fr = [float(f) for f in np.asarray(fracs, dtype=np.float64).reshape(-1)]
        return np.array([[f * float(self._diameters[c]) for f in fr] for c in self.classes], dtype=np.float64).reshape(len(self.classes), len(fr))

    def device_vsd_tau_table(self, device, fracs):
        """vsd_tau_table(fracs) resident on `device` as lib.hip.ops.vsd_grid_errors reads it.  Uploaded once per device (and fractions)."""
        import torch

        from lib.hip import ops

        key = (str(torch.device(device)), tuple(float(f) for f in np.asarray(fracs, dtype=np.float64).reshape(-1)))
        cache = self.__dict__.setdefault("_device_vsd_tau_tables", {})
        if key not in cache:
            cache[key] = ops.vsd_tau_table(self.vsd_tau_table(fracs), device)
        return cache[key]

    def host_pose_errors(self, config, cls_name, RT, pose_gt):
        """the four numbers the three tables below read for one pose: (re, te) of evaluate_pose, ADD or ADD-S, arp_2d"""
        K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float64)
        flipped = se3_mul(RT, RT_Z) if cls_name == "eggbox" and re(RT[:3, :3], pose_gt[:3, :3]) > 90 else RT
        r, t = calc_rt_dist_m(flipped, pose_gt)
        fn = adi if cls_name in SYM_CLASSES else add
        return (r, t, fn(RT[:3, :3], RT[:, 3], pose_gt[:3, :3], pose_gt[:, 3], self._points[cls_name]),
                arp_2d(flipped[:3, :3], flipped[:, 3], pose_gt[:3, :3], pose_gt[:, 3], self._points[cls_name], K))

    @staticmethod
    def _given(errors, key, cls_idx, iter_i, n):
        err = np.asarray(errors[key][cls_idx][iter_i], dtype=np.float64)
        if err.shape != (n,):
            raise ValueError("errors['{}'][{}][{}]: {} values for {} poses".format(key, cls_idx, iter_i, err.shape, n))
        return err

    def _valid(self, all_poses_est, all_poses_gt, cls_idx):
        return bool(len(all_poses_est[cls_idx][0]) and len(all_poses_gt[cls_idx][0]))

    # ------------------------------------------------------------------------------------------------ :329-459
    def evaluate_pose(self, config, all_poses_est, all_poses_gt, logger=None, errors=None):
        print_and_log("evaluating pose", logger)
        rot_thresh_list = np.arange(1, 11, 1)
        trans_thresh_list = np.arange(0.01, 0.11, 0.01)
        num_metric = len(rot_thresh_list)
        num_iter = config.TEST.test_iter
        rot_acc = np.zeros((self.num_classes, num_iter, num_metric))
        trans_acc = np.zeros((self.num_classes, num_iter, num_metric))
        space_acc = np.zeros((self.num_classes, num_iter, num_metric))
        num_valid_class = 0
        show_list = [1, 4, 9]
        for cls_idx, cls_name in enumerate(self.classes):
            if not self._valid(all_poses_est, all_poses_gt, cls_idx):
                continue
            num_valid_class += 1
            gts = all_poses_gt[cls_idx][0]
            for iter_i in range(num_iter):
                ests = all_poses_est[cls_idx][iter_i]
                rd, td = np.zeros(len(gts)), np.zeros(len(gts))
                if errors is not None:
                    rd, td = self._given(errors, "re", cls_idx, iter_i, len(gts)), self._given(errors, "te", cls_idx, iter_i, len(gts))
                else:
                    for j in range(len(gts)):
                        r, t = calc_rt_dist_m(ests[j], gts[j])
                        if cls_name == "eggbox" and r > 90:
                            r, t = calc_rt_dist_m(se3_mul(ests[j], RT_Z), gts[j])
                        rd[j], td[j] = r, t
                r_ok = rd[:, None] < rot_thresh_list[None, :]
                t_ok = td[:, None] < trans_thresh_list[None, :]
                rot_acc[cls_idx, iter_i] = r_ok.mean(0)
                trans_acc[cls_idx, iter_i] = t_ok.mean(0)
                space_acc[cls_idx, iter_i] = np.logical_and(r_ok, t_ok).mean(0)
            print_and_log("------------ {} -----------".format(cls_name), logger)
            print_and_log("{:>24}: {:>7}, {:>7}, {:>7}".format("[rot_thresh, trans_thresh", "RotAcc", "TraAcc", "SpcAcc"), logger)
            for iter_i in range(num_iter):
                print_and_log("** iter {} **".format(iter_i + 1), logger)
                print_and_log("{:<16}{:>8}: {:>7.2f}, {:>7.2f}, {:>7.2f}".format(
                    "average_accuracy", "[{:>2}, {:>5.2f}]".format(-1, -1), np.mean(rot_acc[cls_idx, iter_i, :]) * 100,
                    np.mean(trans_acc[cls_idx, iter_i, :]) * 100, np.mean(space_acc[cls_idx, iter_i, :]) * 100), logger)
                for show_idx in show_list:
                    print_and_log("{:>16}{:>8}: {:>7.2f}, {:>7.2f}, {:>7.2f}".format(
                        "average_accuracy", "[{:>2}, {:>5.2f}]".format(rot_thresh_list[show_idx], trans_thresh_list[show_idx]),
                        rot_acc[cls_idx, iter_i, show_idx] * 100, trans_acc[cls_idx, iter_i, show_idx] * 100,
                        space_acc[cls_idx, iter_i, show_idx] * 100), logger)
        overall = []
        for iter_i in range(num_iter):
            n = max(num_valid_class, 1)
            row = {"RotAcc": np.sum(rot_acc[:, iter_i, :]) / (n * num_metric) * 100,
                   "TraAcc": np.sum(trans_acc[:, iter_i, :]) / (n * num_metric) * 100,
                   "SpcAcc": np.sum(space_acc[:, iter_i, :]) / (n * num_metric) * 100}
            overall.append(row)
            print_and_log("---------- performance over {} classes -----------".format(num_valid_class), logger)
            print_and_log("** iter {} **".format(iter_i + 1), logger)
            print_and_log("{:<16}{:>8}: {:>7.2f}, {:>7.2f}, {:>7.2f}".format(
                "average_accuracy", "[{:>2}, {:>5.2f}]".format(-1, -1), row["RotAcc"], row["TraAcc"], row["SpcAcc"]), logger)
            for show_idx in show_list:
                print_and_log("{:>16}{:>8}: {:>7.2f}, {:>7.2f}, {:>7.2f}".format(
                    "average_accuracy", "[{:>2}, {:>5.2f}]".format(rot_thresh_list[show_idx], trans_thresh_list[show_idx]),
                    np.sum(rot_acc[:, iter_i, show_idx]) / n * 100, np.sum(trans_acc[:, iter_i, show_idx]) / n * 100,
                    np.sum(space_acc[:, iter_i, show_idx]) / n * 100), logger)
        return {"rot_acc": rot_acc, "trans_acc": trans_acc, "space_acc": space_acc, "overall": overall,
                "num_valid_class": num_valid_class}

    # ------------------------------------------------------------------------------------------------ shared by ADD / ARP-2D
    def _threshold_eval(self, config, all_poses_est, all_poses_gt, error_fn, fixed, curve, curve_scale, area_norm, fmt, header,
                        overall_title, output_dir, pkl_name, logger, given=None):
        num_iter = config.TEST.test_iter
        count_all = np.zeros((self.num_classes,), dtype=np.float32)
        count_correct = {k: np.zeros((self.num_classes, num_iter), dtype=np.float32) for k in fixed}
        dx = fmt["dx"]   # the reference passes the python float it built the curve from (:489, :711), not the float32 spacing
        count_correct["mean"] = np.zeros((self.num_classes, num_iter, len(curve)), dtype=np.float32)
        errors = {}
        num_valid_class = 0
        for cls_idx, cls_name in enumerate(self.classes):
            if not self._valid(all_poses_est, all_poses_gt, cls_idx):
                continue
            num_valid_class += 1
            gts = all_poses_gt[cls_idx][0]
            count_all[cls_idx] = len(gts)
            scale = curve_scale(cls_name)
            thr_curve = (curve * np.float32(scale)).astype(np.float32)
            for iter_i in range(num_iter):
                ests = all_poses_est[cls_idx][iter_i]
                if given is not None:
                    err = self._given(given[0], given[1], cls_idx, iter_i, len(gts))
                else:
                    err = np.array([error_fn(cls_name, ests[j], gts[j]) for j in range(len(gts))])
                errors[(cls_name, iter_i)] = err
                for k, frac in fixed.items():
                    count_correct[k][cls_idx, iter_i] = np.sum(err < np.float32(frac * scale))
                count_correct["mean"][cls_idx, iter_i] = (err[:, None] < thr_curve[None, :]).sum(0)
        print_and_log(header, logger)
        plot_data = {}
        sums = {k: np.zeros(num_iter) for k in list(fixed) + ["mean"]}
        per_class = {}
        for cls_idx, cls_name in enumerate(self.classes):
            if count_all[cls_idx] == 0:
                continue
            plot_data[cls_name] = []
            for iter_i in range(num_iter):
                print_and_log("** {}, iter {} **".format(cls_name, iter_i + 1), logger)
                y = count_correct["mean"][cls_idx, iter_i] / float(count_all[cls_idx])
                acc_mean = _simps(y, dx=dx) / area_norm * 100
                sums["mean"][iter_i] += acc_mean
                plot_data[cls_name].append((curve.astype(np.float32), y))
                res = {"auc": acc_mean}
                print_and_log("threshold=[0.0, {}], area: {:.2f}".format(fmt["range"], acc_mean), logger)
                for k in fixed:
                    acc = 100 * float(count_correct[k][cls_idx, iter_i]) / float(count_all[cls_idx])
                    sums[k][iter_i] += acc
                    res[k] = acc
                    print_and_log("threshold={}, correct poses: {}, all poses: {}, accuracy: {:.2f}".format(
                        k, count_correct[k][cls_idx, iter_i], count_all[cls_idx], acc), logger)
                per_class[(cls_name, iter_i)] = res
        if output_dir:
            with open(os.path.join(output_dir, pkl_name), "wb") as f:
                pickle.dump(plot_data, f, protocol=2)
        overall = []
        n = max(num_valid_class, 1)
        for iter_i in range(num_iter):
            print_and_log("---------- {} performance over {} classes -----------".format(overall_title, num_valid_class), logger)
            print_and_log("** iter {} **".format(iter_i + 1), logger)
            row = {"auc": sums["mean"][iter_i] / n}
            print_and_log("threshold=[0.0, {}], area: {:.2f}".format(fmt["range"], row["auc"]), logger)
            for k in fixed:
                row[k] = sums[k][iter_i] / n
                print_and_log("threshold={}, mean accuracy: {:.2f}".format(k, row[k]), logger)
            overall.append(row)
        return {"per_class": per_class, "overall": overall, "count_all": count_all, "count_correct": count_correct, "errors": errors,
                "num_valid_class": num_valid_class}

    # ------------------------------------------------------------------------------------------------ :461-681
    def evaluate_pose_add(self, config, all_poses_est, all_poses_gt, output_dir=None, logger=None, errors=None):
        def err(cls_name, RT, pose_gt):
            fn = adi if cls_name in SYM_CLASSES else add
            return fn(RT[:3, :3], RT[:, 3], pose_gt[:3, :3], pose_gt[:, 3], self._points[cls_name])

        uses_adi = any(c in SYM_CLASSES for c in self.classes)
        return self._threshold_eval(
            config, all_poses_est, all_poses_gt, err, {"0.02": 0.02, "0.05": 0.05, "0.10": 0.10},
            np.arange(0, 0.1, 0.0001).astype(np.float32), lambda c: self._diameters[c], 0.1, {"range": "0.10", "dx": 0.0001},
            "evaluating pose add", "add", output_dir, "{}_xys.pkl".format("adi" if uses_adi else "add"), logger,
            given=None if errors is None else (errors, "add"))

    # ------------------------------------------------------------------------------------------------ :683-
    def evaluate_pose_arp_2d(self, config, all_poses_est, all_poses_gt, output_dir=None, logger=None, errors=None):
        K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float64)

        def err(cls_name, RT, pose_gt):
            if cls_name == "eggbox" and re(RT[:3, :3], pose_gt[:3, :3]) > 90:
                RT = se3_mul(RT, RT_Z)
            return arp_2d(RT[:3, :3], RT[:, 3], pose_gt[:3, :3], pose_gt[:, 3], self._points[cls_name], K)

        return self._threshold_eval(
            config, all_poses_est, all_poses_gt, err, {"2": 2.0, "5": 5.0, "10": 10.0, "20": 20.0},
            np.arange(0, 50, 0.1).astype(np.float32), lambda c: 1.0, 50.0, {"range": "50", "dx": 0.1},
            "evaluating pose average re-projection 2d error", "arp_2d", output_dir, "arp_2d_xys.pkl", logger,
            given=None if errors is None else (errors, "arp_2d"))

    # ------------------------------------------------------------------------------------------------ visible surface discrepancy
    def evaluate_pose_vsd(self, config, errors, logger=None):
        """errors: {"vsd": errors["vsd"][cls][iter] = one list of len(VSD_TAU) errors per pose, "visib_gt" / "drawn_gt":
        [cls][iter] = per pose the visible and the drawn pixels of the ground-truth render} (pred_eval with TEST.VSD fills them from
        dim_vsd_errors).  Per class and iteration: the share of poses with e < VSD_THRESH for every tau, and the mean visible
        fraction |visib_gt| / drawn_gt over the poses whose ground truth draws anything."""
        taus = [float(t) for t in np.asarray(config.TEST.VSD_TAU, dtype=np.float64).reshape(-1)]
        thresh = float(config.TEST.VSD_THRESH)
        num_iter = len(errors["vsd"][0]) if len(errors["vsd"]) else 0
        acc = np.zeros((self.num_classes, num_iter, len(taus)))
        visib = np.full((self.num_classes, num_iter), np.nan)
        count_all = np.zeros((self.num_classes,), dtype=np.float32)
        print_and_log("evaluating pose vsd (delta {}, cost {}, correct below {})".format(
            float(config.TEST.VSD_DELTA), config.TEST.VSD_COST, thresh), logger)
        num_valid_class = 0
        for cls_idx, cls_name in enumerate(self.classes):
            if not len(errors["vsd"][cls_idx][0]):
                continue
            num_valid_class += 1
            count_all[cls_idx] = len(errors["vsd"][cls_idx][0])
            for iter_i in range(num_iter):
                e = np.asarray(errors["vsd"][cls_idx][iter_i], dtype=np.float64).reshape(-1, len(taus))
                acc[cls_idx, iter_i] = (e < thresh).mean(0)
                vis = np.asarray(errors["visib_gt"][cls_idx][iter_i], dtype=np.float64)
                drawn = np.asarray(errors["drawn_gt"][cls_idx][iter_i], dtype=np.float64)
                if np.any(drawn > 0):
                    visib[cls_idx, iter_i] = np.mean(vis[drawn > 0] / drawn[drawn > 0])
                print_and_log("** {}, iter {} **".format(cls_name, iter_i + 1), logger)
                print_and_log("visible fraction of the ground truth: {:.3f}".format(visib[cls_idx, iter_i]), logger)
                for k, tau in enumerate(taus):
                    print_and_log("tau={}, correct poses: {}, all poses: {}, accuracy: {:.2f}".format(
                        tau, int((e[:, k] < thresh).sum()), count_all[cls_idx], acc[cls_idx, iter_i, k] * 100), logger)
        overall = []
        n = max(num_valid_class, 1)
        for iter_i in range(num_iter):
            print_and_log("---------- vsd performance over {} classes -----------".format(num_valid_class), logger)
            print_and_log("** iter {} **".format(iter_i + 1), logger)
            row = {}
            for k, tau in enumerate(taus):
                row[tau] = np.sum(acc[:, iter_i, k]) / n * 100
                print_and_log("tau={}, mean accuracy: {:.2f}".format(tau, row[tau]), logger)
            overall.append(row)
        return {"acc": acc, "visible_fraction": visib, "overall": overall, "count_all": count_all, "taus": taus, "thresh": thresh,
                "num_valid_class": num_valid_class}

    # ------------------------------------------------------------------------------------------------ BOP: MSSD / MSPD
    def evaluate_pose_bop(self, config, errors, logger=None):
        """errors: {"mssd", "mspd"}: errors[key][cls][iter] = one number per pose (pred_eval with TEST.BOP fills them from
        dim_bop_errors; inf = a pair that was not refined).  Per class and iteration: the recall (share of poses with e < threshold)
        at every TEST.BOP_MSSD_THRESH (fractions of the class diameter) and TEST.BOP_MSPD_THRESH (pixels at width 640, scaled by
        W / 640 with W of config.SCALES), their means AR_MSSD and AR_MSPD as the BOP protocol averages them, and the mean over the
        classes per iteration."""
        th_s = np.asarray(config.TEST.BOP_MSSD_THRESH, dtype=np.float64).reshape(-1)
        scales = getattr(config, "SCALES", None)
        width = float(scales[0][1]) if scales else 640.0
        th_p = np.asarray(config.TEST.BOP_MSPD_THRESH, dtype=np.float64).reshape(-1) * (width / 640.0)
        num_iter = len(errors["mssd"][0]) if len(errors["mssd"]) else 0
        rec_s = np.zeros((self.num_classes, num_iter, len(th_s)))
        rec_p = np.zeros((self.num_classes, num_iter, len(th_p)))
        count_all = np.zeros((self.num_classes,), dtype=np.float32)
        print_and_log("evaluating pose bop (mssd below {} of the diameter, mspd below {} px)".format(th_s.tolist(), th_p.tolist()), logger)
        num_valid_class = 0
        for cls_idx, cls_name in enumerate(self.classes):
            if not len(errors["mssd"][cls_idx][0]):
                continue
            num_valid_class += 1
            count_all[cls_idx] = len(errors["mssd"][cls_idx][0])
            for iter_i in range(num_iter):
                e_s = np.asarray(errors["mssd"][cls_idx][iter_i], dtype=np.float64)
                e_p = np.asarray(errors["mspd"][cls_idx][iter_i], dtype=np.float64)
                rec_s[cls_idx, iter_i] = (e_s[:, None] < th_s[None, :] * self._diameters[cls_name]).mean(0)
                rec_p[cls_idx, iter_i] = (e_p[:, None] < th_p[None, :]).mean(0)
                print_and_log("** {}, iter {} **".format(cls_name, iter_i + 1), logger)
                print_and_log("all poses: {}, AR_MSSD: {:.2f}, AR_MSPD: {:.2f}".format(
                    count_all[cls_idx], rec_s[cls_idx, iter_i].mean() * 100, rec_p[cls_idx, iter_i].mean() * 100), logger)
        ar_s = rec_s.mean(2) if len(th_s) else np.zeros((self.num_classes, num_iter))
        ar_p = rec_p.mean(2) if len(th_p) else np.zeros((self.num_classes, num_iter))
        overall = []
        n = max(num_valid_class, 1)
        for iter_i in range(num_iter):
            row = {"AR_MSSD": np.sum(ar_s[:, iter_i]) / n * 100, "AR_MSPD": np.sum(ar_p[:, iter_i]) / n * 100}
            overall.append(row)
            print_and_log("---------- bop performance over {} classes -----------".format(num_valid_class), logger)
            print_and_log("** iter {} **".format(iter_i + 1), logger)
            print_and_log("AR_MSSD: {:.2f}, AR_MSPD: {:.2f}".format(row["AR_MSSD"], row["AR_MSPD"]), logger)
        return {"recall_mssd": rec_s, "recall_mspd": rec_p, "AR_MSSD": ar_s, "AR_MSPD": ar_p, "overall": overall,
                "count_all": count_all, "thresh_mssd": th_s.tolist(), "thresh_mspd": th_p.tolist(),
                "num_valid_class": num_valid_class}

    # ------------------------------------------------------------------------------------------------ BOP: AR_VSD and AR
    def evaluate_pose_bop19(self, config, errors, logger=None):
        """The number BOP ranks by, AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3.  errors: {"mssd", "mspd"} as evaluate_pose_bop takes them,
        "vsd_grid": errors[key][cls][iter] = per pose one list of len(TEST.BOP_VSD_TAU) step-cost VSD errors, at the taus
        vsd_tau_table(TEST.BOP_VSD_TAU) gives the pose's class (pred_eval with TEST.BOP_VSD fills them from dim_vsd_grid_errors), and
        "visib_gt" / "drawn_gt": [cls][iter] = per pose the visible and the drawn pixels of the ground-truth render.
        A pose is a target when drawn_gt > 0 and visib_gt / drawn_gt >= TEST.BOP_MIN_VISIB_FRACT; the others count for none of the
        three recalls.  Recall = the share of targets with e < threshold.  Per class and iteration: recall_vsd over the grid
        BOP_VSD_TAU x BOP_VSD_THRESH and its mean AR_VSD, AR_MSSD and AR_MSPD over the thresholds of evaluate_pose_bop, and AR.
        `overall`: per iteration their means over the classes that have a target, in percent.  `pooled`: per iteration the same four
        with every recall taken over the targets of all classes at once (BOP's own definition), in percent."""
        T = config.TEST
        fracs = np.asarray(T.BOP_VSD_TAU, dtype=np.float64).reshape(-1)
        th_v = np.asarray(T.BOP_VSD_THRESH, dtype=np.float64).reshape(-1)
        th_s = np.asarray(T.BOP_MSSD_THRESH, dtype=np.float64).reshape(-1)
        scales = getattr(config, "SCALES", None)
        width = float(scales[0][1]) if scales else 640.0
        th_p = np.asarray(T.BOP_MSPD_THRESH, dtype=np.float64).reshape(-1) * (width / 640.0)
        min_visib = float(T.BOP_MIN_VISIB_FRACT)
        num_iter = len(errors["vsd_grid"][0]) if len(errors["vsd_grid"]) else 0
        n_cls = self.num_classes
        rec_v = np.zeros((n_cls, num_iter, len(fracs), len(th_v)))
        rec_s = np.zeros((n_cls, num_iter, len(th_s)))
        rec_p = np.zeros((n_cls, num_iter, len(th_p)))
        count_all = np.zeros((n_cls,), dtype=np.float32)
        count_targets = np.zeros((n_cls, num_iter), dtype=np.int64)
        # the hits of every class: summed over the classes they give the pooled recalls
        hit_v = np.zeros((n_cls, num_iter, len(fracs), len(th_v)))
        hit_s = np.zeros((n_cls, num_iter, len(th_s)))
        hit_p = np.zeros((n_cls, num_iter, len(th_p)))
        print_and_log("evaluating pose bop19 (vsd delta {}, tau {} of the diameter, correct below {}; targets: visible fraction >= {})".format(
            float(T.BOP_VSD_DELTA), fracs.tolist(), th_v.tolist(), min_visib), logger)
        for cls_idx, cls_name in enumerate(self.classes):
            if not len(errors["vsd_grid"][cls_idx][0]):
                continue
            count_all[cls_idx] = len(errors["vsd_grid"][cls_idx][0])
            for iter_i in range(num_iter):
                vis = np.asarray(errors["visib_gt"][cls_idx][iter_i], dtype=np.float64)
                drawn = np.asarray(errors["drawn_gt"][cls_idx][iter_i], dtype=np.float64)
                target = np.zeros(drawn.shape, dtype=bool)
                target[drawn > 0] = vis[drawn > 0] / drawn[drawn > 0] >= min_visib
                n = int(target.sum())
                count_targets[cls_idx, iter_i] = n
                e_v = np.asarray(errors["vsd_grid"][cls_idx][iter_i], dtype=np.float64).reshape(-1, len(fracs))[target]
                e_s = self._given(errors, "mssd", cls_idx, iter_i, len(target))[target]
                e_p = self._given(errors, "mspd", cls_idx, iter_i, len(target))[target]
                hit_v[cls_idx, iter_i] = (e_v[:, :, None] < th_v[None, None, :]).sum(0)
                hit_s[cls_idx, iter_i] = (e_s[:, None] < th_s[None, :] * self._diameters[cls_name]).sum(0)
                hit_p[cls_idx, iter_i] = (e_p[:, None] < th_p[None, :]).sum(0)
                if n:
                    rec_v[cls_idx, iter_i] = hit_v[cls_idx, iter_i] / n
                    rec_s[cls_idx, iter_i] = hit_s[cls_idx, iter_i] / n
                    rec_p[cls_idx, iter_i] = hit_p[cls_idx, iter_i] / n
                print_and_log("** {}, iter {} **".format(cls_name, iter_i + 1), logger)
                print_and_log("all poses: {}, targets: {}, AR_VSD: {:.2f}, AR_MSSD: {:.2f}, AR_MSPD: {:.2f}".format(
                    count_all[cls_idx], n, rec_v[cls_idx, iter_i].mean() * 100, rec_s[cls_idx, iter_i].mean() * 100,
                    rec_p[cls_idx, iter_i].mean() * 100), logger)
        ar_v = rec_v.mean((2, 3)) if rec_v.size else np.zeros((n_cls, num_iter))
        ar_s = rec_s.mean(2) if len(th_s) else np.zeros((n_cls, num_iter))
        ar_p = rec_p.mean(2) if len(th_p) else np.zeros((n_cls, num_iter))
        ar = (ar_v + ar_s + ar_p) / 3.0
        overall, pooled, num_valid_class = [], [], []
        for iter_i in range(num_iter):
            valid = int((count_targets[:, iter_i] > 0).sum())
            num_valid_class.append(valid)
            n = max(valid, 1)
            row = {"AR_VSD": np.sum(ar_v[:, iter_i]) / n * 100, "AR_MSSD": np.sum(ar_s[:, iter_i]) / n * 100,
                   "AR_MSPD": np.sum(ar_p[:, iter_i]) / n * 100, "AR": np.sum(ar[:, iter_i]) / n * 100}
            overall.append(row)
            n_all = max(int(count_targets[:, iter_i].sum()), 1)
            pool = {k: float(h[:, iter_i].sum(0).mean() / n_all * 100) if h[:, iter_i].size else 0.0
                    for k, h in (("AR_VSD", hit_v), ("AR_MSSD", hit_s), ("AR_MSPD", hit_p))}
            pool["AR"] = (pool["AR_VSD"] + pool["AR_MSSD"] + pool["AR_MSPD"]) / 3.0
            pooled.append(pool)
            print_and_log("---------- bop19 performance over {} classes -----------".format(valid), logger)
            print_and_log("** iter {} **".format(iter_i + 1), logger)
            print_and_log("AR_VSD: {:.2f}, AR_MSSD: {:.2f}, AR_MSPD: {:.2f}, AR: {:.2f}".format(
                row["AR_VSD"], row["AR_MSSD"], row["AR_MSPD"], row["AR"]), logger)
            print_and_log("pooled over {} targets: AR_VSD: {:.2f}, AR_MSSD: {:.2f}, AR_MSPD: {:.2f}, AR: {:.2f}".format(
                int(count_targets[:, iter_i].sum()), pool["AR_VSD"], pool["AR_MSSD"], pool["AR_MSPD"], pool["AR"]), logger)
        return {"recall_vsd": rec_v, "recall_mssd": rec_s, "recall_mspd": rec_p, "AR_VSD": ar_v, "AR_MSSD": ar_s, "AR_MSPD": ar_p,
                "AR": ar, "overall": overall, "pooled": pooled, "count_all": count_all, "count_targets": count_targets,
                "tau_fracs": fracs.tolist(), "thresh_vsd": th_v.tolist(), "thresh_mssd": th_s.tolist(), "thresh_mspd": th_p.tolist(),
                "min_visib_fract": min_visib, "num_valid_class": num_valid_class}
