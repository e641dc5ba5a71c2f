"""ctypes face of the resident-loop C entry points (include/deepim_hip.h: dim_refiner_create / _create_cls / _create_src /
_set_zoom_filter / _run / _run_k / _destroy).

This is what a host WITHOUT torch binds (INTEGRATION.md shows the same struct for C / cgo callers); torch is used here only to own
the device memory of the arguments, exactly as in the rest of lib/hip."""
import ctypes

import numpy as np
import torch

from . import capi
from .capi import check, current_stream, dptr, lib


class RefinerDesc(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("test_iter", ctypes.c_int), ("K9", ctypes.c_float * 9),
                ("pixel_means_bgr", ctypes.c_float * 3), ("T_means", ctypes.c_float * 3), ("T_stds", ctypes.c_float * 3),
                ("rot_coord", ctypes.c_int), ("znear", ctypes.c_float), ("zfar", ctypes.c_float), ("tex_bilinear", ctypes.c_int),
                ("verts", ctypes.c_void_p), ("uvs", ctypes.c_void_p), ("faces", ctypes.c_void_p), ("mesh_table", ctypes.c_void_p),
                ("n_classes", ctypes.c_int), ("vmax", ctypes.c_int), ("fmax", ctypes.c_int), ("textures", ctypes.c_void_p),
                ("tex_table", ctypes.c_void_p)]


class CRefiner(object):
    """the refinement loop driven entirely by libdeepim_hip.so: same launches as deepim.core.tester.Refiner (FAST_TEST graph)"""

    def __init__(self, config, arg_params, render_machine, batch_size, device="cuda:0"):
        cfg, rm = config, render_machine
        if int(cfg.TEST.get("HYP_NUM", 1) or 1) > 1:
            raise ValueError("the C loop object (dim_refiner_create / dim_refiner_run) refines one hypothesis per pair: TEST.HYP_NUM > 1 "
                             "runs through deepim.core.tester.Refiner")
        if int(cfg.TEST.get("COARSE_VIEWS", 0) or 0) > 0:
            raise ValueError("the C loop object (dim_refiner_create / dim_refiner_run) starts from the poses it is given: TEST.COARSE_VIEWS > 0 "
                             "runs through deepim.core.tester.Refiner")
        if int(cfg.TEST.get("VIEWS", 1) or 1) > 1:
            raise ValueError("the C loop object (dim_refiner_create / dim_refiner_run) is the loop alone, one pose per sample: TEST.VIEWS > 1 "
                             "runs through deepim.core.tester.Refiner")
        self.B, self.T = int(batch_size), int(cfg.TEST.test_iter)
        self.device = torch.device(device)
        names = [n for n in arg_params if n.split("_weight")[0].split("_bias")[0] in
                 ("flow_conv1", "conv2", "conv3", "conv3_1", "conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1", "fc6", "fc7", "rot", "trans")]
        self.params = {n: torch.as_tensor(np.ascontiguousarray(arg_params[n]), dtype=torch.float32).to(self.device) for n in names}
        d = RefinerDesc()
        d.B, d.H, d.W, d.test_iter = self.B, rm.height, rm.width, self.T
        d.K9 = (ctypes.c_float * 9)(*np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32).reshape(9))
        d.pixel_means_bgr = (ctypes.c_float * 3)(*np.asarray(cfg.network.PIXEL_MEANS, np.float32).reshape(3))
        d.T_means = (ctypes.c_float * 3)(*np.asarray(cfg.dataset.trans_means, np.float32).reshape(3))
        d.T_stds = (ctypes.c_float * 3)(*np.asarray(cfg.dataset.trans_stds, np.float32).reshape(3))
        d.rot_coord, d.znear, d.zfar, d.tex_bilinear = capi.rot_coord_id(cfg.network.ROT_COORD), rm.zNear, rm.zFar, int(rm.tex_bilinear)
        d.verts, d.uvs, d.faces, d.mesh_table = rm.verts.data_ptr(), rm.uvs.data_ptr(), rm.faces.data_ptr(), rm.mesh_table.data_ptr()
        d.n_classes, d.vmax, d.fmax = int(rm.mesh_table.shape[0]), rm.vmax, rm.fmax
        d.textures, d.tex_table = rm.textures.data_ptr(), rm.tex_table.data_ptr()
        self._rm = rm   # keeps the mesh table alive
        cnames = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        cptrs = (ctypes.c_void_p * len(names))(*[self.params[n].data_ptr() for n in names])
        self._h = ctypes.c_void_p()
        K = int(cfg.network.get("REGRESSOR_NUM", 1))   # the library checks it against the mesh table's class count
        if tuple(self.params["rot_weight"].shape) != (4 * K, 256) or tuple(self.params["trans_weight"].shape) != (3 * K, 256):
            raise ValueError("rot_weight {} / trans_weight {}: network.REGRESSOR_NUM = {} needs ({}, 256) / ({}, 256)".format(
                tuple(self.params["rot_weight"].shape), tuple(self.params["trans_weight"].shape), K, 4 * K, 3 * K))
        if (d.H, d.W) != (480, 640):   # a camera image of another (4:3) size: the blobs and the renders at it, the network input at 480x640
            check(lib().dim_refiner_create_src(ctypes.byref(self._h), ctypes.byref(d), K, cnames, cptrs, len(names), current_stream()))
        elif K > 1:   # one rot / trans head per class: run() picks each pair's by the class_index it receives
            check(lib().dim_refiner_create_cls(ctypes.byref(self._h), ctypes.byref(d), K, cnames, cptrs, len(names), current_stream()))
        else:
            check(lib().dim_refiner_create(ctypes.byref(self._h), ctypes.byref(d), cnames, cptrs, len(names), current_stream()))
        # TEST.ZOOM_FILTER 'area': the loop's zoom through dim_zoom_net_input_area (any create function; before the first run)
        from deepim.symbols.deepIM_flownet import zoom_filter

        name, max_taps = zoom_filter(cfg)
        if name == "area":
            check(lib().dim_refiner_set_zoom_filter(self._h, max_taps))
        torch.cuda.synchronize(self.device)
        self.poses_iter = torch.zeros((self.T, self.B, 3, 4), dtype=torch.float32, device=self.device)
        self.se3_iter = torch.zeros((self.T, self.B, 7), dtype=torch.float32, device=self.device)
        self.status_iter = torch.zeros((self.T, self.B), dtype=torch.int32, device=self.device)

    def refine(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, K_per_pair=None):
        """K_per_pair: None (dim_refiner_run: the desc's K9) or a (B,9) / (B,3,3) f32 CUDA tensor, the camera of each pair's re-render
        (dim_refiner_run_k)"""
        f32 = torch.float32
        args = (self._h, dptr(image_observed, f32), dptr(image_rendered, f32), dptr(mask_observed, f32), dptr(mask_rendered, f32),
                dptr(src_pose, f32), dptr(class_index, torch.int32), dptr(self.poses_iter, f32), dptr(self.se3_iter, f32),
                dptr(self.status_iter, torch.int32))
        if K_per_pair is None:
            check(lib().dim_refiner_run(*args, current_stream()))
        else:
            if tuple(K_per_pair.shape) not in ((self.B, 9), (self.B, 3, 3)):
                raise ValueError("K_per_pair must be ({0},9) or ({0},3,3), got {1}".format(self.B, tuple(K_per_pair.shape)))
            check(lib().dim_refiner_run_k(*args, dptr(K_per_pair, f32), current_stream()))
        return self.poses_iter

    def close(self):
        if self._h:
            check(lib().dim_refiner_destroy(self._h))
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
