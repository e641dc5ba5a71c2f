"""HIP rasteriser behind the reference's lit LINEMOD renderer API (textured objects, several brightness ratios).

Drop-in for lib/render_glumpy/render_py_light_multi_program.py:
    Render_Py_Light_MultiProgram(class_name_list, model_folder_dict, K, width, height, zNear, zFar, brightness_ratios=[0.4, 0.3, 0.2])
    .render(r, t, light_position, light_intensity, class_name, brightness_k=0, r_type="quat") -> (bgr uint8 HxWx3, depth HxW)
The reference compiles one GL program per (class, brightness ratio); here the ratio is a kernel argument and every mesh lives in one
HBM table.  Shading is the LINEMOD fragment shader (:38-81), in which the light colour scales the diffuse term only:
    colour = texel * ((1 - ratio) + ratio * brightness * light_intensity)
evaluated in the resolve pass of `dim_raster_render_lit_lm` (csrc/raster.hip).  "__background__" entries of the class list are
skipped as in the reference (:105-107); `class_index` of `render_batch` counts the remaining classes from 0.
"""
import numpy as np
import torch

from lib.render_hip.render_py_light_modelnet_multi import load_obj_with_normals, vertex_normals
from lib.render_hip.render_py_multi import Render_Py, pose_1x3x4


class Render_Py_Light_MultiProgram(Render_Py):
    def __init__(self, class_name_list, model_folder_dict, K, width=640, height=480, zNear=0.25, zFar=6.0, brightness_ratios=[0.4, 0.3, 0.2],
                 device="cuda:0", meshes=None, tex_bilinear=False):
        """meshes: optional list, one entry per class that is not "__background__", of (verts, normals, uvs, faces, texture_uint8_HxWx3)
        replacing model_folder_dict[class]/textured.obj and texture_map.png; normals None = area-weighted vertex normals."""
        self._setup(K, width, height, zNear, zFar, device, tex_bilinear)
        self.model_folder_dict = model_folder_dict
        self.class_name_list = list(class_name_list)
        self.classes = [c for c in self.class_name_list if c != "__background__"]
        self.brightness_ratios = list(brightness_ratios)
        if meshes is None:
            from PIL import Image

            meshes = []
            for cls_name in self.classes:
                folder = model_folder_dict[cls_name]
                v, n, t, f = load_obj_with_normals("{}/textured.obj".format(folder), rescale=False, scale=1.0)
                tex = np.asarray(Image.open("{}/texture_map.png".format(folder)).convert("RGB"), dtype=np.uint8)
                meshes.append((v, n, t, f, tex))
        assert len(meshes) == len(self.classes)
        meshes = [(v, vertex_normals(v, f) if n is None else n, t, f, tex) for v, n, t, f, tex in meshes]
        self._upload([(v, t, f, tex) for v, n, t, f, tex in meshes])
        self.normals = torch.from_numpy(np.concatenate([np.ascontiguousarray(n, np.float32) for v, n, t, f, tex in meshes])).to(self.device)
        assert self.normals.shape == self.verts.shape
        self.class_name = self.classes[-1]
        self.brightness_k = 0

    def render_batch(self, class_index, poses, light_position, light_intensity, brightness_k=0, K=None, image=None, depth=None,
                     mask=None, bgr=None, bbox=None, plane_means=None, mask_thr=0.2, status=None, clean_bbox=None):
        """class_index (B,) int32, poses (B,3,4), light_position / light_intensity (B,3) f32, all cuda; one brightness ratio
        (brightness_ratios[brightness_k]) for the batch.  K, outputs, status, clean_bbox: as Render_Py.render_batch."""
        self._render(class_index, poses, K, light_position=light_position, light_intensity=light_intensity,
                     brightness_ratio=self.brightness_ratios[brightness_k], lm=True, plane_means=plane_means, mask_thr=mask_thr, image=image,
                     depth=depth, mask=mask, bgr=bgr, bbox=bbox, status=status, clean_bbox=clean_bbox)

    def render(self, r, t, light_position, light_intensity, class_name, brightness_k=0, r_type="quat"):
        """Reference signature (:156-238); returns host numpy (bgr uint8, depth float32) like the glReadPixels path."""
        pose = pose_1x3x4(r, t, r_type)
        self.class_name = class_name
        self.brightness_k = brightness_k
        d = self.device
        bgr = torch.empty((1, self.height, self.width, 3), dtype=torch.float32, device=d)
        depth = torch.empty((1, 1, self.height, self.width), dtype=torch.float32, device=d)
        lp = torch.tensor(np.asarray(light_position, dtype=np.float32).reshape(1, 3), device=d)
        li = torch.tensor(np.asarray(light_intensity, dtype=np.float32).reshape(1, 3), device=d)
        self.render_batch(torch.tensor([self.classes.index(class_name)], dtype=torch.int32, device=d), torch.from_numpy(pose).to(d), lp, li,
                          brightness_k=brightness_k, bgr=bgr, depth=depth)
        return bgr[0].cpu().numpy().astype(np.uint8), depth[0, 0].cpu().numpy()

