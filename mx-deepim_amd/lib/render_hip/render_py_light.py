"""HIP rasteriser behind the reference's single-object lit LINEMOD renderer API.

Drop-in for lib/render_glumpy/render_py_light.py:
    Render_Py_Light(model_folder, K, width, height, zNear, zFar, brightness_ratios=[0.4, 0.3, 0.2])
    .render(r, t, light_position, light_intensity, brightness_k=0, r_type="quat", K=None) -> (bgr uint8 HxWx3, depth HxW)
The single-class form of Render_Py_Light_MultiProgram: same light rule (:74), same kernels.
"""
import numpy as np
import torch

from lib.render_hip.render_py_light_multi_program import Render_Py_Light_MultiProgram
from lib.render_hip.render_py_multi import quat2mat

_CLASS = "object"


class Render_Py_Light(Render_Py_Light_MultiProgram):
    def __init__(self, model_folder, K, width=640, height=480, zNear=0.25, zFar=6.0, brightness_ratios=[0.4, 0.3, 0.2], device="cuda:0",
                 mesh=None, tex_bilinear=False):
        """mesh: optional (verts, normals, uvs, faces, texture_uint8_HxWx3) replacing the files under model_folder."""
        Render_Py_Light_MultiProgram.__init__(self, [_CLASS], {_CLASS: model_folder}, K, width, height, zNear, zFar, brightness_ratios,
                                              device=device, meshes=None if mesh is None else [mesh], tex_bilinear=tex_bilinear)
        self.model_folder = model_folder

    def render(self, r, t, light_position, light_intensity, brightness_k=0, r_type="quat", K=None):
        """Reference signature (:136-219)."""
        if r_type == "quat":
            R = quat2mat(r)
        elif r_type == "mat":
            R = np.asarray(r)
        self.brightness_k = brightness_k
        pose = np.zeros((1, 3, 4), dtype=np.float32)
        pose[0, :, :3] = R
        pose[0, :, 3] = np.asarray(t, dtype=np.float32).squeeze()
        d = self.device
        bgr = torch.empty((1, self.height, self.width, 3), dtype=torch.float32, device=d)
        depth = torch.empty((1, 1, self.height, self.width), dtype=torch.float32, device=d)
        lp = torch.tensor(np.asarray(light_position, dtype=np.float32).reshape(1, 3), device=d)
        li = torch.tensor(np.asarray(light_intensity, dtype=np.float32).reshape(1, 3), device=d)
        self.render_batch(torch.zeros(1, dtype=torch.int32, device=d), torch.from_numpy(pose).to(d), lp, li, brightness_k=brightness_k, K=K,
                          bgr=bgr, depth=depth)
        return bgr[0].cpu().numpy().astype(np.uint8), depth[0, 0].cpu().numpy()
