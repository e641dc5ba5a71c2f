"""Symmetry transformations of an object model, as the BOP protocol defines them for its symmetry-aware pose errors (MSSD, MSPD:
lib/utils/pose_error.py mssd / mspd, csrc/bop.hip).

A model's `model_info` (one entry of a BOP dataset's models_info.json) may hold
    symmetries_discrete:    a list of 4x4 rigid transformations, each as 16 numbers row-major
    symmetries_continuous:  a list of {"axis": [3], "offset": [3]}: every rotation about `axis` through the point `offset`
with translations and offsets in the unit of the model points.  A continuous symmetry is discretised into
n = ceil(pi / max_sym_disc_step) rotations by 2 pi i / n, i = 0 .. n-1; at the protocol's step of 0.01 that is 315."""
from __future__ import print_function, division

import numpy as np


def rotation_about_axis(angle, axis):
    """3x3 rotation by `angle` (radians) about the direction `axis` (Rodrigues)"""
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    norm = np.sqrt(np.sum(a * a))
    if not norm > 0:
        raise ValueError("symmetry axis must be a non-zero direction, got {!r}".format(axis))
    a = a / norm
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * Kx.dot(Kx)


def get_symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """-> (S,3,4) float64 [R | t], the identity first: every product of a discrete symmetry (the identity among them) with a
    discretised continuous one, discrete outer, continuous inner; a product applies the discrete transformation first."""
    model_info = model_info or {}
    if not max_sym_disc_step > 0:
        raise ValueError("max_sym_disc_step must be > 0, got {!r}".format(max_sym_disc_step))
    disc = [np.eye(4)]
    for s in model_info.get("symmetries_discrete", ()):
        m = np.asarray(s, dtype=np.float64)
        if m.size != 16:
            raise ValueError("symmetries_discrete: 16 numbers (4x4 row-major) per entry, got {}".format(m.size))
        disc.append(m.reshape(4, 4))
    cont = []
    for s in model_info.get("symmetries_continuous", ()):
        offset = np.asarray(s["offset"], dtype=np.float64).reshape(3)
        n = int(np.ceil(np.pi / max_sym_disc_step))
        for i in range(n):
            m = np.eye(4)
            if i:
                m[:3, :3] = rotation_about_axis(2.0 * np.pi * i / n, s["axis"])
                m[:3, 3] = offset - m[:3, :3].dot(offset)   # x -> R (x - offset) + offset
            cont.append(m)
    out = []
    for d in disc:
        for c in (cont or [np.eye(4)]):
            out.append(c.dot(d)[:3])
    return np.ascontiguousarray(np.stack(out))


def symmetry_tables(classes, symmetries, max_sym_disc_step=0.01):
    """the symmetry sets of `classes` (names, in the order that numbers class_index) concatenated, as dim_pm_sym_loss_grad and
    dim_bop_errors read them.  symmetries: {class name: a model_info dict or a ready (S,3,4) set}; a class without an entry gets the
    identity.  -> sym (Stot,3,4) float64, sym_off (n_classes+1,) int32 (class c owns sym[sym_off[c]:sym_off[c+1]], identity first),
    max_sym = the size of the largest set"""
    symmetries = symmetries or {}
    sets = [as_symmetry_set(symmetries.get(c), max_sym_disc_step) for c in classes]
    if not sets:
        raise ValueError("symmetry_tables: no classes")
    for c, s in zip(classes, sets):
        if not np.array_equal(s[0], np.eye(4)[:3]):
            raise ValueError("symmetry_tables: the set of class {!r} must start with the identity".format(c))
    sym_off = np.zeros(len(sets) + 1, dtype=np.int32)
    sym_off[1:] = np.cumsum([s.shape[0] for s in sets])
    return np.ascontiguousarray(np.concatenate(sets)), sym_off, int(max(s.shape[0] for s in sets))


def as_symmetry_set(entry, max_sym_disc_step=0.01):
    """a model_info dict or a ready (S,3,4) array -> (S,3,4) float64"""
    if entry is None or isinstance(entry, dict):
        return get_symmetry_transformations(entry, max_sym_disc_step)
    s = np.ascontiguousarray(np.asarray(entry, dtype=np.float64))
    if s.ndim != 3 or s.shape[1:] != (3, 4) or s.shape[0] < 1:
        raise ValueError("a symmetry set is (S,3,4) with S >= 1, got {}".format(s.shape))
    return s
