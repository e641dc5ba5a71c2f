"""What the zoom custom ops share: sampling an input of any size into the op's (height, width), and the refusal of the ops that are
defined between planes of one size only."""
from lib.hip import ops


def zoom_to(x, zoom_factor, height, width, **kw):
    """x (B,C,Hs,Ws) sampled into (B,C,height,width) with the window `zoom_factor` (fractions of x's own size), as MXNet's
    GridGenerator(target_shape=(height, width)) + BilinearSampler do with such an input.  kw: pre / post / add3 of ops.zoom_planes."""
    if tuple(x.shape[2:]) == (height, width):
        return ops.zoom_planes(x, zoom_factor, **kw)
    return ops.zoom_planes_src(x, zoom_factor, net_size=(height, width), **kw)


def zoomed_shape(shape, height, width):
    return [shape[0], shape[1], height, width]


def require_same_size(op, x, height, width, why):
    if tuple(x.shape[2:]) != (height, width):
        raise ValueError("{}: {} is defined between planes of one size only, got a {}x{} input for height x width = {}x{}".format(
            op, why, x.shape[2], x.shape[3], height, width))
