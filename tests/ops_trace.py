"""Test helper: record the top-level calls into lib.hip.ops (the launch wrappers) as plain JSON-able data.

    with OpsTrace() as tr:
        mod.forward_backward(batch)
    tr.calls   # [[name, args, kwargs], ...] in call order

Tensors become ["T", shape, dtype], numpy arrays ["A", shape], dicts "dict"; numbers, strings, bools and None stay themselves.
Only calls made from outside ops are kept (a wrapper's own inner ops calls are not).  The four pure-arithmetic helpers of the
module (HOST) launch nothing and are left alone: where a size is computed is not part of what runs on the device."""
import functools
import json
import types

import numpy as np
import torch

HOST = ("conv_out_hw", "conv_auto_plan", "pad32", "pad64")


def reduce_arg(v):
    if torch.is_tensor(v):
        return ["T", list(v.shape), str(v.dtype)]
    if isinstance(v, np.ndarray):
        return ["A", list(v.shape)]
    if isinstance(v, dict):
        return "dict"
    if isinstance(v, (list, tuple)):
        return [reduce_arg(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


class OpsTrace(object):
    def __enter__(self):
        from lib.hip import ops

        self.ops, self.calls, self.depth, self.saved = ops, [], 0, {}
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_") and name not in HOST:
                self.saved[name] = fn
                setattr(ops, name, self._wrap(name, fn))
        return self

    def _wrap(self, name, fn):
        @functools.wraps(fn)
        def traced(*args, **kwargs):
            if self.depth == 0:
                self.calls.append([name, [reduce_arg(a) for a in args], {k: reduce_arg(v) for k, v in sorted(kwargs.items())}])
            self.depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self.depth -= 1
        return traced

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)
        return False


def as_json(obj):
    """what `obj` reads back as after a trip through a JSON file (tuples -> lists, int keys -> strings)"""
    return json.loads(json.dumps(obj))
