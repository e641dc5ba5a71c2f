"""GPU: the training step and the test-graph forward launch exactly what tests/golden/launch_trace/ records.

The goldens were recorded (tests/ops_trace.py) on the commit before the encoder geometry table and the backward plan existed, when
every consumer derived its shapes, kernel choices and workspace sizes with a loop of its own.  Equality of every call, in order,
with every scalar and every tensor shape / dtype (workspaces included), and of the buffer sizes, is the statement "same kernels,
same order, same arguments, same buffers".  The plans depend on the CU count, so another device skips.  Values do not enter a
trace: the B = 16 batch is the B = 2 scene repeated."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402
from ops_trace import OpsTrace, as_json  # noqa: E402
from scene import make_train_config, make_train_scene  # noqa: E402

DEV = "cuda:0"
TRACES = os.path.join(GOLDEN, "launch_trace")
CASES = [(2, "f32"), (2, "bf16"), (16, "f32"), (16, "bf16")]
BUFFERS = ("ws", "gpack", "bias_ws", "fold_ws", "wino_ws", "wino_wgrad_ws")


def golden(name):
    with open(os.path.join(TRACES, name + ".json")) as f:
        return json.load(f)


def make_inputs():
    """configuration, parameters and batch of tests/test_gpu_train.py's `setup`"""
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    cfg = make_train_config()
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=True)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    rng = np.random.RandomState(1)
    params["trans_weight"] = (rng.randn(3, 256) * 0.002).astype(np.float32)
    params["rot_weight"][1:] = (rng.randn(3, 256) * 0.01).astype(np.float32)
    params["mask_conv3_weight"] = (rng.randn(1, 770, 3, 3) * 0.02).astype(np.float32)
    return cfg, params, make_train_scene(B=2, seed=99, subdiv=3)["blobs"]


@pytest.fixture(scope="module")
def inputs(hip_lib):
    assert torch.cuda.is_available()
    n_cu, want = int(hip_lib.dim_device_info(None, 0)), golden("train_B2_f32")["n_cu"]
    if n_cu != want:
        pytest.skip("launch plans depend on the CU count: the goldens were recorded on {} CUs, this device has {}".format(want, n_cu))
    return make_inputs()


def device_batch(blobs, B):
    return {k: torch.as_tensor(np.ascontiguousarray(np.concatenate([v] * (B // 2)))).to(DEV) for k, v in blobs.items()}


def net_facts(net):
    return dict(workspace=net.workspace.numel(), conv_plan=net.conv_plan, layer_info=net.layer_info)


def record_train(cfg, params, blobs, B, dtype):
    """one forward_backward + update of a fresh MutableModule -> (module, what the golden holds about it)"""
    from deepim.core.module import MutableModule

    mod = MutableModule(cfg, params, B, compute_dtype=dtype)
    batch = device_batch(blobs, B)
    with OpsTrace() as tr:
        mod.forward_backward(batch)
        mod.update(cfg.TRAIN.lr)
    torch.cuda.synchronize()
    sizes = {k: (getattr(mod, k, None).numel() if getattr(mod, k, None) is not None else 0) for k in BUFFERS}
    return mod, as_json(dict(n_cu=mod.n_cu, sizes=sizes, net=net_facts(mod.net), trace=tr.calls))


def record_forward_test(cfg, params, blobs):
    from deepim.symbols.deepIM_flownet import FlowNetHip

    net = FlowNetHip(cfg, params, 2, device=DEV)
    batch = device_batch(blobs, 2)
    with OpsTrace() as tr:
        net.forward_test(batch)
    torch.cuda.synchronize()
    facts = net_facts(net)
    facts.update(wino=sorted(net.wino), wino5=sorted(net.wino5), wino3s2=sorted(net.wino3s2), wino_m=net.wino_m)
    return as_json(dict(net=facts, trace=tr.calls))


def assert_same(got, want):
    for key in want:
        if key == "trace":
            continue
        assert got[key] == want[key], key
    assert [c[0] for c in got["trace"]] == [c[0] for c in want["trace"]]
    for i, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, (i, a, b)


@pytest.mark.parametrize("B,dtype", CASES)
def test_training_step_launches(inputs, B, dtype):
    cfg, params, blobs = inputs
    want = golden("train_B{}_{}".format(B, dtype))
    _, got = record_train(cfg, params, blobs, B, dtype)
    assert_same(got, {k: v for k, v in want.items() if k not in ("wgrad_splits", "wino_wgrad")})   # those two: tests/test_train_plan_host.py


def test_forward_test_launches(inputs):
    cfg, params, blobs = inputs
    assert_same(record_forward_test(cfg, params, blobs), golden("forward_test_B2"))


def test_two_steps_from_the_same_parameters_agree(inputs):
    """the plan object is reused, not rebuilt: a second backward from the same parameters gives the same gradients, to the bar
    tests/test_gpu_train.py sets for them (not bit-equal: the plane GEMMs share stream-K tiles through atomics)"""
    from deepim.core.module import MutableModule

    cfg, params, blobs = inputs
    mod = MutableModule(cfg, params, 2)
    batch = device_batch(blobs, 2)
    mod.forward_backward(batch)
    assert torch.isfinite(mod.flat_g).all()
    first = mod.get_grads()
    mod.forward_backward(batch)
    assert torch.isfinite(mod.flat_g).all()
    for k, b in mod.get_grads().items():
        a, scale = first[k], np.abs(first[k]).max()
        exact_path = k.startswith(("fc", "rot", "trans", "Convolution", "deconv4", "upsample_flow", "mask_conv3"))
        err = np.abs(a - b).max()
        l2 = np.linalg.norm((a - b).ravel()) / (np.linalg.norm(a.ravel()) + 1e-30)
        print("grad {:28s} max|g| {:.3e}  max err {:.3e}  l2 {:.2e}".format(k, scale, err, l2))
        assert err <= (2e-5 if exact_path else 5e-2) * scale + 1e-9, (k, err, scale)
        assert l2 <= (2e-5 if exact_path else 1e-2), (k, l2)
