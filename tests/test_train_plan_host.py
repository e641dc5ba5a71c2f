"""CPU: the training executor's backward plan (deepim.core.module.plan_backward) needs no device and decides what the executor
decided before the plan existed.

tests/golden/launch_trace/ holds, per case, what that executor allocated (`sizes`), its `wgrad_splits` / `wino_wgrad` tables and the
trace of one step on a 256-CU device; the plan is built here for the same CU count and compared with all three.  A second, literal
table states what the rules give at 256 CUs with the decoder present, so that a reader sees the plan without opening a golden."""
import json
import os

import pytest

from conftest import GOLDEN

CASES = [(2, "f32"), (2, "bf16"), (16, "f32"), (16, "bf16")]
WINO, WINO5 = ("conv3_1", "conv4_1", "conv5_1", "conv6_1"), ("conv2", "conv3")   # the f32 forward's Winograd layers; bf16 has none
DGRAD_CALLS = {"conv2d_dgrad": "gemm", "conv2d_dgrad_lrelu": "fold", "conv2d_dgrad_winograd5x5s2": "wino5", "conv2d_fwd_winograd": "wino"}


def plan(B, dtype, sw=None, n_cu=256):
    from deepim.core import module

    f32 = dtype == "f32"
    return module.plan_backward(B, not f32, True, n_cu, set(WINO if f32 else ()), set(WINO5 if f32 else ()), {n: 4 for n in WINO if f32}, 0,
                                sw or module.read_switches({}))


def brief(layer):
    """'fused 316 / -', 'wino S2 sp15 / wino5', 'fused 8 / wino tile 3', 'fused 5 / gemm 3,2', 'fused 59 / fold'"""
    wg, dg = layer.wgrad, layer.dgrad
    a = "wino S{} sp{}".format(wg.S, wg.splits) if wg.kind == "wino" else "{} {}".format(wg.kind, wg.splits)
    b = {None: "-", "wino": "wino tile {}".format(dg.tile), "gemm": "gemm {},{}".format(dg.tile, dg.splits)}.get(dg.kind, dg.kind)
    return a + " / " + b


@pytest.mark.parametrize("B,dtype", CASES)
def test_plan_equals_what_the_executor_decided(hip_lib, B, dtype):
    with open(os.path.join(GOLDEN, "launch_trace", "train_B{}_{}.json".format(B, dtype))) as f:
        want = json.load(f)
    pl = plan(B, dtype, n_cu=want["n_cu"])
    assert {k: getattr(pl, k) for k in want["sizes"]} == want["sizes"]
    for layer in pl.layers:
        name, wg = layer.geom.name, layer.wgrad
        if name in want["wino_wgrad"]:
            assert (wg.kind, [wg.S, wg.splits]) == ("wino", want["wino_wgrad"][name]), name
        else:
            assert (wg.kind, wg.splits) == ("fused", want["wgrad_splits"][name]), name
    # the input gradients, as launched: once per layer from conv6_1 down to conv2
    calls = [c for c in want["trace"] if c[0] in DGRAD_CALLS and (c[0] != "conv2d_fwd_winograd" or c[2]["slope"] == 1.0)]
    assert len(calls) == 9 and pl.layers[-1].dgrad.kind is None
    for layer, (fn, _, kw) in zip(pl.layers, calls):
        dg = layer.dgrad
        assert dg.kind == DGRAD_CALLS[fn], (layer.geom.name, fn)
        if dg.kind == "gemm":
            assert (dg.tile, dg.splits) == (kw["tile"], kw["splits"]), layer.geom.name
        if dg.kind == "wino":
            assert (dg.tile, dg.m) == (kw["tile"], kw["m"]), layer.geom.name
    # a layer computes its own dz exactly when the layer above did not fold it into its input gradient
    n_dz = sum(1 for c in want["trace"] if c[0] == "lrelu_bwd_bias_grad")
    assert n_dz == sum(1 for layer in pl.layers if layer.own_dz)
    assert [layer.own_dz for layer in pl.layers[1:]] == [layer.dgrad.kind != "fold" for layer in pl.layers[:-1]]
    assert {layer.geom.name: layer.skip for layer in pl.layers if layer.skip} == {"conv5_1": "dconcat2", "conv4_1": "dconcat3"}


@pytest.mark.parametrize("B,dtype", CASES)
def test_bias_workspace_covers_every_call_through_it(hip_lib, B, dtype):
    """every dim_bias_grad / dim_lrelu_bwd_bias_grad call of the recorded step needs, by its own size function, no more than the plan
    without the 64 Ki floats it carries on top of the first layer's size (kept because the goldens record the workspace's shape; the
    kernels stay inside the reported size: tests/test_gpu_conv_workspace_contract.py::test_column_sums)"""
    with open(os.path.join(GOLDEN, "launch_trace", "train_B{}_{}.json".format(B, dtype))) as f:
        want = json.load(f)
    pl = plan(B, dtype, n_cu=want["n_cu"])
    size_fn = {"bias_grad": hip_lib.dim_bias_grad_workspace_floats, "lrelu_bwd_bias_grad": hip_lib.dim_lrelu_bwd_bias_grad_workspace_floats}
    needs = []
    for fn, args, kw in want["trace"]:
        if fn not in size_fn:
            continue
        shape = args[0 if fn == "bias_grad" else 1][1]                 # dz / dy: (N, H, W, row width)
        rows, C = shape[0] * shape[1] * shape[2], args[1 if fn == "bias_grad" else 2]
        needs.append(size_fn[fn](rows, C))
        assert 0 < needs[-1] <= pl.bias_ws == kw["workspace"][1][0], (fn, rows, C, needs[-1])
    assert len(needs) >= 8
    without = max(hip_lib.dim_bias_grad_workspace_floats(B * 240 * 320, 64), max(n for n in needs))
    print("B {} {}: largest need {} floats, allocated {}".format(B, dtype, max(needs), pl.bias_ws))
    assert max(needs) <= without <= pl.bias_ws


# layer: f32 B=2, f32 B=16, bf16 B=2, bf16 B=16   (256 CUs, decoder present; "gemm t,k" = workgroup tile t, split-K k)
TABLE = {
    "flow_conv1": ("fused 316 / -", "fused 316 / -", "fused 256 / -", "fused 256 / -"),
    "conv2": ("wino S2 sp15 / wino5", "wino S2 sp15 / wino5", "fused 59 / fold", "fused 59 / fold"),
    "conv3": ("wino S2 sp4 / wino5", "wino S2 sp4 / wino5", "fused 15 / fold", "fused 15 / fold"),
    "conv3_1": ("wino S1 sp4 / wino tile 3", "wino S1 sp8 / wino tile 4", "fused 32 / fold", "fused 32 / fold"),
    "conv4": ("fused 15 / gemm 3,1", "fused 15 / gemm 3,1", "fused 10 / gemm 9,1", "fused 10 / gemm 9,1"),
    "conv4_1": ("fused 8 / wino tile 3", "wino S1 sp2 / wino tile 4", "fused 8 / fold", "fused 8 / fold"),
    "conv5": ("fused 4 / gemm 3,1", "fused 8 / gemm 3,1", "fused 4 / gemm 3,8", "fused 5 / gemm 3,2"),
    "conv5_1": ("fused 4 / wino tile 3", "wino S1 sp2 / wino tile 3", "fused 4 / gemm 3,8", "fused 5 / gemm 3,2"),
    "conv6": ("fused 1 / gemm 3,1", "fused 4 / gemm 3,1", "fused 1 / gemm 3,8", "fused 2 / gemm 3,8"),
    "conv6_1": ("fused 1 / wino tile 3", "fused 2 / wino tile 3", "fused 1 / gemm 3,8", "fused 1 / gemm 3,4"),
}


def test_plan_table_at_256_cus(hip_lib):
    for col, (B, dtype) in enumerate([(2, "f32"), (16, "f32"), (2, "bf16"), (16, "bf16")]):
        got = {layer.geom.name: brief(layer) for layer in plan(B, dtype).layers}
        assert got == {name: row[col] for name, row in TABLE.items()}, (B, dtype)


def test_switches_reach_the_plan(hip_lib):
    """derived from the rules, at (B = 16, bf16): without split-K every count is 1; without the fold its layers run the patch kernel"""
    from deepim.core import module

    sw = module.read_switches({})
    assert sw == module.read_switches({"DIM_BF16_HALO": "1"}) and all(sw[3:])
    base = plan(16, "bf16", sw)
    assert {layer.dgrad.splits for layer in base.layers} == {1, 2, 4, 8}
    no_splitk = plan(16, "bf16", module.read_switches({"DIM_BF16_DGRAD_SPLITK": "0"}))
    assert {layer.dgrad.splits for layer in no_splitk.layers} == {1}
    assert [layer.dgrad.kind for layer in no_splitk.layers] == [layer.dgrad.kind for layer in base.layers]
    no_fold = plan(16, "bf16", sw._replace(fold_lrelu=False))
    assert no_fold.fold_ws == 0 and all(layer.own_dz for layer in no_fold.layers)
    for a, b in zip(base.layers, no_fold.layers):
        if a.dgrad.kind == "fold":
            assert (b.dgrad.kind, b.dgrad.tile, b.dgrad.splits) == ("gemm", 9, 1), a.geom.name
        else:
            assert b.dgrad == a.dgrad
    assert [layer.geom.name for layer in base.layers if layer.dgrad.kind == "fold"] == ["conv4_1", "conv3_1", "conv3", "conv2"]
