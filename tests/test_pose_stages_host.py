"""Which pose stages are on (deepim.core.pose_stages.stages_on) is asked in one place: the settings functions, refuse_at_source_size and
pred_eval's store must all agree with it, for every shipped yaml, the all-off default and all four stages at once.  No GPU."""
import glob
import os
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs")
YAMLS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CFGS, "*.yaml")))
ALL_ON = {"ICP_ITER": 10, "FLOW_PNP_ITER": 4, "PHOTO_ITER": 4, "SIL_ITER": 6, "FAST_TEST": False}
KEYS = {"icp": "ICP_ITER", "flow_pnp": "FLOW_PNP_ITER", "photo": "PHOTO_ITER", "sil": "SIL_ITER"}


@pytest.fixture(params=["default", "all four on"] + YAMLS)
def cfg(request):
    from deepim.config.config import config, reset_config, update_config

    reset_config()
    if request.param.endswith(".yaml"):
        update_config(os.path.join(CFGS, request.param))
    elif request.param == "all four on":
        config.TEST.update(ALL_ON)
        config.network.PRED_FLOW = True
    yield config
    reset_config()


def test_the_shipped_yamls_are_found():
    assert "deepim_hip_LM_ape_test_photo.yaml" in YAMLS and "deepim_hip_LM_ape_test_sil.yaml" in YAMLS


def test_all_four_on_switches_all_four_on():
    from deepim.config.config import config, reset_config
    from deepim.core.pose_stages import stages_on

    reset_config()
    assert stages_on(config) == ()
    config.TEST.update(ALL_ON)
    assert set(stages_on(config)) == set(KEYS)
    reset_config()


def test_stages_on_is_what_the_settings_report(cfg):
    from deepim.core.pose_stages import STAGE_KEY, stage_settings, stages_on
    from deepim.core.tester import flow_pnp_settings, icp_settings, photo_settings, sil_settings

    assert STAGE_KEY == KEYS
    settings = {"icp": icp_settings, "flow_pnp": flow_pnp_settings, "photo": photo_settings, "sil": sil_settings}
    on = stages_on(cfg)
    assert len(set(on)) == len(on)
    assert set(on) == {name for name, f in settings.items() if f(cfg)[0] > 0}
    assert stage_settings(cfg) == {name: f(cfg) for name, f in settings.items()}


def test_a_foreign_size_refuses_exactly_the_stages_that_are_on(cfg):
    from deepim.core.pose_stages import stages_on
    from deepim.core.tester import refuse_at_source_size

    on = stages_on(cfg)
    kept = {name: cfg.TEST.get(key, 0) for name, key in KEYS.items()}
    # everything else that exists at the network size only is switched off, so that only a stage can be what raises
    cfg.TEST.update({"HYP_NUM": 1, "COARSE_VIEWS": 0, "VSD": False, "BOP_VSD": False, "FAST_TEST": True})
    for name, key in KEYS.items():
        cfg.TEST.update({k: (kept[n] if n == name else 0) for n, k in KEYS.items()})   # this stage alone, as the config has it
        refuse_at_source_size(cfg, (480, 640))
        if name in on:
            with pytest.raises(ValueError, match=r"TEST\.{} is built for SCALES".format(key)):
                refuse_at_source_size(cfg, (960, 1280))
        else:
            refuse_at_source_size(cfg, (960, 1280))


def test_pred_eval_stores_the_loop_and_exactly_the_stages_that_are_on(cfg, hip_lib):
    from deepim.core.pose_stages import stages_on
    from deepim.core.tester import _eval_setup

    on = stages_on(cfg)
    cfg.TEST.update({"VSD": False, "BOP": False, "BOP_VSD": False, "DEVICE_EVAL": False})   # the scorers need a render machine
    refiner = SimpleNamespace(N=1, B=2, P=2, coarse=None, net=SimpleNamespace(device="cpu"))
    st = _eval_setup(cfg, refiner, SimpleNamespace(classes=["ape", "cat"]), None)
    assert {key[0] for key in st.store if isinstance(key, tuple)} == {"loop"} | set(on)
    assert ("flow_rows" in st.store) == ("flow_pnp" in on)
