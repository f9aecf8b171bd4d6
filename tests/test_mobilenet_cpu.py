"""MobileNetV2 / V3 HDEN backbones (torchvision's architectures on the depthwise HIP kernels): construction, key names,
parameter totals, BatchNorm settings and the C ABI of the new kernels.  No GPU needed."""
import os
import re
import warnings

import pytest
import torch

from adam_dehaze_amd import _hip as H
from adam_dehaze_amd import classifier as CL
from tests import _mobilenet_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mobilenet_v2", "mobilenet_v3_large", "mobilenet_v3_small")


def _model(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return CL.FogIntensityClassifier(name, 3, pretrained=False)


@pytest.mark.parametrize("name,keys,params,fd", [("mobilenet_v2", 316, 2552579, 1280),
                                                 ("mobilenet_v3_large", 312, 3218739, 960),
                                                 ("mobilenet_v3_small", 244, 1075491, 576)])
def test_key_count_and_parameter_total(name, keys, params, fd):
    m = _model(name)
    assert len(m.state_dict()) == keys
    assert sum(p.numel() for p in m.parameters()) == params
    assert m.feature_dim == fd


def test_sample_keys_and_shapes():
    v2 = _model("mobilenet_v2").state_dict()
    assert tuple(v2["backbone.features.3.conv.1.0.weight"].shape) == (144, 1, 3, 3)
    assert tuple(v2["backbone.features.1.conv.0.0.weight"].shape) == (32, 1, 3, 3)     # t = 1: the depthwise CNA is conv.0
    assert tuple(v2["backbone.features.1.conv.1.weight"].shape) == (16, 32, 1, 1)
    assert tuple(v2["backbone.features.18.0.weight"].shape) == (1280, 320, 1, 1)
    large = _model("mobilenet_v3_large").state_dict()
    assert tuple(large["backbone.features.4.block.2.fc1.weight"].shape) == (24, 72, 1, 1)
    assert tuple(large["backbone.features.4.block.1.0.weight"].shape) == (72, 1, 5, 5)
    assert tuple(large["backbone.features.16.0.weight"].shape) == (960, 160, 1, 1)
    assert "backbone.features.1.block.0.0.weight" in large and tuple(large["backbone.features.1.block.0.0.weight"].shape) == (16, 1, 3, 3)
    small = _model("mobilenet_v3_small").state_dict()
    assert tuple(small["backbone.features.1.block.1.fc2.weight"].shape) == (16, 8, 1, 1)
    assert tuple(small["backbone.features.12.0.weight"].shape) == (576, 96, 1, 1)
    assert not any(k.startswith("backbone.classifier") for k in small)


def test_v3_batchnorm_eps_and_momentum():
    for name in NAMES:
        bns = [m for m in _model(name).backbone.modules() if isinstance(m, CL.BNParams)]
        assert bns
        want = (1e-5, 0.1) if name == "mobilenet_v2" else (1e-3, 0.01)
        for b in bns:
            assert (b.eps, b.momentum) == want
            st = b.state()
            assert (st.eps, st.momentum) == want
    # the default keeps every existing layer at nn.BatchNorm2d's settings
    st = CL.BNParams(8).state()
    assert (st.eps, st.momentum) == (1e-5, 0.1)


@pytest.mark.parametrize("name", NAMES)
def test_strict_load_of_generated_state_dict(name):
    sd = MR.state_dict(name, seed=1)
    m = _model(name)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("name", NAMES)
def test_create_classifier(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = CL.create_classifier({"classifier": {"model": name, "num_classes": 3, "pretrained": True}})
    assert m.model_name == name and m.feature_dim == MR.FEATURE_DIM[name]


@pytest.mark.parametrize("name", ["efficientnet_b0", "mobilenet_v3_medium", "mobilenet_v1"])
def test_other_names_still_raise(name):
    with pytest.raises(ValueError):
        CL.FogIntensityClassifier(name, 3, pretrained=False)


def test_dense_feature_extractor_unchanged():
    with pytest.raises(ValueError):
        CL.DenseFeatureExtractor("mobilenet_v2", pretrained=False)


def test_restatement_runs_on_cpu():
    # the float64 restatement the GPU tests compare against: shapes, and train-mode BN updates the running statistics
    for name in NAMES:
        sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in MR.state_dict(name, seed=2).items()}
        x = torch.rand(2, 3, 40, 56, dtype=torch.float64)
        logits, f = MR.classifier_forward(x, sd, name)
        assert logits.shape == (2, 3) and f.shape == (2, MR.FEATURE_DIM[name]) and torch.isfinite(logits).all()
        key = "backbone.features.2." + ("conv.0.1" if name == "mobilenet_v2" else "block.1.1")
        rm = sd[key + ".running_mean"].clone()
        MR.classifier_forward(x, sd, name, training=True)
        assert not torch.equal(rm, sd[key + ".running_mean"]) and int(sd[key + ".num_batches_tracked"]) == 1


NEW_SYMBOLS = ("adh_dwconv_pack_weights", "adh_dwconv_num_blocks", "adh_dwconv_fwd", "adh_dwconv_dgrad",
               "adh_dwconv_wgrad_num_blocks", "adh_dwconv_wgrad", "adh_channel_scale", "adh_channel_scale_bwd_num_blocks",
               "adh_channel_scale_bwd")


def test_new_abi_symbols_and_activation_codes():
    header = open(os.path.join(ROOT, "include", "adam_dehaze_hip.h")).read()
    declared = set(re.findall(r"^int\s+(adh_\w+)\s*\(", header, flags=re.M))
    lib = H.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in H._SIGNATURES and hasattr(lib, name), name
    codes = {k: int(v) for k, v in re.findall(r"#define ADH_ACT_(\w+) (\d+)", header)}
    assert codes["RELU6"] == H.ACT_RELU6 == 4
    assert codes["HARDSWISH"] == H.ACT_HARDSWISH == 5
    assert codes["HARDSIGMOID"] == H.ACT_HARDSIGMOID == 6
    assert "depthwise.hip" in open(os.path.join(ROOT, "adam-dehaze_amd", "csrc", "Makefile")).read()
