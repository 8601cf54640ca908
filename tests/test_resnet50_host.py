"""ResNet-50 backbone, host side (no GPU): the BACKBONE / ALPHA rules of Config.finalize(), the layer table against the keras_applications
ResNet50 v1 name list, the Keras parameter totals, the bucket layout of the flat buffers, layer-regex trainability and the .npz round trip."""
import re

import numpy as np
import pytest

from myolo.config import make_config, ShapesConfig
from myolo import engine
from myolo.engine import layer_table, init_state_dict, BUCKET_BACKBONE, BUCKET_YOLO


def _cfg(**kw):
    return make_config(ShapesConfig, BACKBONE="resnet50", IMAGE_SHAPE=[128, 128, 3], **kw)


def _keras_resnet50_names():
    """keras_applications/resnet50.py (Keras 2.2): conv1, bn_conv1, then per block 2a / 2b / 2c (+ 1 in block a), conv then BatchNorm,
    with (kernel shape, BatchNorm channels)"""
    out = [("conv1", (7, 7, 3, 64)), ("bn_conv1", 64)]
    cin = 64
    for st, blocks, (f1, f2, f3) in ((2, "abc", (64, 64, 256)), (3, "abcd", (128, 128, 512)), (4, "abcdef", (256, 256, 1024)),
                                     (5, "abc", (512, 512, 2048))):
        for b in blocks:
            p = "%d%s_branch" % (st, b)
            out += [("res" + p + "2a", (1, 1, cin, f1)), ("bn" + p + "2a", f1),
                    ("res" + p + "2b", (3, 3, f1, f2)), ("bn" + p + "2b", f2),
                    ("res" + p + "2c", (1, 1, f2, f3)), ("bn" + p + "2c", f3)]
            if b == "a":
                out += [("res" + p + "1", (1, 1, cin, f3)), ("bn" + p + "1", f3)]
            cin = f3
    return out


def _is_trunk(name):
    return name in ("conv1", "bn_conv1") or name.startswith("res") or re.match(r"bn\d", name) is not None


@pytest.mark.parametrize("bad", ["resnet101", "vgg16", "ResNet50"])
def test_unknown_backbones_are_rejected(bad):
    with pytest.raises(ValueError, match="only these are built"):
        make_config(ShapesConfig, BACKBONE=bad)


def test_resnet50_needs_alpha_one_and_mobilenet_stays_default():
    with pytest.raises(ValueError, match="ALPHA"):
        _cfg(ALPHA=0.5)
    assert _cfg().BACKBONE == "resnet50"
    assert ShapesConfig().BACKBONE == "mobilenet"


def test_resnet50_sizes_are_held_to_the_audited_mask_head():
    """a forward of more mask-head ROIs than a tested config runs (32 x 147) is refused; BASELINE configs[4] per GPU (16 x 512^2, N_BOX = 3:
    12 288 ROIs) among them, until every launch at that size has been checked against the kernels' 32-bit buffer descriptors"""
    assert engine.RESNET_MAX_MASK_ROIS == 32 * 147
    engine.resnet_check_size(2, 128, 128, 3)
    engine.resnet_check_size(6, 512, 512, 3)                  # 6 x 768 = 4608
    for n, h, nb in ((16, 512, 3), (7, 512, 3), (33, 224, 3), (1, 1024, 5)):
        with pytest.raises(ValueError, match="not been audited"):
            engine.resnet_check_size(n, h, h, nb)
    assert _cfg().GRID_H == 4


def test_layer_table_is_the_keras_resnet50_list():
    t = [(n, k, s) for n, k, s, _ in layer_table(_cfg()) if _is_trunk(n)]
    want = _keras_resnet50_names()
    assert [n for n, _, _ in t] == [n for n, _ in want]
    assert [s for _, _, s in t] == [s for _, s in want]
    assert sum(k == "convb" for _, k, _ in t) == 53 and sum(k == "bn" for _, k, _ in t) == 53
    heads = [(n, s) for n, k, s, _ in layer_table(_cfg()) if not _is_trunk(n)]
    assert heads[0] == ("conv_23", (1, 1, 2048, 3 * 9)) and heads[1] == ("feature_map", (3, 3, 512, 256))


def test_backbone_parameter_totals_are_the_keras_ones():
    sd = init_state_dict(_cfg(), seed=0)
    trunk = {k: v for k, v in sd.items() if _is_trunk(k.split("/")[0])}
    # keras.applications.ResNet50(include_top=False): 23,587,712 parameters, 53,120 of them non-trainable (the moving statistics)
    assert sum(v.size for v in trunk.values()) == 23587712
    assert sum(v.size for k, v in trunk.items() if "moving" in k) == 53120


def test_initialisation_is_keras_he_normal():
    sd = init_state_dict(_cfg(), seed=0)
    k = sd["res4a_branch2b/kernel"]
    sigma = np.sqrt(2.0 / (3 * 3 * 256))
    assert np.abs(k).max() <= 2 * sigma * (1 + 1e-6)                 # truncated at two standard deviations
    assert abs(k.std() / (sigma * 0.8796) - 1) < 0.02                 # the std of a normal truncated at +-2 sigma
    assert not sd["res4a_branch2b/bias"].any() and (sd["bn4a_branch2b/gamma"] == 1).all() and (sd["bn4a_branch2b/moving_variance"] == 1).all()
    a, b = init_state_dict(_cfg(), seed=3), init_state_dict(_cfg(), seed=3)
    assert all(np.array_equal(a[n], b[n]) for n in a)


def test_buckets_follow_the_stages():
    """conv1 ... res3d -> the backbone bucket, res4* / res5* / conv_23 -> the YOLO bucket, the heads where the MobileNet net has them (the Net lays
    the flat buffers out bucket by bucket, so each bucket is one contiguous slice whatever the table order)"""
    cfg = _cfg()
    buckets = {n: bk for n, _, _, bk in layer_table(cfg)}
    mob = {n: bk for n, _, _, bk in layer_table(make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3]))}
    for n, bk in buckets.items():
        if n in ("conv1", "bn_conv1") or re.match(r"(res|bn)[23]", n):
            assert bk == BUCKET_BACKBONE, n
        elif re.match(r"(res|bn)[45]", n) or n == "conv_23":
            assert bk == BUCKET_YOLO, n
        else:
            assert bk == mob[n], n
    assert sum(bk == BUCKET_BACKBONE for bk in buckets.values()) == 2 + (3 * 6 + 2) + (4 * 6 + 2)      # conv1, stage 2, stage 3


def test_layer_regex_trainability_on_keras_names():
    names = [n for n, _, _, _ in layer_table(_cfg())]
    heads = r"(feature_map)|(myolo_mask.*)|(conv_23)"
    stage4up = r"(res[4-5].*)|(bn[4-5].*)|" + heads
    assert [n for n in names if re.fullmatch(heads, n)] == [n for n in names if not _is_trunk(n)]
    sel = [n for n in names if re.fullmatch(stage4up, n)]
    assert "res4a_branch1" in sel and "bn5c_branch2c" in sel and "res3d_branch2c" not in sel and "bn_conv1" not in sel


def test_npz_round_trip(tmp_path):
    sd = init_state_dict(_cfg(), seed=1)
    p = str(tmp_path / "w.npz")
    np.savez(p, **sd)
    back = dict(np.load(p))
    assert set(back) == set(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    from myolo import keras_io
    groups = keras_io.state_to_keras_weights(sd)
    # Keras-named top-level layers (no nested MobileNet model) map back to the same state dict
    flat = {w: a for g in groups.values() for w, a in g}
    assert "res2a_branch2a/kernel:0" in flat and "bn_conv1/moving_mean:0" in flat
    rt = keras_io.keras_weights_to_state(flat)
    assert set(rt) == set(sd) and all(np.array_equal(rt[k], sd[k]) for k in sd)


def test_mobilenet_table_is_unchanged():
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5)
    t = layer_table(cfg)
    assert t[0] == ("conv1", "conv", (3, 3, 3, 16), 0) and t[1] == ("conv1_bn", "bn", 16, 0)
    assert [n for n, _, _, _ in t].count("conv_pw_14") == 1 and not any(n.startswith("res") for n, _, _, _ in t)
    assert len(t) == 2 + 14 * 4 + 2 + 8 + 2
    assert engine.RESNET_STAGES[1][0] == 3
