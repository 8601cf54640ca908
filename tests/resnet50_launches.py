"""The launches of the ResNet-50 trunk at the size the engine ships at: 6 images of 512 x 512, 81 classes, N_BOX 3 (engine.RESNET_MAX_MASK_ROIS).

LAUNCHES lists every distinct (C-ABI entry point, its integer arguments in signature order) that one training step and one inference forward
issue for the trunk, feature_map and conv_23 (Net.trunk_fwd, Net.yolo_head_bwd, Net.trunk_bwd), each with the layers it stands for.  The library
picks its kernel from the entry and these integers (for fixed options), so the table is the list of kernel choices to hold against float64:
tests/test_gpu_resnet50_fullsize.py runs every row as an operator case, and its census records the launches of a real step and asserts that the
table and the engine agree in both directions.  The mask head's launches (4 608 ROIs) are tests/test_gpu_fullsize.py's.

A plain helper module: no GPU, no library needed to import it."""
import contextlib

B, SIZE, NUM_CLASSES, N_BOX = 6, 512, 81, 3

TRAIN, INFER = "train", "infer"

BOTH = (TRAIN, INFER)

# entry point -> [(integer arguments in signature order, phases that issue it, the layers it stands for)]
LAUNCHES = {
    "myolo_add_inplace": [
        ((3145728,), (TRAIN,), "res5[bc]'s input"),
        ((6291456,), (TRAIN,), "res2a's input, res4[bcdef]'s input"),
        ((12582912,), (TRAIN,), "res3[bcd]'s input, C4 (feature_map + YOLO branch)"),
        ((25165824,), (TRAIN,), "res2[bc]'s input"),
    ],
    "myolo_bn_act_bwd": [
        ((1536, 512, 1, 1), (TRAIN,), "bn5[abc]_branch2a, bn5[abc]_branch2b"),
        ((1536, 2048, 0, 1), (TRAIN,), "bn5[abc]_branch2c, bn5a_branch1"),
        ((6144, 256, 1, 1), (TRAIN,), "bn4[abcdef]_branch2a, bn4[abcdef]_branch2b"),
        ((6144, 1024, 0, 1), (TRAIN,), "bn4[abcdef]_branch2c, bn4a_branch1"),
        ((24576, 128, 1, 1), (TRAIN,), "bn3[abcd]_branch2a, bn3[abcd]_branch2b"),
        ((24576, 512, 0, 1), (TRAIN,), "bn3[abcd]_branch2c, bn3a_branch1"),
        ((98304, 64, 1, 1), (TRAIN,), "bn2[abc]_branch2a, bn2[abc]_branch2b"),
        ((98304, 256, 0, 1), (TRAIN,), "bn2[abc]_branch2c, bn2a_branch1"),
        ((393216, 64, 1, 1), (TRAIN,), "bn_conv1"),
    ],
    "myolo_bn_apply_act": [
        ((1536, 512, 1), BOTH, "bn5[abc]_branch2a, bn5[abc]_branch2b"),
        ((6144, 256, 1), BOTH, "bn4[abcdef]_branch2a, bn4[abcdef]_branch2b"),
        ((24576, 128, 1), BOTH, "bn3[abcd]_branch2a, bn3[abcd]_branch2b"),
        ((98304, 64, 1), BOTH, "bn2[abc]_branch2a, bn2[abc]_branch2b"),
    ],
    "myolo_bn_frozen_coeffs_batched": [
        ((53,), (INFER,), "every trunk BatchNorm"),
    ],
    "myolo_bn_stats": [
        ((1536, 512), (TRAIN,), "bn5[abc]_branch2a, bn5[abc]_branch2b"),
        ((1536, 2048), (TRAIN,), "bn5[abc]_branch2c, bn5a_branch1"),
        ((6144, 256), (TRAIN,), "bn4[abcdef]_branch2a, bn4[abcdef]_branch2b"),
        ((6144, 1024), (TRAIN,), "bn4[abcdef]_branch2c, bn4a_branch1"),
        ((24576, 128), (TRAIN,), "bn3[abcd]_branch2a, bn3[abcd]_branch2b"),
        ((24576, 512), (TRAIN,), "bn3[abcd]_branch2c, bn3a_branch1"),
        ((98304, 64), (TRAIN,), "bn2[abc]_branch2a, bn2[abc]_branch2b"),
        ((98304, 256), (TRAIN,), "bn2[abc]_branch2c, bn2a_branch1"),
    ],
    "myolo_colsum": [
        ((1536, 258), (TRAIN,), "conv_23/bias"),
        ((1536, 512), (TRAIN,), "res5[abc]_branch2a/bias, res5[abc]_branch2b/bias"),
        ((1536, 2048), (TRAIN,), "res5[abc]_branch2c/bias, res5a_branch1/bias"),
        ((6144, 256), (TRAIN,), "res4[abcdef]_branch2a/bias, res4[abcdef]_branch2b/bias"),
        ((6144, 1024), (TRAIN,), "res4[abcdef]_branch2c/bias, res4a_branch1/bias"),
        ((24576, 128), (TRAIN,), "res3[abcd]_branch2a/bias, res3[abcd]_branch2b/bias"),
        ((24576, 256), (TRAIN,), "feature_map/bias"),
        ((24576, 512), (TRAIN,), "res3[abcd]_branch2c/bias, res3a_branch1/bias"),
        ((98304, 64), (TRAIN,), "res2[abc]_branch2a/bias, res2[abc]_branch2b/bias"),
        ((98304, 256), (TRAIN,), "res2[abc]_branch2c/bias, res2a_branch1/bias"),
    ],
    "myolo_conv3x3_bwd_data": [
        ((6, 16, 16, 512, 512), (TRAIN,), "res5[abc]_branch2b"),
        ((6, 32, 32, 256, 256), (TRAIN,), "res4[abcdef]_branch2b"),
    ],
    "myolo_conv3x3_bwd_weight": [
        ((6, 16, 16, 512, 512), (TRAIN,), "res5[abc]_branch2b"),
        ((6, 32, 32, 256, 256), (TRAIN,), "res4[abcdef]_branch2b"),
    ],
    "myolo_conv3x3_fwd": [
        ((6, 16, 16, 512, 512), BOTH, "res5[abc]_branch2b"),
        ((6, 32, 32, 256, 256), BOTH, "res4[abcdef]_branch2b"),
    ],
    "myolo_conv3x3_wino_bwd_data": [
        ((6, 64, 64, 128, 128), (TRAIN,), "res3[abcd]_branch2b"),
        ((6, 64, 64, 512, 256), (TRAIN,), "feature_map"),
        ((6, 128, 128, 64, 64), (TRAIN,), "res2[abc]_branch2b"),
    ],
    "myolo_conv3x3_wino_bwd_weight": [
        ((6, 64, 64, 128, 128), (TRAIN,), "res3[abcd]_branch2b"),
        ((6, 64, 64, 512, 256), (TRAIN,), "feature_map"),
        ((6, 128, 128, 64, 64), (TRAIN,), "res2[abc]_branch2b"),
    ],
    "myolo_conv7x7s2_c3_affine_act_fwd": [
        ((1, 6, 512, 512, 64), (INFER,), "conv1 + frozen bn_conv1 + ReLU"),
    ],
    "myolo_conv7x7s2_c3_bnstats_fwd": [
        ((6, 512, 512, 64), (TRAIN,), "conv1 + bn_conv1's statistics"),
    ],
    "myolo_conv7x7s2_c3_bwd_weight": [
        ((6, 512, 512, 64), (TRAIN,), "conv1"),
    ],
    "myolo_gather_s2": [
        ((6, 32, 32, 1024), BOTH, "res5a's input"),
        ((6, 64, 64, 512), BOTH, "res4a's input"),
        ((6, 128, 128, 256), BOTH, "res3a's input"),
    ],
    "myolo_maxpool3x3s2_bwd": [
        ((6, 256, 256, 64), (TRAIN,), "pool1"),
    ],
    "myolo_maxpool3x3s2_fwd": [
        ((0, 6, 256, 256, 64), (INFER,), "pool1"),
        ((1, 6, 256, 256, 64), (TRAIN,), "pool1 (bn_conv1 + ReLU on its load)"),
    ],
    "myolo_pwconv1x1_bwd_data": [
        ((1536, 512, 2048), (TRAIN,), "res5[abc]_branch2c"),
        ((1536, 1024, 512), (TRAIN,), "res5a_branch2a"),
        ((1536, 1024, 2048), (TRAIN,), "res5a_branch1"),
        ((1536, 2048, 258), (TRAIN,), "conv_23"),
        ((1536, 2048, 512), (TRAIN,), "res5[bc]_branch2a"),
        ((6144, 256, 1024), (TRAIN,), "res4[abcdef]_branch2c"),
        ((6144, 512, 256), (TRAIN,), "res4a_branch2a"),
        ((6144, 512, 1024), (TRAIN,), "res4a_branch1"),
        ((6144, 1024, 256), (TRAIN,), "res4[bcdef]_branch2a"),
        ((24576, 128, 512), (TRAIN,), "res3[abcd]_branch2c"),
        ((24576, 256, 128), (TRAIN,), "res3a_branch2a"),
        ((24576, 256, 512), (TRAIN,), "res3a_branch1"),
        ((24576, 512, 128), (TRAIN,), "res3[bcd]_branch2a"),
        ((98304, 64, 64), (TRAIN,), "res2a_branch2a"),
        ((98304, 64, 256), (TRAIN,), "res2[abc]_branch2c, res2a_branch1"),
        ((98304, 256, 64), (TRAIN,), "res2[bc]_branch2a"),
    ],
    "myolo_pwconv1x1_bwd_weight": [
        ((1536, 512, 2048), (TRAIN,), "res5[abc]_branch2c"),
        ((1536, 1024, 512), (TRAIN,), "res5a_branch2a"),
        ((1536, 1024, 2048), (TRAIN,), "res5a_branch1"),
        ((1536, 2048, 258), (TRAIN,), "conv_23"),
        ((1536, 2048, 512), (TRAIN,), "res5[bc]_branch2a"),
        ((6144, 256, 1024), (TRAIN,), "res4[abcdef]_branch2c"),
        ((6144, 512, 256), (TRAIN,), "res4a_branch2a"),
        ((6144, 512, 1024), (TRAIN,), "res4a_branch1"),
        ((6144, 1024, 256), (TRAIN,), "res4[bcdef]_branch2a"),
        ((24576, 128, 512), (TRAIN,), "res3[abcd]_branch2c"),
        ((24576, 256, 128), (TRAIN,), "res3a_branch2a"),
        ((24576, 256, 512), (TRAIN,), "res3a_branch1"),
        ((24576, 512, 128), (TRAIN,), "res3[bcd]_branch2a"),
        ((98304, 64, 64), (TRAIN,), "res2a_branch2a"),
        ((98304, 64, 256), (TRAIN,), "res2[abc]_branch2c, res2a_branch1"),
        ((98304, 256, 64), (TRAIN,), "res2[bc]_branch2a"),
    ],
    "myolo_pwconv1x1_fwd": [
        ((1536, 512, 2048), BOTH, "res5[abc]_branch2c"),
        ((1536, 1024, 512), BOTH, "res5a_branch2a"),
        ((1536, 1024, 2048), BOTH, "res5a_branch1"),
        ((1536, 2048, 258), BOTH, "conv_23"),
        ((1536, 2048, 512), BOTH, "res5[bc]_branch2a"),
        ((6144, 256, 1024), BOTH, "res4[abcdef]_branch2c"),
        ((6144, 512, 256), BOTH, "res4a_branch2a"),
        ((6144, 512, 1024), BOTH, "res4a_branch1"),
        ((6144, 1024, 256), BOTH, "res4[bcdef]_branch2a"),
        ((24576, 128, 512), BOTH, "res3[abcd]_branch2c"),
        ((24576, 256, 128), BOTH, "res3a_branch2a"),
        ((24576, 256, 512), BOTH, "res3a_branch1"),
        ((24576, 512, 128), BOTH, "res3[bcd]_branch2a"),
        ((98304, 64, 64), BOTH, "res2a_branch2a"),
        ((98304, 64, 256), BOTH, "res2[abc]_branch2c, res2a_branch1"),
        ((98304, 256, 64), BOTH, "res2[bc]_branch2a"),
    ],
    "myolo_residual_bwd": [
        ((3145728,), (TRAIN,), "res5[abc]"),
        ((6291456,), (TRAIN,), "res4[abcdef]"),
        ((12582912,), (TRAIN,), "res3[abcd]"),
        ((25165824,), (TRAIN,), "res2[abc]"),
    ],
    "myolo_residual_fwd": [
        ((1536, 2048), BOTH, "res5[abc]"),
        ((6144, 1024), BOTH, "res4[abcdef]"),
        ((24576, 512), BOTH, "res3[abcd]"),
        ((98304, 256), BOTH, "res2[abc]"),
    ],
    "myolo_scatter_s2": [
        ((6, 32, 32, 1024), (TRAIN,), "res5a's input"),
        ((6, 64, 64, 512), (TRAIN,), "res4a's input"),
        ((6, 128, 128, 256), (TRAIN,), "res3a's input"),
    ],
    "myolo_wino_input_transform": [
        ((6, 64, 64, 128), BOTH, "res3[abcd]_branch2b"),
        ((6, 64, 64, 512), BOTH, "feature_map"),
        ((6, 128, 128, 64), BOTH, "res2[abc]_branch2b"),
    ],
    "myolo_wino_multiply_w": [
        ((6, 64, 64, 128, 128), BOTH, "res3[abcd]_branch2b"),
        ((6, 64, 64, 512, 256), BOTH, "feature_map"),
        ((6, 128, 128, 64, 64), BOTH, "res2[abc]_branch2b"),
    ],
    "myolo_wino_output_transform": [
        ((6, 64, 64, 128, 0), BOTH, "res3[abcd]_branch2b"),
        ((6, 64, 64, 256, 0), BOTH, "feature_map"),
        ((6, 128, 128, 64, 0), BOTH, "res2[abc]_branch2b"),
    ],
}


def rows(phase=None):
    """[(entry, integer arguments)] of the table (of one phase, or of both)"""
    return [(e, a) for e, rr in LAUNCHES.items() for a, ph, _ in rr if phase is None or phase in ph]


def int_args(name, args):
    """the integer (int / int64) arguments of a C-ABI call, in signature order (pointers, sizes, floats and the stream left out)"""
    from myolo import _ext as X
    return tuple(int(v) for t, v in zip(X.SIGS[name], args) if t in (X.I, X.L))


@contextlib.contextmanager
def recording(monkeypatch, net, seen):
    """record (entry, integer arguments) of every library call made inside Net.trunk_fwd / yolo_head_bwd / trunk_bwd into the set `seen`"""
    from myolo import _ext as X
    depth = [0]
    real = X.call

    def call(name, *args):
        if depth[0] and name in X.SIGS:
            seen.add((name, int_args(name, args)))
        return real(name, *args)

    def scoped(fn):
        def wrap(*a, **kw):
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return wrap
    with monkeypatch.context() as mp:
        mp.setattr(X, "call", call)
        for m in ("trunk_fwd", "yolo_head_bwd", "trunk_bwd"):
            mp.setattr(net, m, scoped(getattr(net, m)))
        yield seen
