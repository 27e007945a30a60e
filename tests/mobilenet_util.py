"""MobileNet-v1 restated on the numpy oracle's Graph (symbol/mobilenet.py:38-144), for the MobileNet tests.

Independent of rn/graphs.py: the layer table below is written out per layer as the reference's
mobilenet() does, not generated from graphs._MOBILENET_LAYERS."""
from oracle import net as onet

# conv_N_dw / conv_N for N = 2 .. 14: (depthwise channels, stride, pointwise filters), in units of
# base = int(32 * alpha)
LAYERS = [
    (1, 1, 2),    # conv_2   112 -> 112
    (2, 2, 4),    # conv_3   112 -> 56
    (4, 1, 4),    # conv_4
    (4, 2, 8),    # conv_5   56 -> 28
    (8, 1, 8),    # conv_6
    (8, 2, 16),   # conv_7   28 -> 14
    (16, 1, 16),  # conv_8
    (16, 1, 16),  # conv_9
    (16, 1, 16),  # conv_10
    (16, 1, 16),  # conv_11
    (16, 1, 16),  # conv_12
    (16, 2, 32),  # conv_13  14 -> 7
    (32, 1, 32),  # conv_14
]
DW_NAMES = ["conv_%d_dw_conv2d" % n for n in range(2, 15)]


def _unit(g, x, name, k, kernel=(1, 1), stride=(1, 1), pad=(0, 0), groups=1):
    x = g.conv(name + "_conv2d", x, k, kernel, stride, pad, groups=groups)
    x = g.bn(name + "_batchnorm", x, eps=1e-3, fix_gamma=True)  # MXNet's BatchNorm defaults
    return g.relu(name + "_relu", x)


def oracle_mobilenet(num_classes, alpha=1.0):
    """The oracle graph; the final (resolution / 32)^2 window over a (resolution / 32)^2 map is a global
    average pool."""
    base = int(32 * alpha)
    g = onet.Graph()
    g.chan["data"] = 3
    x = _unit(g, "data", "conv_1", base, (3, 3), (2, 2), (1, 1))
    for i, (dw, stride, pw) in enumerate(LAYERS):
        c = base * dw
        x = _unit(g, x, "conv_%d_dw" % (i + 2), c, (3, 3), (stride, stride), (1, 1), groups=c)
        x = _unit(g, x, "conv_%d" % (i + 2), base * pw)
    x = g.gap("global_pool", x)
    x = g.fc("fc", x, num_classes)
    g.softmax("softmax", x)
    return g
