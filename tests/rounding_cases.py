"""Shapes, data and fp64 oracles of the per-element rounding bar (gpu_util.rounding_excess), shared by
test_rounding_bar_cpu.py (the proof that the bar separates one rounding from a truncated store and from a partial
sum kept in bf16) and test_conv_rounding_gpu.py (the kernels under that bar).

A case is (n, c, h, w, k, r, stride, pad[, groups]). Two data regimes:
  gauss: the kernel tests' recipe -- x, dy, add_src ~ N(0, 1), w ~ N(0, 1) / sqrt(r s c / groups), all rounded to bf16;
  exact: x, dy in {-1, 0, 1} (a quarter zeros), w in {-1, 0, 1}, add_src / bias small integers: every partial sum
         is an integer far below 2^24, and a result of magnitude <= 256 is a bf16 value, so a correct kernel
         returns the oracle's bits in any summation order. Long reductions thin w's nonzeros to keep that cap.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from gpu_util import bnrelu_operand  # noqa: F401  (the on-load BatchNorm+ReLU operand, for the GPU file)
from oracle import ops
from test_depthwise_gpu import CASES as _DW_CASES
from test_fwd_stream_gpu import CASES as FWD_STREAM_CASES
from test_kernels_gpu import BIG_CASES, CONV_CASES, GCONV_CASES, GDIRECT_CASES

MAX_TERMS = 2500   # the bar is proven (test_rounding_bar_cpu.py) up to here; longer reductions: the exact regime only
EXACT_CAP = 256    # every integer up to here is a bf16 value

W4_CASE = (2, 256, 14, 14, 128, 1, 1, 0)    # 1x1 / pad 0, > 64 columns both ways: the 4-wave 224x128 tile
BAND_CASES = [  # test_conv3x3_band's
    (3, 64, 56, 56, 64, 3, 1, 1),
    (5, 64, 9, 13, 64, 3, 1, 1),
    (1, 64, 7, 7, 64, 3, 1, 1),
    (2, 64, 20, 56, 64, 3, 1, 1),
]
BAND_PERSIST_N = 40
STEM_GEOMS = [(3, 50, 38), (1, 31, 17)]     # test_stem_band's, without the 224 x 224 one
DGRAD_STREAM_CASES = [  # test_dgrad1x1_stream's
    (3, 256, 14, 14, 64, 1, 1, 0),
    (2, 512, 9, 11, 128, 1, 1, 0),
    (5, 128, 7, 9, 64, 1, 1, 0),
]
GROUPED_DIRECT_CASES = [  # where the direct v_dot2 kernels run: GCONV_CASES' and test_grouped_conv_direct's
    GCONV_CASES[0],                       # 4 per group, stride 1
    GCONV_CASES[1],                       # 8 per group, stride 2
    (3, 128, 15, 13, 128, 3, 1, 1, 32),   # ragged rows
    (2, 128, 12, 12, 128, 3, 2, 1, 32),   # 4 per group, stride 2: the transposed stride-2 data gradient
    (2, 128, 11, 13, 128, 3, 2, 1, 32),   # stride 2, odd input sizes
]
DEPTHWISE_ALL = [(n, c, h, w, c, 3, st, 1, c) for n, c, h, w, st in _DW_CASES]
DEPTHWISE_CASES = [c for c in DEPTHWISE_ALL if c[2] < 56]   # (test_depthwise_gpu holds the 56 x 56 one to the bar)
FC_CASES = [(37, 256, 1, 1, 1000, 1, 1, 0), (37, 2048, 1, 1, 1000, 1, 1, 0)]


def full(case):
    return tuple(case) + (1,) * (9 - len(case))


def stem_case(geom):
    n, h, w = geom
    return (n, 3, h, w, 64, 7, 2, 3)


def nterms(case, direction):
    """Products per output element: r s c / groups forward, r s k / groups for the data gradient (an upper bound
    at stride 2, where a pixel sees a quarter to all of the taps)."""
    n, c, h, w, k, r, st, pd, g = full(case)
    return r * r * (c if direction == "fwd" else k) // g


def all_shapes():
    """Every (case, direction, fp32 output?) the GPU file runs, once."""
    seen = {}
    def add(cases, dirs=("fwd", "dgrad"), f32=False):
        for c in cases:
            for d in dirs:
                seen.setdefault((full(c), d, f32), None)
    add(CONV_CASES)
    add(CONV_CASES, f32=True)
    add(BIG_CASES + [W4_CASE] + BAND_CASES + [(BAND_PERSIST_N,) + c[1:] for c in BAND_CASES] + GCONV_CASES +
        GROUPED_DIRECT_CASES + GDIRECT_CASES + DEPTHWISE_ALL)
    add([stem_case(g) for g in STEM_GEOMS] + list(FWD_STREAM_CASES), dirs=("fwd",))
    add(DGRAD_STREAM_CASES, dirs=("dgrad",))
    add(FC_CASES, dirs=("fwd",), f32=True)
    return list(seen)


# ---------------------------------------------------------------------------------------------- oracles (fp64)
def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))  # (a copy: the cached arrays are read-only)


def conv_fwd64(x, w, st, pd, g=1):
    return F.conv2d(_t(x), _t(w), stride=st, padding=pd, groups=g).numpy()


def conv_dgrad64(dy, w, hw, st, pd, g=1):
    """dx of conv_fwd64 for an h x w input."""
    r = w.shape[2]
    op = tuple(v - ((o - 1) * st - 2 * pd + r) for v, o in zip(hw, dy.shape[2:]))
    return F.conv_transpose2d(_t(dy), _t(w), stride=st, padding=pd, output_padding=op, groups=g).numpy()


# ---------------------------------------------------------------------------------------------- data
def _ternary(rng, shape, p_nonzero):
    return rng.choice([-1.0, 0.0, 1.0], size=shape, p=[p_nonzero / 2, 1 - p_nonzero, p_nonzero / 2])


def make_inputs(case, regime):
    n, c, h, w, k, r, st, pd, g = full(case)
    P, Q = ops.conv_out_hw(h, w, r, r, (st, st), (pd, pd))
    rng = np.random.default_rng(97 if regime == "gauss" else 98)
    if regime == "gauss":
        bf = lambda shape, scale=1.0: ops.bf16_round(rng.standard_normal(shape) * scale)
        x, wt = bf((n, c, h, w)), bf((k, c // g, r, r), 1.0 / np.sqrt(c // g * r * r))
        dy, ya, xa = bf((n, k, P, Q)), bf((n, k, P, Q)), bf((n, c, h, w))
        bias = rng.standard_normal(k).astype(np.float32).astype(np.float64)
    else:
        # a sum of T terms, each nonzero with probability 3/4 pw, has variance 3/4 pw T: at most 1500, so that
        # five standard deviations (194) and an added operand stay below 256
        terms = max(nterms(case, "fwd"), nterms(case, "dgrad"))
        pw = min(2.0 / 3.0, 1500.0 / (0.75 * terms))
        x, wt = _ternary(rng, (n, c, h, w), 0.75), _ternary(rng, (k, c // g, r, r), pw)
        dy = _ternary(rng, (n, k, P, Q), 0.75)
        ya, xa = (rng.integers(-3, 4, s).astype(np.float64) for s in ((n, k, P, Q), (n, c, h, w)))
        bias = rng.integers(-3, 4, k).astype(np.float64)
    return dict(x=x, wt=wt, dy=dy, ya=ya, xa=xa, bias=bias, P=P, Q=Q)


@functools.lru_cache(maxsize=6)
def conv_data(case, regime):
    """Inputs and the oracle's results, computed once per case: y / dx the exact sums, y_sabs / dx_sabs the sums of
    the terms' magnitudes (without the added operands)."""
    n, c, h, w, k, r, st, pd, g = full(case)
    D = make_inputs(case, regime)
    D["y"] = conv_fwd64(D["x"], D["wt"], st, pd, g)
    D["dx"] = conv_dgrad64(D["dy"], D["wt"], (h, w), st, pd, g)
    if regime == "gauss":
        aw = np.abs(D["wt"])
        D["y_sabs"] = conv_fwd64(np.abs(D["x"]), aw, st, pd, g)
        D["dx_sabs"] = conv_dgrad64(np.abs(D["dy"]), aw, (h, w), st, pd, g)
    for v in D.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return D
