"""The per-element rounding bar (gpu_util.rounding_excess) separates right from wrong, on the CPU: for every shape
test_conv_rounding_gpu.py holds to it, a simulated correct output (fp32 accumulation, one round-to-nearest-even to
bf16) has no element above 1, and two simulated mistakes each have some: the same accumulation with the store
TRUNCATED to bf16, and the reduction cut in two halves that are each rounded to bf16 before they are added.
The exact regime's cap (every result an integer of magnitude <= 256) is checked for the same shapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rounding_cases as R
from gpu_util import BF16, F32, rounding_excess
from oracle import ops

SHAPES = [s for s in R.all_shapes() if R.nterms(s[0], s[1]) <= R.MAX_TERMS]
_id = lambda s: "%s-%s%s" % ("x".join(map(str, s[0])), s[1], "-f32out" if s[2] else "")


def _conv32(a, wt, case, direction):
    """The convolution (or its data gradient) accumulated in float32."""
    n, c, h, w, k, r, st, pd, g = case
    a, wt = torch.from_numpy(a.astype(np.float32)), torch.from_numpy(wt.astype(np.float32))
    if direction == "fwd":
        return F.conv2d(a, wt, stride=st, padding=pd, groups=g)
    op = tuple(v - ((o - 1) * st - 2 * pd + r) for v, o in zip((h, w), a.shape[2:]))
    return F.conv_transpose2d(a, wt, stride=st, padding=pd, output_padding=op, groups=g)


def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _halves(wt, case, direction):
    """A mask over w's entries: half of each group's reduction (its channels; the taps where a group has one)."""
    n, c, h, w, k, r, st, pd, g = case
    m = np.zeros(wt.shape, dtype=bool)
    if direction == "fwd" and c // g > 1:
        m[:, :c // g // 2] = True
    elif direction == "dgrad" and k // g > 1:
        m[np.arange(k) % (k // g) < k // g // 2] = True
    else:
        m[:, :, :r // 2 + 1 if r > 1 else 1] = True
    return m


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_bar_separates_one_rounding_from_two(shape):
    case, direction, f32out = shape
    D = R.conv_data(case, "gauss")
    src, ref, sabs = (D["x"], D["y"], D["y_sabs"]) if direction == "fwd" else (D["dy"], D["dx"], D["dx_sabs"])
    nt = R.nterms(case, direction)
    acc = _conv32(src, D["wt"], case, direction)
    m = _halves(D["wt"], case, direction)
    assert m.any() and not m.all()
    rb = lambda t: t.to(torch.bfloat16).float()
    h1, h2 = (rb(_conv32(src, D["wt"] * mm, case, direction)) for mm in (m, ~m))
    part = h1 + h2
    if not bool(((h1 != 0) & (h2 != 0)).any()):
        # one term per element (a 2 x 2 image under a stride-2 depthwise data gradient): nothing to keep in bf16
        assert nt == 9 and torch.equal(rb(part), rb(acc))
        part = None
    if f32out:  # the logits: the fp32 accumulator is the output; a bf16 rounding anywhere is the mistake
        outs = dict(correct=acc, truncated=_truncate_bf16(acc), partial=part)
    else:
        outs = dict(correct=rb(acc), truncated=_truncate_bf16(acc), partial=None if part is None else rb(part))
    outs = {k: v for k, v in outs.items() if v is not None}
    ex = {k: rounding_excess(v.numpy(), ref, sabs, nt, F32 if f32out else BF16) for k, v in outs.items()}
    print("bar", _id(shape), "terms", nt, {k: "max %.3g, %.2f%% above 1" % (v.max(), 100.0 * (v > 1).mean())
                                          for k, v in ex.items()})
    assert ex["correct"].max() <= 1.0
    assert ex["truncated"].max() > 1.0
    assert "partial" not in ex or ex["partial"].max() > 1.0


@pytest.mark.parametrize("shape", R.all_shapes(), ids=_id)
def test_exact_regime_stays_below_the_cap(shape):
    """Integers of magnitude <= 256 with the added operands, and data that exercises the kernel: nonzero outputs
    (a stride-2 1x1 data gradient leaves three pixels in four zero), many of which change when one input channel
    is dropped."""
    case, direction, f32out = shape
    n, c, h, w, k, r, st, pd, g = case
    D = R.conv_data(case, "exact")
    ref, add = (D["y"], D["ya"]) if direction == "fwd" else (D["dx"], D["xa"])
    assert np.array_equal(ref, np.round(ref))
    bias = np.abs(D["bias"]).max() if f32out else 0
    assert np.abs(ref).max() + np.abs(add).max() + bias <= R.EXACT_CAP
    assert np.abs(ref).max() >= 1 and (ref != 0).mean() > 0.1
    if direction == "fwd" and c // g > 1:
        x1 = D["x"].copy()
        x1[:, 0] = 0
        changed = (R.conv_fwd64(x1, D["wt"], st, pd, g) != ref)[:, :k // g]  # (the first group's outputs)
        assert changed.mean() > 0.1


def test_bar_edges():
    """Zero sums allow nothing but zero; NaN never passes; a power of two takes its own half ulp; fp32 outputs take
    the fp32 ulp."""
    ref, sabs = np.array([0.0, 0.0, 1.0, 1.0, 3.0]), np.zeros(5)
    got = np.array([0.0, 1e-30, 1.0 + 2.0 ** -8, np.nan, 3.0 + 2.0 ** -7])
    ex = rounding_excess(got, ref, sabs, 9, BF16)
    assert ex[0] == 0 and ex[1] == np.inf and ex[2] == 1.0 and ex[3] == np.inf and ex[4] == 1.0
    assert rounding_excess(np.array([1.0 + 2.0 ** -23]), np.array([1.0]), np.zeros(1), 9, F32)[0] == 2.0
    d = rounding_excess(np.array([1.0]), np.array([1.0 + 11 * 2.0 ** -24 * 4.0]), np.array([4.0]), 9, F32)
    assert d[0] < 1.0  # delta alone covers (nterms + 2) 2^-24 sabs


def test_torch_oracle_is_the_numpy_oracle():
    """conv_fwd64 / conv_dgrad64 (torch, float64) against oracle.ops on a strided, padded, grouped shape."""
    case = (2, 16, 9, 7, 24, 3, 2, 1, 4)
    n, c, h, w, k, r, st, pd, g = case
    D = R.conv_data(case, "gauss")
    y = ops.conv2d_fwd(D["x"], D["wt"], (st, st), (pd, pd), g)
    dx, _ = ops.conv2d_bwd(D["x"], D["wt"], D["dy"], (st, st), (pd, pd), g)
    assert np.abs(D["y"] - y).max() < 1e-13 and np.abs(D["dx"] - dx).max() < 1e-13
    E = R.conv_data(case, "exact")
    assert np.array_equal(E["y"], ops.conv2d_fwd(E["x"], E["wt"], (st, st), (pd, pd), g))
    assert np.array_equal(E["dx"], ops.conv2d_bwd(E["x"], E["wt"], E["dy"], (st, st), (pd, pd), g)[0])


def test_bnrelu_operand_is_the_fused_multiply_add():
    """bnrelu_operand (float64 multiply-add -> float32 -> ReLU -> bf16) differs from rounding the fp64 value
    straight to bf16 only where the float32 rounding crosses a bf16 tie: rarely, and by one bf16 ulp."""
    rng = np.random.default_rng(3)
    x = ops.bf16_round(rng.standard_normal((4, 64, 9, 9)) * 1.5 + 0.3)
    sc = rng.uniform(0.5, 1.5, 64).astype(np.float32).astype(np.float64)
    sh = (rng.standard_normal(64) * 0.5).astype(np.float32).astype(np.float64)
    a = R.bnrelu_operand(x, sc, sh)
    b = ops.bf16_round(np.maximum(x * sc[None, :, None, None] + sh[None, :, None, None], 0))
    assert (a >= 0).all() and (a == 0).any()
    assert np.abs(a - b).max() <= 2.0 ** -7 * np.abs(b).max()
    assert (a != b).mean() < 1e-3
