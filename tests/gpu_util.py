"""Helpers for GPU parity tests: NCHW numpy <-> NHWC device tensors, direct C-ABI calls."""
import contextlib
import ctypes as C

import numpy as np
import torch

from rn import lib as L

BF16, F32 = L.RN_BF16, L.RN_F32
TUNE_DEFAULTS = {10: 512, 18: 55, 21: 50}  # every other rn_set_tuning key defaults to 0


@contextlib.contextmanager
def tuning(keys):
    """rn_set_tuning key: value for the block, every key back at its default after."""
    try:
        for key, val in keys.items():
            L.call("rn_set_tuning", key, val)
        yield
    finally:
        for key in keys:
            L.call("rn_set_tuning", key, TUNE_DEFAULTS.get(key, 0))


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def bf16_round(a):
    """Round an fp64/fp32 array to bf16 and back (RNE), as the device copy sees it."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32)
    return t.numpy().astype(np.float64)


def bnrelu_operand(x, sc, sh):
    """What a kernel with the BatchNorm+ReLU applied on load stages: bf16(max(fmaf(x, sc, sh), 0)) -- the fused
    multiply-add as a float64 multiply-add (a bf16 times an fp32 value is exact there), rounded to float32 and then
    to bf16. x: NCHW bf16 values, sc / sh: fp32 values per channel; all as float64 arrays."""
    v = (x * sc[None, :, None, None] + sh[None, :, None, None]).astype(np.float32)
    return bf16_round(np.maximum(v, np.float32(0)))


def pad8(c):
    return (c + 7) // 8 * 8


def to_nhwc(x, dtype, dev, cpad=None):
    n, c, h, w = x.shape
    cpad = cpad or pad8(c)
    t = torch.zeros((n, h, w, cpad), dtype=torch.float32)
    t[..., :c] = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1), dtype=np.float32))
    return t.to(tdt(dtype)).to(dev).contiguous()


def from_nhwc(t, c):
    a = t.float().cpu().numpy()
    return a[..., :c].transpose(0, 3, 1, 2).astype(np.float64)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def conv_desc(dtype, n, c, h, w, k, r, s, stride, pad, c_real=None, groups=1):
    d = L.ConvDesc(dtype=dtype, n=n, h=h, w=w, c=pad8(c) if c_real is None else c, c_real=c if c_real is None else c_real,
                   k=k, k_pad=pad8(k), r=r, s=s, stride_h=stride, stride_w=stride, pad_h=pad, pad_w=pad, groups=groups)
    L.call("rn_conv_desc_init", C.byref(d))
    return d


def rounding_excess(got, ref, sabs, nterms, out_dtype):
    """|got - ref| / allowed per element, for a sum of `nterms` products of bf16 values (exact in fp32) and added
    operands accumulated in fp32 and stored once: <= 1 everywhere for any summation order.

    ref: the exact (fp64) sums; sabs: the same sums over the terms' magnitudes (the convolution of |x| and |w|,
    + |add_src| + |bias|); nterms: r s c / groups, + 1 per added operand (an upper bound serves).
      delta   = (nterms + 2) 2^-24 sabs   -- nterms - 1 fp32 additions in any order, each within 2^-24 of its
                                             partial sum, whose magnitude sabs bounds (+ second-order slack)
      allowed = delta + 2^(floor(log2(|ref| + delta)) - 8)    -- half a bf16 ulp at the accumulator's magnitude
    (- 24 for an fp32 output). NaN in got gives inf."""
    got, ref, sabs = (np.asarray(a, dtype=np.float64) for a in (got, ref, sabs))
    delta = (nterms + 2) * 2.0 ** -24 * sabs
    mag = np.abs(ref) + delta
    _, e = np.frexp(mag)  # mag = m 2^e, 0.5 <= m < 1: floor(log2 mag) = e - 1
    half_ulp = np.where(mag > 0, np.ldexp(1.0, e - 1 - (8 if out_dtype == BF16 else 24)), 0.0)
    allowed = delta + half_ulp
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / allowed)  # (an exact zero where nothing is allowed passes)
    return np.where(np.isnan(ratio), np.inf, ratio)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
