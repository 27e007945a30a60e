"""fwd1x1_stream_kernel: the channel-expanding 1x1 / stride-1 forward convolutions (Cin = 64 / 128 into a multiple of
128 channels) streamed with the weights in registers, behind rn_conv_fwd_x (rn_set_tuning 29 = 1: the 224-row tiles,
2: every form at 32 channels per wave, 3: every form at the default width; rn_conv_fwd_streamed).

* per kernel, against the tile run first: y bit for bit, the pivot plane exactly, the partials' per-channel totals
  within fp32 summation-order rounding, rn_bn_fwd_train_part on the partials against the oracle's BatchNorm over the
  stored y, y against the oracle's convolution within one rounding per element (gpu_util.rounding_excess);
* the same call twice: bit for bit (how missing MFMA wait states showed in the streamed data gradient);
* rn_conv_fwd_streamed's rule, on the host.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ops
from rn import lib as L
from gpu_util import BF16, F32, bf16_round, bnrelu_operand, conv_desc, from_nhwc, p, rel_err, rounding_excess, stream, to_nhwc

TOL_BF16 = 1.5e-2  # the bf16 bar of the kernel tests
KEY = 29           # rn_set_tuning: 0 default, 1 the tiles, 2 / 3 every form streamed, at 32 channels per wave / the default width

CASES = [
    (3, 64, 14, 14, 256, 1, 1, 0),   # Cin 64 -> 256; M = 588 = two full blocks + a ragged 140-row block
    (2, 128, 9, 11, 512, 1, 1, 0),   # Cin 128 -> 512; fewer rows than one block
    (5, 64, 7, 9, 128, 1, 1, 0),     # one 128-channel group: 32 channels per wave forced by the shape
]
MODES = ["plain", "stats", "stats_res", "xf_stats", "xf_stats_res"]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    n, c, h, w, k = case[:5]
    rng = np.random.default_rng(61)
    x = bf16_round(rng.standard_normal((n, c, h, w)) * 1.5 + 0.3)
    wt = bf16_round(rng.standard_normal((k, c, 1, 1)) / np.sqrt(c))
    res = bf16_round(rng.standard_normal((n, k, h, w)) + 3.0)  # offset mean: the pivots matter
    sc = rng.uniform(0.5, 1.5, c)
    sh = rng.standard_normal(c) * 0.5
    sh[0], sh[1] = -1.0, 0.7  # clamped inputs; a positive shift (an unmasked padded row would show in the statistics)
    return x, wt, res, sc.astype(np.float32).astype(np.float64), sh.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _oracle(case, xf, add):
    """fp64 convolution of the input -- transformed as the kernel stages it, bf16(max(fmaf(x, sc, sh), 0)): the fma
    rounds to float32 first, which can move a value across a bf16 tie -- + the residual; and the same sum over the
    terms' magnitudes, for the per-element rounding bar."""
    x, wt, res, sc, sh = _inputs(case)
    xa = bnrelu_operand(x, sc, sh) if xf else x
    ref = ops.conv2d_fwd(xa, wt, (1, 1), (0, 0)) + (res if add else 0)
    sabs = ops.conv2d_fwd(np.abs(xa), np.abs(wt), (1, 1), (0, 0)) + (np.abs(res) if add else 0)
    return ref, sabs


class _Dev:
    def __init__(self, case, gpu):
        n, c, h, w, k = case[:5]
        x, wt, res, sc, sh = _inputs(case)
        self.lib = L.load()
        self.d = d = conv_desc(BF16, n, c, h, w, k, 1, 1, 1, 0)
        self.M = n * h * w
        self.nblk = int(self.lib.rn_conv_bnstats_blocks(C.byref(d)))
        self.xd, self.rd = to_nhwc(x, BF16, gpu), to_nhwc(res, BF16, gpu)
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
        self.sc, self.sh = f(sc), f(sh)
        self.wk = torch.zeros(k * d.c, dtype=torch.bfloat16, device=gpu)
        master = torch.from_numpy(np.ascontiguousarray(wt.transpose(0, 2, 3, 1), dtype=np.float32)).reshape(-1).to(gpu)
        L.call("rn_conv_weight_pack", C.byref(d), p(master), p(self.wk), None, stream())
        self.gpu = gpu

    def run(self, mode):
        """One rn_conv_fwd_x into NaN-filled outputs: (y, part or None)."""
        d, k = self.d, self.d.k
        y = torch.full((self.d.n, self.d.h, self.d.w, k), float("nan"), dtype=torch.bfloat16, device=self.gpu)
        part = torch.full((self.nblk * 3 * k,), float("nan"), dtype=torch.float32, device=self.gpu) \
            if "stats" in mode else None
        xf, add = mode.startswith("xf"), mode.endswith("res")
        L.call("rn_conv_fwd_x", C.byref(d), p(self.xd), p(self.wk), p(y), BF16, p(self.rd) if add else None, None,
               p(self.sc) if xf else None, p(self.sh) if xf else None, p(part), stream())
        torch.cuda.synchronize()
        return y, part


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_fwd1x1_stream(gpu, case, mode):
    n, c, h, w, k = case[:5]
    dev = _Dev(case, gpu)
    lib, d, M, nblk = dev.lib, dev.d, dev.M, dev.nblk
    assert lib.rn_conv_bn_part_rows(C.byref(d), 0) == 224 and nblk == -(-M // 224)
    try:
        L.call("rn_set_tuning", KEY, 1)
        assert lib.rn_conv_fwd_streamed(C.byref(d)) == 0
        y0, p0 = dev.run(mode)  # the tile
        streamed = []
        for val in (0, 2, 3):  # (3: the plain Cin = 128 form too at 64 channels per wave, on its tile by default)
            L.call("rn_set_tuning", KEY, val)
            if val >= 2:
                assert lib.rn_conv_fwd_streamed(C.byref(d)) == 1
            assert lib.rn_conv_bn_part_rows(C.byref(d), 0) == 224 and lib.rn_conv_bnstats_blocks(C.byref(d)) == nblk
            streamed.append(dev.run(mode))
    finally:
        L.call("rn_set_tuning", KEY, 0)
    y_ref, y_sabs = _oracle(case, mode.startswith("xf"), mode.endswith("res"))
    assert not torch.isnan(y0).any()
    assert rel_err(from_nhwc(y0, k), y_ref) < TOL_BF16
    # one rounding per element (the streamed outputs below are y0's bits)
    assert rounding_excess(from_nhwc(y0, k), y_ref, y_sabs, c + mode.endswith("res"), BF16).max() <= 1.0
    u = 2.0 ** -24  # fp32 unit round-off
    for y1, p1 in streamed:
        assert not torch.isnan(y1).any()
        assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
        if p1 is None:
            continue
        assert not torch.isnan(p1).any()
        a0, a1 = p0.view(nblk, 3, k).double(), p1.view(nblk, 3, k).double()
        assert torch.equal(a0[:, 2], a1[:, 2])  # the pivot plane
        # the two kernels add the same 224 (or fewer) terms d = v - pivot per block and channel in different orders:
        # each fp32 sum is within (n - 1) u sum|d| of the exact one, + u |d| where v - pivot itself rounds (S2: the
        # fma rounds once per term, d^2 carries d's rounding twice: (n + 2) u sum d^2); n <= 224, twice for two sums
        v = y0.double().view(M, k)
        rows = torch.arange(M, device=gpu) // 224
        dv = v - a0[:, 2][rows]
        sabs = dv.abs().sum(0)
        ssq = (dv * dv).sum(0)
        t0, t1 = a0.sum(0), a1.sum(0)  # merged over the blocks, in float64
        assert bool(((t0[0] - t1[0]).abs() <= 2 * 224 * u * sabs).all())
        assert bool(((t0[1] - t1[1]).abs() <= 2 * 226 * u * ssq).all())
        # (and both describe the stored values: the exact sums, in float64)
        assert bool(((t1[0] - dv.sum(0)).abs() <= 224 * u * sabs).all())
        assert bool(((t1[1] - ssq).abs() <= 226 * u * ssq).all())
        # rn_bn_fwd_train_part on the partials == a BatchNorm over the stored y (test_conv_bnstats_epilogue's bars)
        conv_out = from_nhwc(y1, k)
        gamma = np.random.default_rng(62).uniform(0.5, 1.5, k)
        beta = np.random.default_rng(63).standard_normal(k) * 0.1
        _, cache = ops.bn_train_fwd(conv_out, gamma, beta, 1e-5, False)
        mm_ref, mv_ref = ops.bn_moving_update(np.zeros(k), np.ones(k), cache[3], cache[4], 0.9)
        bd = L.BNDesc(dtype=BF16, m=M, c=k, c_real=k, eps=1e-5, momentum=0.9, fix_gamma=0, relu=1)
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
        g_d, b_d, mm, mv = f(gamma), f(beta), f(np.zeros(k)), f(np.ones(k))
        sm, si, sc, sh = [torch.zeros(k, dtype=torch.float32, device=gpu) for _ in range(4)]
        yb = torch.zeros_like(y1)
        ws = torch.zeros(lib.rn_bn_workspace_bytes(C.byref(bd)) // 4 + 16, dtype=torch.float32, device=gpu)
        L.call("rn_bn_fwd_train_part", C.byref(bd), p(p1), nblk, 224, k, p(y1), p(yb), p(g_d), p(b_d), p(mm), p(mv),
               p(sm), p(si), p(sc), p(sh), p(ws), stream())
        torch.cuda.synchronize()
        assert rel_err(sm.cpu().numpy(), cache[3]) < 1e-6
        assert rel_err(mv.cpu().numpy(), mv_ref) < 1e-5
        assert rel_err(mm.cpu().numpy(), mm_ref) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("width", [0, 2], ids=["cpw64", "cpw32"])
@pytest.mark.parametrize("case", CASES)
def test_fwd1x1_stream_repeat(gpu, case, width):
    """The same call twice into NaN-filled outputs: identical bits (every flag on: transform, residual, statistics)."""
    dev = _Dev(case, gpu)
    try:
        L.call("rn_set_tuning", KEY, width)
        (ya, pa), (yb, pb) = dev.run("xf_stats_res"), dev.run("xf_stats_res")
    finally:
        L.call("rn_set_tuning", KEY, 0)
    assert not torch.isnan(ya).any() and not torch.isnan(pa).any()
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))


# ---------------------------------------------------------------------------------------------- host
def test_fwd_streamed_query():
    """rn_conv_fwd_streamed: 1 for the default-on classes (ResNet-50's stage-1 conv3 / shortcut and stage-2 conv3 at
    batch 256); 0 with rn_set_tuning 29 = 1 and under rn_set_tuning 9 = 1 (256-row statistics blocks); 0 for Cin = 256,
    stride 2, 3x3, grouped, f32 and padded k; 0 once n h w max(k, c) 2 bytes pass 2^31 - 1."""
    lib = L.load()
    q = lambda d: int(lib.rn_conv_fwd_streamed(C.byref(d)))
    mk = lambda n, c, h, w, k, r=1, stride=1, pad=0, dtype=BF16, groups=1: conv_desc(dtype, n, c, h, w, k, r, r, stride,
                                                                                  pad, groups=groups)
    on = [mk(256, 64, 56, 56, 256), mk(256, 128, 28, 28, 512)]
    try:
        for d in on:
            assert q(d) == 1
            assert lib.rn_conv_bn_part_rows(C.byref(d), 0) == 224
        L.call("rn_set_tuning", KEY, 1)
        assert [q(d) for d in on] == [0, 0]
        assert lib.rn_conv_bn_part_rows(C.byref(on[0]), 0) == 224
        L.call("rn_set_tuning", KEY, 0)
        L.call("rn_set_tuning", 9, 1)
        assert [q(d) for d in on] == [0, 0]
    finally:
        L.call("rn_set_tuning", KEY, 0)
        L.call("rn_set_tuning", 9, 0)
    assert q(mk(256, 256, 14, 14, 1024)) == 0            # Cin = 256 (stage 3: the tiles)
    assert q(mk(256, 128, 28, 28, 512, stride=2)) == 0
    assert q(mk(256, 64, 56, 56, 256, r=3, pad=1)) == 0
    assert q(mk(256, 128, 28, 28, 256, groups=2)) == 0
    assert q(mk(256, 64, 56, 56, 256, dtype=F32)) == 0
    dp = L.ConvDesc(dtype=BF16, n=4, h=8, w=8, c=64, c_real=64, k=128, k_pad=136, r=1, s=1, stride_h=1, stride_w=1,
                    pad_h=0, pad_w=0, groups=1)
    L.call("rn_conv_desc_init", C.byref(dp))
    assert q(dp) == 0                                    # padded k
    assert q(mk(255, 128, 64, 64, 1024)) == 1            # 2^31 - 2^23 bytes of y
    assert q(mk(256, 128, 64, 64, 1024)) == 0            # 2^31 bytes
    assert q(mk(512, 128, 64, 64, 1024)) == 0            # 2^32: past an int's wrap-around
