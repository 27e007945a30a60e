"""fwd1x1_lds_stream_kernel: the 1x1 / stride-1 forward convolutions from Cin = 256 into a multiple of 256 channels
(stage 3's conv3) with the 224-row block of x stationary in LDS and the workgroup sweeping the output channels, behind
rn_conv_fwd_x (rn_set_tuning 30 = 1: the 224-row tiles, 2: the kernel whatever the size; rn_conv_fwd_lds_streamed).

Per case (shape, Kout, form, data), the kernel forced with key 30 = 2 after the host's own answers are asserted:
* y bit for bit the tile's (key 30 = 1), as 16-bit words; the same call twice repeats bit for bit (missing MFMA wait
  states showed exactly so in the streamed data gradient);
* the partials bit for bit those of the 4-wave 224x128 tile (rn_set_tuning 11 = 2 puts these small grids on it), and
  against whatever tile key 30 = 1 runs by default the pivot plane exactly and the totals within the fp32
  summation-order bound of test_fwd_stream_gpu.py;
* y within one rounding per element of the fp64 oracle on Gaussian data (gpu_util.rounding_excess), bit for bit on
  ternary / integer data;
* y and part pre-filled with NaN, 224 sentinel rows behind y (and a sentinel block behind part) untouched;
* shift > 0 on most channels: relu(0 sc + sh) != 0, so a row wrongly kept past a short block shows in y and in the
  statistics.
The host test pins rn_conv_fwd_lds_streamed's rule and that rn_conv_fwd_streamed's answers did not move.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rn import lib as L
from gpu_util import BF16, F32, bnrelu_operand, conv_desc, from_nhwc, p, rounding_excess, stream, to_nhwc
from rounding_cases import conv_fwd64, make_inputs

KEY = 30   # rn_set_tuning: 0 default, 1 the tiles, 2 the kernel for every eligible shape
W4 = 11    # rn_set_tuning 11 = 2: the 4-wave 224x128 tile for every eligible 1x1 layer
CIN = 256

# (n, h, w), Kout: 100 rows = one short block; 224 = exactly one block; 588 = two full blocks + 140 rows; 980 = four
# full blocks + 84 rows. Kout 256 / 512 / 1024 = one / two / four column groups (four: the weight prefetch's
# double buffering goes round twice).
ALL_FORMS = [(xf, add, st) for xf in (0, 1) for add in (0, 1) for st in (0, 1)]
STEP_FORMS = [(1, 1, 1), (1, 0, 0)]   # what the training step calls: transform + residual + statistics, transform alone
SHAPES = [((1, 10, 10), 256, STEP_FORMS), ((1, 14, 16), 512, STEP_FORMS), ((3, 14, 14), 512, ALL_FORMS),
          ((3, 14, 14), 1024, STEP_FORMS), ((5, 14, 14), 256, STEP_FORMS)]
CASES = [(nhw, k, form) for nhw, k, forms in SHAPES for form in forms]
_id = lambda c: "%dx%dx%d-k%d-xf%d-add%d-st%d" % (c[0] + (c[1],) + c[2])


@functools.lru_cache(maxsize=None)
def _inputs(nhw, k, regime):
    """x, w, residual (rounding_cases' recipes) and a scale / shift for the transform: Gaussian data with fp32 scale
    and shift; or ternary x and w, an integer residual, scale 1 and shift in {-1, 0, 1, 2}: relu(x + sh) is a small
    integer, every partial sum an integer far below 2^24 and every result a bf16 value (|y| <= 256 asserted)."""
    n, h, w = nhw
    D = make_inputs((n, CIN, h, w, k, 1, 1, 0), regime)
    rng = np.random.default_rng(71)
    if regime == "gauss":
        sc = rng.uniform(0.5, 1.5, CIN)
        sh = rng.standard_normal(CIN) * 0.5 + 0.3
    else:
        sc = np.ones(CIN)
        sh = rng.integers(-1, 3, CIN).astype(np.float64)
    sh[0], sh[1] = -1.0, 1.0   # a clamped channel; a positive shift whatever the draw
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return D["x"], D["wt"], D["ya"], f32(sc), f32(sh)


@functools.lru_cache(maxsize=None)
def _oracle(nhw, k, regime, xf, add):
    """fp64 convolution of the input as the kernel stages it (+ the residual), and the same over the magnitudes."""
    x, wt, res, sc, sh = _inputs(nhw, k, regime)
    xa = bnrelu_operand(x, sc, sh) if xf else x
    ref = conv_fwd64(xa, wt, 1, 0) + (res if add else 0)
    sabs = conv_fwd64(np.abs(xa), np.abs(wt), 1, 0) + (np.abs(res) if add else 0)
    return ref, sabs


class _Dev:
    def __init__(self, nhw, k, regime, gpu):
        n, h, w = nhw
        x, wt, res, sc, sh = _inputs(nhw, k, regime)
        self.lib = L.load()
        self.d = d = conv_desc(BF16, n, CIN, h, w, k, 1, 1, 1, 0)
        self.M, self.k, self.gpu = n * h * w, k, gpu
        self.xd, self.rd = to_nhwc(x, BF16, gpu), to_nhwc(res, BF16, gpu)
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
        self.sc, self.sh = f(sc), f(sh)
        self.wk = torch.zeros(k * CIN, dtype=torch.bfloat16, device=gpu)
        master = torch.from_numpy(np.ascontiguousarray(wt.transpose(0, 2, 3, 1), dtype=np.float32)).reshape(-1).to(gpu)
        L.call("rn_conv_weight_pack", C.byref(d), p(master), p(self.wk), None, stream())

    def run(self, form):
        """One rn_conv_fwd_x into NaN-filled outputs with sentinels behind them: (y with its 224 sentinel rows,
        part with its sentinel block, or None)."""
        xf, add, st = form
        d, k = self.d, self.k
        nblk = int(self.lib.rn_conv_bnstats_blocks(C.byref(d)))
        y = torch.full((self.M + 224, k), float("nan"), dtype=torch.bfloat16, device=self.gpu)
        part = torch.full((nblk + 1, 3, k), float("nan"), dtype=torch.float32, device=self.gpu) if st else None
        L.call("rn_conv_fwd_x", C.byref(d), p(self.xd), p(self.wk), p(y), BF16, p(self.rd) if add else None, None,
               p(self.sc) if xf else None, p(self.sh) if xf else None, p(part), stream())
        torch.cuda.synchronize()
        return y, part


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["gauss", "exact"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fwd1x1_lds_stream(gpu, case, regime):
    nhw, k, form = case
    xf, add, st = form
    dev = _Dev(nhw, k, regime, gpu)
    lib, d, M = dev.lib, dev.d, dev.M
    nblk = -(-M // 224)
    q = lambda: int(lib.rn_conv_fwd_lds_streamed(C.byref(d)))
    geom = lambda: (int(lib.rn_conv_bn_part_rows(C.byref(d), 0)), int(lib.rn_conv_bnstats_blocks(C.byref(d))))
    try:
        L.call("rn_set_tuning", KEY, 1)   # the tile this small grid gets by default
        assert q() == 0 and lib.rn_conv_fwd_streamed(C.byref(d)) == 0
        assert lib.rn_conv_tile(C.byref(d), 0) in (128, 256) and geom() == (224, nblk)
        y0, p0 = dev.run(form)
        L.call("rn_set_tuning", W4, 2)    # the 4-wave 224x128 tile
        assert q() == 0 and lib.rn_conv_tile(C.byref(d), 0) == 128 and geom() == (224, nblk)
        y4, p4 = dev.run(form)
        L.call("rn_set_tuning", W4, 0)
        L.call("rn_set_tuning", KEY, 2)   # the kernel
        assert q() == 1 and lib.rn_conv_fwd_streamed(C.byref(d)) == 0 and geom() == (224, nblk)
        (y1, p1), (y2, p2) = dev.run(form), dev.run(form)
    finally:
        L.call("rn_set_tuning", W4, 0)
        L.call("rn_set_tuning", KEY, 0)
    w16 = lambda t: t.view(torch.int16)
    nan16 = w16(torch.full((224, k), float("nan"), dtype=torch.bfloat16, device=gpu))
    for y in (y0, y4, y1, y2):
        assert not torch.isnan(y[:M]).any()
        assert torch.equal(w16(y[M:]), nan16)                       # the sentinel rows
    assert torch.equal(w16(y1), w16(y2))                            # repeats
    assert torch.equal(w16(y1), w16(y0)) and torch.equal(w16(y1), w16(y4))
    # against the oracle
    ref, sabs = _oracle(nhw, k, regime, xf, add)
    got = from_nhwc(y1[:M].view(nhw[0], nhw[1], nhw[2], k), k)
    if regime == "exact":
        assert np.abs(ref).max() <= 256
        assert np.array_equal(got, ref)
    else:
        assert rounding_excess(got, ref, sabs, CIN + add, BF16).max() <= 1.0
    if not st:
        return
    w32 = lambda t: t.view(torch.int32)
    nan32 = w32(torch.full((3, k), float("nan"), dtype=torch.float32, device=gpu))
    for pt in (p0, p4, p1, p2):
        assert not torch.isnan(pt[:nblk]).any()
        assert torch.equal(w32(pt[nblk]), nan32)                    # the sentinel block
    assert torch.equal(w32(p1), w32(p2))                            # repeats
    assert torch.equal(w32(p1), w32(p4))                            # the 4-wave tile's, bit for bit
    a0, a1 = p0[:nblk].double(), p1[:nblk].double()
    assert torch.equal(a0[:, 2], a1[:, 2])                          # the pivot plane
    # the same <= 224 terms dv = v - pivot per block and channel in another order: each fp32 sum is within
    # (n - 1) u sum|dv| of the exact one, + u |dv| where v - pivot itself rounds (S2: the fma rounds once per term,
    # dv^2 carries dv's rounding twice: (n + 2) u sum dv^2); twice for two sums (test_fwd_stream_gpu.py's bound)
    u = 2.0 ** -24
    v = y1[:M].double()
    dv = v - a1[:, 2][torch.arange(M, device=gpu) // 224]
    sab, ssq = dv.abs().sum(0), (dv * dv).sum(0)
    t0, t1 = a0.sum(0), a1.sum(0)
    assert bool(((t0[0] - t1[0]).abs() <= 2 * 224 * u * sab).all())
    assert bool(((t0[1] - t1[1]).abs() <= 2 * 226 * u * ssq).all())
    # (and they describe the stored values: the exact sums, in float64)
    assert bool(((t1[0] - dv.sum(0)).abs() <= 224 * u * sab).all())
    assert bool(((t1[1] - ssq).abs() <= 226 * u * ssq).all())


# ---------------------------------------------------------------------------------------------- host
def test_fwd_lds_streamed_query():
    """rn_conv_fwd_lds_streamed: 1 for stage 3's conv3 at batch 256; 0 below the size gate and with rn_set_tuning
    30 = 1; 0 for stride 2, 3x3, grouped, f32, padded k and Cin = 128 / 512, whatever key 30 says; and
    rn_conv_fwd_streamed answers as before on all of them."""
    lib = L.load()
    q = lambda d: int(lib.rn_conv_fwd_lds_streamed(C.byref(d)))
    q1 = lambda d: int(lib.rn_conv_fwd_streamed(C.byref(d)))
    mk = lambda n, c, h, w, k, r=1, stride=1, pad=0, dtype=BF16, groups=1: conv_desc(dtype, n, c, h, w, k, r, r, stride,
                                                                                  pad, groups=groups)
    on = mk(256, 256, 14, 14, 1024)
    small = mk(8, 256, 14, 14, 1024)                  # 7 row blocks: below the size gate
    dp = L.ConvDesc(dtype=BF16, n=256, h=14, w=14, c=256, c_real=256, k=512, k_pad=520, r=1, s=1, stride_h=1,
                    stride_w=1, pad_h=0, pad_w=0, groups=1)
    L.call("rn_conv_desc_init", C.byref(dp))
    never = [mk(256, 256, 14, 14, 1024, stride=2), mk(256, 256, 14, 14, 1024, r=3, pad=1),
             mk(256, 256, 14, 14, 1024, groups=2), mk(256, 256, 14, 14, 1024, dtype=F32), dp,
             mk(256, 128, 14, 14, 1024), mk(256, 512, 14, 14, 1024),
             mk(256, 256, 14, 14, 1024 + 128),        # Kout no multiple of 256
             mk(2048, 256, 32, 32, 1024)]             # 2^32 bytes of y: past the buffer descriptors
    before = [0, 0, 0, 0, 0, 1, 0, 0, 0]               # rn_conv_fwd_streamed (Cin = 128: the earlier streamed kernel's)
    try:
        for val, want_on, want_small in ((0, 1, 0), (1, 0, 0), (2, 1, 1)):
            L.call("rn_set_tuning", KEY, val)
            assert (q(on), q(small)) == (want_on, want_small)
            assert [q(d) for d in never] == [0] * len(never)
            assert q1(on) == 0 and q1(small) == 0 and [q1(d) for d in never] == before
            assert lib.rn_conv_bn_part_rows(C.byref(on), 0) == 224
        L.call("rn_set_tuning", KEY, 0)
        L.call("rn_set_tuning", 9, 1)                 # 256-row statistics blocks: the tiles
        assert q(on) == 0
    finally:
        L.call("rn_set_tuning", KEY, 0)
        L.call("rn_set_tuning", 9, 0)
