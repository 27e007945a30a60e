"""Runs, data and fp64 oracle of the weight-gradient bar, shared by test_wgrad_bar_cpu.py (the route of every run
through rn_conv_wgrad_kernel, the exact regime's cap, and the proof that both regimes reject a dropped row, a split
counted twice or not at all and a partial kept in bf16) and test_wgrad_rounding_gpu.py (the kernels).

dW is an fp32 sum over M = n p q rows of products of bf16 values, added into the caller's dW. Two regimes:
  exact: x, dy integers uniform in [-8, 8] (bf16 values; a wider range where M is short, exact_amplitude), dW
         prefilled with integers in [-3, 3]; an input
         transform with in_scale in {1, 2}, in_shift in {-1, 0, 1} (the staged operand relu(x sc + sh) is still an
         integer); int8 codes in [-127, 127] with both extremes, unit 2^-3. Every product, partial, slab entry and
         atomic add is an integer below 2^24 (times the unit), so a correct kernel returns the oracle's fp32 bits
         in any split, order or epilogue -- and partials beyond 256 make anything kept in bf16 on the way show;
  gauss: N(0, 1) data rounded to bf16, real fp32 transform coefficients (the operand from
         gpu_util.bnrelu_operand), an int8 unit that is no power of two, under gpu_util.rounding_excess with an
         fp32 output and nterms = M + 1 (the prefilled dW) + 1 (where a unit multiplies the sum). Only on the
         shapes where test_wgrad_bar_cpu.py proves that bar separates (Run.gauss).

A Run names one launch: the kernel family, the case (n, c, h, w, k, r, stride, pad, groups), the form (plain: rn_conv_
bwd_filter / _ws; xf: rn_conv_bwd_filter_x; i8: rn_conv_bwd_filter_i8; stem: rn_stem_conv_wgrad_p4), the descriptor's
dtype, the rn_set_tuning keys, whether a workspace is given, and what rn_conv_wgrad_kernel must answer: (family, tile
rows, tile columns, slab) and the split count -- MULTI: >= 3 splits with a ragged last one, FEW: any count <= 16, or the
count itself. Split counts are for 256 CUs (rn_set_tuning 21 = 50: 128 for sizing)."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

from gpu_util import BF16, F32, bnrelu_operand
from oracle import ops
from rn import lib as L
from test_depthwise_gpu import CASES as _DW_CASES
from test_kernels_gpu import BIG_CASES, CONV_CASES, GCONV_CASES

TILE, DMA64, DMA128, DMA256, DBAND, GBAND, STREAM, DEPTHWISE = (
    L.RN_WGRAD_TILE, L.RN_WGRAD_DMA64, L.RN_WGRAD_DMA128, L.RN_WGRAD_DMA256, L.RN_WGRAD_DBAND, L.RN_WGRAD_GBAND,
    L.RN_WGRAD_STREAM, L.RN_WGRAD_DEPTHWISE)
FAMILY_NAMES = {TILE: "wgrad_kernel", DMA64: "wgrad_big_kernel[64x128]", DMA128: "wgrad_big_kernel[128x128]",
                DMA256: "wgrad_big_kernel[x256]", DBAND: "wgrad_dband_kernel", GBAND: "wgrad_gband_kernel",
                STREAM: "wgrad_stream_kernel", DEPTHWISE: "dwconv_wgrad_kernel"}
MULTI, FEW = "multi", "few"
EXACT_CAP = 2 ** 24
I8_UNIT_EXACT = 2.0 ** -3
I8_UNIT_GAUSS = float(np.float32(0.0137))

Run = collections.namedtuple("Run", "family case form dtype keys ws want splits c_real gauss")


def full(case):
    return tuple(case) + (1,) * (9 - len(case))


def key_suffix(r):
    """The run's rn_set_tuning keys, -k<key>=<value> each."""
    return "".join("-k%d=%d" % kv for kv in sorted(r.keys.items()))


def run_id(r):
    return "%s-%s%s-%s-%s-%s%s" % (
        FAMILY_NAMES[r.family].replace("wgrad_", "").replace("_kernel", ""), "x".join(map(str, r.case)),
        "" if r.c_real is None else "-creal%d" % r.c_real, r.form, "bf16" if r.dtype == BF16 else "f32",
        "ws" if r.ws else "nows", key_suffix(r))


def epilogue(r):
    return "atomics" if not r.want[3] else "slab+general" if r.keys.get(25) == 1 else "slab"


def out_hw(case):
    n, c, h, w, k, r, st, pd, g = full(case)
    return ops.conv_out_hw(h, w, r, r, (st, st), (pd, pd))


def rows_m(case):
    P, Q = out_hw(case)
    return case[0] * P * Q


# ---------------------------------------------------------------------------------------------- the runs
RUNS = []


def _add(family, case, want, splits, form="plain", dtype=BF16, keys=None, ws=False, c_real=None, gauss=False,
         both_reductions=True):
    """One run; a slab run once per slab reduction (rn_set_tuning 25 = 0: the few-split kernel up to 16 splits,
    1: the general one)."""
    keys = dict(keys or {})
    for k25 in ((0, 1) if want[3] and both_reductions else (None,)):
        kk = dict(keys)
        if k25:
            kk[25] = 1
        RUNS.append(Run(family, full(case), form, dtype, kk, ws, want, splits, c_real, gauss and not k25))


def _tile(case, rows, cols, splits=MULTI, det_keys=None, forms=("plain",), dtype=BF16, keys=None, c_real=None,
          gauss=False):
    """wgrad_kernel with atomics (no workspace) and with slabs (rn_set_tuning 17 = 1)."""
    for form in forms:
        _add(TILE, case, (TILE, rows, cols, 0), splits, form, dtype, keys, False, c_real, gauss)
        _add(TILE, case, (TILE, rows, cols, 1), splits, form, dtype, {**(keys or {}), 17: 1, **(det_keys or {})}, True,
             c_real, gauss)


# wgrad_kernel, bf16: M = 3 23 22 = 1518 rows = 24 stages of 64, 8 stages per split at least: 3 splits of 512, the last 494
_tile((3, 64, 23, 22, 64, 1, 1, 0), 64, 64, 3, det_keys={19: 1})    # (with a workspace it is the stream kernel's)
_tile((3, 24, 23, 22, 40, 1, 1, 0), 64, 64, 3)                      # ragged both ways
_tile((3, 32, 23, 22, 48, 3, 1, 1), 64, 128, 3)
_tile((3, 20, 23, 22, 48, 3, 1, 1), 64, 128, 3, c_real=20)          # c_real != c = 24
_tile((3, 64, 23, 22, 136, 1, 1, 0), 128, 64, 3)
_tile((3, 128, 23, 22, 160, 3, 1, 1), 128, 128, 3, keys={5: 3})
_tile((3, 128, 46, 43, 160, 3, 2, 1), 128, 128, 3, forms=("plain", "xf"), keys={5: 3})  # 3x3 / stride 2 -> 23 x 22
# f32: 32-row stages, M = 3 17 15 = 765 = 24 stages: 3 splits of 256, the last 253
_tile((3, 64, 17, 15, 64, 1, 1, 0), 64, 64, 3, dtype=F32)
_tile((3, 32, 17, 15, 48, 3, 1, 1), 64, 128, 3, dtype=F32)
_tile((3, 64, 17, 15, 136, 1, 1, 0), 128, 64, 3, dtype=F32)
_tile((3, 128, 17, 15, 160, 3, 1, 1), 128, 128, 3, dtype=F32, forms=("plain", "xf"))
for _c in CONV_CASES:   # test_conv_bwd's, one split each: the gauss shapes of this kernel
    _n, _cc, _h, _w, _k, _r = _c[:6]
    _add(TILE, _c, (TILE, 64 if _k <= 64 else 128, 64 if _r * _r * ((_cc + 7) // 8 * 8) <= 64 else 128, 0), FEW,
         keys={5: 3}, gauss=True)
    _add(TILE, _c, (TILE, 64 if _k <= 64 else 128, 64 if _r * _r * ((_cc + 7) // 8 * 8) <= 64 else 128, 0), FEW,
         dtype=F32, gauss=True)

# grouped wgrad_kernel (64 x 64 blocks; the block-diagonal-skip form gdiag where channels in = out <= 32 per group)
GROUPED_MULTI = [(3, 128, 23, 22, 128, 3, 1, 1, 32), (3, 256, 23, 22, 256, 3, 1, 1, 32),
                 (3, 512, 23, 22, 512, 3, 1, 1, 32), (3, 1024, 23, 22, 1024, 3, 1, 1, 32)]
for _c in GROUPED_MULTI:
    for _k14 in (0, 1, 2):   # rn_set_tuning 14: gdiag spread over the waves, off, one wave per block
        # (19 = 1: no image-band kernel, which takes 4 / 8 / 16 per group when it has a workspace)
        _tile(_c, 64, 64, 3, keys={14: _k14} if _k14 else None, det_keys={19: 1})
_tile((3, 128, 23, 22, 256, 3, 1, 1, 32), 64, 64, 3, det_keys={19: 1})           # 4 in, 8 out per group: no gdiag
_tile((3, 128, 17, 15, 128, 3, 1, 1, 32), 64, 64, 3, dtype=F32, det_keys={19: 1})
for _c in GCONV_CASES:
    _tile(_c, 64, 64, FEW, det_keys={19: 1}, gauss=True)

# wgrad_big_kernel 128 x 128 (rn_set_tuning 2 workgroups per CU, 8 M-tiles per split at least: 3 splits of 512)
_add(DMA128, (3, 128, 23, 22, 128, 1, 1, 0), (DMA128, 128, 128, 0), 3)                       # DIR, atomics
_add(DMA128, (3, 128, 23, 22, 128, 1, 1, 0), (DMA128, 128, 128, 1), 3, keys={19: 1}, ws=True)  # (19 = 1: not the stream kernel)
_add(DMA128, (3, 128, 23, 22, 160, 3, 1, 1), (DMA128, 128, 128, 0), 3)                       # gathered, ragged K tile
_add(DMA128, (3, 128, 46, 44, 128, 1, 2, 0), (DMA128, 128, 128, 0), 3)                       # stride 2 -> 23 x 22
for _c in ((3, 128, 23, 22, 128, 1, 1, 0), (3, 128, 46, 44, 128, 1, 2, 0)):
    _add(DMA128, _c, (DMA128, 128, 128, 0), 3, "xf", keys={19: 1})
    _add(DMA128, _c, (DMA128, 128, 128, 1), 3, "xf", keys={19: 1}, ws=True)
    _add(DMA128, _c, (DMA128, 128, 128, 1), 3, "i8", keys={19: 1}, ws=True)
_add(DMA128, (3, 128, 9, 11, 128, 1, 2, 0), (DMA128, 128, 128, 1), FEW, "i8", ws=True, gauss=True)   # test_wgrad_int8_codes'
_add(DMA128, (2, 64, 14, 14, 128, 3, 1, 1), (DMA128, 128, 128, 0), FEW, gauss=True)                  # CONV_CASES[1]

# wgrad_big_kernel x 256 columns (with a workspace; 4 M-tiles per split at least: 6 splits of 256, the last 238)
for _c, _rows, _forms in (((3, 256, 23, 22, 256, 1, 1, 0), 256, ("plain", "xf", "i8")),
                          ((3, 256, 23, 22, 136, 1, 1, 0), 128, ("plain", "xf", "i8")),
                          ((3, 128, 23, 22, 160, 3, 1, 1), 128, ("plain", "i8"))):
    for _f in _forms:
        _add(DMA256, _c, (DMA256, _rows, 256, 1), 6, _f, ws=True)
        if _f != "i8":   # rn_set_tuning 5 = 1 without a workspace: the same tiles with atomics
            _add(DMA256, _c, (DMA256, _rows, 256, 0), 6, _f, keys={5: 1})
for _c in BIG_CASES:   # test_conv_big_tiles': every one of M <= 600 (BIG_CASES[7], <= 64 output channels, is DMA64's below)
    if rows_m(full(_c)) <= 600 and _c[4] >= 128 and _c[5] * _c[5] * _c[1] >= 256:
        _add(DMA256, _c, (DMA256, 256 if _c[4] >= 256 else 128, 256, 1), FEW, ws=True, gauss=True)
# BIG_CASES[2]: 160 columns, fewer than the 256-column tile takes and ending inside the second 128-column tile --
# the 128 x 128 tile's ragged column tile, with and without a workspace (M = 98: one split)
_add(DMA128, BIG_CASES[2], (DMA128, 128, 128, 0), FEW, gauss=True)
_add(DMA128, BIG_CASES[2], (DMA128, 128, 128, 1), FEW, ws=True, gauss=True)
# test_wgrad_int8_codes' 256-column shapes, with the transform where the convolution is 1x1
for _c, _rows, _forms in (((2, 256, 14, 14, 512, 1, 1, 0), 256, ("i8", "xf")), ((2, 512, 7, 9, 128, 1, 1, 0), 128, ("i8", "xf")),
                          ((3, 128, 13, 10, 128, 3, 1, 1), 128, ("i8",))):
    for _f in _forms:
        _add(DMA256, _c, (DMA256, _rows, 256, 1), FEW, _f, ws=True, gauss=True)
_add(DMA128, (3, 128, 9, 11, 128, 1, 2, 0), (DMA128, 128, 128, 1), FEW, "xf", ws=True, gauss=True)

# wgrad_big_kernel 64 x 128: the stem's padded channels (c_real = 3, c = 8; M = 4 20 19 = 1520) and rn_set_tuning 5 = 4
_add(DMA64, (4, 3, 40, 38, 64, 7, 2, 3), (DMA64, 64, 128, 0), 3, c_real=3)
_add(DMA64, (3, 64, 23, 22, 64, 3, 1, 1), (DMA64, 64, 128, 0), 3, keys={5: 4})
_add(DMA64, (3, 64, 23, 22, 64, 3, 1, 1), (DMA64, 64, 128, 1), 3, keys={5: 4, 19: 1}, ws=True)
_add(DMA64, BIG_CASES[7], (DMA64, 64, 128, 0), FEW, keys={5: 4}, gauss=True)   # 25 taps, stride 2, M = 84

# rn_stem_conv_wgrad_p4 (its own rule in rn.h: 2 column tiles, 8 M-tiles per split at least, atomics)
STEM_GEOMS = [(4, 50, 38), (1, 31, 17)]
for _n, _h, _w in STEM_GEOMS:
    _add(DMA64, (_n, 3, _h, _w, 64, 7, 2, 3), (DMA64, 64, 128, 0), 3 if _n == 4 else 1, "stem", c_real=3, gauss=_n == 1)

# wgrad_dband_kernel (whole images per workgroup: the splits are over n)
for _f in ("plain", "xf"):
    _add(DBAND, (11, 64, 9, 13, 64, 3, 1, 1), (DBAND, 0, 0, 1), 6, _f, keys={21: 3}, ws=True)   # 8 CUs: 2 images each, the last 1
    _add(DBAND, (3, 64, 9, 13, 64, 3, 1, 1), (DBAND, 0, 0, 1), 3, _f, ws=True, gauss=True)
# the 128-channel geometry has 4 slices: 8 CUs (rn_set_tuning 21 = 3) give 2 workgroups per slice, so TWO splits of
# 3 + 2 images at any batch; 12 CUs (21 = 5) give 3 splits of 2 + 2 + 1
_add(DBAND, (5, 128, 5, 30, 128, 3, 1, 1), (DBAND, 0, 0, 1), 2, keys={19: 2, 21: 3}, ws=True)
_add(DBAND, (5, 128, 5, 30, 128, 3, 1, 1), (DBAND, 0, 0, 1), 3, keys={19: 2, 21: 5}, ws=True)
_add(DBAND, (9, 256, 14, 14, 256, 3, 1, 1), (DBAND, 0, 0, 1), 5, keys={19: 2}, ws=True)   # 2 images each, the last 1
# (the same kernel geometry as 256 channels; 64 slices on 128 CUs: TWO splits of 3 + 2 images)
_add(DBAND, (5, 512, 7, 7, 512, 3, 1, 1), (DBAND, 0, 0, 1), 2, keys={19: 2}, ws=True)

# wgrad_gband_kernel (rn_set_tuning 23 = 3: 8 CUs)
_add(GBAND, (11, 128, 5, 7, 128, 3, 1, 1, 32), (GBAND, 0, 0, 1), 6, keys={23: 3}, ws=True)
_add(GBAND, (11, 256, 7, 28, 256, 3, 1, 1, 32), (GBAND, 0, 0, 1), 6, keys={23: 3}, ws=True)
_add(GBAND, (5, 512, 7, 14, 512, 3, 1, 1, 32), (GBAND, 0, 0, 1), 3, keys={23: 3}, ws=True)
_add(GBAND, (4, 128, 5, 7, 128, 3, 1, 1, 32), (GBAND, 0, 0, 1), FEW, ws=True, gauss=True)   # test_wgrad_grouped_image_bands'

# wgrad_stream_kernel: M = 765 = 12 M-tiles, 4 per split at least: 3 splits of 256, the last 253
STREAM_KC = [(256, 64), (64, 256), (64, 64), (128, 64), (64, 128), (128, 128), (128, 256), (256, 128)]
for _k, _c in STREAM_KC:
    for _f in ("plain", "xf", "i8"):
        _add(STREAM, (3, _c, 17, 15, _k, 1, 1, 0), (STREAM, 0, 0, 1), 3, _f, ws=True)
        _add(STREAM, (3, _c, 13, 11, _k, 1, 1, 0), (STREAM, 0, 0, 1), 1, _f, ws=True, gauss=True)   # test_wgrad_stream_1x1's: one split
# 68 M-tiles: 17 splits, past the few-split reduction by its own rule
_add(STREAM, (5, 64, 30, 29, 64, 1, 1, 0), (STREAM, 0, 0, 1), 17, ws=True, both_reductions=False)

# dwconv_wgrad_kernel (always slabs; its splits are workgroups over row runs and channel chunks)
for _n, _c, _h, _w, _st in _DW_CASES:
    # (the 56 x 56 case has 33 workgroups: past the few-split reduction by its own rule)
    _add(DEPTHWISE, (_n, _c, _h, _w, _c, 3, _st, 1, _c), (DEPTHWISE, 0, 0, 1), FEW if _h < 56 else 33, ws=True,
         gauss=_n * _h * _w <= 600)

# the FC head: M = 37 rows, K = 1000 ragged
for _c in ((37, 2048, 1, 1, 1000, 1, 1, 0), (37, 256, 1, 1, 1000, 1, 1, 0)):
    _add(DMA128, _c, (DMA128, 128, 128, 0), 1, gauss=True)
    _add(DMA256, _c, (DMA256, 256, 256, 1), 1, ws=True, gauss=True)

FAMILIES = sorted({r.family for r in RUNS})
DATA_KEYS = sorted({(r.case, r.form, r.c_real) for r in RUNS})
GAUSS_KEYS = sorted({(r.case, r.form, r.c_real) for r in RUNS if r.gauss})


def runs_of(family):
    return [r for r in RUNS if r.family == family]


# ---------------------------------------------------------------------------------------------- the host's answer
def make_desc(r):
    n, c, h, w, k, rr, st, pd, g = r.case
    cr = c if r.c_real is None else r.c_real
    cp = 8 if r.form == "stem" or (cr < 8 and g == 1) else (cr + 7) // 8 * 8 if g == 1 else c
    d = L.ConvDesc(dtype=r.dtype, n=n, h=h, w=w, c=cp, c_real=cr, k=k, k_pad=(k + 7) // 8 * 8 if g == 1 else k, r=rr,
                   s=rr, stride_h=st, stride_w=st, pad_h=pd, pad_w=pd, groups=g)
    L.call("rn_conv_desc_init", C.byref(d))
    return d


def ws_bytes_of(lib, d, r):
    if not r.ws:
        return 0
    need = lib.rn_conv_wgrad_i8_ws_bytes(C.byref(d)) if r.form == "i8" else lib.rn_conv_wgrad_ws_bytes(C.byref(d))
    assert need > 0, (run_id(r), need)
    return int(need)


def stem_splits(r):
    """rn_stem_conv_wgrad_p4's fixed rule (rn.h): 2 column tiles of 128, so at most 512 / 2 = 256 splits, of 8
    64-row M-tiles at least; the M-tiles dealt evenly."""
    mt = -(-rows_m(r.case) // 64)
    s = min(256, max(1, mt // 8))
    mps = -(-mt // s) * 64
    return -(-rows_m(r.case) // mps), mps


def query(lib, d, r):
    """(family, rows, cols, slab, splits) of rn_conv_wgrad_kernel under the keys set now."""
    sp, sl = C.c_int32(-7), C.c_int32(-7)
    v = lib.rn_conv_wgrad_kernel(C.byref(d), int(r.form == "xf"), int(r.form == "i8"), ws_bytes_of(lib, d, r),
                                 C.byref(sp), C.byref(sl))
    assert v > 0, (run_id(r), v)
    return (v & 0xff, (v >> 8) & 0xfff, v >> 20, sl.value, sp.value)


def rows_per_split(r, splits):
    """Rows of M in each split but the last: whole images for the band kernels, else whole M-tiles (64 rows; 32 of
    the f32 wgrad_kernel) dealt evenly."""
    M = rows_m(r.case)
    if r.family in (DBAND, GBAND):
        P, Q = out_hw(r.case)
        return -(-r.case[0] // splits) * P * Q
    unit = 32 if r.dtype == F32 else 64
    return -(-(-(-M // unit)) // splits) * unit


def check_route(lib, d, r):
    """The query's answer is the run's: family, tile, slab flag, split count. Returns the split count."""
    if r.form == "stem":
        return stem_splits(r)[0]
    fam, rows, cols, slab, splits = query(lib, d, r)
    assert (fam, rows, cols, slab) == tuple(r.want), (run_id(r), (fam, rows, cols, slab), r.want)
    if lib.rn_device_cu_count() in (0, -1, 256) and r.splits is not None:
        M = rows_m(r.case)
        if r.splits == FEW:
            assert 1 <= splits <= 16, (run_id(r), splits)
        else:
            assert splits == r.splits, (run_id(r), splits, r.splits)
        if isinstance(r.splits, int) and r.splits >= 3 and r.family not in (DBAND, GBAND, DEPTHWISE):
            mps = rows_per_split(r, splits)
            assert -(-M // mps) == splits and M % mps != 0, (run_id(r), "last split not ragged", M, mps)
    if slab and r.keys.get(25) != 1 and r.splits not in (17, 33):
        # (launch_slab_reduce's rule: <= 16 splits of whole 16-byte chunks)
        assert splits <= 16 and lib.rn_conv_weight_numel(C.byref(d)) % 4 == 0, (run_id(r), "few-split reduction meant", splits)
    return splits


# ---------------------------------------------------------------------------------------------- oracle (fp64)
def dw64(x, dy, case):
    """dW[k][c / groups][r][s] of the convolution, float64."""
    n, c, h, w, k, r, st, pd, g = full(case)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return torch.nn.grad.conv2d_weight(t(x), (k, c // g, r, r), t(dy), stride=st, padding=pd, groups=g).numpy()


def exact_amplitude(case):
    """The exact regime's integer range [-a, a]: 8 from 400 rows on; wider where M is short, so that a split's
    partial sums still pass 256 and a partial kept in bf16 shows (test_wgrad_bar_cpu.py checks that, and the 2^24
    cap: a^2 M <= 127^2 64). a <= 127: x, dy and the transformed operand 2 a + 1 stay bf16 values."""
    M = rows_m(case)
    return 8 if M >= 400 else 32 if M >= 64 else 127


def make_inputs(case, form, regime):
    n, c, h, w, k, r, st, pd, g = full(case)
    P, Q = out_hw(case)
    rng = np.random.default_rng(131 if regime == "gauss" else 132)
    D = dict(P=P, Q=Q)
    if regime == "gauss":
        bf = lambda shape: ops.bf16_round(rng.standard_normal(shape))
        D["x"], D["dy"] = bf((n, c, h, w)), bf((n, k, P, Q))
        D["dw0"] = rng.standard_normal((k, c // g, r, r)).astype(np.float32).astype(np.float64)
        D["sc"] = rng.uniform(0.5, 1.5, c).astype(np.float32).astype(np.float64)
        D["sh"] = (rng.standard_normal(c) * 0.5).astype(np.float32).astype(np.float64)
        D["unit"] = I8_UNIT_GAUSS
    else:
        a = exact_amplitude(case)
        D["x"] = rng.integers(-a, a + 1, (n, c, h, w)).astype(np.float64)
        D["dy"] = rng.integers(-a, a + 1, (n, k, P, Q)).astype(np.float64)
        D["dw0"] = rng.integers(-3, 4, (k, c // g, r, r)).astype(np.float64)
        D["sc"] = rng.integers(1, 3, c).astype(np.float64)
        D["sh"] = rng.integers(-1, 2, c).astype(np.float64)
        D["unit"] = I8_UNIT_EXACT
    if form == "i8":
        codes = rng.integers(-127, 128, (n, c, h, w)).astype(np.int8)
        codes[0, :, 0, :] = 127
        codes[-1, :, -1, :] = -127
        D["codes"] = codes
    return D


def operand(D, form):
    """The x the kernel multiplies (NCHW, fp64): x, the BatchNorm+ReLU of it on load, or the int8 codes (their unit
    multiplies the sum once)."""
    if form == "xf":
        return bnrelu_operand(D["x"], D["sc"], D["sh"])
    if form == "i8":
        return D["codes"].astype(np.float64)
    return D["x"]


@functools.lru_cache(maxsize=8)
def wgrad_data(case, form, regime):
    """Inputs and the oracle's results, computed once per (case, form): sum = the fp64 sum of products (before the
    unit), ref = unit * sum + dw0, and in the gauss regime sabs = the same over the magnitudes."""
    D = make_inputs(case, form, regime)
    xo = operand(D, form)
    D["xo"] = xo
    unit = D["unit"] if form == "i8" else 1.0
    D["sum"] = dw64(xo, D["dy"], case)
    D["ref"] = unit * D["sum"] + D["dw0"]
    if regime == "gauss":
        D["sabs"] = unit * dw64(np.abs(xo), np.abs(D["dy"]), case) + np.abs(D["dw0"])
    for v in D.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return D


def nterms(r):
    return rows_m(r.case) + 1 + (r.form == "i8")
