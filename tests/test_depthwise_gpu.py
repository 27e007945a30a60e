"""The depthwise 3x3 kernels (dwconv_fwd_kernel / dwconv_dgrad_kernel / dwconv_wgrad_kernel: bf16, groups = c = k,
pad 1, stride 1 or 2) against the numpy oracle on bf16-rounded inputs, and the same descriptors on the
block-diagonal tiles (rn_set_tuning 28 = 1 at descriptor-init time): y and dx, without and with an add_src, within
one rounding per element (gpu_util.rounding_excess <= 1: fp32 accumulation of the nine products and the added
operand in any order, then half a bf16 ulp) and within 1.5e-2 of max |ref|, the grouped kernels' bar of
tests/test_kernels_gpu.py; dw within 5e-3 of max |ref|."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ops
from rn import lib as L
from gpu_util import BF16, bf16_round, from_nhwc, p, rel_err, rounding_excess, stream, to_nhwc

pytestmark = pytest.mark.gpu

TOL_Y, TOL_DW = 1.5e-2, 5e-3

CASES = [
    # n, c, h, w, stride
    (2, 32, 9, 11, 1),      # odd sizes
    (2, 64, 10, 10, 2),     # stride 2, even sizes: the last dx row / column has taps outside dy
    (2, 1024, 7, 7, 2),     # stride 2, odd sizes; the most channels
    (3, 24, 7, 5, 1),       # 3 chunks (no power of two), narrow rows
    (2, 8, 6, 6, 2),        # one chunk
    (2, 64, 2, 2, 1),       # every window on the border
    (2, 64, 2, 2, 2),
    (1, 512, 14, 14, 1),
    (4, 128, 56, 56, 1),    # seven row runs per column
]


@functools.lru_cache(maxsize=None)
def _data(case):
    """Inputs (bf16-rounded, fp64) and the oracle's results, computed once per case."""
    n, c, h, w, st = case
    rng = np.random.default_rng(28)
    x = bf16_round(rng.standard_normal((n, c, h, w)))
    wt = bf16_round(rng.standard_normal((c, 1, 3, 3)) / 3.0)
    P, Q = ops.conv_out_hw(h, w, 3, 3, (st, st), (1, 1))
    dy = bf16_round(rng.standard_normal((n, c, P, Q)))
    ya = bf16_round(rng.standard_normal((n, c, P, Q)))
    xa = bf16_round(rng.standard_normal((n, c, h, w)))
    y_ref = ops.conv2d_fwd(x, wt, (st, st), (1, 1), c)
    dx_ref, dw_ref = ops.conv2d_bwd(x, wt, dy, (st, st), (1, 1), c)
    # the sums of the terms' magnitudes, for the per-element rounding bar
    y_sabs = ops.conv2d_fwd(np.abs(x), np.abs(wt), (st, st), (1, 1), c)
    dx_sabs = ops.conv2d_bwd(x, np.abs(wt), np.abs(dy), (st, st), (1, 1), c)[0]
    for a in (x, wt, dy, ya, xa, y_ref, dx_ref, dw_ref, y_sabs, dx_sabs):
        a.setflags(write=False)
    return dict(x=x, wt=wt, dy=dy, ya=ya, xa=xa, y=y_ref, dx=dx_ref, dw=dw_ref, P=P, Q=Q, y_sabs=y_sabs,
                dx_sabs=dx_sabs)


def _desc(case, off):
    """A depthwise descriptor initialised with rn_set_tuning 28 = off (1: the block-diagonal path)."""
    n, c, h, w, st = case
    d = L.ConvDesc(dtype=BF16, n=n, h=h, w=w, c=c, c_real=c, k=c, k_pad=c, r=3, s=3, stride_h=st, stride_w=st,
                   pad_h=1, pad_w=1, groups=c)
    L.call("rn_set_tuning", 28, off)
    try:
        L.call("rn_conv_desc_init", C.byref(d))
    finally:
        L.call("rn_set_tuning", 28, 0)
    assert d.grouped_direct == (0 if off else 2)
    return d


def _master(wt, dev):  # [k][r][s][c / groups] fp32
    return torch.from_numpy(np.ascontiguousarray(wt.transpose(0, 2, 3, 1), dtype=np.float32)).reshape(-1).to(dev)


def _run(case, off, gpu, cap=0):
    """Forward and data gradient without and with an add_src, the weight gradient twice. cap: rn_set_tuning 28
    at launch time (>= 2: at most that many workgroups)."""
    n, c, h, w, st = case
    D = _data(case)
    lib = L.load()
    d = _desc(case, off)
    numel = [lib.rn_conv_pack_numel(C.byref(d), which) for which in (0, 1)]
    assert numel == ([64 * 9 * c] * 2 if off else [9 * c] * 2)
    wk = torch.zeros(numel[0], dtype=torch.bfloat16, device=gpu)
    wc = torch.zeros(numel[1], dtype=torch.bfloat16, device=gpu)
    master = _master(D["wt"], gpu)
    L.call("rn_conv_weight_pack", C.byref(d), p(master), p(wk), p(wc), stream())
    xd, dyd, yad, xad = (to_nhwc(D[k], BF16, gpu) for k in ("x", "dy", "ya", "xa"))
    nan = float("nan")  # every output element is written
    y, y2 = (torch.full((n, D["P"], D["Q"], c), nan, dtype=torch.bfloat16, device=gpu) for _ in range(2))
    dx, dx2 = (torch.full((n, h, w, c), nan, dtype=torch.bfloat16, device=gpu) for _ in range(2))
    ws_bytes = lib.rn_conv_wgrad_ws_bytes(C.byref(d))
    assert off or ws_bytes > 0
    ws = torch.zeros(max(ws_bytes // 4, 4), dtype=torch.float32, device=gpu)
    dws = [torch.zeros(c * 9, dtype=torch.float32, device=gpu) for _ in range(2)]
    L.call("rn_set_tuning", 28, cap)
    try:
        L.call("rn_conv_fwd", C.byref(d), p(xd), p(wk), p(y), BF16, None, None, stream())
        L.call("rn_conv_fwd", C.byref(d), p(xd), p(wk), p(y2), BF16, p(yad), None, stream())
        L.call("rn_conv_bwd_data", C.byref(d), p(dyd), p(wc), p(dx), None, stream())
        L.call("rn_conv_bwd_data", C.byref(d), p(dyd), p(wc), p(dx2), p(xad), stream())
        for dw in dws:
            if ws_bytes > 0:
                L.call("rn_conv_bwd_filter_ws", C.byref(d), p(xd), p(dyd), p(dw), p(ws), ws_bytes, stream())
            else:
                L.call("rn_conv_bwd_filter", C.byref(d), p(xd), p(dyd), p(dw), stream())
        torch.cuda.synchronize()
    finally:
        L.call("rn_set_tuning", 28, 0)
    errs = dict(y=rel_err(from_nhwc(y, c), D["y"]), y_add=rel_err(from_nhwc(y2, c), D["y"] + D["ya"]),
                dx=rel_err(from_nhwc(dx, c), D["dx"]), dx_add=rel_err(from_nhwc(dx2, c), D["dx"] + D["xa"]),
                dw=rel_err(dws[0].cpu().numpy().reshape(c, 3, 3, 1).transpose(0, 3, 1, 2), D["dw"]))
    excess = dict(
        y=rounding_excess(from_nhwc(y, c), D["y"], D["y_sabs"], 9, BF16).max(),
        y_add=rounding_excess(from_nhwc(y2, c), D["y"] + D["ya"], D["y_sabs"] + np.abs(D["ya"]), 10, BF16).max(),
        dx=rounding_excess(from_nhwc(dx, c), D["dx"], D["dx_sabs"], 9, BF16).max(),
        dx_add=rounding_excess(from_nhwc(dx2, c), D["dx"] + D["xa"], D["dx_sabs"] + np.abs(D["xa"]), 10, BF16).max())
    print("depthwise", case, "off" if off else "dw", "cap", cap, {k: "%.2e" % v for k, v in errs.items()},
          "rounding excess", {k: "%.3f" % v for k, v in excess.items()})
    for k, v in errs.items():
        assert v < (TOL_DW if k == "dw" else TOL_Y), (k, v)
    for k, v in excess.items():
        assert v <= 1.0, (k, v)
    return dws


@pytest.mark.parametrize("off", [0, 1], ids=["dwconv", "blockdiag"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_depthwise_conv(gpu, case, off):
    dws = _run(case, off, gpu)
    if not off:  # slabs and a fixed summation order: the same bits every run
        assert torch.equal(dws[0].view(torch.int32), dws[1].view(torch.int32))


@pytest.mark.parametrize("case", [(4, 128, 56, 56, 1), (3, 24, 7, 5, 1), (2, 64, 10, 10, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_depthwise_work_item_loop(gpu, case):
    """rn_set_tuning 28 = 4 at launch time: at most 4 workgroups (rounded up to a whole number of chunk
    periods), so every lane loops over many work items -- 25088 items on 1024 lanes in the first case."""
    dws = _run(case, 0, gpu, cap=4)
    assert torch.equal(dws[0].view(torch.int32), dws[1].view(torch.int32))


def test_depthwise_wgrad_needs_the_slab_workspace(gpu):
    case = (2, 32, 9, 11, 1)
    d = _desc(case, 0)
    t = torch.zeros(2 * 9 * 11 * 32, dtype=torch.bfloat16, device=gpu)
    dw = torch.zeros(32 * 9, dtype=torch.float32, device=gpu)
    lib = L.load()
    assert lib.rn_conv_bwd_filter(C.byref(d), p(t), p(t), p(dw), stream()) == -1
    assert b"workspace" in lib.rn_last_error()
    torch.cuda.synchronize()


def test_depthwise_weight_pack_multi(gpu):
    """The fused-update re-pack: rn_conv_weight_pack_multi over two depthwise layers and a dense one writes
    the bytes of the per-layer rn_conv_weight_pack."""
    lib = L.load()
    rng = np.random.default_rng(5)
    descs = [_desc((2, 64, 10, 10, 2), 0), _desc((3, 24, 7, 5, 1), 0)]
    dense = L.ConvDesc(dtype=BF16, n=2, h=6, w=6, c=24, c_real=24, k=40, k_pad=40, r=1, s=1, stride_h=1, stride_w=1,
                       pad_h=0, pad_w=0, groups=1)
    L.call("rn_conv_desc_init", C.byref(dense))
    descs.append(dense)
    masters = [torch.tensor(rng.standard_normal(lib.rn_conv_weight_numel(C.byref(d))), dtype=torch.float32,
                            device=gpu) for d in descs]

    def copies():
        return [[torch.full((lib.rn_conv_pack_numel(C.byref(d), which),), 7.0, dtype=torch.bfloat16, device=gpu)
                 for which in (0, 1)] for d in descs]
    one, multi = copies(), copies()
    for d, m, (wk, wc) in zip(descs, masters, one):
        L.call("rn_conv_weight_pack", C.byref(d), p(m), p(wk), p(wc), stream())
    arr = (L.ConvDesc * 3)(*descs)
    vp = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    L.call("rn_conv_weight_pack_multi", arr, vp(masters), vp([c[0] for c in multi]), vp([c[1] for c in multi]), 3,
           stream())
    torch.cuda.synchronize()
    for (a0, a1), (b0, b1) in zip(one, multi):
        assert torch.equal(a0.view(torch.int16), b0.view(torch.int16))
        assert torch.equal(a1.view(torch.int16), b1.view(torch.int16))
    # and the layout itself: [tap][c], the data-gradient copy with the taps mirrored
    w0 = masters[0].cpu().numpy().reshape(64, 9)
    assert np.array_equal(one[0][0].float().cpu().numpy().reshape(9, 64), bf16_round(w0.T).astype(np.float32))
    assert np.array_equal(one[0][1].float().cpu().numpy().reshape(9, 64), bf16_round(w0[:, ::-1].T).astype(np.float32))
