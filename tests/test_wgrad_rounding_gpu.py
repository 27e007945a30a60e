"""Every weight-gradient kernel held to exact sums at its split seams, and to the fp32 rounding bar.

include/rn.h promises dw += x^T dy, accumulated in fp32. For every run of wgrad_cases.RUNS (one per kernel family x
shape x form x epilogue x slab reduction; test_wgrad_bar_cpu.py shows what each regime rejects):
  exact: integer data whose every product, partial, slab entry and atomic add is an integer below 2^24: the oracle's
         fp32 bits in any split, order or epilogue. The first differing (k, r, s, c) names the place;
  gauss: N(0, 1) data against the fp64 oracle within gpu_util.rounding_excess <= 1 for an fp32 output (derived, not
         fitted), on the shapes where the CPU file proves that the bar separates.
Each run sets its rn_set_tuning keys, asserts rn_conv_wgrad_kernel's answer (family, tile, epilogue, splits: >= 3 with
a ragged last one at every seam case), gives a NaN-filled workspace of rn_conv_wgrad_ws_bytes / _i8_ws_bytes plus a
tail, prefills dW (the contract is +=) and calls the entry point the executor uses for that form. Slab runs repeat
the call and compare bits, and their workspace's tail must still be NaN. One line per call is printed (DESIGN.md
records the ratios)."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_cases as W
from rn import lib as L
from gpu_util import BF16, p, rounding_excess, stream, tdt, to_nhwc, tuning

pytestmark = pytest.mark.gpu

TAIL = 64  # floats past the workspace the host asked for


def _params(family):
    return [pytest.param(r, regime, id="%s-%s" % (W.run_id(r), regime))
            for r in W.runs_of(family) for regime in (("exact", "gauss") if r.gauss else ("exact",))]


def verify(tag, got, D, nt, regime):
    """got: dW as the device holds it, [k][r][s][c / groups] fp32 (numpy)."""
    ref = D["ref"].transpose(0, 2, 3, 1)
    if regime == "exact":
        want = np.ascontiguousarray(ref, dtype=np.float32)
        assert np.array_equal(want.astype(np.float64), ref), tag
        same = got.view(np.int32) == want.view(np.int32)
        if not same.all():
            at = tuple(int(v) for v in np.argwhere(~same)[0])
            raise AssertionError("%s: %d of %d elements differ, first at (k, r, s, c) = %s: got %r, exact %r" % (
                tag, int((~same).sum()), same.size, at, float(got[at]), float(want[at])))
        print("wgrad", tag + ": exact, bit for bit, max |dW| %g" % np.abs(ref).max())
        return
    ex = rounding_excess(got, ref, D["sabs"].transpose(0, 2, 3, 1), nt, L.RN_F32)
    print("wgrad", tag + ": gauss max ratio %.4f (%d terms)" % (ex.max(), nt))
    if ex.max() > 1.0:
        at = tuple(int(v) for v in np.unravel_index(np.argmax(ex), ex.shape))
        raise AssertionError("%s: %.3g x the allowed error at (k, r, s, c) = %s, %.2f%% of the elements above 1" % (
            tag, ex.max(), at, 100.0 * (ex > 1).mean()))


def _stem_image(D, d, r, gpu):
    """test_stem_band's zero-bordered NHWC4 image."""
    n, c, h, w, k, rr, st, pd, g = r.case
    hp = max(h + 2 * pd, (d.p - 1) * st + 8)
    wp = max(w + 2 * pd, (d.q - 1) * st + 8)
    hp, wp = hp + hp % 2, wp + wp % 2
    assert L.load().rn_stem_p4_supported(C.byref(d), hp, wp) == 1
    img = np.zeros((n, hp, wp, 4), np.float32)
    img[:, pd:pd + h, pd:pd + w, :c] = D["x"].transpose(0, 2, 3, 1)
    return torch.tensor(img.reshape(-1), dtype=torch.bfloat16, device=gpu), hp, wp


def run_wgrad(gpu, r, regime):
    lib = L.load()
    n, c, h, w, k, rr, st, pd, g = r.case
    D = W.wgrad_data(r.case, r.form, regime)
    shape = (k, rr, rr, c // g)
    outs = []
    with tuning(r.keys):
        d = W.make_desc(r)
        assert (d.p, d.q) == (D["P"], D["Q"]) and lib.rn_conv_weight_numel(C.byref(d)) == int(np.prod(shape))
        splits = W.check_route(lib, d, r)
        if isinstance(r.splits, int) and r.splits >= 3:
            assert splits >= 3, (W.run_id(r), splits)
        need = W.ws_bytes_of(lib, d, r)
        ws = torch.full((need // 4 + TAIL,), float("nan"), dtype=torch.float32, device=gpu) if need else None
        dyd = to_nhwc(D["dy"], r.dtype, gpu, d.k_pad)
        f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float32, device=gpu)
        if r.form == "i8":
            xd = torch.from_numpy(np.ascontiguousarray(D["codes"].transpose(0, 2, 3, 1))).to(gpu)
            unit = f([D["unit"]])
        elif r.form == "stem":
            xd, hp, wp = _stem_image(D, d, r, gpu)
        else:
            xd = to_nhwc(D["x"], r.dtype, gpu, d.c)
        if r.form == "xf":
            assert d.c == c
            sc, sh = f(D["sc"]), f(D["sh"])
        dw0 = np.ascontiguousarray(D["dw0"].transpose(0, 2, 3, 1), dtype=np.float32).reshape(-1)
        for _ in range(2 if r.want[3] else 1):
            dw = torch.from_numpy(dw0).to(gpu)
            if r.form == "i8":
                L.call("rn_conv_bwd_filter_i8", C.byref(d), p(xd), p(unit), p(dyd), p(dw), p(ws), need, stream())
            elif r.form == "stem":
                L.call("rn_stem_conv_wgrad_p4", C.byref(d), p(xd), p(dyd), p(dw), hp, wp, stream())
            elif r.form == "xf":
                L.call("rn_conv_bwd_filter_x", C.byref(d), p(xd), p(dyd), p(dw), p(sc), p(sh), p(ws), need, stream())
            elif r.ws:
                L.call("rn_conv_bwd_filter_ws", C.byref(d), p(xd), p(dyd), p(dw), p(ws), need, stream())
            else:
                L.call("rn_conv_bwd_filter", C.byref(d), p(xd), p(dyd), p(dw), stream())
            torch.cuda.synchronize()
            outs.append(dw.cpu().numpy().reshape(shape))
    tag = "%s %s %s %s" % (W.FAMILY_NAMES[r.family] + ("[f32]" if r.dtype != BF16 else ""), W.run_id(r).split("-")[1],
                           r.form, W.epilogue(r) + " x%d" % splits + W.key_suffix(r))
    verify(tag, outs[0], D, W.nterms(r), regime)
    if r.want[3]:   # slabs: one writer per element, the reduction in split order
        assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), tag + ": not the same bits run to run"
        assert bool(torch.isnan(ws[need // 4:]).all()), tag + ": wrote past the workspace it asked for"


@pytest.mark.parametrize("run,regime", _params(W.TILE))
def test_wgrad_kernel(gpu, run, regime):
    """The register-staged tiles 64x64, 64x128, 128x64, 128x128 in bf16 and f32, with the input transform, grouped
    (block-diagonal-skip and plain), with atomics and, under rn_set_tuning 17 = 1, slabs."""
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.DMA64))
def test_wgrad_big_kernel_64x128(gpu, run, regime):
    """The stem's padded channels, rn_set_tuning 5 = 4, and rn_stem_conv_wgrad_p4 over the padded NHWC4 image."""
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.DMA128))
def test_wgrad_big_kernel_128x128(gpu, run, regime):
    """Direct, gathered, stride-2, transform and int8-code forms; atomics and slabs; the FC head without a workspace."""
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.DMA256))
def test_wgrad_big_kernel_256_columns(gpu, run, regime):
    """128- and 256-row K tiles, direct and gathered, transform and int8-code forms, slabs and (rn_set_tuning 5 = 1)
    atomics; the FC head with a workspace."""
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.DBAND))
def test_wgrad_dband_kernel(gpu, run, regime):
    """The three geometries, plain and with the transform, several images per workgroup and a short last split."""
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.GBAND))
def test_wgrad_gband_kernel(gpu, run, regime):
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.STREAM))
def test_wgrad_stream_kernel(gpu, run, regime):
    """The 8 (K, C) pairs in 3 forms at 3 splits with a ragged last one, and one case of 17 splits (the general slab
    reduction by its own rule)."""
    run_wgrad(gpu, run, regime)


@pytest.mark.parametrize("run,regime", _params(W.DEPTHWISE))
def test_dwconv_wgrad_kernel(gpu, run, regime):
    run_wgrad(gpu, run, regime)
