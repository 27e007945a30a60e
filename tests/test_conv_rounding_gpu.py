"""Every bf16 forward and data-gradient convolution kernel held to ONE rounding per element.

include/rn.h promises y = sum (+ bias) (+ add_src), accumulated in fp32 and stored once. Two regimes per kernel:
  gauss: N(0, 1) data rounded to bf16 against the fp64 oracle, every element within gpu_util.rounding_excess <= 1
         (the fp32 accumulation bound for any summation order + half an ulp of the output type: derived, not
         fitted; test_rounding_bar_cpu.py shows it rejects a truncated store and a partial sum kept in bf16 at
         every shape used here -- reductions longer than rounding_cases.MAX_TERMS run the exact regime only);
  exact: ternary / small-integer data whose every partial sum is an integer: the oracle's bits, in any order. The
         first differing (n, p, q, k) names the place.
Each kernel family runs forward, forward + add_src, data gradient, data gradient + add_src into NaN-filled outputs,
after asserting through the host's own answers (rn_conv_tile, rn_conv_fwd_streamed, rn_conv_dgrad_streamed,
d.grouped_direct) that the intended kernel runs. The largest ratio per call is printed (DESIGN.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rounding_cases as R
from rn import lib as L
from gpu_util import BF16, F32, conv_desc, from_nhwc, p, rounding_excess, stream, tdt, to_nhwc, tuning

pytestmark = pytest.mark.gpu

REGIMES = ["gauss", "exact"]
WAYS = ("fwd", "fwd_add", "dgrad", "dgrad_add")
_cid = lambda c: "x".join(map(str, c))


def _master(wt, dev):  # [k][r][s][c / groups] fp32
    return torch.from_numpy(np.ascontiguousarray(wt.transpose(0, 2, 3, 1), dtype=np.float32)).reshape(-1).to(dev)


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=tdt(dtype), device=dev)


def verify(tag, out, nch, ref, sabs, nt, out_dtype, regime):
    """out: the NHWC device tensor, its first nch channels against ref (NCHW, fp64)."""
    if regime == "exact":
        assert np.abs(ref).max() <= R.EXACT_CAP, tag
        o = out[..., :nch].cpu().contiguous()
        want = torch.from_numpy(np.ascontiguousarray(ref.transpose(0, 2, 3, 1))).to(o.dtype)
        iv = torch.int16 if o.dtype == torch.bfloat16 else torch.int32
        same = o.view(iv) == want.view(iv)
        if not bool(same.all()):
            at = tuple(int(v) for v in torch.nonzero(~same)[0])
            raise AssertionError("%s: %d of %d elements differ, first at (n, p, q, k) = %s: got %r, exact %r" % (
                tag, int((~same).sum()), same.numel(), at, float(o[at]), float(want[at])))
        print("rounding", tag, "exact: bit for bit, max |ref| %d" % np.abs(ref).max())
        return
    ex = rounding_excess(from_nhwc(out, nch), ref, sabs, nt, out_dtype)
    print("rounding", tag, "gauss: max ratio %.3f (%d terms)" % (ex.max(), nt))
    if ex.max() > 1.0:
        at = tuple(int(v) for v in np.unravel_index(np.argmax(ex), ex.shape))
        raise AssertionError("%s: %.3g x the allowed error at (n, k, p, q) = %s, %.2f%% of the elements above 1" % (
            tag, ex.max(), at, 100.0 * (ex > 1).mean()))


def make_desc(case, dtype):
    n, c, h, w, k, r, st, pd, g = R.full(case)
    if g == 1:
        return conv_desc(dtype, n, c, h, w, k, r, r, st, pd)
    d = L.ConvDesc(dtype=dtype, n=n, h=h, w=w, c=c, c_real=c, k=k, k_pad=k, r=r, s=r, stride_h=st, stride_w=st,
                   pad_h=pd, pad_w=pd, groups=g)
    L.call("rn_conv_desc_init", C.byref(d))
    return d


def run_conv(gpu, family, case, regime, keys=None, expect=None, dtype=BF16, y_dtype=None, bias=False, ways=WAYS):
    """rn_conv_fwd / rn_conv_bwd_data of `case` under the tuning `keys` (set for the descriptor, the weight copies
    and the launches; restored after), each way checked in `regime`. expect(lib, d): which kernel the host picks."""
    case = R.full(case)
    n, c, h, w, k, r, st, pd, g = case
    y_dtype = dtype if y_dtype is None else y_dtype
    if regime == "gauss":  # (the bar is proven up to MAX_TERMS)
        ways = [wy for wy in ways if R.nterms(case, wy.split("_")[0]) <= R.MAX_TERMS]
    D = R.conv_data(case, regime)
    lib = L.load()
    outs = {}
    with tuning(keys or {}):
        d = make_desc(case, dtype)
        assert (d.p, d.q) == (D["P"], D["Q"])
        if expect is not None:
            expect(lib, d)
        wk = torch.zeros(lib.rn_conv_pack_numel(C.byref(d), 0), dtype=tdt(dtype), device=gpu)
        wc = torch.zeros(lib.rn_conv_pack_numel(C.byref(d), 1), dtype=tdt(dtype), device=gpu)
        master = _master(D["wt"], gpu)
        assert master.numel() == lib.rn_conv_weight_numel(C.byref(d))
        L.call("rn_conv_weight_pack", C.byref(d), p(master), p(wk), p(wc), stream())
        xd, dyd = to_nhwc(D["x"], dtype, gpu, d.c), to_nhwc(D["dy"], dtype, gpu, d.k_pad)
        yad, xad = to_nhwc(D["ya"], y_dtype, gpu, d.k_pad), to_nhwc(D["xa"], dtype, gpu, d.c)
        bd = torch.tensor(D["bias"], dtype=torch.float32, device=gpu) if bias else None
        for way in ways:
            add = way.endswith("_add")
            if way.startswith("fwd"):
                outs[way] = y = _nan((n, d.p, d.q, d.k_pad), y_dtype, gpu)
                L.call("rn_conv_fwd", C.byref(d), p(xd), p(wk), p(y), y_dtype, p(yad) if add else None, p(bd), stream())
            else:
                outs[way] = dx = _nan((n, h, w, d.c), dtype, gpu)
                L.call("rn_conv_bwd_data", C.byref(d), p(dyd), p(wc), p(dx), p(xad) if add else None, stream())
        torch.cuda.synchronize()
    for way, out in outs.items():
        fwd, add = way.startswith("fwd"), way.endswith("_add")
        ref, nch = (D["y"], k) if fwd else (D["dx"], c)
        extra = [D["ya"] if fwd else D["xa"]] * add + [D["bias"][None, :, None, None]] * (fwd and bias)
        sabs = None
        if regime == "gauss":
            sabs = (D["y_sabs"] if fwd else D["dx_sabs"]) + sum(np.abs(e) for e in extra)
        nt = R.nterms(case, "fwd" if fwd else "dgrad") + len(extra)
        verify("%s %s %s" % (family, _cid(case), way), out, nch, ref + sum(extra), sabs, nt,
               y_dtype if fwd else dtype, regime)


def tile_is(lib, d, mode, want):
    got = lib.rn_conv_tile(C.byref(d), mode)
    assert got == want, ("rn_conv_tile", mode, got, want)


# ------------------------------------------------------------------------------------------ igemm_kernel
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", R.CONV_CASES, ids=_cid)
def test_igemm_kernel(gpu, case, dtype, regime):
    """The 128-row kernel (rn_set_tuning 4 = 1: no 256-row tile; rn_conv_tile is 0). The f32 descriptor is fed the
    same bf16-valued data, so its fp32 products are exact too and its output takes the fp32 bar."""
    def expect(lib, d):
        tile_is(lib, d, 0, 0)
        tile_is(lib, d, 1, 0)
        assert lib.rn_conv_fwd_streamed(C.byref(d)) == 0
    run_conv(gpu, "igemm_kernel[%s]" % ("bf16" if dtype == BF16 else "f32"), case, regime, {4: 1}, expect, dtype)


# ------------------------------------------------------------------------------------------ igemm_big_kernel
@pytest.fixture(params=[(0, 0, 512), (0, 0, 8), (1, 0, 0), (1, 1, 512)],
                ids=["rows224", "rows224_persist8", "rows256_mfma32", "rows256_mfma16"])
def tile_variant(request):
    """rn_set_tuning 9 (224-row tiles on / off) x 8 (MFMA shape) x 10 (persistent grid), as test_kernels_gpu's."""
    rows, mfma, persist = request.param
    return {9: rows, 8: mfma, 10: persist}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", [2, 3], ids=["cols256", "cols128"])
@pytest.mark.parametrize("case", R.BIG_CASES, ids=_cid)
def test_igemm_big_kernel(gpu, case, mode, tile_variant, regime):
    """The 256 / 224-row tiles (rn_set_tuning 4 = 2: 256 columns, 3: 128), 64 columns where the output has <= 64."""
    n, c, h, w, k = case[:5]
    def expect(lib, d):
        tile_is(lib, d, 0, 64 if k <= 64 else 256 if mode == 2 else 128)
        tile_is(lib, d, 1, 64 if c <= 64 else 256 if mode == 2 else 128)
    run_conv(gpu, "igemm_big_kernel", case, regime, {**tile_variant, 4: mode}, expect)


@pytest.mark.parametrize("regime", REGIMES)
def test_igemm_big_kernel_four_waves(gpu, regime):
    """rn_set_tuning 11 = 2: the 4-wave one-buffer 224x128 tile on a 1x1 / pad-0 convolution, both directions."""
    def expect(lib, d):
        tile_is(lib, d, 0, 128)
        tile_is(lib, d, 1, 128)
    run_conv(gpu, "igemm_big_kernel[w4]", R.W4_CASE, regime, {11: 2}, expect)


# ------------------------------------------------------------------------------------------ conv3x3c64_band_kernel
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("band", [0, 1], ids=["band", "tile"])
@pytest.mark.parametrize("case", R.BAND_CASES, ids=_cid)
def test_conv3x3c64_band_kernel(gpu, case, band, persist, regime):
    """rn_set_tuning 26 = 0: the image-band kernel for the plain forward and data gradient (the host has no query
    for it: 3x3 / stride 1 / pad 1, 64 -> 64, w <= 56 is its rule in rn.h), 26 = 1: the 64-column tile, which also
    serves the calls with an add_src either way. persist: a batch of 40, several bands per workgroup."""
    if persist:
        case = (R.BAND_PERSIST_N,) + case[1:]
    def expect(lib, d):
        assert (d.c, d.k, d.k_pad, d.r, d.s, d.stride_h, d.pad_h) == (64, 64, 64, 3, 3, 1, 1) and d.w <= 56
        tile_is(lib, d, 0, 64)
        tile_is(lib, d, 1, 64)
    run_conv(gpu, "conv3x3c64_band_kernel" if band == 0 else "igemm_big_kernel[3x3c64]", case, regime, {26: band},
             expect)


# ------------------------------------------------------------------------------------------ the stem
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", [0, 2], ids=["stem_band", "tile"])
@pytest.mark.parametrize("geom", R.STEM_GEOMS, ids=_cid)
def test_stem_conv_fwd_p4(gpu, geom, mode, regime):
    """rn_stem_conv_fwd_p4: stem_band_kernel (rn_set_tuning 26 = 0) and the small-C tile (26 = 2) over the padded
    4-channel image, as test_stem_band lays it out. Forward only."""
    case = R.full(R.stem_case(geom))
    n, c, h, w, k, r, st, pd, g = case
    D = R.conv_data(case, regime)
    d = conv_desc(BF16, n, 8, h, w, k, r, r, st, pd, c_real=c)
    hp = max(h + 2 * pd, (d.p - 1) * st + 8)
    wp = max(w + 2 * pd, (d.q - 1) * st + 8)
    hp, wp = hp + hp % 2, wp + wp % 2
    img = np.zeros((n, hp, wp, 4), np.float32)
    img[:, pd:pd + h, pd:pd + w, :c] = D["x"].transpose(0, 2, 3, 1)
    x4 = torch.tensor(img.reshape(-1), dtype=torch.bfloat16, device=gpu)
    w4 = torch.zeros((k * 256,), dtype=torch.bfloat16, device=gpu)
    L.call("rn_stem_weight_pack_p4", C.byref(d), p(_master(D["wt"], gpu)), p(w4), stream())
    lib = L.load()
    with tuning({26: mode}):
        assert (d.stride_h, d.k, d.k_pad) == (2, 64, 64) and wp % 2 == 0 and wp <= 232 and d.q <= 112  # the band's rule
        tile_is(lib, d, 0, 64)  # (the tile it falls back to)
        y = _nan((n, d.p, d.q, d.k_pad), BF16, gpu)
        L.call("rn_stem_conv_fwd_p4", C.byref(d), p(x4), p(w4), p(y), hp, wp, stream())
        torch.cuda.synchronize()
    verify("%s %s fwd" % ("stem_band_kernel" if mode == 0 else "igemm_big_kernel[stem]", _cid(case)), y, k, D["y"],
           D.get("y_sabs"), R.nterms(case, "fwd"), BF16, regime)


# ------------------------------------------------------------------------------------------ fwd1x1_stream_kernel
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("key", [0, 2, 3, 1], ids=["default", "cpw32", "every_form", "tile"])
@pytest.mark.parametrize("case", R.FWD_STREAM_CASES, ids=_cid)
def test_fwd1x1_stream_kernel(gpu, case, key, regime):
    """rn_conv_fwd_x plain, with the residual, with the BatchNorm+ReLU on load, with both (rn_set_tuning 29; 1: the
    224-row tile these forms are bit-compared with elsewhere). The transformed operand is what the kernel stages:
    bf16(max(fmaf(x, sc, sh), 0))."""
    case = R.full(case)
    n, c, h, w, k, r, st, pd, g = case
    D = R.conv_data(case, regime)
    rng = np.random.default_rng(61)
    if regime == "gauss":
        sc = rng.uniform(0.5, 1.5, c).astype(np.float32).astype(np.float64)
        sh = (rng.standard_normal(c) * 0.5).astype(np.float32).astype(np.float64)
    else:  # x in {-1, 0, 1} -> {0, 1, 2, 3}: integers still
        sc, sh = rng.integers(1, 3, c).astype(np.float64), rng.integers(-1, 2, c).astype(np.float64)
    xa = R.bnrelu_operand(D["x"], sc, sh)
    y_xf = R.conv_fwd64(xa, D["wt"], 1, 0)
    sabs_xf = R.conv_fwd64(xa, np.abs(D["wt"]), 1, 0) if regime == "gauss" else None
    lib = L.load()
    outs = {}
    with tuning({29: key}):
        d = make_desc(case, BF16)
        assert lib.rn_conv_fwd_streamed(C.byref(d)) == (0 if key == 1 else 1)
        assert lib.rn_conv_tile(C.byref(d), 0) >= 128  # (the tile of key 1, and of the plain Cin = 128 form by default)
        wk = torch.zeros(lib.rn_conv_pack_numel(C.byref(d), 0), dtype=torch.bfloat16, device=gpu)
        L.call("rn_conv_weight_pack", C.byref(d), p(_master(D["wt"], gpu)), p(wk), None, stream())
        xd, rd = to_nhwc(D["x"], BF16, gpu), to_nhwc(D["ya"], BF16, gpu)
        f = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
        scd, shd = f(sc), f(sh)
        for form in ("plain", "res", "xf", "xf_res"):
            xf, add = form.startswith("xf"), form.endswith("res")
            outs[form] = y = _nan((n, h, w, k), BF16, gpu)
            L.call("rn_conv_fwd_x", C.byref(d), p(xd), p(wk), p(y), BF16, p(rd) if add else None, None,
                   p(scd) if xf else None, p(shd) if xf else None, None, stream())
        torch.cuda.synchronize()
    for form, y in outs.items():
        xf, add = form.startswith("xf"), form.endswith("res")
        # (rn.h, key 29: by default the plain Cin = 128 form stays on its tile; 2 and 3 stream every form)
        streamed = key != 1 and (key >= 2 or c == 64 or form != "plain")
        fam = "fwd1x1_stream_kernel" if streamed else "igemm_big_kernel[1x1 expand]"
        ref = (y_xf if xf else D["y"]) + (D["ya"] if add else 0)
        sabs = None if regime == "exact" else (sabs_xf if xf else D["y_sabs"]) + (np.abs(D["ya"]) if add else 0)
        verify("%s %s %s" % (fam, _cid(case), form), y, k, ref, sabs, c + add, BF16, regime)


# ------------------------------------------------------------------------------------------ dgrad1x1_stream_kernel
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("key", [0, 2, 1], ids=["cpw64", "cpw32", "tile"])
@pytest.mark.parametrize("case", R.DGRAD_STREAM_CASES, ids=_cid)
def test_dgrad1x1_stream_kernel(gpu, case, key, regime):
    """rn_conv_bwd_data_bnred in its reduce / reduce_add forms (the stored dx is the plain data gradient (+ add_src);
    the BN-backward partials are test_dgrad1x1_stream's subject), rn_set_tuning 27; 1: the 224-row tile."""
    case = R.full(case)
    n, c, h, w, k, r, st, pd, g = case
    D = R.conv_data(case, regime)
    rng = np.random.default_rng(51)
    lib = L.load()
    outs = {}
    with tuning({27: key}):
        d = make_desc(case, BF16)
        assert lib.rn_conv_dgrad_streamed(C.byref(d)) == (0 if key == 1 else 1)
        assert lib.rn_conv_tile(C.byref(d), 1) >= 128
        wc = torch.zeros(lib.rn_conv_pack_numel(C.byref(d), 1), dtype=torch.bfloat16, device=gpu)
        L.call("rn_conv_weight_pack", C.byref(d), p(_master(D["wt"], gpu)), None, p(wc), stream())
        f = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float32, device=gpu)
        mean, sc, sh = f(rng.standard_normal(c) * 0.2), f(rng.uniform(0.5, 1.5, c)), f(rng.standard_normal(c) * 0.3)
        xbd, dyd, xad = to_nhwc(D["x"], BF16, gpu), to_nhwc(D["dy"], BF16, gpu), to_nhwc(D["xa"], BF16, gpu)
        nrb = lib.rn_conv_bnred_blocks(C.byref(d))
        assert nrb == -(-n * h * w // 224)
        for form in ("reduce", "reduce_add"):
            part = torch.full((nrb * d.c * 2,), float("nan"), dtype=torch.float32, device=gpu)
            outs[form] = dx = _nan((n, h, w, d.c), BF16, gpu)
            L.call("rn_conv_bwd_data_bnred", C.byref(d), p(dyd), p(wc), p(dx), p(xad) if form == "reduce_add" else None,
                   p(xbd), p(mean), p(sc), p(sh), 1, p(part), stream())
            torch.cuda.synchronize()
            assert not torch.isnan(part).any()
    fam = "igemm_big_kernel[1x1 dgrad bnred]" if key == 1 else "dgrad1x1_stream_kernel"
    for form, dx in outs.items():
        add = form == "reduce_add"
        ref = D["dx"] + (D["xa"] if add else 0)
        sabs = None if regime == "exact" else D["dx_sabs"] + (np.abs(D["xa"]) if add else 0)
        verify("%s %s %s" % (fam, _cid(case), form), dx, c, ref, sabs, k + add, BF16, regime)


# ------------------------------------------------------------------------------------------ grouped
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("skip", [0, 1], ids=["zero_block_skip", "every_block"])
@pytest.mark.parametrize("case", R.GCONV_CASES, ids=_cid)
def test_grouped_block_diagonal_tiles(gpu, case, skip, regime):
    """rn_set_tuning 15 = 1 at rn_conv_desc_init: the block-diagonal 64-column tiles (13 = 1: the MFMAs of the zero
    blocks too)."""
    def expect(lib, d):
        assert d.grouped_direct == 0
        assert lib.rn_conv_pack_numel(C.byref(d), 0) > lib.rn_conv_weight_numel(C.byref(d)) or d.c // d.groups >= 64
    run_conv(gpu, "igemm[block-diagonal]", case, regime, {15: 1, 13: skip}, expect)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", R.GROUPED_DIRECT_CASES, ids=_cid)
def test_grouped_direct_kernels(gpu, case, regime):
    """rn_set_tuning 15 = 0: grouped_direct_kernel and, at stride 2, grouped_dgrad_s2_kernel (4 per group, 8 per
    group at stride 2): d.grouped_direct = 1, the compact weight copies, no tile."""
    n, c = case[:2]
    def expect(lib, d):
        assert d.grouped_direct == 1
        for which in (0, 1):
            assert lib.rn_conv_pack_numel(C.byref(d), which) == c * 9 * (c // d.groups)
            tile_is(lib, d, which, 0)
    run_conv(gpu, "grouped_direct_kernel" if case[6] == 1 else "grouped_direct_kernel / grouped_dgrad_s2_kernel",
             case, regime, {15: 0}, expect)


# ------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("off", [0, 1], ids=["dwconv", "blockdiag"])
@pytest.mark.parametrize("case", R.DEPTHWISE_CASES, ids=_cid)
def test_depthwise_kernels(gpu, case, off, regime):
    """dwconv_fwd_kernel / dwconv_dgrad_kernel (d.grouped_direct = 2), and the same descriptors on the
    block-diagonal tiles (rn_set_tuning 28 = 1 at rn_conv_desc_init)."""
    def expect(lib, d):
        assert d.grouped_direct == (0 if off else 2)
        assert lib.rn_conv_pack_numel(C.byref(d), 0) == (64 if off else 1) * 9 * d.c
    run_conv(gpu, "igemm[depthwise block-diagonal]" if off else "dwconv_fwd_kernel / dwconv_dgrad_kernel", case, regime,
             {28: off}, expect)


# ------------------------------------------------------------------------------------------ the FC head
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("det", [0, 1], ids=["splitk_atomics", "deterministic"])
@pytest.mark.parametrize("case", R.FC_CASES, ids=_cid)
def test_fc_head_logits(gpu, case, det, regime):
    """A 1x1 convolution over a 1x1 image with a bias, fp32 logits from a bf16 descriptor (igemm_kernel; split-K
    with fp32 atomics for the 2048-deep reduction unless rn_set_tuning 17 = 1), without and with an fp32 add_src."""
    def expect(lib, d):
        assert (d.h, d.w, d.p, d.q) == (1, 1, 1, 1)
    run_conv(gpu, "igemm_kernel[fc %s]" % ("deterministic" if det else "split-K"), case, regime, {17: det}, expect,
             y_dtype=F32, bias=True, ways=("fwd", "fwd_add"))
