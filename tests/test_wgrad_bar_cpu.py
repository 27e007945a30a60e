"""The weight-gradient bar of test_wgrad_rounding_gpu.py, checked without a GPU.

Route: for every run of wgrad_cases.RUNS, rn_conv_wgrad_kernel (no launch, no device) answers the intended family,
tile, epilogue and split count -- >= 3 splits with a ragged last one where a seam is meant, <= 16 where the
few-split reduction is meant, 17 for the stream case that must pass it (split counts for 256 CUs only: that part
skips itself on another chip; the GPU file repeats the assertion).
Exact regime: the oracle's dW + prefill is an integer array below 2^24, mostly nonzero, and every simulated mistake
changes its bits: a zeroed first row, last row, row on either side of every split seam, the last split added twice
or left out, one split's partial rounded to bf16 (at least a tenth of the elements).
Gauss regime: for every gauss shape, a simulated correct result (fp32 partials per split, their fp32 sum, the add
into dW) stays at or below 1 under gpu_util.rounding_excess, a dropped row and a partial kept in bf16 exceed it.
Every family keeps a gauss shape; the exact regime leaves out no run."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_cases as W
from gpu_util import BF16, F32, bf16_round, rounding_excess, tuning
from oracle import ops
from rn import lib as L


# ---------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("run", W.RUNS, ids=W.run_id)
def test_route(run):
    lib = L.load()
    with tuning(run.keys):
        d = W.make_desc(run)
        assert (d.p, d.q) == W.out_hw(run.case)
        splits = W.check_route(lib, d, run)
    if isinstance(run.splits, int) and lib.rn_device_cu_count() in (-1, 0, 256):
        assert splits == run.splits


def test_route_covers_what_the_issue_lists():
    """Every family has an exact run in each epilogue it has and with both slab reductions; multi-split runs exist
    for every family whose splits are over M; one run passes 16 splits."""
    for fam in W.FAMILIES:
        runs = W.runs_of(fam)
        slabs = [r for r in runs if r.form != "stem" and r.want[3]]
        assert slabs and any(r.keys.get(25) == 1 for r in slabs) and any(r.keys.get(25) != 1 for r in slabs), fam
        if fam in (W.TILE, W.DMA64, W.DMA128, W.DMA256):
            assert any(r.form != "stem" and not r.want[3] for r in runs), fam   # atomics
        if fam != W.DEPTHWISE:
            assert any(isinstance(r.splits, int) and r.splits >= 3 for r in runs), fam
        assert any(r.gauss for r in runs), fam
    assert any(r.splits == 17 for r in W.runs_of(W.STREAM))
    assert {r.form for r in W.RUNS} == {"plain", "xf", "i8", "stem"}
    assert {(r.want[1], r.want[2]) for r in W.runs_of(W.TILE)} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {(r.want[1], r.want[2]) for r in W.runs_of(W.DMA256)} == {(128, 256), (256, 256)}


def test_query_refusals_leave_the_last_error():
    """-1 where the launch would be refused (deterministic mode without a workspace, int8 codes on an unsupported
    shape, a depthwise gradient without its slab), the out-parameters and rn_last_error untouched; a workspace too
    small for the stream kernel's slab falls through to the tile it would launch."""
    lib = L.load()
    assert lib.rn_set_tuning(3, 1) == -1   # (a known message to find again)
    before = lib.rn_last_error()
    sp, sl = C.c_int32(-7), C.c_int32(-7)
    q = lambda d, xf, i8, ws: lib.rn_conv_wgrad_kernel(C.byref(d), xf, i8, ws, C.byref(sp), C.byref(sl))
    r = W.Run(W.STREAM, W.full((3, 64, 17, 15, 64, 1, 1, 0)), "plain", BF16, {}, True, None, None, None, False)
    d = W.make_desc(r)
    with tuning({17: 1}):
        assert q(d, 0, 0, 0) == -1
    i8bad = W.make_desc(r._replace(case=W.full((2, 256, 8, 8, 64, 1, 2, 0))))
    assert q(i8bad, 0, 1, 1 << 30) == -1
    dw = W.make_desc(r._replace(case=(2, 32, 9, 11, 32, 3, 1, 1, 32)))
    assert q(dw, 0, 0, 0) == -1 and q(dw, 0, 0, 8) == -1
    assert lib.rn_conv_wgrad_kernel(None, 0, 0, 0, None, None) == -1 and q(d, 0, 0, -1) == -1
    assert (sp.value, sl.value) == (-7, -7) and lib.rn_last_error() == before
    need = lib.rn_conv_wgrad_ws_bytes(C.byref(d))
    assert q(d, 0, 0, need) & 0xff == W.STREAM and sl.value == 1
    if lib.rn_device_cu_count() in (-1, 0, 256):
        assert sp.value == 3 and need == 3 * 64 * 64 * 4
        assert q(d, 0, 0, need - 4) & 0xff == W.STREAM and sp.value == 2   # no more splits than the workspace holds
    v = q(d, 0, 0, 64 * 64 * 4 - 4)   # not one slab: wgrad_kernel with atomics
    assert (v & 0xff, (v >> 8) & 0xfff, v >> 20, sl.value) == (W.TILE, 64, 64, 0)
    assert lib.rn_conv_wgrad_kernel(C.byref(d), 0, 0, need, None, None) & 0xff == W.STREAM   # nullable outputs


# ---------------------------------------------------------------------------------------------- oracle
def test_torch_oracle_is_the_numpy_oracle():
    """dw64 (torch, float64) against oracle.ops.conv2d_bwd on a strided, padded, grouped shape, both regimes."""
    case = (2, 16, 9, 7, 24, 3, 2, 1, 4)
    for regime in ("gauss", "exact"):
        D = W.wgrad_data(case, "plain", regime)
        dw = ops.conv2d_bwd(D["x"], np.zeros((24, 4, 3, 3)), D["dy"], (2, 2), (1, 1), 4)[1]
        if regime == "exact":
            assert np.array_equal(D["sum"], dw)
        else:
            assert np.abs(D["sum"] - dw).max() < 1e-12


# ---------------------------------------------------------------------------------------------- exact regime
def _mistake_keys():
    seen = {}
    for r in W.RUNS:
        s = r.splits if isinstance(r.splits, int) else 1
        seen.setdefault((r.case, r.form, r.c_real, W.rows_per_split(r, s) if s > 1 else W.rows_m(r.case)), None)
    return list(seen)


def _row_mask(D, case, lo, hi):
    """dy with only the rows lo <= m < hi of M = (n, p, q) kept."""
    n, k = D["dy"].shape[:2]
    keep = np.zeros(n * D["P"] * D["Q"], dtype=bool)
    keep[lo:hi] = True
    return D["dy"] * keep.reshape(n, 1, D["P"], D["Q"])


_kid = lambda t: "%s%s-%s-per%d" % ("x".join(map(str, t[0])), "" if t[2] is None else "-creal%d" % t[2], t[1], t[3])


@pytest.mark.parametrize("key", _mistake_keys(), ids=_kid)
def test_exact_regime_rejects_mistakes(key):
    case, form, c_real, mps = key
    D = W.wgrad_data(case, form, "exact")
    M = W.rows_m(case)
    unit = D["unit"] if form == "i8" else 1.0
    ref = D["ref"]
    # the cap: integers (over the unit) below 2^24, not trivially small
    assert np.array_equal(D["sum"], np.round(D["sum"])) and np.array_equal(D["dw0"], np.round(D["dw0"]))
    assert np.abs(D["sum"]).max() + 3 < W.EXACT_CAP
    assert np.abs(W.dw64(np.abs(D["xo"]), np.abs(D["dy"]), case)).max() + 3 < W.EXACT_CAP   # every partial too
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    assert (ref != 0).mean() > 0.5
    part = lambda lo, hi: unit * W.dw64(D["xo"], _row_mask(D, case, lo, hi), case)
    seams = [j * mps for j in range(1, -(-M // mps))]
    rows = sorted({0, M - 1} | set(seams) | {s - 1 for s in seams})
    for m in rows:   # one row zeroed
        assert np.any(part(m, m + 1) != 0), ("row", m)
    last = part(seams[-1] if seams else 0, M)
    assert np.any(last != 0)   # added twice or left out
    first = part(0, mps)
    changed = bf16_round(first) != first
    print("exact", _kid(key), "max |sum| %d, a bf16 partial changes %.0f%% of the elements" % (
        np.abs(D["sum"]).max(), 100 * changed.mean()))
    assert changed.mean() >= 0.1


# ---------------------------------------------------------------------------------------------- gauss regime
def _split_masks(D):
    """dy cut into partial sums as a kernel's splits would: by image, or by halves of an only image's rows."""
    n, k, P, Q = D["dy"].shape
    if n > 1:
        cuts = [(i, i + 1, 0, P) for i in range(n)]
    else:
        cuts = [(0, 1, 0, (P + 1) // 2), (0, 1, (P + 1) // 2, P)]
    for a, b, p0, p1 in cuts:
        m = np.zeros((n, 1, P, Q))
        m[a:b, :, p0:p1] = 1
        yield m


def _dw32(x, dy, case):
    n, c, h, w, k, r, st, pd, g = W.full(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return torch.nn.grad.conv2d_weight(t(x), (k, c // g, r, r), t(dy), stride=st, padding=pd, groups=g)


@pytest.mark.parametrize("key", W.GAUSS_KEYS, ids=lambda t: _kid(t + (0,)))
def test_gauss_bar_separates(key):
    case, form, c_real = key
    assert W.rows_m(case) <= 600
    D = W.wgrad_data(case, form, "gauss")
    nt = W.rows_m(case) + 1 + (form == "i8")
    unit = torch.tensor(D["unit"] if form == "i8" else 1.0, dtype=torch.float32)
    dw0 = torch.from_numpy(D["dw0"].astype(np.float32))
    parts = [_dw32(D["xo"], D["dy"] * m, case) for m in _split_masks(D)]
    assert len(parts) >= 2
    total = lambda ps: dw0 + unit * sum(ps[1:], ps[0])
    dropped = np.array(D["dy"])
    dropped[-1, :, -1, -1] = 0    # the last row of M
    dparts = [_dw32(D["xo"], dropped * m, case) for m in _split_masks(D)]
    outs = dict(correct=total(parts), dropped_row=total(dparts),
                bf16_partial=total([parts[0].to(torch.bfloat16).float()] + parts[1:]))
    ex = {k: rounding_excess(v.numpy(), D["ref"], D["sabs"], nt, F32) for k, v in outs.items()}
    print("bar", _kid(key + (0,)), "terms", nt, {k: "max %.3g" % v.max() for k, v in ex.items()})
    assert ex["correct"].max() <= 1.0
    assert ex["dropped_row"].max() > 1.0
    assert ex["bf16_partial"].max() > 1.0


def test_exact_regime_leaves_out_no_run():
    """The GPU file runs every Run exact; gauss is the subset proven above."""
    assert {(r.case, r.form, r.c_real) for r in W.RUNS} == set(W.DATA_KEYS)
    assert set(W.GAUSS_KEYS) <= set(W.DATA_KEYS)
    # the shape lists the runs are drawn from, restated here: none of their shapes is left out of either regime
    from test_depthwise_gpu import CASES as dw_cases
    from test_kernels_gpu import BIG_CASES, CONV_CASES, GCONV_CASES
    named = [W.full(c) for c in CONV_CASES + GCONV_CASES + [c for c in BIG_CASES if W.rows_m(W.full(c)) <= 600]]
    named += [(3, c, 13, 11, k, 1, 1, 0, 1) for k, c in W.STREAM_KC]
    named += [(n, c, h, w, c, 3, st, 1, c) for n, c, h, w, st in dw_cases]
    plain = {r.case for r in W.RUNS if r.form == "plain"}
    gauss = {r.case for r in W.RUNS if r.form == "plain" and r.gauss}
    for case in named:
        assert case in plain, case
        assert case in gauss or W.rows_m(case) > 600, case   # (the 56 x 56 depthwise map: exact only)


def test_f32_bar_edges():
    """What test_rounding_bar_cpu.test_bar_edges leaves of the fp32-output bar: a zero sum over zero terms allows
    only zero, NaN never passes, a power of two takes its own half fp32 ulp, and the allowance grows with nterms."""
    z = np.zeros(3)
    ex = rounding_excess(np.array([0.0, 1e-38, np.nan]), z, z, 100, F32)
    assert ex[0] == 0 and ex[1] == np.inf and ex[2] == np.inf
    assert rounding_excess(np.array([1.0 + 2.0 ** -24]), np.array([1.0]), np.zeros(1), 100, F32)[0] == 1.0
    assert rounding_excess(np.array([1.0 - 2.0 ** -24]), np.array([1.0]), np.zeros(1), 100, F32)[0] == 1.0
    few, many = (rounding_excess(np.array([1.0 + 2.0 ** -16]), np.array([1.0]), np.array([8.0]), n, F32)[0]
                 for n in (8, 1518))
    assert few > 1.0 > many
