"""QIL on the MI355X: rn_qil_fwd / rn_qil_bwd / rn_weight_qil_pack / rn_weight_qil_bwd / rn_sgd_mom_update*_lrm
against their numpy float32 restatements (tests/qil_util.py), a training step of a small QIL network against the
fp64 restatement replaying the device's own discrete decisions, the reference route (attach_quantize_node with
"QIL", training, checkpoint), and every kernel of a step of a two-units-per-stage QIL network layer by layer
(tests/layerwise.py, tests/qil_layerwise.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxnet as mx
import qil_util as U
from gpu_util import BF16, F32, p, stream, tdt
from rn import lib as L

pytestmark = pytest.mark.gpu

# 16: one code chunk; 4160 = 16 * 260: more than one block of the codes kernel; 1001 * 48: many blocks (a multiple
# of 16 too), two grid-stride rounds of the fp32 backward; + 3: a tail that is no multiple of either chunk size.
# The grids' caps (8192 blocks forward, 2048 backward) are passed once each in test_beyond_the_grid_caps
SIZES = [16, 4160, 1001 * 48, 1001 * 48 + 3]
DTYPES = [F32, BF16]
POINTS = [(0.25, 0.75), (0.0, 1.0)]
SHAPE = (2, 3, 16, 16)


def _store(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(tdt(dtype)).to(dev)


def _load(t):
    return t.float().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fwd(dev, dtype, x, pp, cc, nbits, want_codes, want_out=True):
    n = x.size
    xd = _store(x, dtype, dev)
    pc = torch.tensor([77.0, pp, 77.0, cc, 77.0], dtype=torch.float32, device=dev)
    out = torch.full((n,), 77.0, dtype=tdt(dtype), device=dev) if want_out else None
    codes = torch.full((n,), -9, dtype=torch.int8, device=dev) if want_codes else None
    unit = torch.zeros(1, dtype=torch.float32, device=dev)
    rc = L.load().rn_qil_fwd(dtype, n, p(xd), C.c_void_p(pc.data_ptr() + 4), C.c_void_p(pc.data_ptr() + 12), nbits,
                             p(out), p(codes), p(unit), stream())
    torch.cuda.synchronize()
    pcv = _load(pc)
    assert (pcv[[0, 2, 4]] == 77.0).all()  # (the parameters' neighbours)
    return rc, out, codes, unit, pcv[1], pcv[3]


# ----------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("pc", POINTS)
@pytest.mark.parametrize("nbits", [1, 4, 7, 8])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_bit_for_bit(gpu, dtype, n, nbits, pc):
    """Values, and with nbits <= 7 and n a multiple of 16 the codes, bit for bit against the float32 restatement;
    the three forms (values only, codes only, both) agree."""
    pp, cc = pc
    x = U.edge_inputs(n, dtype == BF16, pp, cc, seed=n + nbits)
    a = np.abs(x)
    for sgn in (x > 0, x < 0):
        assert (sgn & (a == f32(cc))).any() and (sgn & (a > f32(cc))).any()
        assert (sgn & (a == f32(pp))).any() or pp == 0
    if pp > 0:
        assert ((a < f32(pp)) & (a > 0)).any()
        assert (x == 0.5).any() and (x == -0.5).any()
    assert (x == 0).any()  # (with p == 0: x == 0 inside the interval)
    want, wq, wunit, _, _ = U.qil_fwd_ref(x, pp, cc, nbits, to_bf16=dtype == BF16)
    assert np.abs(want).max() == 1.0 and wq.max() == 2 ** nbits - 1 and wq.min() == -(2 ** nbits - 1)
    if nbits == 1 and pp > 0:  # the one exact tie: half away gives +-1, half even would give 0
        assert (wq[x == 0.5] == 1).all() and (wq[x == -0.5] == -1).all()
    rc, out, _, u, p1, c1 = _fwd(gpu, dtype, x, pp, cc, nbits, want_codes=False)
    assert rc == 0 and (p1, c1) == (f32(pp), f32(cc))
    assert np.array_equal(_bits(_load(out)), _bits(want))
    assert _load(u)[0] == wunit == f32(1) / f32(2 ** nbits - 1)
    if nbits <= 7 and n % 16 == 0:
        rc, out2, codes, u2, _, _ = _fwd(gpu, dtype, x, pp, cc, nbits, want_codes=True)
        assert rc == 0 and torch.equal(out, out2) and _load(u2)[0] == wunit
        assert np.array_equal(codes.cpu().numpy(), wq.astype(np.int8))
        rc, _, codes3, _, _, _ = _fwd(gpu, dtype, x, pp, cc, nbits, want_codes=True, want_out=False)
        assert rc == 0 and torch.equal(codes, codes3)


f32 = np.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_clamps_the_parameters(gpu, dtype):
    n = 4160
    x = U.edge_inputs(n, dtype == BF16, 0.0, 1.0, seed=9)
    rc, out, codes, _, p1, c1 = _fwd(gpu, dtype, x, -0.5, 1.5, 4, want_codes=True)
    assert rc == 0 and p1 == 0.0 and c1 == 1.0 and not np.signbit(p1)
    rc, out2, codes2, _, _, _ = _fwd(gpu, dtype, x, 0.0, 1.0, 4, want_codes=True)
    assert torch.equal(out, out2) and torch.equal(codes, codes2)
    assert np.array_equal(_bits(_load(out)), _bits(U.qil_fwd_ref(x, -0.5, 1.5, 4, to_bf16=dtype == BF16)[0]))


def test_forward_codes_refusals(gpu):
    x = U.edge_inputs(4160, False, 0.25, 0.75, seed=1)
    rc, out, codes, _, _, _ = _fwd(gpu, F32, x, 0.25, 0.75, 8, want_codes=True)
    assert rc == -1 and b"nbits <= 7" in L.load().rn_last_error()
    assert (codes.cpu().numpy() == -9).all() and (_load(out) == 77.0).all()  # nothing was launched
    rc, out, codes, _, _, _ = _fwd(gpu, F32, x[:4150], 0.25, 0.75, 4, want_codes=True)
    assert rc == -1 and b"multiple of 16" in L.load().rn_last_error()
    assert (codes.cpu().numpy() == -9).all() and (_load(out) == 77.0).all()


# ----------------------------------------------------------------------------- 2. backward
def _bwd(dev, dtype, x, dy, pp, cc, add=None, alias=False):
    lib = L.load()
    n = x.size
    xd, dyd = _store(x, dtype, dev), _store(dy, dtype, dev)
    addd = _store(add, dtype, dev) if add is not None else None
    dx = dyd if alias else torch.full((n,), 55.0, dtype=tdt(dtype), device=dev)
    pc = torch.tensor([pp, cc], dtype=torch.float32, device=dev)
    dg = torch.full((5,), 123.0, dtype=torch.float32, device=dev)  # (written, not accumulated; neighbours untouched)
    nws = int(lib.rn_qil_bwd_ws_bytes(n))
    assert nws == 2 * 4 * min(max(-(-n // 2048), 1), 2048)
    ws = torch.full((nws // 4 + 1,), -1.0, dtype=torch.float32, device=dev)
    rc = lib.rn_qil_bwd(dtype, n, p(xd), p(dyd), p(pc), C.c_void_p(pc.data_ptr() + 4), p(dx), p(addd),
                        C.c_void_p(dg.data_ptr() + 4), C.c_void_p(dg.data_ptr() + 12), p(ws), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.rn_last_error()
    dgv = _load(dg)
    assert (dgv[[0, 2, 4]] == 123.0).all() and _load(ws)[-1] == -1.0
    assert np.array_equal(_load(pc), np.array([pp, cc], dtype=np.float32))  # (read only)
    return _load(dx), dgv[1], dgv[3]


def _check_sums(n, itemsize, got, want, tag):
    """|fp32 sum - exact sum| <= (k + m) * 2^-24 * sum |terms|: k the longest chain of fp32 additions a term passes
    through (qil_util.qil_bwd_chain, from the launch geometry), m = 6 the fp32 roundings of one term and of the scale
    (qil_util.QIL_TERM_ROUNDINGS: the difference 1, the product 1, c - p twice as it enters squared, the square 1,
    the division 1; dy * s is exact). First order in 2^-24."""
    k = U.qil_bwd_chain(n, itemsize)
    for name, g, (w, asum) in zip(("dp", "dc"), got, want):
        bound = (k + U.QIL_TERM_ROUNDINGS) * 2.0 ** -24 * asum
        print("%s n %d: %s %.9g, fp64 %.9g, |diff| %.3g, bound %.3g (k = %d)" % (tag, n, name, g, w,
                                                                                 abs(float(g) - w), bound, k))
        assert asum > 0 and abs(float(g) - w) <= bound, (name, g, w, bound)


@pytest.mark.parametrize("pc", POINTS)
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward(gpu, dtype, n, with_add, pc):
    pp, cc = pc
    rng = np.random.RandomState(n + 7 * with_add)
    x = U.edge_inputs(n, dtype == BF16, pp, cc, seed=n)
    rd = (lambda a: U.bf16(a)) if dtype == BF16 else (lambda a: a)
    dy = rd(rng.randn(n).astype(np.float32))
    add = rd(rng.randn(n).astype(np.float32)) if with_add else None
    dx, dp, dc = _bwd(gpu, dtype, x, dy, pp, cc, add)
    want_dx, wp, wc, ap, ac = U.qil_bwd_ref(x, dy, pp, cc, add, to_bf16=dtype == BF16)
    assert np.array_equal(_bits(dx), _bits(want_dx))
    _check_sums(n, 2 if dtype == BF16 else 4, (dp, dc), ((wp, ap), (wc, ac)), "dtype %d" % dtype)
    if not with_add:  # the restatement's sums are QIL.py's autograd (fp64, from the same float32 inputs)
        ref = U.qil_fp64(x, pp, cc, 4, dy=dy)
        assert abs(ref["dp"] - wp) <= 1e-9 * max(ap, 1) and abs(ref["dc"] - wc) <= 1e-9 * max(ac, 1)
        inside = (np.abs(x) >= f32(pp)) & (np.abs(x) <= f32(cc)) & (x != 0)
        assert np.array_equal(ref["dx"] != 0, inside & (dy != 0))
    dx2, dp2, dc2 = _bwd(gpu, dtype, x, dy, pp, cc, add)  # bit-reproducible from run to run
    assert np.array_equal(_bits(dx2), _bits(dx)) and _bits(dp2) == _bits(dp) and _bits(dc2) == _bits(dc)


def test_backward_chain_lengths():
    """The bound's k, by hand: n = 16 fp32 is 4 chunks on 4 threads of one block: 4 serial adds + 6 + 2, one
    partial in one lane; n = 48051 bf16 is 24 blocks, 6006 chunks on 6144 threads (one round of 8) and a 3-element
    tail, 24 partials in one lane; the capped grid: 2048 partials, 32 in each of 64 lanes."""
    assert U.qil_bwd_chain(16, 4) == 4 + 6 + 2 + 1 + 1
    assert U.qil_bwd_chain(1001 * 48 + 3, 2) == 8 + 1 + 6 + 2 + 24 + 1
    assert U.qil_bwd_chain(2048 * 2048 * 8, 2) == 8 * 8 + 6 + 2 + 32 + 64


def test_backward_in_place_and_whole_interval(gpu):
    n = 1001 * 48 + 3
    rng = np.random.RandomState(11)
    for dtype in DTYPES:
        x = U.edge_inputs(n, dtype == BF16, 0.25, 0.75, seed=5)
        dy = rng.randn(n).astype(np.float32)
        dy = U.bf16(dy) if dtype == BF16 else dy
        dx, dp, dc = _bwd(gpu, dtype, x, dy, 0.25, 0.75, alias=True)  # dx aliases dy
        want_dx, wp, wc, ap, ac = U.qil_bwd_ref(x, dy, 0.25, 0.75, to_bf16=dtype == BF16)
        assert np.array_equal(_bits(dx), _bits(want_dx))
        _check_sums(n, 2 if dtype == BF16 else 4, (dp, dc), ((wp, ap), (wc, ac)), "aliased")
        # c above every |x| and p = 0: dx == dy * alpha at every x != 0 (and 0 at x == 0: sign has no gradient)
        xs = (x * f32(0.5)).astype(np.float32)
        assert np.abs(xs).max() < 1.0
        dx, _, _ = _bwd(gpu, dtype, xs, dy, 0.0, 1.0)
        alpha = U.qil_coef_ref(0.0, 1.0)[2]
        full = (dy * alpha).astype(np.float32)
        full = U.bf16(full) if dtype == BF16 else full
        assert alpha == 1.0 and np.array_equal(dx[xs != 0], full[xs != 0]) and not dx[xs == 0].any()
        assert (xs == 0).any()


def test_beyond_the_grid_caps(gpu):
    """Sizes at which the capped grids stride more than once (the only other path of the kernels): the fp32 values
    forward past 8192 * 256 chunks of 4, the bf16 codes forward past 8192 * 256 chunks of 16, the bf16 backward
    past 2048 * 256 chunks of 8 (where the chains of dp / dc are their longest per thread)."""
    pp, cc, nbits = 0.25, 0.75, 4
    n = 8192 * 256 * 4 + 4 * 300 + 1
    x = U.edge_inputs(n, False, pp, cc, seed=2)
    rc, out, _, _, _, _ = _fwd(gpu, F32, x, pp, cc, nbits, want_codes=False)
    assert rc == 0 and np.array_equal(_bits(_load(out)), _bits(U.qil_fwd_ref(x, pp, cc, nbits)[0]))
    n = 8192 * 256 * 16 + 16 * 5
    x = U.edge_inputs(n, True, pp, cc, seed=3)
    rc, out, codes, _, _, _ = _fwd(gpu, BF16, x, pp, cc, nbits, want_codes=True)
    want, wq, _, _, _ = U.qil_fwd_ref(x, pp, cc, nbits, to_bf16=True)
    assert rc == 0 and np.array_equal(_bits(_load(out)), _bits(want))
    assert np.array_equal(codes.cpu().numpy(), wq.astype(np.int8))
    n = 2048 * 256 * 8 * 2 + 8 * 77 + 5
    x = x[:n]
    dy = U.bf16(np.random.RandomState(4).randn(n).astype(np.float32))
    dx, dp, dc = _bwd(gpu, BF16, x, dy, pp, cc)
    want_dx, wp, wc, ap, ac = U.qil_bwd_ref(x, dy, pp, cc, to_bf16=True)
    assert U.qil_bwd_chain(n, 2) == 3 * 8 + 1 + 6 + 2 + 32 + 64
    assert np.array_equal(_bits(dx), _bits(want_dx))
    _check_sums(n, 2, (dp, dc), ((wp, ap), (wc, ac)), "capped")


# ----------------------------------------------------------------------------- 3. the weight path
WEIGHTS = [dict(k=16, rs=9, c_real=3, c=16, k_pad=16), dict(k=32, rs=1, c_real=16, c=16, k_pad=32)]


@pytest.mark.parametrize("int8", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_pack_and_backward(gpu, dtype, int8):
    """rn_weight_qil_pack over a 3x3 weight (k = 16, c_real = 3, channel stride 16) and a 1x1 weight (k = 32,
    c = 16) in one call -- the second with parameters outside [0, 1], clamped and written back --, then
    rn_weight_qil_bwd on each: the copies against the restatement, their padding still zero, the in-place dw bit for
    bit and dp / dc within the summation bound."""
    lib = L.load()
    rng = np.random.RandomState(3)
    nbits = 4
    points = [(0.0625, 0.5), (-0.25, 1.75)]
    items, keep, masters = [], [], []
    for w_, (pp, cc) in zip(WEIGHTS, points):
        k, rs, cr, cs, kp = w_["k"], w_["rs"], w_["c_real"], w_["c"], w_["k_pad"]
        m = U.edge_inputs(k * rs * cr, False, max(pp, 0.0), min(cc, 1.0), seed=k).astype(np.float32) * f32(0.5)
        m[:4] = [max(pp, 0.0), -min(cc, 1.0), 0.0, min(cc, 1.0) * 2]
        masters.append(m)
        t = dict(master=torch.from_numpy(m).to(gpu), qw=torch.full((m.size,), 9.0, device=gpu),
                 unit=torch.zeros(1, device=gpu), pc=torch.tensor([pp, cc], dtype=torch.float32, device=gpu),
                 codes=torch.zeros(k * rs * cs, dtype=torch.int8, device=gpu) if int8 else None,
                 krsc=None if int8 else torch.zeros(k * rs * cs, dtype=tdt(dtype), device=gpu),
                 crsk=torch.zeros(cs * rs * kp, dtype=tdt(dtype), device=gpu))
        keep.append(t)
        items.append(L.WQilItem(master=t["master"].data_ptr(), qw=t["qw"].data_ptr(), unit=t["unit"].data_ptr(),
                                p=t["pc"].data_ptr(), c=t["pc"].data_ptr() + 4,
                                w_codes=t["codes"].data_ptr() if int8 else None,
                                w_krsc=None if int8 else t["krsc"].data_ptr(), w_crsk=t["crsk"].data_ptr(),
                                k=k, rs=rs, c_real=cr, c_stride=cs, k_pad=kp, nbits=nbits))
    arr = (L.WQilItem * len(items))(*items)
    dev_items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(gpu)
    nws = int(lib.rn_weight_qil_ws_bytes(len(items)))
    assert nws == 4 * 4 * len(items)
    ws = torch.full((nws // 4 + 1,), -1.0, device=gpu)
    assert lib.rn_weight_qil_pack(p(dev_items), len(items), dtype, p(ws), stream()) == 0, lib.rn_last_error()
    torch.cuda.synchronize()
    assert _load(ws)[-1] == -1.0
    rd = (lambda a: U.bf16(a)) if dtype == BF16 else (lambda a: a)
    for w_, (pp, cc), m, t in zip(WEIGHTS, points, masters, keep):
        k, rs, cr, cs, kp = w_["k"], w_["rs"], w_["c_real"], w_["c"], w_["k_pad"]
        v, q, unit, p1, c1 = U.qil_fwd_ref(m, pp, cc, nbits)
        assert np.array_equal(_load(t["pc"]), np.array([p1, c1], dtype=np.float32))  # clamped, written back
        assert np.array_equal(_bits(_load(t["qw"])), _bits(v)) and _load(t["unit"])[0] == unit
        assert (np.abs(q) == 15).any() and (q == 0).any()
        v3, q3 = v.reshape(k, rs, cr), q.reshape(k, rs, cr)
        if int8:
            got = t["codes"].cpu().numpy().reshape(k, rs, cs)
            assert np.array_equal(got[..., :cr], q3.astype(np.int8)) and not got[..., cr:].any()
        else:
            got = _load(t["krsc"]).reshape(k, rs, cs)
            assert np.array_equal(_bits(got[..., :cr]), _bits(rd(v3))) and not got[..., cr:].any()
        got = _load(t["crsk"]).reshape(cs, rs, kp)
        assert np.array_equal(_bits(got[:cr, :, :k]), _bits(rd(v3.transpose(2, 1, 0))))
        assert not got[cr:].any() and not got[:, :, k:].any()
        # the backward, in place over the fp32 gradient
        n = m.size
        dw = rng.randn(n).astype(np.float32)
        dwd = torch.from_numpy(dw).to(gpu)
        dg = torch.full((5,), 123.0, device=gpu)
        bws = torch.full((int(lib.rn_qil_bwd_ws_bytes(n)) // 4 + 1,), -1.0, device=gpu)
        rc = lib.rn_weight_qil_bwd(n, p(t["master"]), p(dwd), p(t["pc"]), C.c_void_p(t["pc"].data_ptr() + 4),
                                   C.c_void_p(dg.data_ptr() + 4), C.c_void_p(dg.data_ptr() + 12), p(bws), stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.rn_last_error()
        dgv = _load(dg)
        assert (dgv[[0, 2, 4]] == 123.0).all() and _load(bws)[-1] == -1.0
        want_dx, wp, wc, ap, ac = U.qil_bwd_ref(m, dw, p1, c1)
        assert np.array_equal(_bits(_load(dwd)), _bits(want_dx))
        _check_sums(n, 4, (dgv[1], dgv[3]), ((wp, ap), (wc, ac)), "weight k %d" % k)


# ----------------------------------------------------------------------------- 4. the optimizer
def _sgd_tables(gpu, seed=5):
    rng = np.random.RandomState(seed)
    sizes = [1000, 1, 4099]
    offs = np.cumsum([0] + [((s + 3) // 4) * 4 for s in sizes])[:-1]
    total = int(offs[-1] + sizes[-1] + 4)
    w, g = rng.randn(total).astype(np.float32), rng.randn(total).astype(np.float32)
    m = (rng.randn(total) * 0.1).astype(np.float32)
    return sizes, offs, w, g, m


def _run_sgd(gpu, name, sizes, offs, w, g, m, wds, lrms, lr, pack):
    lib = L.load()
    t = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=gpu)  # noqa: E731
    wd_, gd, md = t(w), t(g), t(m)
    offs_d, sizes_d, wds_d = t(offs, torch.int64), t(sizes, torch.int64), t(wds)
    lrm_d = t(lrms) if lrms is not None else None
    sc = (C.c_float(lr), None, C.c_float(0.9), C.c_float(1 / 32.), C.c_float(-1.0), stream())
    head = (len(sizes), p(offs_d), p(sizes_d), p(wds_d)) + ((p(lrm_d),) if name.endswith("_lrm") else ())
    if pack:
        tab = np.zeros(len(sizes), dtype=[("krsc", "<u8"), ("crsk", "<u8"), ("k", "<i4"), ("rs", "<i4"),
                                          ("creal", "<i4"), ("c", "<i4"), ("kpad", "<i4"), ("pad", "<i4")])
        work = np.zeros((64, 4), dtype=np.int32)
        nwork = lib.rn_sgd_pack_work(len(sizes), np.asarray(sizes, np.int64).ctypes.data_as(C.c_void_p),
                                     tab.ctypes.data_as(C.c_void_p), work.ctypes.data_as(C.c_void_p), 64)
        assert nwork > 0
        tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(gpu)
        work_d = torch.from_numpy(work[:nwork].copy()).to(gpu)
        L.call(name, *head, p(wd_), p(gd), p(md), p(tab_d), p(work_d), nwork, F32, *sc)
    else:
        L.call(name, *head, p(wd_), p(gd), p(md), None, F32, *sc)
    torch.cuda.synchronize()
    return wd_.cpu().numpy(), md.cpu().numpy()


@pytest.mark.parametrize("pack", [False, True])
def test_sgd_lr_multipliers(gpu, pack):
    """Three tensors with multipliers (1, 0.01, 1): bit for bit against the float32 restatement; with NULL and with
    all ones bit-identical to the old entry point on the same inputs; the gaps between the tensors untouched."""
    sizes, offs, w, g, m = _sgd_tables(gpu)
    wds = np.array([1e-4, 0.0, 1e-4], dtype=np.float32)
    old, new = ("rn_sgd_mom_update_pack", "rn_sgd_mom_update_pack_lrm") if pack else \
        ("rn_sgd_mom_update", "rn_sgd_mom_update_lrm")
    lr = 0.1
    w0, m0 = _run_sgd(gpu, old, sizes, offs, w, g, m, wds, None, lr, pack)
    for lrms in (None, np.ones(3, dtype=np.float32)):
        w1, m1 = _run_sgd(gpu, new, sizes, offs, w, g, m, wds, lrms, lr, pack)
        assert np.array_equal(_bits(w1), _bits(w0)) and np.array_equal(_bits(m1), _bits(m0))
    lrms = np.array([1.0, 0.01, 1.0], dtype=np.float32)
    w1, m1 = _run_sgd(gpu, new, sizes, offs, w, g, m, wds, lrms, lr, pack)
    sl = [slice(int(o), int(o) + s) for o, s in zip(offs, sizes)]
    rw, rm = U.sgd_lrm_ref([w[s] for s in sl], [g[s] for s in sl], [m[s] for s in sl], wds, lrms, lr, 0.9, 1 / 32.)
    for s, a, b in zip(sl, rw, rm):
        assert np.array_equal(_bits(w1[s]), _bits(a)) and np.array_equal(_bits(m1[s]), _bits(b))
    # the one tensor whose multiplier is not 1 is the old kernel's at the learning rate f32(lr) * f32(0.01)
    lr_eff = float(f32(f32(lr) * f32(0.01)))
    w2, m2 = _run_sgd(gpu, old, sizes, offs, w, g, m, wds, None, lr_eff, pack)
    assert np.array_equal(_bits(w1[sl[1]]), _bits(w2[sl[1]])) and np.array_equal(_bits(m1[sl[1]]), _bits(m2[sl[1]]))
    assert not np.array_equal(w1[sl[1]], w0[sl[1]])
    gaps = np.ones(w.size, dtype=bool)
    for s in sl:
        gaps[s] = False
    assert np.array_equal(w1[gaps], w[gaps]) and np.array_equal(m1[gaps], m[gaps])


# ----------------------------------------------------------------------------- 5. plan routing on the device
def _bound(sym, monkeypatch, int8_env=None):
    if int8_env is None:
        monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    else:
        monkeypatch.setenv("RN_INT8_MFMA", int8_env)
    mod = mx.mod.Module(sym, context=[mx.gpu(0)], precision="float32")
    mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    return mod.executor


def test_plan_routing(gpu, monkeypatch):
    ex = _bound(U.qil_unit_net(abits=4, wbits=4), monkeypatch)
    convs = [op for op in ex.plan.ops if op.kind == "conv"]
    qils = [op for op in ex.plan.ops if op.kind == "qil"]
    assert len(convs) == 4 and all(op.int8 and op.wk8 is not None for op in convs)
    assert len(qils) == 5 and [op.emit_codes for op in qils] == [op.name != "fc1_data" for op in qils]
    assert all((op.codes is not None) == op.emit_codes for op in qils)
    names = [c[0] for c in ex._bwd]
    assert names.count("rn_weight_qil_bwd") == 5 and names.count("rn_qil_bwd") == 5
    for i, n in enumerate(names):  # right after its weight gradient, on the weight gradients' stream
        if n == "rn_weight_qil_bwd":
            assert names[i - 1].startswith("rn_conv_bwd_filter") and (i in ex._side_idx) == ((i - 1) in ex._side_idx)
    assert [c[0] for c in ex.wpack_calls].count("rn_weight_qil_pack") == 1
    for sym, env in ((U.qil_unit_net(abits=8, wbits=4), None), (U.qil_unit_net(), "0")):
        ex = _bound(sym, monkeypatch, env)
        assert not any(op.int8 for op in ex.plan.ops if op.kind == "conv")
        assert not any(op.emit_codes or op.codes is not None for op in ex.plan.ops if op.kind == "qil")


# ----------------------------------------------------------------------------- 6. training steps
@pytest.fixture(scope="module")
def unit_case():
    """Seed, scales and points as tests/test_qil_cpu.py::test_cpu_context_step_against_fp64 checks them on
    mx.cpu(): elements below, inside and above every interval, every point's gradient non-zero."""
    sym = U.qil_unit_net(abits=4, wbits=4)
    params = U.init_qil_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    return sym, params, data, label


@pytest.mark.parametrize("int8", ["1", "0"])
def test_training_step_against_fp64(gpu, monkeypatch, unit_case, int8):
    """One fp32 step of stem conv -> bottleneck unit (256 -> 64 -> 64 -> 256, projection shortcut, 8 x 8, batch 2)
    -> head, every weight and activation of the unit and the fc a 4-bit QIL: probabilities, every gradient (each
    pruning and clipping point's too; each gamma's zero) and every parameter after the SGD step with the variables'
    lr_mult / wd_mult, against the fp64 restatement replaying the device's ReLU masks, QIL codes, interval flags
    and |x| > c masks (pact_util.check_step's bar and tolerances)."""
    sym, params, data, label = unit_case
    monkeypatch.setenv("RN_INT8_MFMA", int8)
    res = U.module_step(sym, params, data, label, mx.gpu(0), steps=2)
    ex = res["mod"].executor
    assert all(op.int8 == (int8 == "1") for op in ex.plan.ops if op.kind == "conv")
    assert ex.opt_lrms is not None
    U.check_step(res, sym, params, data, label, step=0)
    points = [k for k in params if k.endswith(("_pruning_point", "_clipping_point"))]
    assert len(points) == 20 and all(res["grads"][0][k][0] != 0 for k in points)
    # the thresholds moved at lr * 0.01 without decay; the second forward read what the first update left
    lr, rescale = 0.1, 1.0 / SHAPE[0]
    lre = f32(f32(lr) * f32(0.01))
    for k in points:
        g = res["grads"][0][k].astype(np.float32)
        w0 = params[k].astype(np.float32)
        step = (lre * (f32(rescale) * g).astype(np.float32)).astype(np.float32)
        assert np.array_equal(res["args"][0][k], (w0 - step).astype(np.float32)), k
    for k, d in res["decisions"][1]["qil"].items():
        assert f32(d["p"]) == res["args"][0][k][0]
        assert f32(d["c"]) == res["args"][0][k.replace("_pruning_point", "_clipping_point")][0]
        if "values" in d:
            assert np.array_equal(d["values"].astype(np.float32), (d["codes"].astype(np.float32) / f32(15)))


def test_attached_graph_trains_and_checkpoints_on_gpu(gpu, tmp_path, monkeypatch):
    """The config-style run of tests/test_qil_cpu.py on mx.gpu(): attach_quantize_node with "QIL" weights and
    activations on ResNet-20 (core/graph_optimize.py:159-292 restated in tests/qil_util.py), bf16, three steps,
    checkpoint and reload with the pruning points, clipping points and gammas intact."""
    from graph_passes import shape_dict
    from rn import graphs
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    base = graphs.resnet20_cifar()
    shapes = shape_dict(base, (4, 3, 32, 32), (4,))
    data, label = U.batch((4, 3, 32, 32), 10, seed=5)
    w, a = U.qil_settings()
    sym = U.attach_quantize_node(base, shapes, w, a, skip_quantize_counts={"Convolution": 1})
    mod = mx.mod.Module(sym, context=[mx.gpu(0)])
    mod.bind([("data", (4, 3, 32, 32))], [("softmax_label", (4,))])
    mx.random.seed(3)
    mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
    mod.init_optimizer(optimizer="sgd", optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
    b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    for _ in range(3):
        mod.forward(b, is_train=True)
        mod.backward()
        mod.update()
    assert np.isfinite(mod.get_outputs()[0].asnumpy()).all()
    plan = mod.executor.plan
    assert plan.summary()["qil"] == 19 and sum(1 for op in plan.ops if op.kind == "conv" and op.int8) == 20
    prefix = str(tmp_path / "qil")
    mod.save_checkpoint(prefix, 3)
    sym2, arg, aux = mx.model.load_checkpoint(prefix, 3)
    now = {k: v.asnumpy() for k, v in mod.get_params()[0].items()}
    names = [k for k in arg if k.endswith(("_pruning_point", "_clipping_point")) or
             (k.endswith("_gamma") and k[:-6] + "_pruning_point" in arg)]
    assert len(names) == 3 * (19 + 21) and not any("point" in k for k in aux)
    assert all(np.array_equal(arg[k].asnumpy(), now[k]) for k in names)
    # every activation's clipping point has a gradient and moved (it is clamped only by the next forward); a weight's
    # is clamped by the pack that follows the update, so it reads at most 1.0, a pruning point at least 0
    act_c = [k for k in names if k.endswith("_clipping_point") and "_weight_" not in k]
    assert len(act_c) == 19 and all(now[k][0] != 1.0 for k in act_c)
    assert all(now[k][0] <= 1.0 for k in names if k.endswith("_weight_clipping_point"))
    assert all(now[k][0] >= 0.0 for k in names if k.endswith("_weight_pruning_point"))
    assert any(now[k][0] != 0.0 for k in names if k.endswith("_pruning_point"))
    decayed = [k for k in names if k.endswith("_gamma")]
    assert all(0.999 < now[k][0] < 1.0 for k in decayed)  # (zero gradient, decayed by its name)
    again = mx.mod.Module(sym2, context=[mx.gpu(0)])
    again.bind([("data", (4, 3, 32, 32))], [("softmax_label", (4,))], for_training=False)
    again.set_params(arg, aux)
    back = {k: v.asnumpy() for k, v in again.get_params()[0].items()}
    assert all(np.array_equal(back[k], now[k]) for k in names)


# ----------------------------------------------------------------------------- 7. the network, layer by layer
def _qil_net():
    """Two bottleneck units per stage (tests/test_pact_gpu.py's network) with 4-bit QIL weights and activations:
    29 activation quantizers, conv0 (Quantization_int8) + 28 QIL-fed convolutions + fc1. Clipping points start at
    0.25: at 1.0 the Xavier weights of the wide layers (|w| ~ 0.02) would all take the codes 0 and 1."""
    from rn import graphs
    return graphs.resnet_int8([2, 2, 2, 2], 4, [64, 256, 512, 1024, 2048], 1000, "float32", True, act_op="QIL",
                              weight_op="QIL", wbits=4, abits=4, qil_init=0.25)


@pytest.mark.parametrize("precision,warm", [("bfloat16", 1), ("float32", 0)], ids=["bf16_warm", "fp32"])
def test_qil_network_layerwise(gpu, monkeypatch, precision, warm):
    """Every kernel of one training step of the QIL network at 8 x 64 x 64 against its recompute from the device's
    own inputs (tests/layerwise.py with tests/qil_layerwise.py's QIL checks): each rn_qil_fwd and each weight of
    rn_weight_qil_pack bit for bit, the int8 MFMA convolutions behind the 4-bit codes as exact sums of the device's
    codes, each rn_qil_bwd's dx and each rn_weight_qil_bwd's in-place dw bit for bit, their dp / dc within the
    kernels' summation bound and in their own slots of the flat gradient buffer. lr = 1e-10 for the warm step: this
    initialisation's threshold gradients reach 1e9 (quantized weights of magnitude up to 1 in front of every
    BatchNorm), and at 0.001 the warm step throws the clipping points below the pruning points, where the
    operator is not defined (the reference asserts p < c there)."""
    import layerwise
    from qil_layerwise import QilChecker
    from test_step_bf16_gpu import _layerwise
    monkeypatch.setattr(layerwise, "Checker", QilChecker)
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    ck = _layerwise(_qil_net(), 8, 64, precision, warm=warm, lr=1e-10)
    convs = [op for op in ck.ex.plan.ops if op.kind == "conv"]
    qils = [op for op in ck.ex.plan.ops if op.kind == "qil"]
    assert len(convs) == 28 and len(qils) == 29
    assert all(op.int8 and op.qsrc.kind == "qil" and op.qweight["family"] == "qil" for op in convs)
    assert [op.name for op in qils if op.codes is None] == ["fc1_data"]
    assert not ck.skipped, ck.skipped
    assert not ck.fwd_skipped, ck.fwd_skipped
    # the inputs exercise the quantizers: every weight has elements inside its interval and reaches more than one
    # code; every activation has elements inside and above it (but the pooled fc input: means that all sit above
    # 0.25) and reaches the top code
    st = ck.qil_stats
    assert len(st) == 29 + 29
    print("inside %.3f .. %.3f, above %.3f .. %.3f, lowest top code %d" % (
        min(s["inside"] for s in st.values()), max(s["inside"] for s in st.values()),
        min(s["above"] for s in st.values()), max(s["above"] for s in st.values()),
        min(s["max_code"] for s in st.values())))
    assert all(0.0 <= s["p"] < s["c"] <= 1.0 for s in st.values()), st
    acts = {op.name for op in qils}
    assert all(s["inside"] > 0.01 and s["max_code"] >= 2 for k, s in st.items() if k not in acts), st
    assert all(st[k]["above"] > 0.01 and st[k]["max_code"] == 15 for k in acts), st
    assert all(st[k]["inside"] > 0.01 for k in acts if k != "fc1_data"), st
    if warm:
        assert any(s["c"] != 0.25 for s in st.values())
    else:
        assert all(s["c"] == 0.25 and s["p"] == 0.0 for s in st.values())
    with_terms = [c for c in ck.qil_bwd if c["name"] != "fc1_data"]
    assert len(ck.qil_bwd) == 58 and all(c["dp"] != 0.0 and c["dc"] != 0.0 for c in with_terms), ck.qil_bwd
    bad = ck.failures()
    assert not bad, bad[:10]
    count = lambda kind: sum(1 for r in ck.rec if r[0] == kind)  # noqa: E731
    assert count("qil") == 29 and count("weight_qil") == 29 and count("weight_quant") == 1  # (conv0)
    assert ck.covered["rn_qil_bwd"] == 29 and ck.covered["rn_weight_qil_bwd"] == 29
    assert count("qil_bwd") == 29 and count("weight_qil_bwd") == 29
    assert count("conv_fwd_i8") == 28
    with_add = [c for c in ck.qil_bwd if c["add"]]  # the second reader of each stage-first act1 adds in place
    assert len(with_add) >= 4 and all(c["aliased"] for c in with_add), ck.qil_bwd
