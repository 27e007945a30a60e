"""GDRQ on the MI355X: rn_gdrq_fwd (quantize pass and threshold update), rn_weight_gdrq_pack and rn_gdrq_bwd against
their numpy float32 restatements (tests/gdrq_util.py), the plan's int8 routing, a training step of a small GDRQ
network against the fp64 restatement replaying the device's own discrete decisions, the attached ResNet-20 in both
node forms, and run-to-run determinism."""
import ctypes as C

import numpy as np
import pytest
import torch

import gdrq_util as U
import mxnet as mx
from gpu_util import BF16, F32, p, stream, tdt
from rn import lib as L

pytestmark = pytest.mark.gpu

# 16: one code chunk, one block; 4160 = 16 * 260: more than one block of the codes kernel and three of the sum;
# 1001 * 48 + 3: many blocks and a tail that is no multiple of either chunk size (values only: no codes there).
# The reduction grid's cap (2048 blocks) is passed in test_threshold_update_beyond_the_grid_cap
SIZES = [16, 4160, 1001 * 48 + 3]
DTYPES = [F32, BF16]
SHAPE = (2, 3, 16, 16)


def _store(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(tdt(dtype)).to(dev)


def _load(t):
    return t.float().cpu().numpy()


def _fwd(dev, dtype, x, alpha, nbits, want_codes, update=0, ktimes=3.0, lamda=0.001, n_real=None, want_out=True):
    lib = L.load()
    n = x.size
    xd = _store(x, dtype, dev)
    a = torch.tensor([77.0, alpha, 77.0], dtype=torch.float32, device=dev)  # (the neighbours stay untouched)
    out = torch.full((n,), 77.0, dtype=tdt(dtype), device=dev) if want_out else None
    codes = torch.full((n,), -99, dtype=torch.int8, device=dev) if want_codes else None
    unit = torch.zeros(1, dtype=torch.float32, device=dev)
    nws = int(lib.rn_gdrq_ws_bytes(n))
    assert nws == 4 * min(max(-(-n // 2048), 1), 2048)
    ws = torch.full((nws // 4 + 1,), -1.0, dtype=torch.float32, device=dev)
    rc = lib.rn_gdrq_fwd(dtype, n, n if n_real is None else n_real, p(xd), C.c_void_p(a.data_ptr() + 4), nbits,
                         update, ktimes, lamda, p(out), p(codes), p(unit), p(ws), stream())
    torch.cuda.synchronize()
    av = _load(a)
    assert av[0] == 77.0 and av[2] == 77.0 and _load(ws)[-1] == -1.0
    return rc, out, codes, unit, np.float32(av[1])


def _half_unit_alpha(nbits):
    """alpha with unit = alpha / L = 0.5 exactly (1.5, 7.5, 63.5): every odd multiple of 0.25 is a representable tie,
    in bf16 too (63.25 has 8 significant bits)."""
    return np.float32((2 ** nbits - 1) * 0.5)


# ----------------------------------------------------------------------------- 1. forward, update = 0
@pytest.mark.parametrize("nbits", [2, 4, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_bit_for_bit(gpu, dtype, n, nbits):
    alpha, levels = _half_unit_alpha(nbits), 2 ** nbits - 1
    x = U.edge_inputs(n, dtype == BF16, alpha, np.float32(0.5), seed=n + nbits, levels=levels)
    assert (x > alpha).any() and (x < -alpha).any() and (x == alpha).any() and (x == -alpha).any()
    r = x[np.abs(x) < alpha] / np.float32(0.5)
    ties = np.abs(r - np.trunc(r)) == 0.5
    assert (ties & (r > 0)).any() and (ties & (r < 0)).any()  # (exact ties of both signs are in)
    want, wq, wunit = U.gdrq_fwd_ref(x, alpha, nbits, to_bf16=dtype == BF16)
    assert wunit == np.float32(0.5) and wq.min() == -levels and wq.max() == levels
    rc, out, _, u, a1 = _fwd(gpu, dtype, x, alpha, nbits, want_codes=False)
    assert rc == 0 and a1 == alpha  # (update = 0: alpha is read only)
    assert np.array_equal(_load(out), want) and _load(u)[0] == wunit
    if n % 16 == 0:
        rc, out2, codes, u, _ = _fwd(gpu, dtype, x, alpha, nbits, want_codes=True)
        assert rc == 0 and torch.equal(out, out2) and _load(u)[0] == wunit
        q = codes.cpu().numpy()
        assert q.dtype == np.int8 and q.min() == -levels and np.array_equal(q, wq.astype(np.int8))
        rc, _, codes3, _, _ = _fwd(gpu, dtype, x, alpha, nbits, want_codes=True, want_out=False)
        assert rc == 0 and torch.equal(codes, codes3)  # codes only


def test_forward_refusals_and_nonpositive_alpha(gpu):
    x = U.edge_inputs(4160, False, np.float32(6.0), np.float32(0.4), seed=1)
    rc, out, codes, _, _ = _fwd(gpu, F32, x, np.float32(6.0), 8, want_codes=True)
    assert rc == -1 and b"nbits <= 7" in L.load().rn_last_error()
    assert (codes.cpu().numpy() == -99).all() and (_load(out) == 77.0).all()  # nothing was launched
    rc, _, _, _, _ = _fwd(gpu, F32, x[:4150], np.float32(6.0), 4, want_codes=True)
    assert rc == -1 and b"multiple of 16" in L.load().rn_last_error()
    rc, out, _, _, _ = _fwd(gpu, F32, x, np.float32(6.0), 8, want_codes=False)  # eight bits: values only
    assert rc == 0 and np.array_equal(_load(out), U.gdrq_fwd_ref(x, 6.0, 8)[0])
    for alpha in (0.0, -1.0):
        rc, out, codes, _, _ = _fwd(gpu, F32, x, np.float32(alpha), 4, want_codes=True)
        assert rc == 0 and not _load(out).any() and not codes.cpu().numpy().any()


# ----------------------------------------------------------------------------- 2. forward, update = 1
def _check_update(gpu, dtype, x, nbits, count=None, ktimes=3.0):
    """alpha0 = 0 and lamda = -1 make the update exact -- alpha = 0 + (-1) * (0 - thr) = thr --, so the device's
    float32 threshold itself is held to the chain bound; then the update as configured, from that threshold."""
    n = x.size
    bf = dtype == BF16
    thr64 = U.gdrq_thr_ref(x, ktimes, count)
    k = U.gdrq_sum_chain(n, 2 if bf else 4)
    want_codes = n % 16 == 0 and nbits <= 7
    rc, out, codes, u, thr = _fwd(gpu, dtype, x, 0.0, nbits, want_codes, update=1, ktimes=ktimes, lamda=-1.0,
                                  n_real=count)
    assert rc == 0, L.load().rn_last_error()
    print("n %d dtype %d: thr %.9g, fp64 %.9g, rel %.3g, bound %.3g (k = %d)"
          % (n, dtype, thr, thr64, abs(float(thr) - thr64) / thr64, k * 2.0 ** -24, k))
    assert abs(float(thr) - thr64) <= k * 2.0 ** -24 * thr64
    want, wq, wunit = U.gdrq_fwd_ref(x, thr, nbits, to_bf16=bf)  # from the device's own alpha: bit for bit
    assert np.array_equal(_load(out), want) and _load(u)[0] == wunit
    if want_codes:
        assert np.array_equal(codes.cpu().numpy(), wq.astype(np.int8))
    rc, out2, _, _, thr2 = _fwd(gpu, dtype, x, 0.0, nbits, want_codes, update=1, ktimes=ktimes, lamda=-1.0,
                                n_real=count)
    assert rc == 0 and thr2.tobytes() == thr.tobytes() and torch.equal(out, out2)  # bit-identical from run to run
    # the reference's update and its sign, every operation rounded to float32
    rc, out, _, u, a1 = _fwd(gpu, dtype, x, 1.0, nbits, False, update=1, ktimes=ktimes, lamda=0.001, n_real=count)
    assert rc == 0 and a1.tobytes() == U.gdrq_ema_ref(1.0, thr, 0.001).tobytes()
    assert (a1 > 1.0) == (thr < 1.0)  # (alpha moves AWAY from the threshold: alpha + lamda * (alpha - thr))
    want, _, wunit = U.gdrq_fwd_ref(x, a1, nbits, to_bf16=bf)
    assert np.array_equal(_load(out), want) and _load(u)[0] == wunit
    return thr


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_threshold_update(gpu, dtype, n):
    x = U.edge_inputs(n, dtype == BF16, np.float32(2.0), np.float32(2.0 / 15), seed=n)
    _check_update(gpu, dtype, x, 4)


def test_threshold_update_divides_by_the_real_count(gpu):
    """Padded channels: 11 real channels of 16, the padding zero. The sum runs over all n elements, the mean
    divides by rows * 11."""
    rows, c, cp = 300, 11, 16
    x = np.zeros((rows, cp), dtype=np.float32)
    x[:, :c] = U.edge_inputs(rows * c, False, np.float32(2.0), np.float32(2.0 / 15), seed=9).reshape(rows, c)
    for dtype in DTYPES:
        xs = U.bf16(x) if dtype == BF16 else x
        thr = _check_update(gpu, dtype, xs.reshape(-1), 4, count=rows * c)
        assert abs(float(thr) / U.gdrq_thr_ref(xs, 3.0) - cp / c) < 1e-5  # (not the padded count's mean)


def test_threshold_update_beyond_the_grid_cap(gpu):
    """bf16 past 2048 * 256 chunks of 8: every block strides more than once, the per-thread chain is its longest."""
    n = 2048 * 256 * 8 * 2 + 8 * 77 + 5
    assert U.gdrq_sum_chain(n, 2) == 3 * 8 + 1 + 6 + 2 + 32 + 64 + 3 + 1
    x = U.edge_inputs(n, True, np.float32(2.0), np.float32(2.0 / 15), seed=4)
    _check_update(gpu, BF16, x, 4)


# ----------------------------------------------------------------------------- 3. the weight pack
def _pad8(v):
    return (v + 7) // 8 * 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_pack(gpu, dtype):
    """Three weights in one call: a 1x1 64 -> 256, a 3x3 64 -> 64, and an FC-shaped 100 -> 10 (ragged channels and
    columns: c 104, k_pad 16). The third keeps its alpha (fix_alpha)."""
    lib = L.load()
    bf = dtype == BF16
    rng = np.random.RandomState(3)
    shapes = [(256, 1, 64), (64, 9, 64), (10, 1, 100)]
    fixed = [False, False, True]
    alpha0 = [0.5, 0.5, 0.3]
    keep, items, bufs = [], [], []
    for (K, RS, cr), fx, a0 in zip(shapes, fixed, alpha0):
        w = (rng.randn(K, RS, cr) * 0.1).astype(np.float32)
        w[0, 0, :4] = [1.0, -1.0, 0.3, -0.3]  # (beyond any of the thresholds, and equal to the fixed one)
        c, kp = _pad8(cr), _pad8(K)
        t = dict(w=w, master=torch.from_numpy(w).to(gpu), qw=torch.full((K * RS * cr,), 7.0, device=gpu),
                 unit=torch.zeros(1, device=gpu), alpha=torch.tensor([a0], dtype=torch.float32, device=gpu),
                 codes=torch.zeros(K * RS * c, dtype=torch.int8, device=gpu),
                 krsc=torch.zeros(K * RS * c, dtype=tdt(dtype), device=gpu),
                 crsk=torch.zeros(c * RS * kp, dtype=tdt(dtype), device=gpu), c=c, kp=kp)
        assert t["master"].data_ptr() % 16 == 0
        bufs.append(t)
        items.append(L.WGdrqItem(master=t["master"].data_ptr(), qw=t["qw"].data_ptr(), unit=t["unit"].data_ptr(),
                                 alpha=t["alpha"].data_ptr(), w_codes=t["codes"].data_ptr(),
                                 w_krsc=t["krsc"].data_ptr(), w_crsk=t["crsk"].data_ptr(), k=K, rs=RS, c_real=cr, c=c,
                                 k_pad=kp, nbits=4, fix_alpha=int(fx), ktimes=3.0))
    arr = (L.WGdrqItem * len(items))(*items)
    dev_items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(gpu)
    keep.append(dev_items)
    nws = int(lib.rn_weight_gdrq_ws_bytes(len(items)))
    assert nws == 4 * 65 * len(items)
    ws = torch.full((nws // 4 + 1,), -1.0, dtype=torch.float32, device=gpu)
    alphas = []
    for _ in range(2):
        rc = lib.rn_weight_gdrq_pack(p(dev_items), len(items), dtype, p(ws), stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.rn_last_error()
        alphas.append([np.float32(_load(t["alpha"])[0]) for t in bufs])
    assert _load(ws)[-1] == -1.0
    assert [a.tobytes() for a in alphas[0]] == [a.tobytes() for a in alphas[1]]  # bit-identical from run to run
    for t, (K, RS, cr), fx, a0, a in zip(bufs, shapes, fixed, alpha0, alphas[0]):
        if fx:
            assert a == np.float32(a0)
        else:
            thr64, k = U.gdrq_thr_ref(t["w"], 3.0), U.wgdrq_sum_chain(t["w"].size)
            print("weight %s: alpha %.9g, fp64 %.9g, bound %.3g (k = %d)" % ((K, RS, cr), a, thr64,
                                                                              k * 2.0 ** -24 * thr64, k))
            assert abs(float(a) - thr64) <= k * 2.0 ** -24 * thr64
        v, codes, krsc, crsk, unit = U.wgdrq_pack_ref(t["w"], a, 4, t["c"], t["kp"], bf)
        assert _load(t["unit"])[0] == unit
        assert np.array_equal(_load(t["qw"]).reshape(K, RS, cr), v)
        got = t["codes"].cpu().numpy().reshape(K, RS, t["c"])
        assert np.array_equal(got, codes) and got.min() == -15 and got.max() == 15  # clipped to +-L
        assert np.array_equal(_load(t["krsc"]).reshape(K, RS, t["c"]), krsc)
        assert np.array_equal(_load(t["crsk"]).reshape(t["c"], RS, t["kp"]), crsk)


# ----------------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n", [4160, 1001 * 48 + 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_includes_the_boundary(gpu, dtype, n, with_add):
    """dx = dy * [|x| <= alpha] with elements exactly at +alpha and -alpha, bit for bit -- and rn_quant_int8_bwd on
    the same operands zeroes exactly those elements (its mask is strict), which is why GDRQ has its own kernel."""
    lib = L.load()
    alpha = np.float32(1.25)
    bf = dtype == BF16
    rng = np.random.RandomState(n + 7 * with_add)
    x = U.edge_inputs(n, bf, alpha, np.float32(alpha / 15), seed=n)
    at = np.abs(x) == alpha
    assert (x == alpha).any() and (x == -alpha).any() and (np.abs(x) > alpha).any()
    rd = U.bf16 if bf else (lambda v: v)
    dy = rd(np.abs(rng.randn(n)).astype(np.float32) + 1.0)  # (no small gradient hides a mask, with the add either)
    add = rd(rng.randn(n).astype(np.float32)) if with_add else None
    xd, dyd = _store(x, dtype, gpu), _store(dy, dtype, gpu)
    addd = _store(add, dtype, gpu) if with_add else None
    a = torch.tensor([alpha], dtype=torch.float32, device=gpu)
    dx = torch.full((n,), 55.0, dtype=tdt(dtype), device=gpu)
    assert lib.rn_gdrq_bwd(dtype, n, p(xd), p(dyd), p(a), p(dx), p(addd), stream()) == 0, lib.rn_last_error()
    torch.cuda.synchronize()
    want = U.gdrq_bwd_ref(x, dy, alpha, add, to_bf16=bf)
    assert np.array_equal(_load(dx), want)
    strict = torch.full((n,), 55.0, dtype=tdt(dtype), device=gpu)
    assert lib.rn_quant_int8_bwd(dtype, n, p(xd), p(dyd), p(strict), p(a), 0, p(addd), stream()) == 0
    torch.cuda.synchronize()
    differs = _load(strict) != _load(dx)
    assert np.array_equal(differs, at)
    # in place: dx aliases dy
    assert lib.rn_gdrq_bwd(dtype, n, p(xd), p(dyd), p(a), p(dyd), p(addd), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_load(dyd), want)


# ----------------------------------------------------------------------------- 5. plan routing
def _bound(sym, monkeypatch, int8_env=None, precision="float32"):
    if int8_env is None:
        monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    else:
        monkeypatch.setenv("RN_INT8_MFMA", int8_env)
    mod = mx.mod.Module(sym, context=[mx.gpu(0)], precision=precision)
    mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    return mod


def test_plan_routing(gpu, monkeypatch):
    ex = _bound(U.gdrq_unit_net(), monkeypatch).executor
    convs = [op for op in ex.plan.ops if op.kind == "conv"]
    acts = [op for op in ex.plan.ops if op.kind == "gdrq"]
    assert len(convs) == 4 and all(op.int8 and op.qsrc.kind == "gdrq" for op in convs)
    assert len(acts) == 5 and [op.emit_codes for op in acts] == [op.name != "fc1_data" for op in acts]
    assert all((op.codes is not None) == op.emit_codes for op in acts)
    fwd = [c[0] for c in ex._fwd_train]
    assert fwd.count("rn_gdrq_fwd") == 5 and fwd.count("rn_conv_fwd_i8") == 4
    assert [c[0] for c in ex._bwd].count("rn_gdrq_bwd") == 5
    assert [c[0] for c in ex.unfused_packs].count("rn_weight_gdrq_pack") == 1
    for sym, env in ((U.gdrq_unit_net(abits=8), None), (U.gdrq_unit_net(wbits=8), None), (U.gdrq_unit_net(), "0")):
        ex = _bound(sym, monkeypatch, env).executor
        assert not any(op.int8 for op in ex.plan.ops if op.kind == "conv")
        assert not any(op.emit_codes or op.codes is not None for op in ex.plan.ops if op.kind == "gdrq")
    for sym, kind in ((U.gdrq_unit_net(weight_op="Quantization_int8", wbits=8), "gdrq"),
                      (U.gdrq_unit_net(act_op="PACT"), "pact")):
        ex = _bound(sym, monkeypatch).executor
        assert all(op.int8 and op.qsrc.kind == kind for op in ex.plan.ops if op.kind == "conv")


def test_int8_switch_changes_the_routing_only(gpu, monkeypatch):
    """RN_INT8_MFMA=0 against the default on the same parameters and batch: every quantizer's codes are the
    restatement's on the input it read, in both modes (the decisions are a function of the inputs alone); the
    quantizers whose inputs do not pass a quantized convolution -- every weight, conv1's and the shortcut's data --
    make identical decisions in the two modes."""
    sym = U.gdrq_unit_net()
    params, aux = U.init_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    dec = {}
    for env in ("1", "0"):
        monkeypatch.setenv("RN_INT8_MFMA", env)
        res = U.module_step(sym, params, aux, data, label, mx.gpu(0), steps=1)
        ex = res["mod"].executor
        assert all(op.int8 == (env == "1") for op in ex.plan.ops if op.kind == "conv")
        dec[env] = res["decisions"][0]["gdrq"]
    assert set(dec["1"]) == set(dec["0"]) == set(aux)
    same_inputs = [k for k in aux if k.endswith("_weight_alpha")] + ["unit1_conv1_data_alpha", "unit1_sc_data_alpha"]
    for k in same_inputs:
        assert np.array_equal(dec["1"][k]["codes"], dec["0"][k]["codes"]), k
        assert dec["1"][k]["alpha"] == dec["0"][k]["alpha"] and dec["1"][k]["unit"] == dec["0"][k]["unit"]
    for env in ("1", "0"):
        for k, d in dec[env].items():
            v, q, unit = U.gdrq_fwd_ref(d["x"], d["alpha"], 4)
            assert unit == np.float32(d["unit"]) and np.array_equal(q, d["codes"]), (env, k)
            assert np.array_equal(v, d["values"].astype(np.float32)), (env, k)


# ----------------------------------------------------------------------------- 6. training steps
# seeds and scales as tests/test_gdrq_cpu.py checks them on the CPU (test_fp32_torch_step_meets_the_code_condition,
# both cases): init_net seed 0, batch seed 1, unit-normal data, activations' alpha 1.0; "moving": lamda 0.01
CASES = {"fixed": dict(act_fix_alpha=True), "moving": dict(act_fix_alpha=False, lamda=0.01)}


@pytest.mark.parametrize("int8", ["1", "0"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_training_step_against_fp64(gpu, monkeypatch, case, int8):
    """One fp32 step of stem conv -> bottleneck unit (256 -> 64 -> 64 -> 256, projection shortcut, 8 x 8, batch 2)
    -> head with the GDRQ setting (4-bit weights following 3 * mean|w|, 4-bit activations clipped at 1.0, fixed or
    moving): probabilities, every gradient, every parameter after the SGD step and every alpha, against the fp64
    restatement replaying the device's ReLU masks, GDRQ codes (weights' too) and |x| <= alpha masks."""
    sym = U.gdrq_unit_net(**CASES[case])
    params, aux = U.init_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    monkeypatch.setenv("RN_INT8_MFMA", int8)
    res = U.module_step(sym, params, aux, data, label, mx.gpu(0), steps=2)
    ex = res["mod"].executor
    assert all(op.int8 == (int8 == "1") for op in ex.plan.ops if op.kind == "conv")
    figs = U.check_step(res, sym, params, aux, data, label, step=0)
    assert set(figs["alphas"]) == set(aux) and len(aux) == 10
    acts = [k for k in aux if k.endswith("_data_alpha")]
    moved = [k for k in acts if res["decisions"][0]["gdrq"][k]["alpha"] != 1.0]
    assert len(moved) == (0 if case == "fixed" else 5)
    # the second step: a weight's alpha in the checkpointable state is the one of the UPDATED weight (recomputed by
    # the repack after the update), and the second forward quantizes with exactly that alpha
    for k in aux:
        d0, d1 = res["decisions"][0]["gdrq"][k], res["decisions"][1]["gdrq"][k]
        if k.endswith("_weight_alpha"):
            assert np.float32(res["aux"][0][k][0]) == np.float32(d1["alpha"]) != np.float32(d0["alpha"]), k
        assert np.float32(d1["unit"]) == np.float32(np.float32(d1["alpha"]) / np.float32(15)), k


@pytest.fixture
def deterministic(monkeypatch):
    monkeypatch.setenv("RN_DETERMINISTIC", "1")
    L.call("rn_set_tuning", 17, 1)
    yield
    L.call("rn_set_tuning", 17, 0)


def test_attached_resnet20_both_forms_and_checkpoint(gpu, tmp_path, monkeypatch, deterministic):
    """The config-style run of tests/test_gdrq_cpu.py on mx.gpu(): attach_quantize_node with GDRQ (Custom) and
    GDRQ_CXX (contrib) on ResNet-20, bf16, two steps: both forms lower to the same plan and give the same outputs
    (deterministic mode: bit for bit); a checkpoint reload reproduces step 3's forward."""
    from graph_passes import shape_dict
    from rn import graphs
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    base = graphs.resnet20_cifar()
    shapes = shape_dict(base, (4, 3, 32, 32), (4,))
    data, label = U.batch((4, 3, 32, 32), 10, seed=5)
    b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
    probs, plans = {}, {}
    for op_name in ("GDRQ", "GDRQ_CXX"):
        w, a = U.gdrq_settings(op_name)
        sym = U.attach_quantize_node(base, shapes, w, a, skip_quantize_counts={"Convolution": 1})
        mod = mx.mod.Module(sym, context=[mx.gpu(0)])
        mod.bind([("data", (4, 3, 32, 32))], [("softmax_label", (4,))])
        mx.random.seed(3)
        mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
        mod.init_optimizer(optimizer="sgd", optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
        for _ in range(2):
            mod.forward(b, is_train=True)
            mod.backward()
            mod.update()
        probs[op_name] = mod.get_outputs()[0].asnumpy().copy()
        plans[op_name] = [(op.kind, op.name, getattr(op, "int8", None), getattr(op, "emit_codes", None),
                           (getattr(op, "qweight", None) or {}).get("family")) for op in mod.executor.plan.ops]
        assert np.isfinite(probs[op_name]).all()
    assert plans["GDRQ"] == plans["GDRQ_CXX"] and sum(1 for o in plans["GDRQ"] if o[0] == "gdrq") == 19
    assert sum(1 for o in plans["GDRQ"] if o[0] == "conv" and o[2] and o[4] == "gdrq") == 20
    np.testing.assert_array_equal(probs["GDRQ"], probs["GDRQ_CXX"])
    prefix = str(tmp_path / "gdrq")
    mod.save_checkpoint(prefix, 2)
    sym2, arg, auxp = mx.model.load_checkpoint(prefix, 2)
    alphas = [k for k in auxp if k.endswith("_alpha")]
    assert len(alphas) == 40 and all(auxp[k].shape == (1,) and auxp[k].asnumpy()[0] > 0 for k in alphas)
    m2 = mx.mod.Module(sym2, context=[mx.gpu(0)])
    m2.bind([("data", (4, 3, 32, 32))], [("softmax_label", (4,))])
    m2.init_params(arg_params=arg, aux_params=auxp)
    m2.forward(b, is_train=True)
    mod.forward(b, is_train=True)
    np.testing.assert_array_equal(m2.get_outputs()[0].asnumpy(), mod.get_outputs()[0].asnumpy())
    # inference reads the alphas and never writes them
    before = {k: v.asnumpy().copy() for k, v in m2.get_params()[1].items() if k.endswith("_alpha")}
    m2.forward(b, is_train=False)
    after = m2.get_params()[1]
    assert all(np.array_equal(after[k].asnumpy(), v) for k, v in before.items())


def test_two_runs_are_bitwise_equal(gpu, monkeypatch, deterministic):
    """Two runs of two steps of the unit network with moving activation thresholds, deterministic mode: outputs,
    gradients, parameters and alphas are bitwise equal (the threshold sums use no atomics)."""
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    sym = U.gdrq_unit_net(**CASES["moving"])
    params, aux = U.init_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    runs = [U.module_step(sym, params, aux, data, label, mx.gpu(0), steps=2) for _ in range(2)]
    for step in range(2):
        assert runs[0]["prob"][step].tobytes() == runs[1]["prob"][step].tobytes()
        for kind in ("grads", "args", "aux"):
            for k, v in runs[0][kind][step].items():
                assert v.tobytes() == runs[1][kind][step][k].tobytes(), (step, kind, k)
    assert any(runs[0]["aux"][1][k][0] != runs[0]["aux"][0][k][0] for k in aux)
