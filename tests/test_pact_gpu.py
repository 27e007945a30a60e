"""PACT on the MI355X: rn_pact_fwd / rn_pact_bwd against their numpy float32 restatements (tests/pact_util.py), the
plan's int8 routing, a training step of a small PACT network against the fp64 restatement replaying the device's
own discrete decisions, and every kernel of a step of a two-units-per-stage PACT network layer by layer
(tests/layerwise.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxnet as mx
import pact_util as U
from gpu_util import BF16, F32, p, stream, tdt
from rn import lib as L

pytestmark = pytest.mark.gpu

# 16: one code chunk; 4160 = 16 * 260: more than one block of the codes kernel; 1001 * 48: many blocks (a multiple
# of 16 too), two grid-stride rounds of the fp32 backward; + 3: a tail that is no multiple of either chunk size.
# The grids' caps (8192 blocks forward, 2048 backward) are passed once each in test_beyond_the_grid_caps
SIZES = [16, 4160, 1001 * 48, 1001 * 48 + 3]
DTYPES = [F32, BF16]
SHAPE = (2, 3, 16, 16)


def _store(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(tdt(dtype)).to(dev)


def _load(t):
    return t.float().cpu().numpy()


def _inputs(n, dtype, gamma, unit, seed):
    return U.edge_inputs(n, dtype == BF16, gamma, unit, seed)


def _fwd(dev, dtype, x, gamma, nbits, want_codes, want_out=True):
    n = x.size
    xd = _store(x, dtype, dev)
    g = torch.tensor([gamma], dtype=torch.float32, device=dev)
    out = torch.full((n,), 77.0, dtype=tdt(dtype), device=dev) if want_out else None
    codes = torch.full((n,), -9, dtype=torch.int8, device=dev) if want_codes else None
    unit = torch.zeros(1, dtype=torch.float32, device=dev)
    rc = L.load().rn_pact_fwd(dtype, n, p(xd), p(g), nbits, p(out), p(codes), p(unit), stream())
    torch.cuda.synchronize()
    return rc, out, codes, unit


# ----------------------------------------------------------------------------- 1. forward values
@pytest.mark.parametrize("nbits", [4, 7, 8])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_values_bit_for_bit(gpu, dtype, n, nbits):
    gamma = np.float32(7.5)  # 4 bits: unit = 0.5 exactly, every odd multiple of 0.25 a representable tie
    unit = np.float32(gamma / np.float32(2 ** nbits - 1))
    x = _inputs(n, dtype, gamma, unit, seed=n + nbits)
    assert (x < 0).any() and (x > gamma).any() and (x == gamma).any()
    if nbits == 4:
        a = x[x < gamma] / unit
        assert (np.abs(a - np.trunc(a)) == 0.5).sum() >= 2  # (exact ties are in)
    rc, out, _, u = _fwd(gpu, dtype, x, gamma, nbits, want_codes=False)
    assert rc == 0
    want, _, wunit = U.pact_fwd_ref(x, gamma, nbits, to_bf16=dtype == BF16)
    assert np.array_equal(_load(out), want)
    assert _load(u)[0] == wunit
    assert (_load(out)[x < 0] < 0).any()  # no lower clip: negative inputs pass through the grid


def test_forward_nonpositive_gamma_writes_zeros(gpu):
    x = _inputs(4160, F32, np.float32(2.0), np.float32(0.25), seed=3)
    for gamma in (0.0, -1.0):
        rc, out, codes, _ = _fwd(gpu, F32, x, np.float32(gamma), 4, want_codes=True)
        assert rc == 0 and not _load(out).any() and not codes.cpu().numpy().any()


# ----------------------------------------------------------------------------- 2. forward codes
@pytest.mark.parametrize("nbits", [4, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_codes(gpu, dtype, nbits):
    n = 1001 * 48
    gamma = np.float32(6.0)
    levels = 2 ** nbits - 1
    unit = np.float32(gamma / np.float32(levels))
    x = np.abs(_inputs(n, dtype, gamma, unit, seed=nbits))
    rc, out, codes, u = _fwd(gpu, dtype, x, gamma, nbits, want_codes=True)
    assert rc == 0
    want, wcodes, wunit = U.pact_fwd_ref(x, gamma, nbits, to_bf16=dtype == BF16)
    q = codes.cpu().numpy().astype(np.float32)
    assert _load(u)[0] == wunit == np.float32(gamma / np.float32(levels))
    assert q.min() >= 0 and q.max() == levels  # (elements at and above gamma take the last code)
    assert np.array_equal(q, wcodes)
    stored = (q * wunit).astype(np.float32)
    assert np.array_equal(_load(out), U.bf16(stored) if dtype == BF16 else stored)
    assert np.array_equal(_load(out), want)
    rc2, out2, _, _ = _fwd(gpu, dtype, x, gamma, nbits, want_codes=False)
    assert rc2 == 0 and torch.equal(out, out2)  # the values-only form gives the same values
    rc3, _, codes3, _ = _fwd(gpu, dtype, x, gamma, nbits, want_codes=True, want_out=False)
    assert rc3 == 0 and torch.equal(codes, codes3)  # codes only


def test_forward_codes_refuse_eight_bits(gpu):
    x = np.abs(_inputs(4160, F32, np.float32(6.0), np.float32(0.1), seed=1))
    rc, out, codes, _ = _fwd(gpu, F32, x, np.float32(6.0), 8, want_codes=True)
    assert rc == -1
    assert b"nbits <= 7" in L.load().rn_last_error()
    assert (codes.cpu().numpy() == -9).all() and (_load(out) == 77.0).all()  # nothing was launched
    rc, _, _, _ = _fwd(gpu, F32, x[:4150], np.float32(6.0), 4, want_codes=True)
    assert rc == -1 and b"multiple of 16" in L.load().rn_last_error()


# ----------------------------------------------------------------------------- 3. backward
def _bwd(dev, dtype, x, dy, gamma, add=None, alias=False):
    lib = L.load()
    n = x.size
    xd, dyd = _store(x, dtype, dev), _store(dy, dtype, dev)
    addd = _store(add, dtype, dev) if add is not None else None
    dx = dyd if alias else torch.full((n,), 55.0, dtype=tdt(dtype), device=dev)
    g = torch.tensor([gamma], dtype=torch.float32, device=dev)
    dg = torch.full((3,), 123.0, dtype=torch.float32, device=dev)  # (written, not accumulated; neighbours untouched)
    nws = int(lib.rn_pact_bwd_ws_bytes(n))
    assert nws == 4 * min(max(-(-n // 2048), 1), 2048)
    ws = torch.full((nws // 4 + 1,), -1.0, dtype=torch.float32, device=dev)
    rc = lib.rn_pact_bwd(dtype, n, p(xd), p(dyd), p(g), p(dx), p(addd), C.c_void_p(dg.data_ptr() + 4), p(ws),
                         stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.rn_last_error()
    dgv = _load(dg)
    assert dgv[0] == 123.0 and dgv[2] == 123.0 and _load(ws)[-1] == -1.0
    return _load(dx), dgv[1]


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward(gpu, dtype, n, with_add):
    gamma = np.float32(1.25)
    rng = np.random.RandomState(n + 7 * with_add)
    x = _inputs(n, dtype, gamma, np.float32(gamma / 15), seed=n)
    rd = (lambda a: U.bf16(a)) if dtype == BF16 else (lambda a: a)
    dy = rd(rng.randn(n).astype(np.float32))
    add = rd(rng.randn(n).astype(np.float32)) if with_add else None
    dx, dg = _bwd(gpu, dtype, x, dy, gamma, add)
    want_dx, want_dg, abs_sum = U.pact_bwd_ref(x, dy, gamma, add, to_bf16=dtype == BF16)
    assert np.array_equal(dx, want_dx)
    assert abs_sum > 0  # (something is clipped: elements equal to gamma and above it)
    # |fp32 sum - exact sum| <= k * 2^-24 * sum |terms|, k the longest chain of fp32 additions a term passes
    # through (pact_util.pact_bwd_chain, from the launch geometry): first order in 2^-24, k <= 129 here
    k = U.pact_bwd_chain(n, 2 if dtype == BF16 else 4)
    bound = k * 2.0 ** -24 * abs_sum
    print("n %d dtype %d: dgamma %.9g, fp64 %.9g, |diff| %.3g, bound %.3g (k = %d)"
          % (n, dtype, dg, want_dg, abs(dg - want_dg), bound, k))
    assert abs(float(dg) - want_dg) <= bound
    dx2, dg2 = _bwd(gpu, dtype, x, dy, gamma, add)  # bit-reproducible from run to run
    assert np.array_equal(dx2, dx) and np.float32(dg2).tobytes() == np.float32(dg).tobytes()


def test_backward_chain_lengths():
    """The bound's k, by hand: n = 16 fp32 is 4 chunks on 4 threads of one block: 4 serial adds + 6 + 2, one
    partial in one lane; n = 48051 bf16 is 24 blocks, 6006 chunks on 6144 threads (one round of 8) and a 3-element
    tail, 24 partials in one lane; the capped grid: 2048 partials, 32 in each of 64 lanes."""
    assert U.pact_bwd_chain(16, 4) == 4 + 6 + 2 + 1 + 1
    assert U.pact_bwd_chain(1001 * 48 + 3, 2) == 8 + 1 + 6 + 2 + 24 + 1
    assert U.pact_bwd_chain(2048 * 2048 * 8, 2) == 8 * 8 + 6 + 2 + 32 + 64


def test_backward_in_place_and_nothing_clipped(gpu):
    n = 1001 * 48 + 3
    rng = np.random.RandomState(11)
    for dtype in DTYPES:
        gamma = np.float32(1.25)
        x = _inputs(n, dtype, gamma, np.float32(gamma / 15), seed=5)
        dy = rng.randn(n).astype(np.float32)
        dy = U.bf16(dy) if dtype == BF16 else dy
        dx, dg = _bwd(gpu, dtype, x, dy, gamma, alias=True)  # dx aliases dy
        want_dx, want_dg, abs_sum = U.pact_bwd_ref(x, dy, gamma, to_bf16=dtype == BF16)
        assert np.array_equal(dx, want_dx)
        assert abs(float(dg) - want_dg) <= U.pact_bwd_chain(n, 2 if dtype == BF16 else 4) * 2.0 ** -24 * abs_sum
        big = np.float32(np.abs(x).max() * 2)
        dx, dg = _bwd(gpu, dtype, x, dy, big)
        assert np.array_equal(dx, dy) and dg == 0.0 and not np.signbit(dg)


def test_beyond_the_grid_caps(gpu):
    """Sizes at which the capped grids stride more than once (the only other path of the three kernels): the
    fp32 values forward past 8192 * 256 chunks of 4, the bf16 codes forward past 8192 * 256 chunks of 16, the bf16
    backward past 2048 * 256 chunks of 8 (where the dgamma chain is its longest per thread)."""
    gamma, nbits = np.float32(3.0), 4
    unit = np.float32(gamma / 15)
    n = 8192 * 256 * 4 + 4 * 300 + 1
    x = _inputs(n, F32, gamma, unit, seed=2)
    rc, out, _, _ = _fwd(gpu, F32, x, gamma, nbits, want_codes=False)
    assert rc == 0 and np.array_equal(_load(out), U.pact_fwd_ref(x, gamma, nbits)[0])
    n = 8192 * 256 * 16 + 16 * 5
    x = np.abs(_inputs(n, BF16, gamma, unit, seed=3))
    rc, out, codes, _ = _fwd(gpu, BF16, x, gamma, nbits, want_codes=True)
    want, wcodes, _ = U.pact_fwd_ref(x, gamma, nbits, to_bf16=True)
    assert rc == 0 and np.array_equal(_load(out), want) and np.array_equal(codes.cpu().numpy(), wcodes.astype(np.int8))
    n = 2048 * 256 * 8 * 2 + 8 * 77 + 5
    x = x[:n]
    dy = U.bf16(np.random.RandomState(4).randn(n).astype(np.float32))
    dx, dg = _bwd(gpu, BF16, x, dy, gamma)
    want_dx, want_dg, abs_sum = U.pact_bwd_ref(x, dy, gamma, to_bf16=True)
    k = U.pact_bwd_chain(n, 2)
    assert k == 3 * 8 + 1 + 6 + 2 + 32 + 64
    print("n %d: dgamma %.9g, fp64 %.9g, bound %.3g" % (n, dg, want_dg, k * 2.0 ** -24 * abs_sum))
    assert np.array_equal(dx, want_dx) and abs(float(dg) - want_dg) <= k * 2.0 ** -24 * abs_sum


# ----------------------------------------------------------------------------- 4. plan routing
def _bound(sym, monkeypatch, int8_env=None):
    if int8_env is None:
        monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    else:
        monkeypatch.setenv("RN_INT8_MFMA", int8_env)
    mod = mx.mod.Module(sym, context=[mx.gpu(0)], precision="float32")
    mod.bind([("data", SHAPE)], [("softmax_label", (SHAPE[0],))])
    return mod.executor


def test_plan_routing(gpu, monkeypatch):
    ex = _bound(U.pact_unit_net(abits=4), monkeypatch)
    convs = [op for op in ex.plan.ops if op.kind == "conv"]
    pacts = [op for op in ex.plan.ops if op.kind == "pact"]
    assert len(convs) == 4 and all(op.int8 for op in convs)
    assert len(pacts) == 5 and [op.emit_codes for op in pacts] == [op.name != "fc1_data" for op in pacts]
    assert all((op.codes is not None) == op.emit_codes for op in pacts)
    for sym, env in ((U.pact_unit_net(abits=8), None), (U.pact_unit_net(abits=4), "0")):
        ex = _bound(sym, monkeypatch, env)
        assert not any(op.int8 for op in ex.plan.ops if op.kind == "conv")
        assert not any(op.emit_codes or op.codes is not None for op in ex.plan.ops if op.kind == "pact")
    # a PACT reading a tensor that no ReLU produced: its convolution multiplies the values
    data = mx.sym.Variable("data")
    x = mx.sym.Convolution(data=data, num_filter=64, kernel=(3, 3), stride=(2, 2), pad=(1, 1), no_bias=True,
                           name="conv0")
    from rn import graphs
    q = graphs.quant_conv("qneg", mx.sym.BatchNorm(x, fix_gamma=False, name="bn"), 64, (1, 1), (1, 1),
                          in_channels=64, act_op="PACT", abits=4)
    head = mx.sym.Pooling(data=mx.sym.Activation(mx.sym.BatchNorm(q, name="bn1"), act_type="relu"),
                          global_pool=True, kernel=(1, 1), pool_type="avg")
    s = mx.sym.SoftmaxOutput(mx.sym.FullyConnected(mx.sym.Flatten(head), num_hidden=4, name="fc"), name="softmax")
    ex = _bound(s, monkeypatch)
    assert [op.int8 for op in ex.plan.ops if op.kind == "conv"] == [False]
    assert [op.emit_codes for op in ex.plan.ops if op.kind == "pact"] == [False]


# ----------------------------------------------------------------------------- 5, 6. training steps
@pytest.fixture(scope="module")
def unit_case():
    """Seed and scales as tests/test_pact_cpu.py::test_cpu_context_step_against_fp64 checks them on mx.cpu(): the
    fp32 run's PACT codes stay within the cap against the free-running fp64 restatement (1 % of a node's elements,
    one code)."""
    sym = U.pact_unit_net(abits=4, wbits=8, pact_init=2.0)
    params = U.init_net(sym, SHAPE, seed=0)
    data, label = U.batch(SHAPE, 8, seed=1)
    return sym, params, data, label


@pytest.mark.parametrize("int8", ["1", "0"])
def test_training_step_against_fp64(gpu, monkeypatch, unit_case, int8):
    """One fp32 step of stem conv -> bottleneck unit (256 -> 64 -> 64 -> 256, projection shortcut, 8 x 8, batch 2)
    -> head, every activation quantizer a 4-bit PACT, 8-bit Quantization_int8 weights: probabilities, every
    gradient (each PACT gamma's too) and every parameter after the SGD step with weight decay, against the fp64
    restatement replaying the device's ReLU masks, quantized weights, PACT codes and x < gamma masks."""
    sym, params, data, label = unit_case
    monkeypatch.setenv("RN_INT8_MFMA", int8)
    res = U.module_step(sym, params, data, label, mx.gpu(0), steps=2)
    ex = res["mod"].executor
    assert all(op.int8 == (int8 == "1") for op in ex.plan.ops if op.kind == "conv")
    U.check_step(res, sym, params, data, label, step=0)
    gammas = [k for k in params if k.endswith("_data_gamma")]
    assert len(gammas) == 5
    clipped = [k for k in gammas if res["grads"][0][k][0] != 0]
    assert len(clipped) >= 4, {k: res["grads"][0][k] for k in gammas}
    # the second step of the same Module reads the gamma the first update left: it moved by more than its weight
    # decay alone (lr * wd * gamma = 2e-5 here), and the unit the second forward wrote is f32(gamma_new / L)
    lr, wd = 0.1, 1e-4
    for k in gammas:
        g0, g1 = np.float32(params[k][0]), np.float32(res["args"][0][k][0])
        if k in clipped:
            assert abs(float(g1) - float(g0) * (1 - lr * wd)) > 1e-4, (k, g0, g1)
        d = res["decisions"][1]["pact"][k]
        assert np.float32(d["gamma"]) == g1
        assert np.float32(d["unit"]) == np.float32(g1 / np.float32(15)), (k, d["unit"], g1)
        assert np.array_equal(d["values"].astype(np.float32), (d["codes"].astype(np.float32) * np.float32(d["unit"])))


def test_attached_graph_trains_and_checkpoints_on_gpu(gpu, tmp_path, monkeypatch):
    """The config-style run of tests/test_pact_cpu.py on mx.gpu(): attach_quantize_node with PACT (Custom) and
    PACT_CXX (contrib) activations on ResNet-20, bf16, two steps, checkpoint; both forms lower to the same plan."""
    from graph_passes import shape_dict
    from rn import graphs
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    base = graphs.resnet20_cifar()
    shapes = shape_dict(base, (4, 3, 32, 32), (4,))
    data, label = U.batch((4, 3, 32, 32), 10, seed=5)
    probs, plans = {}, {}
    for op_name in ("PACT", "PACT_CXX"):
        w, a = U.pact_settings(op_name, abits=4, init_value=3.0)
        sym = U.attach_quantize_node(base, shapes, w, a, skip_quantize_counts={"Convolution": 1})
        mod = mx.mod.Module(sym, context=[mx.gpu(0)])
        mod.bind([("data", (4, 3, 32, 32))], [("softmax_label", (4,))])
        mx.random.seed(3)
        mod.init_params(mx.init.Xavier(rnd_type="gaussian", factor_type="in", magnitude=2))
        mod.init_optimizer(optimizer="sgd", optimizer_params={"learning_rate": 0.1, "wd": 1e-4, "momentum": 0.9})
        b = mx.io.DataBatch(data=[mx.nd.array(data)], label=[mx.nd.array(label)])
        for _ in range(2):
            mod.forward(b, is_train=True)
            mod.backward()
            mod.update()
        probs[op_name] = mod.get_outputs()[0].asnumpy().copy()
        plans[op_name] = [(op.kind, op.name, getattr(op, "int8", None), getattr(op, "emit_codes", None))
                          for op in mod.executor.plan.ops]
        assert np.isfinite(probs[op_name]).all()
        prefix = str(tmp_path / op_name)
        mod.save_checkpoint(prefix, 2)
        _, arg, _ = mx.model.load_checkpoint(prefix, 2)
        gam = [k for k in arg if k.endswith("_gamma") and sym.attr_dict()[k].get("__init__")]
        assert len(gam) == 19 and any(arg[k].asnumpy()[0] != np.float32(3.0) for k in gam)
        assert all(0 < arg[k].asnumpy()[0] < 4 for k in gam)
    assert plans["PACT"] == plans["PACT_CXX"] and sum(1 for o in plans["PACT"] if o[0] == "pact") == 19
    assert sum(1 for o in plans["PACT"] if o[0] == "conv" and o[2]) == 20  # every conv but the skipped first
    np.testing.assert_allclose(probs["PACT"], probs["PACT_CXX"], atol=0.05)


# ----------------------------------------------------------------------------- 7. the network, layer by layer
def _pact_net(abits):
    """Two bottleneck units per stage: the smallest resnet_int8 graph with every unit form -- a stage-first unit
    whose act1 two PACTs read (conv1's and the shortcut's) at stride 1 and at stride 2, identity units, stage 1's
    64 -> 64 3x3, the pooled fc input. 29 PACTs, conv0 + 28 PACT-fed convolutions + fc1. pact_init = 1.0: at the
    default 8.0 no element of this initialisation is clipped (PACT)."""
    from rn import graphs
    return graphs.resnet_int8([2, 2, 2, 2], 4, [64, 256, 512, 1024, 2048], 1000, "float32", True, act_op="PACT",
                              wbits=8, abits=abits, pact_init=1.0)


@pytest.mark.parametrize("precision,abits,warm", [("bfloat16", 4, 1), ("bfloat16", 8, 1), ("float32", 4, 0)],
                         ids=["bf16_a4", "bf16_a8", "fp32_a4"])
def test_pact_network_layerwise(gpu, monkeypatch, precision, abits, warm):
    """Every kernel of one training step of the PACT network at 8 x 64 x 64 against its recompute from the
    device's own inputs (tests/layerwise.py): each rn_pact_fwd bit for bit (unit, values, int8 codes), the int8
    MFMA convolutions behind the 4-bit codes (stride-2 3x3, stride-2 1x1 shortcut, stage 1's 3x3) as exact sums
    of the device's codes, bf16 storage of the 8-bit values, each rn_pact_bwd's dx bit for bit -- the second
    reader of a stage-first act1 accumulating in place -- and its dgamma within the kernel's summation bound, in
    its own slot of the flat gradient buffer. lr = 0.001 for the warm step: at 0.1 it throws the thresholds to
    -1.8 .. 3.1 (three non-positive, one PACT clipping everything)."""
    from test_step_bf16_gpu import _layerwise
    monkeypatch.delenv("RN_INT8_MFMA", raising=False)
    ck = _layerwise(_pact_net(abits), 8, 64, precision, warm=warm, lr=0.001)
    # routing, before the numbers
    convs = [op for op in ck.ex.plan.ops if op.kind == "conv"]
    pacts = [op for op in ck.ex.plan.ops if op.kind == "pact"]
    assert len(convs) == 28 and len(pacts) == 29
    if abits == 4:
        assert all(op.int8 and op.qsrc.kind == "pact" for op in convs)
        assert [op.name for op in pacts if op.codes is None] == ["fc1_data"]
    else:
        assert not any(op.int8 for op in convs) and not any(op.codes is not None for op in pacts)
    assert not ck.skipped, ck.skipped
    assert not ck.fwd_skipped, ck.fwd_skipped
    # the inputs exercise the clip path (conditions on the inputs, sized from the fp32 CPU executor: 2.4 % ..
    # 16.9 % clipped per PACT, gammas 0.972 .. 1.021 after the warm step)
    assert sorted(ck.pact_stats) == sorted(op.name for op in pacts)
    st = ck.pact_stats
    print("clipped fraction %.4f .. %.4f, gamma %.4f .. %.4f, lowest top code %d" % (
        min(s["clipped"] for s in st.values()), max(s["clipped"] for s in st.values()),
        min(s["gamma"] for s in st.values()), max(s["gamma"] for s in st.values()),
        min(s["max_code"] for s in st.values())))
    bad = {k: s for k, s in st.items() if not 0.01 <= s["clipped"] <= 0.5}
    assert not bad, bad
    bad = {k: s for k, s in st.items() if not 0.5 < s["gamma"] < 1.5}
    assert not bad, bad
    if abits == 4:
        assert all(s["max_code"] == 15 for s in st.values()), st
    if warm:
        assert all(s["gamma"] != 1.0 for s in st.values()), st
    else:
        assert all(s["gamma"] == 1.0 for s in st.values()), st
    assert len(ck.pact_bwd) == 29 and all(c["dgamma"] != 0.0 for c in ck.pact_bwd), ck.pact_bwd
    # the numbers
    bad = ck.failures()
    assert not bad, bad[:10]
    count = lambda kind: sum(1 for r in ck.rec if r[0] == kind)  # noqa: E731
    assert count("pact") == 29
    assert ck.covered["rn_pact_bwd"] == 29 and count("pact_bwd") == 29
    assert count("weight_quant") == 30  # conv0, 28 convolutions, fc1
    assert count("conv_fwd_i8") == (28 if abits == 4 else 0)
    assert count("conv_fwd") == (1 if abits == 4 else 29)  # (conv0 in the stem, always on the values)
    # the second reader of each stage-first act1 adds into the gradient the first one wrote
    with_add = [c for c in ck.pact_bwd if c["add"]]
    assert len(with_add) >= 4 and all(c["aliased"] for c in with_add), ck.pact_bwd
