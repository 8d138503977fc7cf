"""End-to-end on the reference's only OCR fixture (misc/textline.bin.png, 'performance analysis'):
the reference's own CLI test (test-ocr.sh:4-8) through the drop-in drivers, and step-by-step parity
of online SGD on that line against the oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

from common import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "clstm_amd", "bin")
FIXTURE = os.path.join(ROOT, "tests", "golden", "textline.bin.png")
GT = open(os.path.join(ROOT, "tests", "golden", "textline.gt.txt"), encoding="utf-8").read().rstrip("\n")


def fixture_frames(tmp_path):
    out = tmp_path / "n.raw"
    subprocess.run([os.path.join(BIN, "clstm_hosttool"), "normalize", FIXTURE, str(out), "48"], check=True,
                   capture_output=True)
    data = open(out, "rb").read()
    w, h = struct.unpack("<ii", data[:8])
    return np.frombuffer(data[8:], np.float32).reshape(w, h).copy()     # [T][48]


@pytest.mark.gpu
def test_reference_cli_test_ocr(tmp_path):
    """test-ocr.sh: train 201 iterations on the fixture (lrate 1e-2), load _ocrtest-200.clstm,
    clstmocr must print 'performance analysis'."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    lst = tmp_path / "list.txt"
    png = tmp_path / "textline.bin.png"
    png.write_bytes(open(FIXTURE, "rb").read())
    (tmp_path / "textline.gt.txt").write_text(GT + "\n", encoding="utf-8")
    lst.write_text(str(png) + "\n")
    env = dict(os.environ, ntrain="201", hidden="50", lrate="1e-2", save_name=str(tmp_path / "_ocrtest"), seed="0.222")
    r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), str(lst)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "#: ntrain = 201" in r.stderr                     # the reference's parameter echo (utils.h:161-167)
    assert "TRU performance analysis" in r.stdout and "saving" in r.stdout
    model = tmp_path / "_ocrtest-200.clstm"
    assert model.exists()
    env2 = dict(os.environ, load=str(model))
    r2 = subprocess.run([os.path.join(BIN, "clstmocr"), str(lst)], env=env2, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert "performance analysis" in r2.stdout
    # clstmocr.cc:96-97 writes the recognised text next to the image (<base>.txt)
    assert (tmp_path / "textline.bin.txt").read_text().strip() == "performance analysis"
    # resume: the saved trial attribute makes training continue at 201 (clstmocrtrain.cc:157)
    env3 = dict(os.environ, load=str(model), ntrain="203", save_name="", lrate="1e-2")
    r3 = subprocess.run([os.path.join(BIN, "clstmocrtrain"), str(lst)], env=env3, capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0 and "start 201" in r3.stdout


@pytest.mark.gpu
def test_fixture_online_sgd_matches_oracle(tmp_path, ora32):
    """CLSTMOCR::train on the fixture line, batch = 1 (BASELINE.json configs[1]): decodes must be
    identical to the oracle's at every step, parameters stay within float noise."""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    x = fixture_frames(tmp_path)
    chars = sorted(set(GT))
    codec = [0] + [ord(c) for c in chars]
    tr = np.array([codec.index(ord(c)) for c in GT], np.int32)
    nc = len(codec)
    p0 = init_params(48, 100, nc, seed=0.222)
    ref = OracleNet(ora32, 48, 100, nc, init=False)
    ref.set_params(p0); ref.set_lr(1e-2, 0.9)
    net = Network(48, 100, nc)
    net.set_params(p0); net.setLearningRate(1e-2, 0.9)
    for step in range(12):
        want_dec = ref.train_line(x, tr).tolist()
        net.set_inputs([x]); net.forward()
        got_dec = net.decode()[0].tolist()
        net.ctc([tr]); net.backward(); net.update()
        assert got_dec == want_dec, "decode differs at step %d" % step
        assert_close(net.get_params(), ref.get_params(), rtol=1e-4, atol=1e-9, scale_atol=1e-4, what="params step %d" % step)


@pytest.mark.gpu
def test_reference_cli_test_filter(tmp_path):
    """test-filter.sh:5-9: clstmfiltertrain learns 'hello' -> 'hello' in 1001 iterations (lrate 1e-2),
    clstmfilter with _filter-1000.clstm prints hello.  (run-cmu is the same path on misc/cmu-*.txt.)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    txt = tmp_path / "_filter.txt"
    txt.write_text("hello\thello\n")
    env = dict(os.environ, hidden="20", ntrain="1001", neps="0", report_every="200", save_every="1000", lrate="1e-2",
               save_name=str(tmp_path / "_filter"))
    r = subprocess.run([os.path.join(BIN, "clstmfiltertrain"), str(txt)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "INP hello" in r.stdout
    model = tmp_path / "_filter-1000.clstm"
    assert model.exists()
    r2 = subprocess.run([os.path.join(BIN, "clstmfilter"), str(txt)], env=dict(os.environ, load=str(model)),
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "hello" in r2.stdout.split("\n")


@pytest.mark.gpu
def test_full_bench_shape_minibatch_vs_oracle(ora32):
    """BASELINE configs[2] at full size -- BiLSTM(100), H=48, 83 classes, 64 lines of T=200, 25 labels:
    every activation, delta, CTC posterior, decode, the minibatch gradient and the updated parameters of the
    HIP path against the oracle (the oracle needs ~1 s for this).  Activations: 1e-4 relative.  The CTC
    posteriors of a 200-frame line amplify the ~1e-6 input differences of the two f32 mat-mul orders by
    two orders of magnitude (lattice values of magnitude 5*S carry the log-domain sums), so `aligned` and
    everything downstream of it is held to 1e-3 here; with identical inputs the CTC kernel matches the
    oracle to 1e-4 (tests/test_ops_parity.py::test_ctc_vs_oracle, T = 200)."""
    from common import Backend
    from test_net_parity import run_case
    run_case(Backend("hip"), ora32, 48, 100, 83, [200] * 64, scale=10.0, seed=11, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3)


@pytest.mark.gpu
def test_full_bench_shape_128_lines_fill_the_chip(ora32):
    """The same shape with 128 lines: 256 recurrence workgroups = one per CU, no idle half of the chip -- the forward pass
    runs as separate launches (batched gate GEMM, recurrence, fused softmax), the backward recurrence shares its launch
    with the weight-gradient items without spare CUs.  Same bars as the 64-line case."""
    from common import Backend
    from test_net_parity import run_case
    run_case(Backend("hip"), ora32, 48, 100, 83, [200] * 128, scale=10.0, seed=13, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3)


@pytest.mark.gpu
def test_full_bench_shape_ragged_lines(ora32):
    """Same architecture, ragged line lengths U{150..250} and a one-frame line in the same minibatch."""
    from common import Backend
    from test_net_parity import run_case
    rng = np.random.default_rng(3)
    T = [int(t) for t in rng.integers(150, 251, 15)] + [1]
    run_case(Backend("hip"), ora32, 48, 100, 83, T, scale=10.0, seed=12, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3)


@pytest.mark.gpu
def test_full_bench_shape_ragged_64_lines(ora32):
    """The ragged minibatch `bench.py --ragged` times: 64 lines of T ~ U{150..250} (the 16-line test above is not
    the shape the bench line runs).  Same bars as the fixed-T full-shape test."""
    from common import Backend
    from test_net_parity import run_case
    rng = np.random.default_rng(1000)
    T = [int(t) for t in rng.integers(150, 251, 64)]
    run_case(Backend("hip"), ora32, 48, 100, 83, T, scale=10.0, seed=14, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["fixed", "ragged"])
@pytest.mark.parametrize("strict", [False, True])
def test_full_bench_shape_trained_weights_real_line_crops(ora32, shape, strict):
    """The bench shape in the TRAINED regime: the weight set after 500 oracle online-SGD
    steps on the reference's fixture (tests/trained_weights.py: the oracle then reads the fixture as "performance analysis",
    max |parameter| ~8, 17 % of the input-gate activations saturated, mean max posterior 0.98) on 64 REAL line crops of the
    normalised fixture with jitter (T = 200, and the ragged T ~ U{150..250}), each with the transcript the oracle decodes on
    it -- peaked posteriors: the 1e-5 floor + renormalisation of ctc.cc:62-66, log_add's |x - y| > 10 cut-off
    (tensor.h:78-85) and limexp (ctc.cc:88-92) are hit on most frames, where the noise inputs of the tests above give
    near-uniform posteriors.  Decodes bit-exact; CTC posteriors / deltas / gradient / update 1e-3 as in
    test_full_bench_shape_minibatch_vs_oracle; both backward arithmetics (default split products and strict_f32).

    Saved activations: 1e-4 relative, over an absolute floor that the float64 oracle sets per state array.  With these
    weights (|w| up to 8) the recurrence is no longer contractive: a 1e-7 difference in h_t (two float32 summation orders)
    grows along the 200 steps, and the FLOAT32 ORACLE ITSELF is 1e-5..1e-4 away from the float64 oracle at the worst entry.
    No float32 implementation (Eigen's included) can be held closer to another than both are to exact arithmetic, so the
    floor is 3 x max |oracle32 - oracle64| of that array (never below 1e-5), and the referee check is explicit: the HIP
    activations must be as close to the float64 oracle as the float32 oracle's are (within 3x + 1e-6; both printed)."""
    _trained_crops_case(ora32, shape, strict, forced_mfma=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["fixed", "ragged"])
@pytest.mark.parametrize("strict", [False, True])
def test_full_bench_shape_trained_weights_forced_batched_kernels(ora32, shape, strict):
    """The SAME 64 crops, weights, bars and referee check as the test above through the other kernel family: the recurrences
    batched over 16 lines on the MFMA (lstm_mfma.h f16 x 2, lstm_mfma_bwd.h bf16 x 2; the default from 640 lines per GPU on),
    forced with fwd_mfma = 2 / bwd_mfma = 2 -- path counters 16 / 17 must move.  strict: the forced option wins over
    clstm_net_set_strict_f32 (include/clstm_abi.h), which then still selects the f32 MFMA for the weight-gradient products.
    The 640-line minibatches by the library's own rule: tests/test_mfma_bench_shapes.py."""
    _trained_crops_case(ora32, shape, strict, forced_mfma=True)


def _trained_crops_case(ora32, shape, strict, forced_mfma):
    import ctypes
    from common import Backend, oracle_minibatch
    from oracle.oracle import Oracle, OracleNet
    from test_net_parity import run_case
    from trained_weights import NC, NH, NI, fixture_crops, trained_like_params
    params, reads_fixture = trained_like_params(ora32)
    assert reads_fixture
    dec_net = OracleNet(ora32, NI, NH, NC, init=False)
    dec_net.set_params(params)
    rng = np.random.default_rng(21 if shape == "fixed" else 22)
    T = [200] * 64 if shape == "fixed" else [int(t) for t in rng.integers(150, 251, 64)]
    lines, trs = fixture_crops(rng, T, dec_net)
    assert sum(len(t) > 1 for t in trs) >= 60          # the trained net reads the crops
    keys = [(0, d, w) for d in (0, 1) for w in ("gi", "gf", "go", "ci", "state", "outputs")]
    dkeys = [(0, d, w) for d in (0, 1) for w in ("d_gi", "d_gf", "d_go", "d_ci")]
    ex = oracle_minibatch(Oracle("f64"), OracleNet, params.astype(np.float64), NI, NH, NC, lines, trs, states=keys + dkeys)
    o32 = oracle_minibatch(ora32, OracleNet, params, NI, NH, NC, lines, trs, states=keys + dkeys)
    exact, ora = ex["states"], o32["states"]
    e_ora = {k: max(float(np.abs(ora[k][b] - exact[k][b]).max()) for b in range(len(T))) for k in keys}
    # deltas and the gradient inherit that: their bar is 1e-3 of the array's largest entry, or 3 x what the float32 oracle
    # itself is away from the float64 oracle on that line, whichever is larger
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    d_tol = {k: max(1e-3, 3.0 * max(rel(ora[k][b], exact[k][b]) for b in range(len(T)))) for k in dkeys}
    g_tol = max(1e-3, 3.0 * rel(o32["derivs"], ex["derivs"]))
    print("trained %s: float32 oracle vs float64 oracle: gradient %.3g of max, gate deltas up to %.3g of a line's max"
          % (shape, rel(o32["derivs"], ex["derivs"]), max(d_tol.values()) / 3.0))
    be = Backend("hip")

    def count(which):
        out = ctypes.c_longlong(0)
        be.lib.call("clstm_debug_path_count", which, ctypes.byref(out))
        return out.value
    try:
        if forced_mfma:
            be.lib.call("clstm_debug_set_option", b"fwd_mfma", 2)
            be.lib.call("clstm_debug_set_option", b"bwd_mfma", 2)
        before, routed = (count(16), count(17)), count(21)
        net, _ = run_case(be, ora32, NI, NH, NC, T, lr=1e-4, ctc_rtol=1e-3, grad_tol=g_tol, params=params, lines=lines,
                          trs=trs, strict_f32=strict, act_atol={k: max(1e-5, 3.0 * e_ora[k]) for k in keys}, delta_tol=d_tol)
        net2 = net.__class__(NI, NH, NC, lib=net.lib)        # (run_case's net has been updated: a fresh forward pass)
        net2.set_params(params)
        net2.set_inputs(lines)
        net2.forward()
        after = count(16), count(17)
        assert count(21) == routed, "the batched forward kernel handed the minibatch to the per-line kernels"
        if forced_mfma:
            assert after == (before[0] + 2, before[1] + 1), "the batched kernels did not run: %s -> %s" % (before, after)
        else:
            assert after == before, "64 lines took the batched kernels: %s -> %s" % (before, after)
        for k in keys:
            got = net2.split(net2.state(*k))
            e_hip = max(float(np.abs(got[b] - exact[k][b]).max()) for b in range(len(T)))
            print("trained %s%s %s: max |hip - f64| %.3g, max |oracle32 - f64| %.3g" % (shape, " (batched kernels)" if forced_mfma else "", k, e_hip, e_ora[k]))
            assert e_hip <= 3.0 * e_ora[k] + 1e-6, (k, e_hip, e_ora[k])
    finally:
        be.lib.call("clstm_debug_set_option", None, 0)


@pytest.mark.gpu
def test_configs4_ragged_lines_both_precisions(ora32):
    """BASELINE configs[4] architecture on RAGGED lines, T ~ U{300..500}, 32 lines (two 16-line blocks x two directions = four
    groups of the persistent kernels, lines dropping out of the lock-step at different steps), weights at 2 x the reference's
    init (contractive: float32 rounding is not amplified, see ..._strict_at_reference_init).  Exact-f32 path: every saved
    activation of four lines and all softmax outputs inside the 1e-4 bar, decodes identical, gradient at the qualified 1e-3.
    bf16 mode: the stated tolerances of test_configs4_full_shape_bf16_vs_oracle."""
    from common import Backend, synth_lines
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    c = C4
    rng = np.random.default_rng(46)
    T = [int(t) for t in rng.integers(300, 501, 32)]
    keep = (0, 11, 21, 31)
    params = init_params(c["ni"], c["nh"], c["nc"], seed=0.222) * 2.0
    lines = synth_lines(rng, T, c["ni"])
    trs = [rng.integers(1, c["nc"], c["L"]).astype(np.int32) for _ in T]
    ref = OracleNet(ora32, c["ni"], c["nh"], c["nc"], init=False)
    ref.set_params(params)
    want = ref.minibatch(lines, trs, keep=keep)
    be = Backend("hip")
    for precision in (0, 2):
        net = Network(c["ni"], c["nh"], c["nc"], lib=be.lib)
        net.set_params(params)
        if precision:
            net.set_gemm_precision(precision)
        net.set_inputs(lines)
        net.forward()
        got = net.split(net.outputs())
        dec = [d.tolist() for d in net.decode()]
        same = sum(dec[b] == want["decode"][b].tolist() for b in range(len(T)))
        if precision == 0:
            for b in range(len(T)):
                assert_close(got[b], want["outputs"][b], rtol=1e-4, atol=2e-6, what="softmax outputs line %d" % b)
            for layer in (0, 1):
                for d in (0, 1):
                    for which in ("gi", "gf", "go", "ci", "state", "outputs"):
                        s = net.split(net.state(layer, d, which))
                        for b in keep:
                            assert_close(s[b], _c4_state(want["kept"][b], layer, d, which), rtol=1e-4, atol=2e-6,
                                         what="L%d dir%d %s line %d" % (layer, d, which, b))
            assert same == len(T)
        net.ctc(trs)
        net.backward()
        g = net.get_grads()
        gerr = float(np.abs(g - want["derivs"]).max() / np.abs(want["derivs"]).max())
        if precision == 0:
            assert gerr < 1e-3, gerr
        else:
            err = max(float(np.abs(got[b] - want["outputs"][b]).max()) for b in range(len(T)))
            print("ragged configs[4] bf16 vs the f32 oracle: max |dz| %.3g, %d / %d decodes identical, gradient error %.3g of max" % (err, same, len(T), gerr))
            assert np.isfinite(g).all() and err < 1e-2 and same >= len(T) - 1 and gerr < 1.5e-3


@pytest.mark.gpu
def test_stacked_bilstm512_shape_vs_oracle(ora32):
    """BASELINE configs[4] architecture (2 x BiLSTM(512), H=64, 100 classes) on a few short lines: the
    lock-step MFMA recurrence and the stacked dX GEMM at their real widths (K = 512 / 2048 / 4096)."""
    from common import Backend
    from test_net_parity import run_case
    run_case(Backend("hip"), ora32, 64, [512, 512], 100, [24, 17, 9], scale=3.0, seed=13, lr=1e-4)


@pytest.mark.gpu
def test_lockstep_launch_loop_replayed_as_hipgraph(ora32):
    """On a real (capturable) stream the per-step launches of the lock-step recurrence are captured into a
    hipGraph at the first pass and replayed afterwards: first pass, replay and the plain-launch path on the
    default stream must give identical gradients."""
    import torch
    from common import Backend, synth_lines
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    be = Backend("hip")
    rng = np.random.default_rng(31)
    ni, nh, nc, T = 8, 132, 7, [21, 30, 9]
    params = OracleNet(ora32, ni, nh, nc, seed=0.222).get_params() * 10.0
    lines = synth_lines(rng, T, ni)
    trs = [rng.integers(1, nc, max(1, t // 3)).astype(np.int32) for t in T]

    def run(net, reps):
        out = []
        for _ in range(reps):
            net.set_inputs(lines)
            net.forward()
            net.ctc(trs)
            net.backward()
            out.append(net.get_grads().copy())
        return out

    net0 = Network(ni, nh, nc, lib=be.lib)
    net0.set_params(params)
    ref = run(net0, 1)[0]
    st = torch.cuda.Stream()
    try:
        be.lib.call("clstm_set_stream", st.cuda_stream)
        net1 = Network(ni, nh, nc, lib=be.lib)
        net1.set_params(params)
        first, replay = run(net1, 2)
        be.lib.call("clstm_synchronize")
    finally:
        be.lib.call("clstm_set_stream", 0)
    assert np.array_equal(first, ref)
    assert np.array_equal(replay, ref)


@pytest.mark.gpu
def test_clstmocrtrain_minibatch_driver(tmp_path):
    """batch=4 through the C++ driver (prefetch thread + CLSTMOCR::train_batch): four copies of the fixture per
    update at a quarter of the learning rate is the online run of test-ocr.sh with the same summed gradient, so
    200 updates must again learn 'performance analysis'."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    lst = tmp_path / "list.txt"
    png = tmp_path / "textline.bin.png"
    png.write_bytes(open(FIXTURE, "rb").read())
    (tmp_path / "textline.gt.txt").write_text(GT + "\n", encoding="utf-8")
    lst.write_text(str(png) + "\n")
    env = dict(os.environ, ntrain="804", batch="4", hidden="50", lrate="2.5e-3", save_every="200", report_every="200",
               save_name=str(tmp_path / "_mb"), seed="0.222")
    r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), str(lst)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    model = tmp_path / "_mb-800.clstm"
    assert model.exists(), r.stdout[-1000:]
    r2 = subprocess.run([os.path.join(BIN, "clstmocr"), str(lst)], env=dict(os.environ, load=str(model)),
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert "performance analysis" in r2.stdout


def _lrand48_stream():
    """glibc lrand48() without srand48(): X <- (0x5DEECE66D X + 0xB) mod 2^48, result X >> 17.  glibc's state starts
    at X0 = 0 (zero-initialised static data; POSIX's 0x1234ABCD330E only applies after srand48), so the first draw is 0."""
    x = 0
    while True:
        x = (0x5DEECE66D * x + 0xB) & ((1 << 48) - 1)
        yield x >> 17


@pytest.mark.gpu
def test_run_cmu_driver_matches_oracle(tmp_path, ora32):
    """BASELINE configs[0], `run-cmu` (run-cmu:2-12, clstmfiltertrain.cc:66-153): the first 1000 lines of
    misc/cmu-train.txt through the C++ driver on the GPU against the oracle's online SGD on the same sample
    sequence.  The environment is run-cmu's (note that `hidden=50` is not a variable the driver reads -- the
    reference trains nhidden=100 -- and that `neps` stays 3, clstmhl.h:53).  Decoded strings of every trial must be
    identical; the weights after 120 updates within 1e-5 + 1e-3 |w| (online float32 SGD, two summation orders)."""
    from clstm_amd.init import init_params
    from oracle.oracle import OracleNet
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    src = os.path.join(ROOT, "tests", "golden", "cmu-train-1000.txt")
    samples = []
    for line in open(src, encoding="utf-8").read().split("\n"):
        if not line or line.startswith("#") or "\t" not in line:
            continue
        a, b = line.split("\t", 1)
        if a and b:
            samples.append((a, b))
    icodec = sorted({0} | {ord(c) for a, _ in samples for c in a})
    codec = sorted({0} | {ord(c) for _, b in samples for c in b})
    N, neps, nh = 120, 3, 100
    env = dict(os.environ, ntrain=str(N + 1), hidden="50", test_every="50000", lrate="3e-4", report_every="1",
               save_every=str(N), save_name=str(tmp_path / "cmu"), neps="3")
    env.pop("seed", None)
    r = subprocess.run([os.path.join(BIN, "clstmfiltertrain"), src], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "got %d inputs, 0 tests" % len(samples) in r.stdout
    outs = [l[4:] for l in r.stdout.split("\n") if l.startswith("OUT ") or l == "OUT"]
    inps = [l[4:] for l in r.stdout.split("\n") if l.startswith("INP ")]
    assert len(outs) == N + 1 and len(inps) == N + 1
    ref = OracleNet(ora32, len(icodec), nh, len(codec), init=False)
    ref.set_params(init_params(len(icodec), nh, len(codec), seed=0.1))
    ref.set_lr(3e-4, 0.9)
    rnd = _lrand48_stream()
    for trial in range(N):
        a, b = samples[next(rnd) % len(samples)]
        assert inps[trial] == a
        cs = [icodec.index(ord(c)) for c in a]
        T = len(cs) * (neps + 1) + neps
        x = np.zeros((T, len(icodec)), np.float32)
        for i, c in enumerate(cs):
            x[neps + i * (neps + 1), c] = 1.0
        dec = ref.train_line(x, np.array([codec.index(ord(c)) for c in b], np.int32))
        assert "".join(chr(codec[k]) for k in dec) == outs[trial].strip(), "decode differs at trial %d" % trial
    raw = tmp_path / "p.f32"
    subprocess.check_call([os.path.join(BIN, "clstm_hosttool"), "params", str(tmp_path / ("cmu-%d.clstm" % N)), str(raw)])
    got = np.fromfile(raw, np.float32)
    assert_close(got, ref.get_params(), rtol=1e-3, atol=1e-5, what="weights after %d run-cmu updates" % N)


@pytest.mark.gpu
def test_full_shape_ctc_on_the_gpus_own_outputs(ora32):
    """Why the full-shape test above holds `aligned` to 1e-3 only: the lattice amplifies the ~1e-6 differences of the
    two softmax outputs (GPU vs oracle), not an error of the CTC kernel.  Fed the SAME posteriors -- the GPU's own
    softmax outputs at the bench shape, 64 lines of T = 200 through the net path -- the device CTC matches the
    oracle's ctc_align_targets to 1e-4 on `aligned` and on the deltas."""
    from common import Backend, synth_lines
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    be = Backend("hip")
    rng = np.random.default_rng(11)
    ni, nh, nc, T = 48, 100, 83, [200] * 64
    params = OracleNet(ora32, ni, nh, nc, seed=0.222).get_params() * 10.0
    lines = synth_lines(rng, T, ni)
    trs = [rng.integers(1, nc, 25).astype(np.int32) for _ in T]
    net = Network(ni, nh, nc, lib=be.lib)
    net.set_params(params)
    net.set_inputs(lines)
    net.forward()
    probs = net.split(net.outputs())
    aligned = net.split(net.ctc(trs, want_aligned=True))
    for b in range(len(T)):
        want = ora32.ctc_align_classes(probs[b], ora32.mktargets(trs[b]))
        assert_close(aligned[b], want, rtol=1e-4, atol=1e-6, what="aligned (GPU posteriors), line %d" % b)


@pytest.mark.gpu
def test_full_shape_gradient_error_vs_float64(ora32, ora64):
    """The 1e-3 gradient tolerance of the full-shape tests, qualified: against the float64 oracle (the reference's
    `double=1` build) the GPU's minibatch gradient is as close as the float32 oracle's own -- the distance between the
    two float32 results is rounding noise of float32 summation orders, not a defect of either."""
    from common import Backend, oracle_minibatch, synth_lines
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    be = Backend("hip")
    rng = np.random.default_rng(21)
    ni, nh, nc, T = 48, 100, 83, [200] * 16
    params = OracleNet(ora32, ni, nh, nc, seed=0.222).get_params() * 10.0
    lines = synth_lines(rng, T, ni)
    trs = [rng.integers(1, nc, 25).astype(np.int32) for _ in T]
    g64 = oracle_minibatch(ora64, OracleNet, params, ni, nh, nc, lines, trs)["derivs"].astype(np.float64)
    g32 = oracle_minibatch(ora32, OracleNet, params, ni, nh, nc, lines, trs)["derivs"].astype(np.float64)
    net = Network(ni, nh, nc, lib=be.lib)
    net.set_params(params)
    net.set_inputs(lines); net.forward(); net.ctc(trs); net.backward()
    g = net.get_grads().astype(np.float64)
    scale = np.abs(g64).max()
    e_gpu, e_f32 = np.abs(g - g64).max() / scale, np.abs(g32 - g64).max() / scale
    print("max |g - g64| / max|g64|: GPU %.3g, f32 oracle %.3g" % (e_gpu, e_f32))
    assert e_gpu <= max(2.0 * e_f32, 2e-5), (e_gpu, e_f32)
    assert e_gpu < 1e-3 and e_f32 < 1e-3


# ---- BASELINE configs[4] at its stated size, anchored on the oracle ---------------------------------------------------
C4 = dict(ni=64, nh=[512, 512], nc=100, T=[400] * 64, L=50, scale=4.0, keep=(0, 21, 42, 63))


@pytest.fixture(scope="module")
def configs4_case(ora32, ora64):
    """2 x BiLSTM(512), H = 64, 100 classes, 64 lines x 400 frames, transcripts of 50 labels (clstm_prefab.cc:86-109
    `bidi2`, clstm.cc:600-653) through the f32 AND the f64 oracle, OpenMP over lines (oracle/clstm_oracle.c:
    ora_minibatch_lines).  The f64 run qualifies what float32 summation order can do at this depth (2 x 400 dependent
    steps per layer): a result is as good as the reference's own arithmetic when its distance from the f64 result is
    no larger than the f32 oracle's."""
    import time
    from common import synth_lines
    from clstm_amd.init import init_params
    from oracle.oracle import OracleNet
    c = C4
    rng = np.random.default_rng(44)
    params = init_params(c["ni"], c["nh"], c["nc"], seed=0.222) * c["scale"]
    lines = synth_lines(rng, c["T"], c["ni"])
    trs = [rng.integers(1, c["nc"], c["L"]).astype(np.int32) for _ in c["T"]]
    res = {"params": params, "lines": lines, "trs": trs}
    for name, ora in (("f32", ora32), ("f64", ora64)):
        net = OracleNet(ora, c["ni"], c["nh"], c["nc"], init=False)
        net.set_params(params)
        t0 = time.time()
        res[name] = net.minibatch(lines, trs, keep=c["keep"])
        print("oracle %s: 64 lines x 400 frames of 2 x BiLSTM(512) fwd + CTC + bwd in %.1f s on %d host threads"
              % (name, time.time() - t0, min(64, os.cpu_count() or 1)))
    return res


def _rel_excess(a, b, rtol, atol):
    """largest |a - b| / (atol + rtol |b|): <= 1 means inside the bar"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())


def _c4_state(view, layer, d, which):
    s = view.state(layer, d, which)[:, 0, :]
    return s[::-1] if d == 1 else s


@pytest.mark.gpu
def test_configs4_full_shape_f32_vs_oracle(configs4_case):
    """BASELINE configs[4] at FULL size, exact-f32 path of the library against the oracle: softmax outputs of all 25,600
    frames and every gate activation / cell state / output of both layers and directions on four of the lines (first,
    last, two in between), CTC argmax decodes of all 64 lines IDENTICAL, `aligned` and the minibatch gradient at the
    qualified tolerance of the B1 full-shape test.

    The bar for every gate activation, cell state and layer output is the north star's 1e-4 relative (+ 2e-6 absolute
    floor) against the f32 oracle, STRICTLY (round 4: a regression in the gates can no longer hide behind the float64
    criterion).  For the softmax outputs only, where the two float32 results are further apart than that, the float64 oracle
    decides: at this depth (2 layers x 400
    dependent steps of 512 cells whose recurrent gain is close to 1) float32 rounding is amplified until the f32 ORACLE
    itself sits 7e-6 (outputs of ~1e-2, i.e. 7e-4 relative) from the float64 result, so no float32 implementation can
    be within 1e-4 of another.  There the GPU must be as close to float64 as the reference's own float32 arithmetic is
    (factor 2, the criterion of test_full_shape_gradient_error_vs_float64).  Both numbers are printed per quantity."""
    from common import Backend
    from clstm_amd.net import Network
    c, r = C4, configs4_case
    want, w64 = r["f32"], r["f64"]
    net = Network(c["ni"], c["nh"], c["nc"], lib=Backend("hip").lib)
    net.set_params(r["params"])
    net.set_inputs(r["lines"])
    net.forward()
    report, bad = [], []

    def judge(name, got, f32, f64, strict):
        """got / f32 / f64: lists of arrays.  strict: the north star's 1e-4 bar against the f32 oracle, nothing else (every
        gate activation, cell state and layer output); not strict (the softmax outputs only: values of ~1e-2 behind two
        layers x 400 dependent steps, where the f32 oracle itself sits 7e-4 relative from float64): inside the bar OR as
        close to float64 as the f32 oracle is (factor 2)."""
        ex = max(_rel_excess(g, a, 1e-4, 2e-6) for g, a in zip(got, f32))
        e_gpu = max(float(np.abs(g - b).max()) for g, b in zip(got, f64))
        e_f32 = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(f32, f64))
        ok = ex <= 1.0 or (not strict and e_gpu <= 2.0 * e_f32)
        report.append("%-22s excess over the 1e-4 bar vs f32 oracle %7.3g | max dist from f64: GPU %.3g, f32 oracle %.3g%s"
                      % (name, ex, e_gpu, e_f32, "" if ok else "   <-- FAIL"))
        if not ok:
            bad.append(name)

    got = net.split(net.outputs())
    judge("softmax outputs", got, want["outputs"], w64["outputs"], strict=False)
    for layer in (0, 1):
        for d in (0, 1):
            for which in ("gi", "gf", "go", "ci", "state", "outputs"):
                s = net.split(net.state(layer, d, which))
                judge("L%d dir%d %s" % (layer, d, which), [s[b] for b in c["keep"]],
                      [_c4_state(want["kept"][b], layer, d, which) for b in c["keep"]],
                      [_c4_state(w64["kept"][b], layer, d, which) for b in c["keep"]], strict=True)
    print("\n".join(report))
    assert not bad, bad
    dec = net.decode()
    mism = [b for b in range(64) if dec[b].tolist() != want["decode"][b].tolist()]
    print("CTC argmax decodes: %d / 64 identical to the oracle" % (64 - len(mism)))
    assert not mism, mism
    al = net.split(net.ctc(r["trs"], want_aligned=True))
    for b in range(64):
        assert_close(al[b], want["aligned"][b], rtol=1e-3, atol=1e-6, what="aligned line %d" % b)
    net.backward()
    g = net.get_grads().astype(np.float64)
    g32, g64 = want["derivs"].astype(np.float64), w64["derivs"].astype(np.float64)
    scale = np.abs(g64).max()
    eg, e32 = np.abs(g - g64).max() / scale, np.abs(g32 - g64).max() / scale
    print("minibatch gradient, max |g - g64| / max |g64|: GPU %.3g, f32 oracle %.3g; GPU vs f32 oracle %.3g"
          % (eg, e32, np.abs(g - g32).max() / scale))
    assert_close(g, g32, rtol=1e-3, atol=1e-9, scale_atol=1e-3, what="minibatch gradient")
    assert eg <= max(2.0 * e32, 2e-5), (eg, e32)


@pytest.mark.gpu
def test_configs4_full_shape_f32_strict_at_reference_init(ora32):
    """The same architecture and size with the weights the reference itself starts from -- rinit 'negbiased', scale 0.01
    (clstm.cc:30-36, batches.cc:28-40), times 2 so that the gates leave 0.5 -- where the recurrence is contractive and
    float32 rounding is not amplified: here the north star's 1e-4 relative bar holds for the softmax outputs of all
    25,600 frames and every saved activation of four lines, strictly against the f32 oracle, and the decodes are equal."""
    import time
    from common import Backend, synth_lines
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    c = C4
    rng = np.random.default_rng(45)
    params = init_params(c["ni"], c["nh"], c["nc"], seed=0.222) * 2.0
    lines = synth_lines(rng, c["T"], c["ni"])
    trs = [rng.integers(1, c["nc"], c["L"]).astype(np.int32) for _ in c["T"]]
    ref = OracleNet(ora32, c["ni"], c["nh"], c["nc"], init=False)
    ref.set_params(params)
    t0 = time.time()
    want = ref.minibatch(lines, trs, keep=c["keep"])
    print("oracle f32: %.1f s" % (time.time() - t0))
    net = Network(c["ni"], c["nh"], c["nc"], lib=Backend("hip").lib)
    net.set_params(params)
    net.set_inputs(lines)
    net.forward()
    got = net.split(net.outputs())
    for b in range(64):
        assert_close(got[b], want["outputs"][b], what="softmax outputs line %d" % b)
    for layer in (0, 1):
        for d in (0, 1):
            for which in ("gi", "gf", "go", "ci", "state", "outputs"):
                s = net.split(net.state(layer, d, which))
                for b in c["keep"]:
                    assert_close(s[b], _c4_state(want["kept"][b], layer, d, which), what="state (%d, %d, %s) line %d" % (layer, d, which, b))
    dec = net.decode()
    assert all(dec[b].tolist() == want["decode"][b].tolist() for b in range(64))
    al = net.split(net.ctc(trs, want_aligned=True))
    for b in range(64):
        assert_close(al[b], want["aligned"][b], rtol=1e-3, atol=1e-6, what="aligned line %d" % b)
    net.backward()
    assert_close(net.get_grads(), want["derivs"], rtol=1e-3, atol=1e-9, scale_atol=1e-3, what="minibatch gradient")


@pytest.mark.gpu
def test_configs4_full_shape_bf16_vs_oracle(configs4_case):
    """BASELINE configs[4] at FULL size in precision mode 2 (bf16 MFMA operands in the lock-step recurrence and the
    hoisted GEMMs, f32 accumulation / state / softmax / CTC -- what `bench.py --config b2 --bf16` times) against the
    ORACLE.  Stated tolerance, not parity (bf16 has 8 bits of mantissa): softmax outputs within 1e-2 absolute, per-frame
    argmax differs in < 2 % of the frames, CTC decodes of >= 62 / 64 lines identical, minibatch gradient within 1.5e-3 of
    its largest entry.  Measured on MI355X: 4.7e-3, 0.84 %, 64 / 64, 7.3e-4 (<= 2x measured everywhere)."""
    from common import Backend
    from clstm_amd.net import Network
    c, r = C4, configs4_case
    want = r["f32"]
    be = Backend("hip")
    net = Network(c["ni"], c["nh"], c["nc"], lib=be.lib)
    net.set_params(r["params"])
    net.set_gemm_precision(2)
    net.set_inputs(r["lines"])
    net.forward()
    got = net.split(net.outputs())
    dec = [d.tolist() for d in net.decode()]
    net.ctc(r["trs"])
    net.backward()
    g = net.get_grads()
    import ctypes
    for which, idx in (("persistent forward", 0), ("persistent backward", 1), ("bf16-source W_x.x", 2), ("bf16-source x.d", 3),
                       ("contraction-major W.d", 4), ("input projection inside the persistent forward kernel (layer 1)", 6),
                       ("W.d x-part read from the layer below's bf16 outputs (layer 2)", 8)):
        cnt = ctypes.c_longlong(0)
        be.lib.call("clstm_debug_path_count", idx, ctypes.byref(cnt))
        assert cnt.value > 0, "the %s kernel did not run" % which
    assert np.isfinite(g).all() and all(np.isfinite(o).all() for o in got)
    err = max(float(np.abs(got[b] - want["outputs"][b]).max()) for b in range(64))
    flips = float(np.mean([(got[b].argmax(1) != want["outputs"][b].argmax(1)).mean() for b in range(64)]))
    same = sum(dec[b] == want["decode"][b].tolist() for b in range(64))
    gerr = float(np.abs(g - want["derivs"]).max() / np.abs(want["derivs"]).max())
    print("configs[4] bf16 vs the f32 ORACLE: max |dz| %.3g, argmax flips %.3g %% of frames, %d / 64 decodes identical, "
          "gradient error %.3g of max" % (err, 100 * flips, same, gerr))
    assert err < 1e-2 and flips < 2e-2 and same >= 62 and gerr < 1.5e-3


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [7, 11, 23])
def test_fused_launches_randomised_stress(seed):
    """scripts/gpu_stress_overlap.py: 60 random batch geometries (1..89 lines, longest line 8..260 frames, 33..120 cells) with both
    fused launches forced (overlap mode 2) against the plain path of the same library: gradients within 5e-5 of the largest
    entry, and no wait of either launch may run into its watchdog (seed 7, case 4 -- lines of 13..16 frames -- is the geometry
    that caught the forward launch waiting for a flag nobody raises)."""
    env = dict(os.environ, SEED=str(seed), NCASE="60")
    r = subprocess.run([os.sys.executable, os.path.join(ROOT, "scripts", "gpu_stress_overlap.py")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "stress ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


# ---- trajectories at the bench shapes, the chip-filling minibatch, the one-call step ------------------
def _trajectory(ora, ni, nh, nc, Ts, L, scale, nsteps, lr, mom, one_call, precision=0, seed=70, grad_tol=1e-3, nthreads=None, on_step=None):
    """`nsteps` consecutive minibatch updates (a fresh synthetic minibatch every step, momentum carried) on the GPU and in the
    oracle (reference semantics: every line an independent fwd/CTC/bwd accumulating into Params.d on top of the carried
    mom * d, then ONE sgd_update -- clstmhl.h:201-223, clstm.cc:201-217, clstm_compute.cc:553-563; OpenMP over lines).
    Every step: the CTC argmax decodes of all lines IDENTICAL; afterwards the parameters within the tolerance the accepted
    gradient tolerance implies -- a gradient accepted within grad_tol of its largest entry moves d by that, and v by lr x the
    accumulated d error: after step k (1-based) sum_{j<=k} sum_{i<=j} mom^(j-i) of them -- and the momentum buffer within
    grad_tol of ITS largest entry times the same geometric factor.
    `nthreads`: host threads of the oracle (default: one per CPU of the machine); `on_step(step, net)`: called behind every
    step's checks.  Returns the GPU net."""
    import torch
    from common import Backend, synth_lines
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    from oracle.oracle import OracleNet
    lib = Backend("hip").lib
    rng = np.random.default_rng(seed)
    params = init_params(ni, nh, nc, seed=0.222) * scale
    ref = OracleNet(ora, ni, nh, nc, init=False)
    ref.set_params(params); ref.set_lr(lr, mom)
    net = Network(ni, nh, nc, lib=lib)
    net.set_params(params); net.setLearningRate(lr, mom)
    if precision:
        net.set_gemm_precision(precision)
    d_fac = v_fac = 0.0
    for step in range(1, nsteps + 1):
        lines = synth_lines(rng, Ts, ni)
        trs = [rng.integers(1, nc, L).astype(np.int32) for _ in Ts]
        want = ref.minibatch(lines, trs, nthreads=nthreads)
        gmax = float(np.abs(want["derivs"]).max())          # (Params.d right before the update: carried momentum + this minibatch)
        ref.update()
        if one_call:                                         # what the bench times: clstm_net_train_step, inputs resident in HBM
            x_dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(lines, 0), np.float32)).cuda()
            net.train_step(Ts, x_dev, trs)
        else:
            net.set_inputs(lines); net.forward(); net.ctc(trs); net.backward(); net.update()
        dec = net.decode()                                   # (the step's forward outputs are still in place behind the update)
        mism = [b for b in range(len(Ts)) if dec[b].tolist() != want["decode"][b].tolist()]
        assert not mism, "step %d: CTC argmax decodes differ on lines %s" % (step, mism)
        d_fac = mom * d_fac + 1.0
        v_fac += d_fac
        assert_close(net.get_params(), ref.get_params(), rtol=1e-5, atol=1e-7 + v_fac * lr * grad_tol * gmax,
                     what="parameters after step %d" % step)
        assert_close(net.get_derivs(), ref.get_derivs(), rtol=grad_tol, atol=1e-9, scale_atol=d_fac * grad_tol,
                     what="momentum buffer after step %d" % step)
        if on_step is not None:
            on_step(step, net)
    lib.call("clstm_synchronize")
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("one_call", [False, True], ids=["sequence_of_calls", "clstm_net_train_step"])
def test_three_minibatch_steps_at_the_bench_shape_vs_oracle(ora32, one_call):
    """BASELINE configs[2] at full size, THREE consecutive updates (lr 1e-4, momentum 0.9): 64 lines x 200 frames, a fresh
    minibatch per step -- through the sequence of calls and through the one-call clstm_net_train_step the bench times
    (fused forward launch, fused backward launch, update riding the slab reduction), each against the oracle."""
    _trajectory(ora32, 48, 100, 83, [200] * 64, 25, 10.0, 3, 1e-4, 0.9, one_call)


@pytest.mark.gpu
def test_256_lines_fill_every_cu_twice_vs_oracle(ora32):
    """The size `saturated` in the bench line quotes: 256 lines x 200 frames = 512 recurrence workgroups on 256 CUs (two per
    CU, dispatched longest first), forward pass as separate launches.  Every saved activation, delta, CTC posterior, decode,
    gradient and the update of all 256 lines against the oracle, bars of the 64-line case."""
    from common import Backend
    from test_net_parity import run_case
    run_case(Backend("hip"), ora32, 48, 100, 83, [200] * 256, scale=10.0, seed=15, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("one_call", [True], ids=["clstm_net_train_step"])
def test_two_minibatch_steps_at_configs4_f32_vs_oracle(ora32, one_call):
    """BASELINE configs[4] at full size in the exact-f32 mode, TWO consecutive updates through the one-call step (stacked net:
    the reductions stage the gradient, one k_update applies the whole step): decodes of all 64 lines identical at both steps,
    parameters and momentum within the derived tolerance (weights at the reference's own initial scale x 2, where the
    recurrence is contractive: test_configs4_full_shape_f32_strict_at_reference_init)."""
    _trajectory(ora32, 64, [512, 512], 100, [400] * 64, 50, 2.0, 2, 1e-4, 0.9, one_call, seed=71)
