"""clstm_net_predict: recognition of a whole minibatch in one call, through the NO-SAVE forms of the narrow-layer forward kernels
(lstm_seq.h / lstm_fwd_fused.h / lstm_mfma.h with SAVE = false).  The acceptance property is bit identity with the training
forward pass (clstm_net_set_inputs + clstm_net_forward + clstm_net_decode) -- no tolerance anywhere except against the oracle,
where the project's activation bar (common.RTOL / ATOL) applies.  Every case runs on the host emulator (CPU suite) and on the
MI355X (-m gpu) unless it names a kernel family only the GPU has (fused launch at its default rule, batched MFMA)."""
import ctypes

import numpy as np
import pytest

from common import ATOL, RTOL, assert_close, synth_lines
from narrow_rule import fused_forward

NOSAVE_LINE, NOSAVE_FUSED, NOSAVE_MFMA = 22, 23, 15      # clstm_debug_path_count (include/clstm_abi.h)
TRAIN_FUSED, TRAIN_MFMA, ROUTED = 5, 16, 21


def count(backend, which):
    out = ctypes.c_longlong(0)
    backend.lib.call("clstm_debug_path_count", which, ctypes.byref(out))
    return out.value


def counters(backend):
    return {k: count(backend, k) for k in (NOSAVE_LINE, NOSAVE_FUSED, NOSAVE_MFMA, TRAIN_FUSED, TRAIN_MFMA)}


def moved(before, after):
    return {k: after[k] - before[k] for k in before if after[k] != before[k]}


class Options:
    """experiment options (clstm_debug_set_option) for one `with` block, forgotten afterwards"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        return self

    def __call__(self, name, value):
        self.lib.call("clstm_debug_set_option", name.encode(), int(value))

    def __exit__(self, *exc):
        self.lib.call("clstm_debug_set_option", None, 0)


def varied_params(backend, ni, nh, nc, lines, uni=False):
    """random weights large enough for peaked, varied posteriors, with the blank's bias set so that the blank wins about half of
    the frames of `lines` (trivial_decode emits a class when a blank follows it): decodes are not empty.  Tuned on a throwaway net."""
    from clstm_amd.net import Network
    net = Network(ni, nh, nc, unidirectional=uni, lib=backend.lib)
    params = np.random.default_rng(5).normal(0, 0.3, net.nparams).astype(np.float32)
    net.set_params(params)
    net.set_inputs(lines)
    net.forward()
    z = net.outputs().astype(np.float64)
    margin = np.log(np.maximum(z[:, 1:].max(1), 1e-30)) - np.log(np.maximum(z[:, 0], 1e-30))
    sm_ni = (1 if uni else 2) * net.nhidden[-1]
    params[net.nparams - nc * (1 + sm_ni)] += np.float32(np.median(margin))
    return params


def make_net(backend, ni, nh, nc, params, uni=False, strict=False, overlap=None, precision=0):
    from clstm_amd.net import Network
    net = Network(ni, nh, nc, unidirectional=uni, lib=backend.lib)
    net.set_params(params)
    if strict:
        net.set_strict_f32(True)
    if overlap is not None:
        net.set_overlap(overlap)
    if precision:
        net.set_gemm_precision(precision)
    return net


def raw_predict(net, lines):
    """clstm_net_predict_h with every output; returns the PACKED arrays (cls, loc, conf, cnt)"""
    from clstm_amd.abi import f32, i32, ptr
    net.T = [len(x) for x in lines]
    net.N = int(sum(net.T))
    x = f32(np.concatenate([f32(x).reshape(-1, net.ninput) for x in lines], 0))
    t = i32(net.T)
    cls, loc = np.full(net.N, -7, np.int32), np.full(net.N, -7, np.int32)
    conf, cnt = np.full(net.N, -7.0, np.float32), np.full(len(net.T), -7, np.int32)
    net.lib.call("clstm_net_predict_h", net.h, ptr(t), len(net.T), ptr(x), ptr(cls), ptr(loc), ptr(conf), ptr(cnt))
    return cls, loc, conf, cnt


def raw_decode(net):
    from clstm_amd.abi import ptr
    cls, loc = np.full(net.N, -7, np.int32), np.full(net.N, -7, np.int32)
    cnt = np.full(len(net.T), -7, np.int32)
    net.lib.call("clstm_net_decode", net.h, ptr(cls), ptr(loc), ptr(cnt))
    return cls, loc, cnt


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_identity(backend, net, lines, want_nosave, nlaunch=1, allow_nan=False, training_form=None):
    """predict FIRST (nothing of a forward pass is lying around in the buffers), then forward + decode on the same net, then predict
    again (buffers of a training pass around it): Z, classes / locs / counts, conf = Z[loc, cls] and the h of every layer and
    direction must be the same bytes; the no-save counter moves for predict only, the training counters for forward only.
    training_form: the one counter predict is expected to move instead -- a family without a no-save instantiation.
    Returns (Z, counts)."""
    nl, nd = len(net.nhidden), 1 if net.unidirectional else 2
    results = []
    for rnd in range(2):
        c0 = counters(backend)
        cls, loc, conf, cnt = raw_predict(net, lines)
        c1 = counters(backend)
        z = net.outputs()
        hs = [net.state(l, d, "outputs") for l in range(nl) for d in range(nd)]
        dcls, dloc, dcnt = raw_decode(net)                       # clstm_net_decode works on the predicted minibatch
        if training_form is not None:
            assert moved(c0, c1) == {training_form: nlaunch}, (rnd, moved(c0, c1))
        elif want_nosave is not None:
            assert moved(c0, c1) == {want_nosave: nlaunch}, (rnd, moved(c0, c1))     # (so no training counter moved)
        results.append((cls, loc, conf, cnt, z, hs))
        assert np.array_equal(dcnt, cnt)
        if rnd == 0:
            c0 = counters(backend)
            net.set_inputs(lines)
            net.forward()
            c1 = counters(backend)
            for k in (NOSAVE_LINE, NOSAVE_FUSED, NOSAVE_MFMA):
                assert c1[k] == c0[k], "forward moved a no-save counter"
            zf = net.outputs()
            fcls, floc, fcnt = raw_decode(net)
            hf = [net.state(l, d, "outputs") for l in range(nl) for d in range(nd)]
            fmoved = moved(c0, c1)
    off = np.concatenate([[0], np.cumsum(net.T)])
    for rnd, (cls, loc, conf, cnt, z, hs) in enumerate(results):
        assert same_bytes(z, zf), "Z differs (round %d): max |d| %g" % (rnd, np.nanmax(np.abs(z - zf)))
        assert np.array_equal(cnt, fcnt), rnd
        for b in range(len(net.T)):
            o, n = off[b], cnt[b]
            assert np.array_equal(cls[o:o + n], fcls[o:o + n]) and np.array_equal(loc[o:o + n], floc[o:o + n]), (rnd, b)
            assert same_bytes(conf[o:o + n], zf[o + loc[o:o + n], cls[o:o + n]]), (rnd, b)
        for a, b in zip(hs, hf):
            assert same_bytes(a, b), "h differs (round %d)" % rnd
    if not allow_nan:
        assert np.isfinite(zf).all()
    print("family moved by forward:", fmoved, " decoded classes:", int(results[0][3].sum()))
    assert net.N < 10 or results[0][3].sum() > 0, "inconclusive: nothing decoded, conf was compared on no entry"
    return zf, results[0][3]


CASES = [
    # name,            ni, nh,       nc,  T,                     uni,   strict
    ("one_line_T37",   48, [100],    83,  [37],                  False, False),
    ("ragged_T1_T2",   10, [30],     11,  [1, 2, 17, 5, 30, 2],  False, False),
    ("unidirectional", 48, [64],     83,  [12, 7, 19],           True,  False),
    ("nh30",           12, [30],     20,  [9, 14],               False, False),
    ("nh64",           48, [64],     83,  [11, 16],              False, False),
    ("nh128",          48, [128],    83,  [8, 13],               False, False),
    ("two_layers",     9,  [20, 12], 15,  [6, 21, 13],           False, False),
    ("nc_above_smx",   10, [16],     120, [7, 18],               False, False),
    ("strict_f32",     48, [100],    83,  [10, 15],              False, True),
]


@pytest.mark.parametrize("name,ni,nh,nc,T,uni,strict", CASES, ids=[c[0] for c in CASES])
def test_predict_bit_identical_to_forward(backend, name, ni, nh, nc, T, uni, strict):
    rng = np.random.default_rng(11)
    lines = synth_lines(rng, T, ni)
    net = make_net(backend, ni, nh, nc, varied_params(backend, ni, nh, nc, lines, uni), uni=uni, strict=strict)
    check_identity(backend, net, lines, NOSAVE_LINE, nlaunch=len(nh))


def test_predict_fused_forced_small(backend):
    """the fused forward launch (producers + recurrence + softmax consumers) with the recurrence role in its no-save form, forced
    onto a small minibatch (clstm_net_set_overlap(2)) so that the emulator covers it too: the progress word that rides the H store
    still feeds the consumers -- or the outputs would not be the training launch's"""
    ni, nh, nc = 48, [100], 83
    rng = np.random.default_rng(12)
    lines = synth_lines(rng, [21, 3, 37, 16], ni)
    assert fused_forward(nh, False, nc, len(lines), 2, backend.kind)      # (the rule admits it: tests/narrow_rule.py)
    net = make_net(backend, ni, nh, nc, varied_params(backend, ni, nh, nc, lines), overlap=2)
    c0 = count(backend, TRAIN_FUSED)
    check_identity(backend, net, lines, NOSAVE_FUSED)
    assert count(backend, TRAIN_FUSED) == c0 + 1      # the one forward() call of check_identity took the fused launch too


@pytest.mark.gpu
def test_predict_fused_64x200_gpu():
    """64 x 200: the fused forward launch by the library's own rule"""
    from common import Backend
    backend = Backend("hip")
    ni, nh, nc = 48, [100], 83
    rng = np.random.default_rng(13)
    lines = synth_lines(rng, [200] * 64, ni)
    assert fused_forward(nh, False, nc, 64, None, "hip", tmax=200)        # (by the default rule, overlap = 1: tests/narrow_rule.py)
    net = make_net(backend, ni, nh, nc, varied_params(backend, ni, nh, nc, lines))
    c0 = count(backend, TRAIN_FUSED)
    check_identity(backend, net, lines, NOSAVE_FUSED)
    assert count(backend, TRAIN_FUSED) == c0 + 1


# ---- 2. batched MFMA recurrence (GPU) ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nh,nlines,forced", [(100, 640, False), (100, 48, True), (64, 48, True), (128, 48, True)])
def test_predict_mfma_gpu(nh, nlines, forced):
    from common import Backend
    backend = Backend("hip")
    with Options(backend.lib) as options:
        if forced:
            options("fwd_mfma", 2)
        _mfma_case(backend, nh, nlines, forced)


def _mfma_case(backend, nh, nlines, forced):
    ni, nc = 48, 83
    rng = np.random.default_rng(14)
    T = [int(t) for t in rng.integers(150, 251, nlines)] if not forced else [int(t) for t in rng.integers(20, 90, nlines)]
    lines = synth_lines(rng, T, ni)
    net = make_net(backend, ni, [nh], nc, varied_params(backend, ni, [nh], nc, lines))
    c0, r0 = count(backend, TRAIN_MFMA), count(backend, ROUTED)
    # 128 cells: the batched recurrence has no no-save instantiation (it would spill: lstm_mfma.h) -- predict runs its training form
    tf = TRAIN_MFMA if nh == 128 else None
    check_identity(backend, net, lines, NOSAVE_MFMA, training_form=tf)
    assert count(backend, TRAIN_MFMA) == c0 + (3 if tf else 1)
    assert count(backend, ROUTED) == r0                # inputs in range: the routed twins returned at their first branch
    # one pixel = 300: the device hands the minibatch to the routed per-line twins (their no-save form under predict)
    lines[3] = lines[3].copy()
    lines[3][min(5, len(lines[3]) - 1), 7] = 300.0
    z, _ = check_identity(backend, net, lines, NOSAVE_MFMA, training_form=tf)
    assert count(backend, ROUTED) == r0 + 3            # predict, forward, predict
    assert np.isfinite(z).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nh,precision", [([256], 0), ([100], 1)])
def test_predict_wide_and_bf16_run_the_unchanged_forward_gpu(nh, precision):
    """out of scope for no-save (lstm_wide.h, the bf16 modes): predict runs today's forward pass -- same results, no no-save
    counter moves"""
    from common import Backend
    backend = Backend("hip")
    ni, nc = 48, 83
    rng = np.random.default_rng(15)
    lines = synth_lines(rng, [9, 14, 6, 11], ni)
    net = make_net(backend, ni, nh, nc, varied_params(backend, ni, nh, nc, lines), precision=precision)
    c0 = counters(backend)
    check_identity(backend, net, lines, None)
    c1 = counters(backend)
    for k in (NOSAVE_LINE, NOSAVE_FUSED, NOSAVE_MFMA):
        assert c1[k] == c0[k]
    # and nothing is refused afterwards: the activations ARE saved
    raw_predict(net, lines)
    net.state(0, 0, "gi")


# ---- 3. oracle --------------------------------------------------------------------------------------------------------
def test_predict_matches_oracle_on_trained_weights(backend, ora32):
    """trained-like weights on real-line crops (tests/trained_weights.py): every line's decode equals the oracle's, outputs within
    the activation bar.  GPU: 64 crops x T = 200 (the fused launch); emulator: 8 crops, T <= 60."""
    from oracle.oracle import OracleNet
    from trained_weights import NC, NH, NI, fixture_crops, trained_like_params
    params, _ = trained_like_params(ora32)
    rng = np.random.default_rng(16)
    T = [200] * 64 if backend.kind == "hip" else [int(t) for t in rng.integers(30, 61, 8)]
    lines, _ = fixture_crops(rng, T)
    net = make_net(backend, NI, [NH], NC, params)
    dec, locs, confs = net.predict(lines)
    z = net.split(net.outputs())
    ref = OracleNet(ora32, NI, NH, NC, init=False)
    ref.set_params(params)
    nonempty = 0
    for b, x in enumerate(lines):
        ref.set_inputs(x)
        want = ref.forward()[:, 0, :]
        assert_close(z[b], want, rtol=RTOL, atol=ATOL, what="outputs of line %d" % b)
        assert dec[b].tolist() == np.asarray(ref.decode()).tolist(), b
        assert same_bytes(confs[b], z[b][locs[b], dec[b]])
        nonempty += len(dec[b]) > 0
    assert nonempty >= len(lines) // 2, "inconclusive: the trained-like model decodes almost nothing"


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
def test_accessors_refuse_after_predict_and_training_recovers(backend):
    from clstm_amd.abi import ClstmError
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nh, nc = 8, [10], 7
    rng = np.random.default_rng(17)
    net = make_net(backend, ni, nh, nc, init_params(ni, nh, nc, seed=0.222) * 20.0)
    net.enable_input_deltas(True)
    T = [5, 9, 3]
    lines = synth_lines(rng, T, ni)
    trs = [rng.integers(1, nc, 2).astype(np.int32) for _ in T]
    net.predict(lines)
    refusing = [lambda: net.ctc(trs), lambda: net.backward(), lambda: net.state(0, 0, "gi"), lambda: net.state(0, 1, "state"),
                lambda: net.state(0, 0, "d_gi"), lambda: net.get_states(), lambda: net.input_deltas()]
    for f in refusing:
        with pytest.raises(ClstmError, match="clstm_net_predict"):
            f()
        assert b"clstm_net_predict" in backend.lib.dll.clstm_last_error()
    net.state(0, 0, "outputs")      # which = 5 works
    net.outputs(); net.decode()
    # a training step on the same net: succeeds, and its states are readable again
    p0 = net.get_params()
    x = backend.up(np.concatenate(lines, 0))
    net.train_step_prepared(Network.prepare_step(T, trs), x)
    backend.sync()
    assert not np.array_equal(net.get_params(), p0)
    for which in ("gi", "state", "outputs", "d_go"):
        assert np.isfinite(net.state(0, 0, which)).all()
    # bad minibatches are refused BEFORE the net is touched: the trained minibatch is still the current one
    z = net.outputs()
    from clstm_amd.abi import f32, i32, ptr
    cnt = np.zeros(2, np.int32)
    xx = f32(np.zeros((4, ni)))
    for bad in ([3, -1], [0, 0]):
        with pytest.raises(ClstmError):
            backend.lib.call("clstm_net_predict_h", net.h, ptr(i32(bad)), 2, ptr(xx), None, None, None, ptr(cnt))
    with pytest.raises(ClstmError):
        backend.lib.call("clstm_net_predict_h", net.h, ptr(i32([2, 2])), 2, ptr(xx), None, None, None, None)   # counts_h is required
    assert same_bytes(net.outputs(), z)
    net.state(0, 0, "gi")
    # NULL classes / locs / conf are fine
    backend.lib.call("clstm_net_predict_h", net.h, ptr(i32([2, 2])), 2, ptr(xx), None, None, None, ptr(cnt))


def test_refused_set_batch_leaves_the_minibatch_intact(backend):
    """clstm_net_set_batch validates the line lengths before it changes the net: after a declaration with a negative length is
    refused, forward + decode of the minibatch declared before give the bytes they gave before"""
    from clstm_amd.abi import ClstmError, i32, ptr
    ni, nh, nc = 12, [30], 20
    rng = np.random.default_rng(19)
    lines = synth_lines(rng, [9, 1, 14, 30], ni)
    net = make_net(backend, ni, nh, nc, varied_params(backend, ni, nh, nc, lines))
    net.set_inputs(lines)
    net.forward()
    z, (cls, loc, cnt) = net.outputs(), raw_decode(net)
    assert cnt.sum() > 0
    with pytest.raises(ClstmError, match="negative line length"):
        backend.lib.call("clstm_net_set_batch", net.h, ptr(i32([7, -1])), 2)
    net.forward()
    fcls, floc, fcnt = raw_decode(net)
    assert same_bytes(net.outputs(), z)
    assert same_bytes(fcnt, cnt) and same_bytes(fcls, cls) and same_bytes(floc, loc)


# ---- 5. training is undisturbed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", [[10], [7, 5]])
def test_training_trajectory_undisturbed_by_predict(backend, nh):
    """A: six clstm_net_train_step_next steps, each declaring its successor.  B: the same, with a predict of ANOTHER minibatch (other
    bs, other T; one of them holds a NaN pixel) after every step -- which drops the declaration, so the next step takes the
    ordinary path.  Parameters and derivs equal as bytes after every step; no update skipped; no error reported."""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nc = 8, 7
    rng = np.random.default_rng(23)
    p0 = init_params(ni, nh, nc, seed=0.222) * 20
    a, b = Network(ni, nh, nc, lib=backend.lib), Network(ni, nh, nc, lib=backend.lib)
    for n in (a, b):
        n.set_params(p0)
        n.setLearningRate(1e-2, 0.9)
    batches = []
    for k in range(7):
        T = [int(t) for t in rng.integers(3, 12, 2 + k % 3)]
        trs = [rng.integers(1, nc, max(1, t // 3)).astype(np.int32) for t in T]
        x = backend.up(np.ascontiguousarray(np.concatenate(synth_lines(rng, T, ni), 0), np.float32))
        batches.append((Network.prepare_step(T, trs), x))
    prev = p0.astype(np.float32)
    for k in range(6):
        prep, x = batches[k]
        a.train_step_prepared(prep, x, batches[k + 1][0], batches[k + 1][1])
        b.train_step_prepared(prep, x, batches[k + 1][0], batches[k + 1][1])
        other = synth_lines(rng, [int(t) for t in rng.integers(1, 15, 4 + k)], ni)
        if k == 2:
            other[1][0, 3] = np.nan
        dec, _, _ = b.predict(other)
        assert len(dec) == 4 + k
        pa, pb = a.get_params(), b.get_params()
        assert same_bytes(pa, pb), k
        assert same_bytes(a.get_derivs(), b.get_derivs()), k
        assert not np.array_equal(pa, prev), "step %d applied no update" % k
        prev = pa
    backend.sync()      # raises if a device error word (the NaN flag among them) was armed


# ---- 6. memory ------------------------------------------------------------------------------------------------------------
def test_predict_reserves_less_device_memory(backend):
    """fresh net after predict of 256 x 100 against a twin after clstm_net_set_batch of the same minibatch: smaller by at least
    D + dH (N . ndir . 5 . no . 4 bytes, from the shapes)"""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nh, nc = (48, 100, 83) if backend.kind == "hip" else (8, 12, 10)
    rng = np.random.default_rng(29)
    params = init_params(ni, [nh], nc, seed=0.222)
    T = [100] * 256
    N, ndir = sum(T), 2
    lines = [rng.random((t, ni), np.float32) for t in T]

    def pair():
        p, t = make_net(backend, ni, [nh], nc, params), make_net(backend, ni, [nh], nc, params)
        b0 = p.device_bytes()
        assert b0 == t.device_bytes() and b0 >= 3 * 4 * p.nparams
        p.predict(lines)
        t.set_batch(T)
        return p.device_bytes(), t.device_bytes()
    bp, bt = pair()
    print("device bytes after predict %d, after set_batch %d, gap %d, D + dH %d" % (bp, bt, bt - bp, N * ndir * 5 * nh * 4))
    assert bp < bt
    assert bt - bp >= N * ndir * 5 * nh * 4
    if backend.kind == "hip":
        with Options(backend.lib) as options:
            options("fwd_mfma", 2)
            mp, mt = pair()
        print("forced batched-MFMA family: after predict %d, after set_batch %d, gap %d (per-line family gap %d; layer 0 keeps G "
              "for its routed twins, C and S are gone in both)" % (mp, mt, mt - mp, bt - bp))
        assert mt - mp >= N * ndir * 5 * nh * 4


def test_predict_device_frames_equal_host_frames(backend):
    """clstm_net_predict (frames resident on the device: one ingest launch that also carries the line offsets) against
    clstm_net_predict_h, ragged lines, twice with another geometry in between"""
    from clstm_amd.abi import i32, ptr
    ni, nh, nc = 12, [30], 20
    rng = np.random.default_rng(31)
    geoms = [[9, 1, 14, 30], [5, 22], [9, 1, 14, 30]]
    lines0 = synth_lines(rng, geoms[0], ni)
    net = make_net(backend, ni, nh, nc, varied_params(backend, ni, nh, nc, lines0))
    decoded = 0
    for T in geoms:
        lines = lines0 if T is geoms[0] else synth_lines(rng, T, ni)
        cls_h, loc_h, conf_h, cnt_h = raw_predict(net, lines)
        z_h = net.outputs()
        N = sum(T)
        x_d = backend.up(np.concatenate(lines, 0))
        cls, loc = np.full(N, -7, np.int32), np.full(N, -7, np.int32)
        conf, cnt = np.full(N, -7.0, np.float32), np.full(len(T), -7, np.int32)
        c0 = count(backend, NOSAVE_LINE)
        backend.lib.call("clstm_net_predict", net.h, ptr(i32(T)), len(T), ptr(x_d), ptr(cls), ptr(loc), ptr(conf), ptr(cnt))
        assert count(backend, NOSAVE_LINE) == c0 + 1
        assert same_bytes(net.outputs(), z_h) and np.array_equal(cnt, cnt_h)
        off = np.concatenate([[0], np.cumsum(T)])
        for b in range(len(T)):
            o, k = off[b], cnt[b]
            assert np.array_equal(cls[o:o + k], cls_h[o:o + k]) and np.array_equal(loc[o:o + k], loc_h[o:o + k])
            assert same_bytes(conf[o:o + k], conf_h[o:o + k])
        decoded += int(cnt.sum())
    assert decoded > 0
