"""The softmax layer's input deltas x.d = z.d . W computed by the top layer's backward recurrence workgroups themselves, in front of
their first step (clstm_amd/csrc/lstm_xd_prologue.h, experiment option xd_prologue, path counter 26), against the product launch
it replaces (xd_prologue=0): the prologue restates that launch's arithmetic expression for expression, so everything downstream
of dH is compared AS BYTES -- the gate deltas of every layer and direction, the fresh gradient, the parameters and the momentum
buffer after each of two consecutive steps (a fresh minibatch per step: the first step's dH cannot satisfy the second), the input
deltas where enabled.  Counter 26 moves by one per step exactly where NarrowPlan::xd (runtime.inc:narrow_plan) says the case is eligible.

Every net runs with overlap mode 2: these line counts are far below what mode 1 overlaps, and the prologue belongs to the
overlapped backward launch.  Which cases are eligible follows from the launch rule, not from the result:
  * the overlapped launch needs a reporting lane that owns no cell, i.e. a cell count that is no multiple of 16: LSTM(16) and
    BiLSTM(128) keep the plain backward pass and the separate product (counter 0) -- lstm17_uni and bilstm120 are their
    neighbours that ARE eligible and reach ndir = 1 and eight column tiles on eight waves;
  * lines x directions x 4 <= 3 x CUs: the emulator has 16 CUs, every case here has at most 4 bidirectional lines;
  * layers of fewer than four waves (and every layer on the emulator) run the overlapped pass as two launches: there the
    prologue sits in front of the per-line backward kernel (lstm_bwd_xd_kernel), on the GPU from four waves on in front of the
    recurrence role of the fused launch (lstm_bwd_dw_kernel)."""
import numpy as np
import pytest

from common import bits, synth_lines
from test_net_parity import set_opt, _forget_debug_options, _path_count  # noqa: F401  (autouse fixture)

DELTAS = ("d_gi", "d_gf", "d_go", "d_ci")
PC_XD_PROLOGUE = 26

# id: (ni, nh, nc, T, unidirectional, settings, eligible)
T1 = [65, 1, 17, 16]
CASES = {
    # partial 32- and 16-row tiles, a 1-frame line, 3 k-blocks with a ragged k tail, the bench's <7, 25, 3> instantiation
    "bilstm100_nc83": (48, [100], 83, T1, False, dict(input_deltas=True), True),
    # one column tile, K < 32: two all-zero k-blocks
    "bilstm9_nc5": (6, [9], 5, [21, 13, 17], False, dict(), True),
    # K = 33 (one element in the second block); 16 cells: no overlapped launch, hence no prologue
    "lstm16_uni_nc33": (8, [16], 33, [40, 7], True, dict(), False),
    "lstm17_uni_nc33": (8, [17], 33, [40, 7], True, dict(), True),
    # K exactly one block; 128 cells: no overlapped launch
    "bilstm128_nc32": (8, [128], 32, [20, 64], False, dict(), False),
    "bilstm120_nc32": (8, [120], 32, [20, 64], False, dict(), True),
    # only the top layer's launch carries a prologue; the lower layer's dH still comes from backward_input_deltas
    "stacked_7_5": (6, [7, 5], 5, [18, 11], False, dict(input_deltas=True), True),
    "bilstm100_two_terms": (48, [100], 83, T1, False, dict(opts={"split_terms": 2}), True),
    "bilstm100_strict_f32": (48, [100], 83, T1, False, dict(strict=True), False),
    # nc just above the bound of three k-blocks (XD_MAX_K = 96)
    "bilstm9_nc97": (6, [9], 97, [21, 13, 17], False, dict(), False),
    "bilstm9_nc96": (6, [9], 96, [21, 13, 17], False, dict(), True),
}


def run_steps(backend, case, xd, nsteps=2):
    """`nsteps` training steps of the case's net with option xd_prologue = xd -> ([per step: {name: array}], [counter 26 per step])"""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nh, nc, T, uni, cfg, _ = CASES[case]
    for name, value in cfg.get("opts", {}).items():
        set_opt(backend, name, value)
    set_opt(backend, "xd_prologue", xd)
    rng = np.random.default_rng(11)
    net = Network(ni, nh, nc, unidirectional=uni, lib=backend.lib)
    net.set_params(init_params(ni, nh, nc, seed=0.222, unidirectional=uni) * (10 if max(nh) >= 100 else 20))
    net.setLearningRate(1e-3, 0.9)
    net.set_overlap(2)
    if cfg.get("strict"):
        net.set_strict_f32(True)
    if cfg.get("input_deltas"):
        net.enable_input_deltas(True)
    dirs = (0,) if uni else (0, 1)
    steps, moved = [], []
    for _ in range(nsteps):
        x = backend.up(np.concatenate(synth_lines(rng, T, ni), 0))
        trs = [rng.integers(1, nc, max(1, t // 3)).astype(np.int32) for t in T]
        before = _path_count(backend, PC_XD_PROLOGUE)
        net.train_step(T, x, trs)
        backend.sync()
        moved.append(_path_count(backend, PC_XD_PROLOGUE) - before)
        _, timeouts = net.overlap_stats()
        assert timeouts == 0
        got = {"gradient": net.get_grads(), "params": net.get_params(), "momentum": net.get_derivs()}
        for l in range(len(nh)):
            for d in dirs:
                for w in DELTAS:
                    got["%s layer %d dir %d" % (w, l, d)] = net.state(l, d, w)
        if cfg.get("input_deltas"):
            got["input deltas"] = net.input_deltas()
        assert all(np.isfinite(a).all() for a in got.values())
        steps.append(got)
    return steps, moved


def assert_same_bytes(on, off, what):
    for step, (a, b) in enumerate(zip(on, off)):
        assert a.keys() == b.keys()
        for name in a:
            bad = np.flatnonzero(bits(a[name]).ravel() != bits(b[name]).ravel())
            assert bad.size == 0, "%s, step %d, %s: %d of %d entries differ, first at %d: %r with the prologue, %r without" % (
                what, step, name, bad.size, a[name].size, bad[0], a[name].ravel()[bad[0]], b[name].ravel()[bad[0]])


@pytest.mark.parametrize("case", list(CASES))
def test_prologue_equals_the_product_launch_bit_for_bit(backend, case):
    eligible = CASES[case][6]
    on, moved_on = run_steps(backend, case, 1)
    off, moved_off = run_steps(backend, case, 0)
    print("%s on %s: counter 26 moved %r with the option on, %r off" % (case, backend.kind, moved_on, moved_off))
    assert moved_on == [1 if eligible else 0] * 2
    assert moved_off == [0, 0]
    assert np.abs(on[0]["d_gi layer %d dir 0" % (len(CASES[case][1]) - 1)]).max() > 0      # (there ARE deltas to compare)
    assert_same_bytes(on, off, case)


@pytest.mark.gpu
def test_prologue_at_the_bench_shape_three_declared_steps():
    """64 lines x 200 frames, BiLSTM(100), 83 classes -- lstm_bwd_dw_kernel<7, 25, 3> with 128 recurrence workgroups, seven full
    rounds of 32 frames less 24 -- three steps through train_step_prepared: the first two declare the next minibatch
    (clstm_net_train_step_next: its ingest rides the step's last launch), the third consumes the declared one.  The same bytes with
    the option on and off: gradient, parameters and momentum buffer after every step; the gate deltas and the CTC argmax decodes
    after the third (a step that declared its successor has no current minibatch any more: the library refuses to address its
    states and outputs)."""
    from common import Backend
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    backend = Backend("hip")
    ni, nh, nc, T = 48, 100, 83, [200] * 64

    def run(xd):
        set_opt(backend, "xd_prologue", xd)
        rng = np.random.default_rng(5)
        net = Network(ni, nh, nc, lib=backend.lib)
        net.set_params(init_params(ni, nh, nc, seed=0.222) * 10.0)
        net.setLearningRate(1e-4, 0.9)
        batches = []
        for _ in range(3):
            x = backend.up(np.concatenate(synth_lines(rng, T, ni), 0))
            batches.append((Network.prepare_step(T, [rng.integers(1, nc, 25).astype(np.int32) for _ in T]), x))
        steps, moved = [], []
        for i in range(3):
            before = _path_count(backend, PC_XD_PROLOGUE)
            nxt = batches[i + 1] if i < 2 else (None, None)
            net.train_step_prepared(batches[i][0], batches[i][1], nxt[0], nxt[1])
            backend.sync()
            moved.append(_path_count(backend, PC_XD_PROLOGUE) - before)
            assert net.overlap_stats()[1] == 0
            got = {"gradient": net.get_grads(), "params": net.get_params(), "momentum": net.get_derivs()}
            if i == 2:
                got["decodes"] = np.concatenate([d.astype(np.float32) for d in net.decode()] + [np.zeros(1, np.float32)])
                for d in (0, 1):
                    for w in DELTAS:
                        got["%s dir %d" % (w, d)] = net.state(0, d, w)
            steps.append(got)
        return steps, moved

    try:
        on, moved_on = run(1)
        off, moved_off = run(0)
    finally:
        backend.lib.call("clstm_debug_set_option", None, 0)
    assert moved_on == [1, 1, 1] and moved_off == [0, 0, 0]
    assert np.abs(on[2]["d_gi dir 0"]).max() > 0
    assert_same_bytes(on, off, "bench shape")
