"""The producer form of the softmax layer's input deltas (experiment option xd_prologue=2, path counter 27): every recurrence
workgroup of the top layer's fused backward launch computes only the 32 frames of dH it visits first, helper workgroups of the same
launch compute the other rounds in the order the recurrence reaches them and publish a rounds-complete word, and the recurrence
checks that word before its prefetch enters a round it did not make (clstm_amd/csrc/lstm_xd_prologue.h, lstm_bwd_dw.h,
lstm_seq.h).  Every round restates the product launch's arithmetic, so whoever computes a frame, everything downstream of dH is
compared AS BYTES across xd_prologue = 0 (the product launch), 1 (the whole prologue) and 2: gate deltas of every layer and
direction, the fresh gradient, parameters and momentum buffer after each of two consecutive steps of the SAME net with a fresh
minibatch per step -- ready words left by the first pass must not satisfy the second.

Which form runs follows from the launch rule (runtime.inc:narrow_plan, restated in tests/narrow_rule.py), not from the result:
  * form 2 needs form 1's eligibility (test_xd_prologue.py) AND the one-launch form of the overlapped pass -- a real GPU and a layer
    of four or more waves -- AND a CU for every item: lines x directions x 2 <= CUs.  There counter 27 moves by one per step and
    counter 26 stays put;
  * everything else asked for 2 runs 1 unchanged: the host emulator (SMALL_CASES) and layers below four waves move counter 26
    exactly as option 1 does and never counter 27;
  * what is ineligible for 1 (16 / 128 cells: no overlapped launch; nc = 97 > XD_MAX_K) moves neither.
Shapes: the smallest at which the round logic can go wrong -- T = 32 (no item), 33 (an item of one frame), 64 (exactly one full
item round), 65 (a full round and a one-frame tail); T = 200 (six item rounds per workgroup, the short round visited last in both
directions); a ragged minibatch from 0 to 100 frames; eight column tiles; one direction; no k tail."""
import numpy as np
import pytest

from common import bits, synth_lines
from narrow_rule import xd_form
from test_net_parity import set_opt, _forget_debug_options, _path_count  # noqa: F401  (autouse fixture)

DELTAS = ("d_gi", "d_gf", "d_go", "d_ci")
PC_XD_PROLOGUE, PC_XD_PRODUCERS = 26, 27

# id: (ni, nh, nc, T, unidirectional, eligible for form 1, four or more waves)
CASES = {
    "bilstm100_T32_33_64_65": (48, [100], 83, [32, 33, 64, 65], False, True, True),
    "bilstm100_T200_two_lines": (48, [100], 83, [200, 200], False, True, True),
    "bilstm100_ragged_with_empty_line": (48, [100], 83, [1, 100, 0, 47, 96, 33], False, True, True),   # (six lines: the emulator's 16 CUs admit 3 x 16 / 8)
    "bilstm120_nc32_eight_tiles": (8, [120], 32, [70, 64], False, True, True),
    "lstm100_uni": (48, [100], 83, [65, 40], True, True, True),
    "bilstm100_nc96_no_k_tail": (48, [100], 96, [70, 33], False, True, True),
    "bilstm100_nc97": (48, [100], 97, [70, 33], False, False, True),
    "lstm16_uni_nc33": (8, [16], 33, [40, 70], True, False, False),
    "bilstm128_nc32": (8, [128], 32, [40, 64], False, False, True),
    # below four waves: the two-launch form of the overlapped pass, which keeps the whole prologue
    "bilstm9_nc5_two_launch_form": (6, [9], 5, [70, 13, 40], False, True, False),
}
# (far above what the emulator's 16 CUs admit: GPU only)  192 recurrence workgroups: the bound of NarrowPlan::dwx on 256 CUs -- eligible for
# form 1, but form 2 wants a CU of its own for every dH item, i.e. recurrence workgroups on at most half of the MI355X's 256 CUs;
# 128 recurrence workgroups: that bound
CUS = 256
GPU_CASES = {
    "bilstm100_96_lines_T40": (48, [100], 83, [40] * 96, False, True, True),
    "bilstm100_64_lines_T40": (48, [100], 83, [40] * 64, False, True, True),
}
# the emulator walks every lane of every wave: one step of a few dozen frames (a one-frame item on the GPU; a layer below four waves;
# a layer without an overlapped launch)
SMALL_CASES = {
    "bilstm100_T33_9": (48, [100], 83, [33, 9], False, True, True),
    "bilstm9_nc5": (6, [9], 5, [40, 13], False, True, False),
    "lstm16_uni_nc33": (8, [16], 33, [40, 7], True, False, False),
}


def run_steps(backend, case, xd, nsteps=2):
    """`nsteps` training steps with option xd_prologue = xd -> ([per step: {name: array}], [(counter 26, counter 27) moved per step])"""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nh, nc, T, uni = case[:5]
    set_opt(backend, "xd_prologue", xd)
    rng = np.random.default_rng(11)
    net = Network(ni, nh, nc, unidirectional=uni, lib=backend.lib)
    net.set_params(init_params(ni, nh, nc, seed=0.222, unidirectional=uni) * (10 if max(nh) >= 100 else 20))
    net.setLearningRate(1e-3, 0.9)
    net.set_overlap(2)
    dirs = (0,) if uni else (0, 1)
    steps, moved = [], []
    for _ in range(nsteps):
        x = backend.up(np.concatenate(synth_lines(rng, T, ni), 0))
        trs = [rng.integers(1, nc, max(1, t // 3) if t else 0).astype(np.int32) for t in T]
        before = [_path_count(backend, c) for c in (PC_XD_PROLOGUE, PC_XD_PRODUCERS)]
        net.train_step(T, x, trs)
        backend.sync()
        moved.append(tuple(_path_count(backend, c) - b for c, b in zip((PC_XD_PROLOGUE, PC_XD_PRODUCERS), before)))
        _, timeouts = net.overlap_stats()
        assert timeouts == 0
        got = {"gradient": net.get_grads(), "params": net.get_params(), "momentum": net.get_derivs()}
        for l in range(len(nh)):
            for d in dirs:
                for w in DELTAS:
                    got["%s layer %d dir %d" % (w, l, d)] = net.state(l, d, w)
        assert all(np.isfinite(a).all() for a in got.values())
        steps.append(got)
    return steps, moved


def assert_same_bytes(a_steps, b_steps, what):
    for step, (a, b) in enumerate(zip(a_steps, b_steps)):
        assert a.keys() == b.keys()
        for name in a:
            bad = np.flatnonzero(bits(a[name]).ravel() != bits(b[name]).ravel())
            assert bad.size == 0, "%s, step %d, %s: %d of %d entries differ, first at %d: %r against %r" % (
                what, step, name, bad.size, a[name].size, bad[0], a[name].ravel()[bad[0]], b[name].ravel()[bad[0]])


def expected_moves(backend, case):
    """(counter 26, counter 27) per step under options 0, 1, 2 -- from the launch rule"""
    eligible, four_waves = case[5], case[6]
    nrec = len(case[3]) * (1 if case[4] else 2)
    producers = eligible and four_waves and backend.kind == "hip" and 2 * nrec <= CUS
    form = xd_form(case[1], case[4], case[2], len(case[3]), 2, backend.kind, ni=case[0], tmax=max(case[3]), frames=sum(case[3]))
    assert (form != 0, form == 2) == (eligible, producers), (form, eligible, producers)      # (the case table agrees with the restated rule)
    one = (1, 0) if eligible else (0, 0)
    return (0, 0), one, ((0, 1) if producers else one)


def check_case(backend, name, case, options=(0, 1, 2), nsteps=2):
    outs, moves = {}, {}
    for xd in options:
        outs[xd], moves[xd] = run_steps(backend, case, xd, nsteps)
    want = expected_moves(backend, case)
    print("%s on %s: counters (26, 27) moved %s under xd_prologue = %r" % (name, backend.kind, " / ".join(repr(moves[xd]) for xd in options), options))
    for xd in options:
        assert moves[xd] == [want[xd]] * nsteps, "xd_prologue=%d" % xd
    base = options[0]
    assert np.abs(outs[base][0]["d_gi layer 0 dir 0"]).max() > 0      # (there ARE deltas to compare)
    for xd in options[1:]:
        assert_same_bytes(outs[xd], outs[base], "%s: option %d against option %d" % (name, xd, base))


_HIP = []


def hip_backend():
    from common import Backend
    if not _HIP:
        _HIP.append(Backend("hip"))
    return _HIP[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + list(GPU_CASES))
def test_three_forms_give_the_same_bytes(name):
    backend = hip_backend()
    try:
        check_case(backend, name, CASES.get(name) or GPU_CASES[name])
    finally:
        backend.lib.call("clstm_debug_set_option", None, 0)


@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_option_two_without_the_one_launch_form_is_option_one(backend, name):
    """The host emulator runs the overlapped pass as two launches: asked for 2 it runs the whole prologue, counter 26 moves as under
    1, counter 27 never, and the bytes are those of 1 (which test_xd_prologue.py compares with the product launch).  On the GPU the
    same cases take whatever expected_moves derives from the rule."""
    check_case(backend, name, SMALL_CASES[name], options=(1, 2), nsteps=1)


@pytest.mark.gpu
def test_producers_at_the_bench_shape_three_declared_steps():
    """64 lines x 200 frames, BiLSTM(100), 83 classes -- lstm_bwd_dw_kernel<7, 25, 3>: 128 recurrence workgroups, 128 dH items of six
    rounds each -- three steps through train_step_prepared, the first two declaring their successor.  Options 2 and 1: the same
    gradient, parameters and momentum buffer after every step, the same gate deltas after the third."""
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    backend = hip_backend()
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
            before = [_path_count(backend, c) for c in (PC_XD_PROLOGUE, PC_XD_PRODUCERS)]
            nxt = batches[i + 1] if i < 2 else (None, None)
            net.train_step_prepared(batches[i][0], batches[i][1], nxt[0], nxt[1])
            backend.sync()
            moved.append(tuple(_path_count(backend, c) - b for c, b in zip((PC_XD_PROLOGUE, PC_XD_PRODUCERS), before)))
            assert net.overlap_stats()[1] == 0
            got = {"gradient": net.get_grads(), "params": net.get_params(), "momentum": net.get_derivs()}
            if i == 2:
                for d in (0, 1):
                    for w in DELTAS:
                        got["%s dir %d" % (w, d)] = net.state(0, d, w)
            steps.append(got)
        return steps, moved

    try:
        two, moved_two = run(2)
        one, moved_one = run(1)
    finally:
        backend.lib.call("clstm_debug_set_option", None, 0)
    assert moved_two == [(0, 1)] * 3 and moved_one == [(1, 0)] * 3
    assert np.abs(two[2]["d_gi dir 0"]).max() > 0
    assert_same_bytes(two, one, "bench shape")
