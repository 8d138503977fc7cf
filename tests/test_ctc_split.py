"""CTC alignment with several workgroups per line (ctc.h: ctc_nsplit, ctc_line_splits, ctc_part_frames).

A line whose match scores and both lattices stay in LDS may be served by 2 or 4 workgroups: each computes phases A to D in full and emits
only its own frames.  What this file holds the library to:

  bytes    Dz and aligned are the same bytes under ctc_split = 1, 2, 4 and under the default rule, at the per-op ABI and through training
           steps (updated parameters and momentum buffer bit for bit).  ctc_split = 1 is held to the f32 oracle at the project bar (rtol
           1e-4, atol 1e-6 on the posteriors, atol 2e-6 on the deltas); the split forms are then covered by identity.
  path     every case states which of its lines split and asserts it from the library's own plan (clstm_debug_ctc_plan: form 0 and
           lm_lds 1) and the forced count from clstm_debug_ctc_split -- a case cannot pass by running one workgroup per line unnoticed.
  ranges   ctc_part_frames, the function the kernel calls: contiguous, disjoint, together [0, T), at most ceil(T / n) frames each.
  rule     ctc_nsplit: the largest n of 4, 2, 1 with bs * n <= CUs, and the option's 1 / 2 / 4 overriding it.

Lines, targets and posteriors are made as tests/test_ctc_path_sweep.py makes them (same functions, so a line listed in both files has the
same inputs)."""
import numpy as np
import pytest

from common import assert_close, synth_lines
from clstm_amd.abi import ptr
from test_ctc_path_sweep import oracle_line
from test_net_parity import set_opt, _forget_debug_options  # noqa: F401  (the fixture forgets the options after every test)
from test_ops_parity import ctc_plan, ctc_via_abi

SHORT = 0
SPLITS = (1, 2, 4)

# {minibatch: (nc, [(T, kind, n, m)], [the line splits])} -- kind / n / m as in tests/test_ctc_path_sweep.py
CASES = {
    # parts without frames (T < 4), one frame per part, uneven parts; a transcript of ONE label (lines 0-2); a label three times (line 6)
    "tiny": (83, [(1, "mk", 1, 1), (2, "mk", 1, 1), (3, "mk", 1, 1), (4, "mk", 2, 2), (5, "mk", 2, 2), (7, "mk", 3, 3), (33, "mk", 6, 2)],
             [True] * 7),
    # the headline line: 200 frames, 51 states (one label twice)
    "headline": (83, [(200, "mk", 25, 24)], [True]),
    # every label distinct; a label five times
    "labels": (83, [(60, "mk", 20, 20), (60, "mk", 20, 4)], [True, True]),
    # the lanemap bound: 257 frames take the generic phases C / D
    "lanemap": (83, [(256, "mk", 12, 12), (257, "mk", 12, 12)], [True, True]),
    # the flat bound: 210 frames x 83 classes are staged class by class
    "flat": (83, [(209, "mk", 12, 12), (210, "mk", 12, 12)], [True, True]),
    # 64 | 65 states: the second runs two states per lane with its lattices in memory and must not split (the 60-frame companion sizes
    # the carve so that the 64 class columns of the first fit behind its lattices)
    "s64": (83, [(20, "cl", 64, 64), (20, "mk", 32, 32), (60, "mk", 3, 3)], [True, False, True]),
    # the sweep's lds-cap family: both lattices fit LDS | do not (52 | 53 states); the scores behind them fit | do not (25 | 26 classes)
    "lds-cap": (40, [(40, "cl", 52, 39), (40, "cl", 53, 39), (40, "cl", 40, 25), (40, "cl", 40, 26), (10, "mk", 31, 31)],
                [False, False, True, False, True]),
    # an eligible line beside an empty line, a tiled line and a short line of 65 states
    "mixed": (83, [(100, "mk", 10, 10), (0, "mk", 2, 2), (513, "mk", 12, 12), (20, "mk", 32, 32)], [True, False, False, False]),
}
REGIMES = ("noise", "peaked10")


def nsplit_of(lib, bs, ncu):
    """clstm_debug_ctc_split: workgroups per line that splits, under the option as it stands (ncu 0: this device's CUs)"""
    out = np.zeros(1, np.int32)
    lib.call("clstm_debug_ctc_split", int(bs), int(ncu), ptr(out))
    return int(out[0])


def splits_of(recs):
    """which lines split, from the plan's records: short form, match scores (and so both lattices) in LDS"""
    return [bool(r["form"] == SHORT and r["lds_lat"] and r["lm_lds"]) for r in recs]


@pytest.fixture(scope="module")
def hostlib():
    from common import emu_lib
    return emu_lib()


# ---- bytes, at the per-op ABI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", list(CASES))
def test_split_outputs_are_the_same_bytes(backend, ora32, name, regime):
    nc, lines, want_split = CASES[name]
    data = [oracle_line(ora32, nc, line, regime) for line in lines]
    probs, states = [d[0] for d in data], [d[1] for d in data]
    assert splits_of(ctc_plan(backend, probs, states)[1]) == want_split
    got = {}
    for n in SPLITS:
        set_opt(backend, "ctc_split", n)
        assert nsplit_of(backend.lib, len(lines), 0) == n          # forced: whatever the device's CUs are
        got[n] = ctc_via_abi(backend, probs, states)
    set_opt(backend, "ctc_split", 0)
    got[0] = ctc_via_abi(backend, probs, states)                   # the default rule (one CU per workgroup of the launch)
    assert nsplit_of(backend.lib, len(lines), 0) in SPLITS
    al, dz, loff = got[1]
    for i, (p, st, want) in enumerate(data):
        if not len(p):
            continue
        what = "%s %s line %d" % (name, regime, i)
        assert_close(al[loff[i]:loff[i + 1]], want, rtol=1e-4, atol=1e-6, what="aligned, " + what)
        assert_close(dz[loff[i]:loff[i + 1]], want - p, rtol=1e-4, atol=2e-6, what="delta, " + what)
    for n in (2, 4, 0):
        assert np.array_equal(got[n][0].view(np.uint32), al.view(np.uint32)), "aligned differs, ctc_split=%d, %s %s" % (n, name, regime)
        assert np.array_equal(got[n][1].view(np.uint32), dz.view(np.uint32)), "Dz differs, ctc_split=%d, %s %s" % (n, name, regime)


def test_outputs_without_aligned(backend, ora32):
    """aligned == NULL (what a training step passes): the deltas alone, the same bytes"""
    nc, lines, _ = CASES["tiny"]
    data = [oracle_line(ora32, nc, line, "noise") for line in lines]
    probs, states = [d[0] for d in data], [d[1] for d in data]
    loff = np.concatenate([[0], np.cumsum([len(p) for p in probs])]).astype(np.int32)
    soff = np.concatenate([[0], np.cumsum([len(s) for s in states])]).astype(np.int32)
    st = np.concatenate(states).astype(np.int32)
    got = {}
    for n in SPLITS:
        set_opt(backend, "ctc_split", n)
        P_ = backend.up(np.concatenate(probs, 0))
        D_ = backend.zeros((loff[-1], nc))
        backend.lib.call("clstm_ctc_align_batch", ptr(P_), ptr(D_), None, nc, ptr(loff), ptr(st), ptr(soff), len(probs))
        got[n] = backend.down(D_)
    assert got[1].any()
    for n in (2, 4):
        assert np.array_equal(got[n].view(np.uint32), got[1].view(np.uint32)), n


# ---- bytes, through training steps -----------------------------------------------------------------------------------------------------
def test_training_steps_are_the_same_bytes(backend):
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    ni, nh, nc = 8, [10], 83
    rng = np.random.default_rng(11)
    p0 = init_params(ni, nh, nc, seed=0.222) * 20
    batches = []
    for T in ([33, 7, 3, 50], [5, 64, 1, 20]):
        trs = [rng.integers(1, nc, max(1, t // 4)).astype(np.int32) for t in T]
        batches.append((T, np.concatenate(synth_lines(rng, T, ni), 0), trs))
    for T, _, trs in batches:                                      # every line of every step splits
        states = [np.zeros(2 * len(tr) + 1, np.int32) for tr in trs]
        for s, tr in zip(states, trs):
            s[1::2] = tr
        assert all(splits_of(ctc_plan(backend, [np.zeros((t, nc), np.float32) for t in T], states)[1]))
    got = {}
    for n in SPLITS:
        set_opt(backend, "ctc_split", n)
        assert nsplit_of(backend.lib, 4, 0) == n
        net = Network(ni, nh, nc, lib=backend.lib)
        net.set_params(p0)
        net.setLearningRate(1e-3, 0.9)
        for T, x, trs in batches:
            xd = backend.up(x)
            net.train_step(T, xd, trs)
        got[n] = (net.get_params(), net.get_derivs())
        del net
    assert not np.array_equal(got[1][0], p0.astype(np.float32)) and got[1][1].any()
    for n in (2, 4):
        assert np.array_equal(got[n][0].view(np.uint32), got[1][0].view(np.uint32)), "parameters differ, ctc_split=%d" % n
        assert np.array_equal(got[n][1].view(np.uint32), got[1][1].view(np.uint32)), "momentum buffer differs, ctc_split=%d" % n


# ---- the frame ranges, host only -------------------------------------------------------------------------------------------------------
def test_part_frames_tile_the_line(hostlib):
    r = np.zeros(2, np.int32)
    for n in SPLITS:
        for T in range(601):
            at = 0
            for k in range(n):
                hostlib.call("clstm_debug_ctc_part_frames", T, n, k, ptr(r))
                lo, hi = int(r[0]), int(r[1])
                assert lo == at and lo <= hi <= T, (T, n, k, lo, hi)            # contiguous, disjoint, in order
                assert hi - lo <= -(-T // n), (T, n, k, lo, hi)                  # at most ceil(T / n) frames
                at = hi
            assert at == T, (T, n)                                               # together [0, T)


# ---- the rule, host only ---------------------------------------------------------------------------------------------------------------
def test_the_rule(hostlib):
    try:
        for bs in (1, 16, 64, 65, 76, 77, 128, 129, 256):
            for ncu in (16, 104, 256, 304):
                hostlib.call("clstm_debug_set_option", b"ctc_split", 0)
                want = max(n for n in SPLITS if n == 1 or bs * n <= ncu)
                assert nsplit_of(hostlib, bs, ncu) == want, (bs, ncu)
                for forced in SPLITS:
                    hostlib.call("clstm_debug_set_option", b"ctc_split", forced)
                    assert nsplit_of(hostlib, bs, ncu) == forced, (bs, ncu, forced)
        # the headline minibatch on the chip it is measured on, and the legs that keep one workgroup per line
        hostlib.call("clstm_debug_set_option", b"ctc_split", 0)
        assert nsplit_of(hostlib, 64, 256) == 4 and nsplit_of(hostlib, 128, 256) == 2 and nsplit_of(hostlib, 256, 256) == 1
        from clstm_amd.abi import ClstmError
        hostlib.call("clstm_debug_set_option", b"ctc_split", 3)
        with pytest.raises(ClstmError, match="ctc_split"):
            nsplit_of(hostlib, 64, 256)
    finally:
        hostlib.call("clstm_debug_set_option", None, 0)
