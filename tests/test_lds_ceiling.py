"""The dynamic-LDS ceiling of a kernel (clstm_amd/csrc/runtime.inc: allow_dynamic_lds) grows with the request and survives a smaller one.

A launch that carves more than 64 KiB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize raised on its kernel first.  The
library has ONE rule for that, keyed by the kernel: raise when a launch asks for more than the kernel has been given, never lower.  Each
test makes three calls in one process, on the calling thread's one workspace: a first carve, a larger one, the first again.  Every call
is compared with the referee the kernel's own test file has (imported, not restated), at that file's own bar.  On the emulator there is
no ceiling and these are plain correctness cases; the device run is the one that exercises the rule: a kernel whose ceiling was never
raised, was raised once for good, or did not outlast the smaller call refuses its launch there.

Shapes: the smallest that cross 64 KiB (65536 bytes = 16384 words), from the host layout functions.
  alignment  the carve is read from clstm_debug_ctc_plan and asserted: 6 frames x 5 classes below, 60 frames x 101 classes above.
  score      score_lds_layout (ctc_score.h) puts tile * ncp words into the posterior tile; tile = min(256, 20480 / 101, T) = T = 180 and
             ncp = 101: 180 * 101 * 4 = 72720 bytes by that term alone.  One call with every output launches the sum and the max-plus
             kernel, which carves 8 * T words more.
  beam       beam_lds_words below restates beam_lds_layout and plan_ctc_beam (ctc_beam.h, ctc_run.inc) and the test asserts what it
             says.  beam = 32 at 101 classes: the fixed part is 9096 words (14008 with a language model), a line's sections
             [hash | nodes | class lists | log posteriors] come behind it while they fit the rest of 36864 words.
               plain, every section in LDS   T = 20: 2048 + 3 * 641 + 2 * 20 * 64 + 20 * 101 = 8551 -> 17647 words = 70588 bytes
               LM, every section it may      T = 8:  1024 + 5 * 257 + 8 * 101 = 3117 -> 17125 words = 68500 bytes
             The other instantiation runs when a section of some line does NOT fit, so it has no carve below 64 KiB at lines a test can
             afford (every section would have to miss 27768 words of room: more than 12000 frames).  Its sequence is first above
             64 KiB, larger, first again:
               plain  T = 64: 8192 + 3 * 2049 + 2 * 64 * 64 = 22531 (the posteriors, 6464, do not fit) -> 126508 bytes; T = 80 -> 140844
               LM     T = 64: 8192 + 5 * 2049 = 18437 (the posteriors do not fit) -> 129780 bytes; T = 70 -> 133620
  The score's and the beam's carves cannot be read back through the ABI.  A kernel trace of this file on the device
  (profiles/refactor_batched_calls.txt) shows the kernels and grids of the three calls of every case; its LDS column holds a kernel's
  static LDS only (0 for these kernels), so the dynamic sizes stand on the arithmetic above.

The narrow net's batched MFMA recurrences carve a compile-time constant per kernel (MfmaGeom::SMEM, above 64 KiB), so their ceiling has
one size and no order of requests; tests/test_mfma_recurrence.py and tests/test_mfma_bench_shapes.py launch them on the device.
"""
import functools

import numpy as np
import pytest

import test_ctc_beam as tb
import test_ctc_beam_lm as tl
import test_ctc_score as ts
from common import assert_close
from test_net_parity import set_opt, _forget_debug_options  # noqa: F401  (the fixture forgets the options after every test)
from test_ops_parity import ctc_plan, ctc_via_abi

F32 = np.float32
KIB64 = 65536
NC_SMALL, NC_BIG = 5, 101


# ---- alignment: ctc_align_kernel<false>, and <true> through the option ctc_float ---------------------------------------------
@functools.lru_cache(maxsize=None)
def align_case(ora32, T, L, nc):
    rng = np.random.default_rng(100 * T + nc)
    p = rng.random((T, nc)).astype(F32) ** 4
    p = (p / p.sum(1, keepdims=True)).astype(F32)
    st = ora32.mktargets(rng.integers(1, nc, L))
    return p, st, ora32.ctc_align_classes(p, st)


@pytest.mark.parametrize("ctc_float", [0, 1])
def test_alignment(backend, ora32, ctc_float):
    """the bars of test_ops_parity.py: test_ctc_vs_oracle, and test_ctc_float_logadd_option for the option"""
    small, big = align_case(ora32, 6, 2, NC_SMALL), align_case(ora32, 60, 20, NC_BIG)
    carve = [ctc_plan(backend, [c[0]], [c[1]])[0]["smem"] for c in (small, big)]
    print("alignment carves: %d, %d bytes" % tuple(carve))
    assert carve[0] <= KIB64 < carve[1], carve
    rtol, atol, datol = (1e-3, 1e-4, 1e-4) if ctc_float else (1e-4, 1e-6, 2e-6)
    set_opt(backend, "ctc_float", ctc_float)
    for what, (p, st, want) in (("first", small), ("larger", big), ("first again", small)):
        al, dz, _ = ctc_via_abi(backend, [p], [st])
        assert_close(al, want, rtol=rtol, atol=atol, what="aligned, %s call" % what)
        assert_close(dz, want - p, rtol=rtol, atol=datol, what="delta, %s call" % what)


# ---- score: ctc_score_kernel<false> and <true> in one call ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_case(T, S, nc):
    rng = np.random.default_rng(10 * T + nc)
    classes = ts.states_for(rng, S, nc)
    return ts.Case(ts.peaked_probs(rng, T, classes, nc), classes, "T=%d S=%d nc=%d" % (T, S, nc))


def test_score(backend):
    small, big = score_case(6, 3, NC_SMALL), score_case(180, 41, NC_BIG)
    assert 6 * (NC_SMALL | 1) * 4 < KIB64 // 2 and 180 <= 20480 // NC_BIG and 180 * (NC_BIG | 1) * 4 > KIB64   # the posterior tile alone
    for c in (small, big, small):
        ts.run_cases(backend, [c], NC_SMALL if c is small else NC_BIG)


# ---- beam: ctc_beam_kernel<all in LDS, language model> in its four instantiations ------------------------------------------------
BEAM_LDS_WORDS, BEAM_MAX = 36 * 1024, 32   # ctc_beam.h


def beam_lds_words(T, nc, beam, lm):
    """(LDS words of a launch with this one line, whether every section that may lies in LDS): beam_lds_layout and plan_ctc_beam"""
    K = nc - 1 if lm else min(nc - 1, 2 * beam)
    fixed = 4 * (beam + beam * K) + 2 * 7 * BEAM_MAX + 2 * BEAM_MAX + 2 * (2 * K + 2) + 4 + (5 * BEAM_MAX if lm else 0)
    fixed += fixed & 1
    nn = 1 + T * beam
    H = 64
    while H < 2 * nn:
        H *= 2
    used, all_lds = 0, True
    for s, need in enumerate((H, (5 if lm else 3) * nn, 2 * T * K, T * nc)):
        if lm and s == 2:
            continue                      # (the complete class list: always in the workspace)
        if used + need <= BEAM_LDS_WORDS - fixed:
            used += need
        else:
            all_lds = False
    return fixed + used, all_lds


@functools.lru_cache(maxsize=None)
def beam_lm(nc):
    return tl.random_lm(7 + nc, 2, nc, weight=0.5, bonus=0.2)


@functools.lru_cache(maxsize=None)
def beam_line(T, nc, beam, lm):
    rng = np.random.default_rng(1000 * T + nc)
    probs = tb.peaked_probs(rng, T, rng.integers(1, nc, max(1, T // 4)), nc, 0.9)
    what = "T=%d nc=%d beam=%d%s" % (T, nc, beam, " lm" if lm else "")
    return tl.Line(probs, beam, beam_lm(nc), what) if lm else tb.Line(probs, beam, what)


#             lm, all in LDS, (T, nc, beam) of the first call, of the larger one
BEAM_CASES = [(False, True, (6, NC_SMALL, 4), (20, NC_BIG, 32)), (False, False, (64, NC_BIG, 32), (80, NC_BIG, 32)),
              (True, True, (6, NC_SMALL, 4), (8, NC_BIG, 32)), (True, False, (64, NC_BIG, 32), (70, NC_BIG, 32))]


@pytest.mark.parametrize("lm,all_lds,first,larger", BEAM_CASES)
def test_beam(backend, lm, all_lds, first, larger):
    nbest = 4
    w0, w1 = beam_lds_words(*first, lm), beam_lds_words(*larger, lm)
    print("beam carves: %d, %d bytes" % (4 * w0[0], 4 * w1[0]))
    assert w0[1] == w1[1] == all_lds and w0[0] < w1[0] and 4 * w1[0] > KIB64, (w0, w1)
    assert (4 * w0[0] <= KIB64) == all_lds, w0   # (the instantiation for a section outside LDS has no small carve: see above)
    for shape in (first, larger, first):
        T, nc, beam = shape
        ln = beam_line(T, nc, beam, lm)
        assert ln.gauge(nbest)[0], "the line proves too little: undecided by the referee alone"
        if lm:
            got, _ = tl.call_beam_lm(backend, [ln.probs], nc, beam, nbest, beam_lm(nc))
            assert ln.check(nbest, nc, got[0])
        else:
            got, _ = tb.call_beam(backend, [ln.probs], nc, beam, nbest)
            assert ln.check(nbest, nc, got[0])[0]
