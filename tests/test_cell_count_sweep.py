"""Parity sweep over hidden sizes at every edge of the per-line recurrence's instantiations (lstm_seq.h and the launches built on it).

The recurrence is specialised by cell count ((NK4, KU) from runtime.inc:narrow_class), by workgroup size (net.inc:Net::build,
nthreads = 64 * ceil(no / 16): 1 to 8 waves, workgroups of more than four waves staggered into group A = waves 0..3 and group B = the
rest, devintrin.h:stag_on) and by launch form (plain, fused forward, overlapped backward as one or two launches, the x.d prologue forms,
no-save).  tests/narrow_rule.py restates the rule (runtime.inc:narrow_plan) ONCE in Python, and every case asserts the path counters the
rule predicts -- which form ran follows from the rule, never from the result -- and that the library's own plan for its shape
(clstm_debug_narrow_plan) is the restated one.

Every oracle comparison is test_net_parity.run_case at its default bars (1e-4 / 2e-6 on saved activations, bit-exact decodes, 1e-4 on
CTC posteriors, deltas, the minibatch gradient and the momentum buffer, the derived bar on the update), weights init x 12, lr 1e-3.
Line lengths are chosen for the loops' edges: T = [37, 16, 1, 20, 6, 2, 17] -- a second 32-frame x.d round, the fused forward's
16-frame chunk exactly and plus one, the backward's three rotating operand sets and its 6-step body at 1, 2 and 6; the byte comparison
of the x.d forms uses T = [65, 1, 33, 0, 16, 6] -- a full round plus a one-frame tail, a one-frame item, an empty line.

The host emulator (-m "not gpu") runs the lowest size of every (NK4, KU, waves) class through the default rule, overlap = 2, the x.d
forms and recognition, with 6 inputs, 9 classes and the first four lengths; the MI355X (-m gpu) runs everything.

Each test prints `SWEEP <case> class=(NK4, KU, waves) moved=<counters> worst=<largest error / bar> <per quantity>`.
`python tests/test_cell_count_sweep.py [pytest output of a GPU run]` prints the table of DESIGN.md from geometry() and the rules."""
import contextlib
import re
import sys

import numpy as np
import pytest

from common import ATOL, ROOT, RTOL, synth_lines
if ROOT not in sys.path:          # (run as a script for the table: no conftest.py has put the package on the path)
    sys.path.insert(0, ROOT)
import test_net_parity
from test_net_parity import run_case, set_opt, _forget_debug_options, _path_count  # noqa: F401  (autouse fixture)
from test_predict import NOSAVE_FUSED, NOSAVE_LINE, TRAIN_FUSED, check_identity, count, make_net, varied_params
from test_xd_producers import check_case
from narrow_rule import assert_net_plans_agree, cus, fused_forward, geometry, klass, narrow, overlapped, xd_form  # noqa: F401

SIZES = [1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 63, 64, 65, 79, 80, 81, 95, 96, 97, 100, 101, 111, 112, 113, 120, 127, 128]
WIDE = 129                                  # the smallest size that takes lstm_wide.h by itself (narrow_class finds no instantiation)
T_ORACLE = [37, 16, 1, 20, 6, 2, 17]
T_BYTES = [65, 1, 33, 0, 16, 6]
SCALE, LR = 12.0, 1e-3
PC_FWD_FUSED, PC_LINE_NOSAVE, PC_FUSED_NOSAVE, PC_XD_PROLOGUE, PC_XD_PRODUCERS = 5, 22, 23, 26, 27
COUNTERS = (PC_FWD_FUSED, PC_LINE_NOSAVE, PC_FUSED_NOSAVE, PC_XD_PROLOGUE, PC_XD_PRODUCERS)


# ---- 1. the rule: tests/narrow_rule.py ---------------------------------------------------------------------------------------------
def expected_training(nh, uni, nc, nlines, overlap, kind, strict=False):
    """({counter: moves} of one forward + backward, overlapped backward passes)"""
    moves = {}
    if fused_forward(nh, uni, nc, nlines, overlap, kind):
        moves[PC_FWD_FUSED] = 1
    form = xd_form(nh, uni, nc, nlines, overlap, kind, strict)
    if form:
        moves[PC_XD_PRODUCERS if form == 2 else PC_XD_PROLOGUE] = 1
    return moves, sum(overlapped(no, overlap) for no in nh)


def classes():
    """{(nk4, ku, waves): [cell counts]} for 1..128 cells"""
    out = {}
    for no in range(1, 129):
        out.setdefault(klass(no), []).append(no)
    return out


# one size per class, not a multiple of 16 (nor of 4): the lowest of the class
LOWEST = [members[0] for members in classes().values()]


def test_the_sweep_covers_every_class_at_both_ends():
    """for every (nk4, ku, waves) class the rule yields for 1..128 cells: its lowest and its highest cell count and one that is not a
    multiple of 4 are swept -- a later change to the tables makes the gap visible here"""
    assert len(classes()) == 9 and {k[:2] for k in classes()} == {(1, 4), (2, 8), (4, 16), (7, 28), (7, 25), (8, 32)}
    for k, members in classes().items():
        swept = [no for no in SIZES if klass(no) == k]
        assert members[0] in swept and members[-1] in swept, (k, members[0], members[-1], swept)
        assert any(no % 4 for no in swept), (k, swept)
    assert all(no % 16 and no % 4 for no in LOWEST) and LOWEST == [1, 17, 33, 49, 65, 81, 97, 101, 113]
    assert geometry(WIDE)[0] is None and narrow(WIDE - 1)
    # the edges this sweep exists for, from the rule: group B of one wave, (7, 28) with seven waves, the 8-wave partial workgroup
    assert geometry(65)[:4] == (7, 28, 5, 1) and geometry(101)[:4] == (7, 28, 7, 3) and geometry(100)[:4] == (7, 25, 7, 3)
    assert geometry(113)[:4] == (8, 32, 8, 4) and geometry(63)[:4] == (4, 16, 4, 0) and geometry(64)[4]
    # the fused forward: bidirectional 81..112, one direction up to 120, never a size whose last lane owns a cell
    assert [no for no in range(1, 130) if fused_forward([no], False, 83, 7, 2, "hip")] == [no for no in range(81, 113) if no % 16]
    assert [no for no in range(1, 130) if fused_forward([no], True, 83, 7, 2, "hip")] == [no for no in range(81, 121) if no % 16]


# ---- the measuring wrapper --------------------------------------------------------------------------------------------------------
QUANTITIES = ("softmax outputs", "state", "aligned", "delta", "minibatch gradient", "params after update", "momentum buffer")


@contextlib.contextmanager
def recording():
    """every assert_close of run_case, recorded as max |a - b| / bar per compared quantity before it asserts"""
    worst = {}
    real = test_net_parity.assert_close

    def measured(a, b, rtol=RTOL, atol=ATOL, what="", scale_atol=0.0):
        a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
        if a64.shape == b64.shape and b64.size:
            bar = atol + scale_atol * float(np.abs(b64).max()) + rtol * np.abs(b64)
            with np.errstate(invalid="ignore"):
                frac = float(np.nan_to_num(np.abs(a64 - b64) / bar, nan=np.inf).max())
            q = next(q for q in QUANTITIES if what.startswith(q))
            worst[q] = max(worst.get(q, 0.0), frac)
        real(a, b, rtol=rtol, atol=atol, what=what, scale_atol=scale_atol)
    test_net_parity.assert_close = measured
    try:
        yield worst
    finally:
        test_net_parity.assert_close = real


def report(name, nh, moved, passes, worst):
    k = klass(nh[-1])
    print("SWEEP %s class=%r moved=%r overlapped=%d worst=%.3f %s" % (
        name, k, moved, passes, max(worst.values()) if worst else 0.0, " ".join("%s=%.3f" % (q.replace(" ", "_"), f) for q, f in worst.items())))


def oracle_case(backend, ora32, name, nh, uni=False, overlap=None, strict=False, split_terms=None):
    """one net, one minibatch against the oracle; the counters must move as the rule says"""
    emu = backend.kind == "emu"
    ni, nc = (6, 9) if emu else (48, 83)
    T = T_ORACLE[:4] if emu else T_ORACLE
    if split_terms is not None:
        set_opt(backend, "split_terms", split_terms)          # (read when the net is created)
    want_moves, want_passes = expected_training(nh, uni, nc, len(T), overlap, backend.kind, strict)
    assert_net_plans_agree(backend.lib, nh, ni=ni, uni=uni, nc=nc, nlines=len(T), tmax=max(T), frames=sum(T), overlap=overlap, strict=strict,
                           kind=backend.kind, split_terms=3 if split_terms is None else split_terms)
    before = {c: _path_count(backend, c) for c in COUNTERS}
    net, moved, passes, timeouts = None, None, -1, -1
    with recording() as worst:
        try:
            net, _ = run_case(backend, ora32, ni, nh if len(nh) > 1 else nh[0], nc, T, uni=uni, scale=SCALE, lr=LR, overlap=overlap, strict_f32=strict)
        finally:
            moved = {c: _path_count(backend, c) - before[c] for c in COUNTERS if _path_count(backend, c) != before[c]}
            if net is not None:
                passes, timeouts = net.overlap_stats()
            report(name, nh, moved, passes, worst)
    assert moved == want_moves, (moved, want_moves)
    assert (passes, timeouts) == (want_passes, 0), (passes, timeouts, want_passes)
    assert set(worst) == set(QUANTITIES)


def both(sizes, emu_sizes):
    """(backend, size) pairs: the emulator's subset, everything on the GPU"""
    return [("emu", no) for no in emu_sizes] + [pytest.param("hip", no, marks=pytest.mark.gpu) for no in sizes]


def only_gpu(cases):
    return [pytest.param("hip", c, marks=pytest.mark.gpu) for c in cases]


def ids(v):
    return str(v).replace(" ", "") if not isinstance(v, str) else v


# ---- 3a / 3b: every cell count, bidirectional -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,no", both(SIZES + [WIDE], LOWEST), indirect=["backend"], ids=ids)
def test_default_rule_bidirectional(backend, ora32, no):
    """the launches the library picks by itself for a small minibatch: plain per-line forward and backward, nothing overlapped"""
    oracle_case(backend, ora32, "default bidi %d" % no, [no])


@pytest.mark.parametrize("backend,no", both(SIZES + [WIDE], LOWEST), indirect=["backend"], ids=ids)
def test_overlap_forced_bidirectional(backend, ora32, no):
    """overlap = 2: the fused forward (81..111 cells) and the overlapped backward -- one launch from four waves on, two below, none
    where the last lane owns a cell -- with the x.d prologue in the form narrow_plan picks; no wait ran into its watchdog"""
    oracle_case(backend, ora32, "overlap2 bidi %d" % no, [no], overlap=2)


# ---- 3c: one direction -- the only way into lstm_fwd_fused_kernel<8, 32> (113..120 cells) -------------------------------------------
UNI_SIZES = [49, 50, 63, 65] + [no for no in SIZES if no >= 81] + [115, 121]


@pytest.mark.parametrize("backend,no", only_gpu(UNI_SIZES), indirect=["backend"], ids=ids)
def test_overlap_forced_unidirectional(backend, ora32, no):
    """113, 115 and 120 cells take the 8-wave fused forward; 121 and 127 (31 column tiles and more) must decline it and still pass"""
    assert fused_forward([no], True, 83, len(T_ORACLE), 2, "hip") == (81 <= no <= 120 and no % 16 != 0)
    oracle_case(backend, ora32, "overlap2 uni %d" % no, [no], uni=True, overlap=2)


# ---- 3d: the <N, K, 0> and <N, K, 2> variants of the overlapped backward, one size per class ----------------------------------------
@pytest.mark.parametrize("backend,no", only_gpu(LOWEST), indirect=["backend"], ids=ids)
def test_overlap_forced_strict_f32(backend, ora32, no):
    """clstm_net_set_strict_f32: the weight-gradient items on the f32 MFMA (lstm_bwd_dw_kernel<N, K, 0>), x.d as a launch of its own"""
    oracle_case(backend, ora32, "overlap2 strict %d" % no, [no], overlap=2, strict=True)


@pytest.mark.parametrize("backend,no", only_gpu(LOWEST), indirect=["backend"], ids=ids)
def test_overlap_forced_two_split_terms(backend, ora32, no):
    """split_terms = 2: hi + lo bf16 terms, three products (lstm_bwd_dw_kernel<N, K, 2> / lstm_bwd_xd_kernel<N, K, 2>)"""
    oracle_case(backend, ora32, "overlap2 terms2 %d" % no, [no], overlap=2, split_terms=2)


# ---- 3g: stacked nets whose lower layer's 2 x no is no multiple of 16 -----------------------------------------------------------------
@pytest.mark.parametrize("overlap", [None, 2], ids=["default", "overlap2"])
@pytest.mark.parametrize("backend,nh", only_gpu([[65, 49], [50, 113]]), indirect=["backend"], ids=ids)
def test_stacked(backend, ora32, nh, overlap):
    """the K tail of the hoisted W_x product and of the inter-layer dX (130 and 100 input columns of the upper layer); only a net of
    one layer is fused-forward eligible, so counter 5 stays put, and both layers' backward passes overlap when forced"""
    oracle_case(backend, ora32, "stacked %r %s" % (nh, overlap), nh, overlap=overlap)


# ---- 3e: the three xd_prologue forms as bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,no", both(LOWEST + [64, 112], LOWEST), indirect=["backend"], ids=ids)
def test_xd_forms_same_bytes(backend, no):
    """test_xd_producers.check_case, options 0 / 1 / 2 over two steps: on the GPU four waves and more move counter 27, fewer counter 26;
    the emulator counter 26 throughout; 64 and 112 cells (no overlapped launch) neither"""
    emu = backend.kind == "emu"
    ni, nc = (6, 9) if emu else (48, 83)
    T = T_BYTES[:4] if emu else T_BYTES
    eligible = xd_form([no], False, nc, len(T), 2, backend.kind) != 0
    assert eligible == (no % 16 != 0)
    print("SWEEP xd bytes %d class=%r" % (no, klass(no)))
    # The emulator walks every lane of every wave, and asked for 2 it runs 1 (test_xd_producers compares those two there): option 2
    # against 0, one step -- a second step is about the ready words of form 2, which only the GPU runs -- keeps its nine cases near 30 s.
    options, nsteps = ((0, 2), 1) if emu else ((0, 1, 2), 2)
    check_case(backend, "bilstm%d" % no, (ni, [no], nc, T, False, eligible, geometry(no)[2] >= 4), options=options, nsteps=nsteps)


# ---- 3f: recognition ------------------------------------------------------------------------------------------------------------------
def recognition_lines(backend, rng):
    emu = backend.kind == "emu"
    ni, nc = (6, 9) if emu else (48, 83)
    return ni, nc, synth_lines(rng, T_ORACLE[:4] if emu else T_ORACLE, ni)


@pytest.mark.parametrize("backend,no", both(LOWEST, LOWEST), indirect=["backend"], ids=ids)
def test_predict_per_line_no_save(backend, no):
    """predict against forward as bytes (Z, decodes, conf, h) through lstm_fwd_kernel<N, K, false> of every class"""
    ni, nc, lines = recognition_lines(backend, np.random.default_rng(11))
    print("SWEEP predict %d class=%r" % (no, klass(no)))
    net = make_net(backend, ni, [no], nc, varied_params(backend, ni, [no], nc, lines))
    check_identity(backend, net, lines, NOSAVE_LINE)


FUSED_BIDI = [no for no in SIZES if fused_forward([no], False, 83, len(T_ORACLE), 2, "hip")]
FUSED_UNI = [81, 113, 115, 120]
FUSED_CASES = [(no, False) for no in FUSED_BIDI] + [(no, True) for no in FUSED_UNI]
FUSED_EMU = [(no, False) for no in FUSED_BIDI if no in LOWEST] + [(113, True)]


@pytest.mark.parametrize("backend,case", both(FUSED_CASES, FUSED_EMU), indirect=["backend"], ids=ids)
def test_predict_fused_no_save(backend, case):
    """the fused launch with the recurrence role in its no-save form (lstm_fwd_fused_kernel<N, K, false>), forced as
    test_predict.test_predict_fused_forced_small does, at every swept size the fused forward admits"""
    no, uni = case
    ni, nc, lines = recognition_lines(backend, np.random.default_rng(12))
    assert fused_forward([no], uni, nc, len(lines), 2, backend.kind)
    print("SWEEP predict fused %d %s class=%r" % (no, "uni" if uni else "bidi", klass(no)))
    net = make_net(backend, ni, [no], nc, varied_params(backend, ni, [no], nc, lines, uni), uni=uni, overlap=2)
    c0 = count(backend, TRAIN_FUSED)
    check_identity(backend, net, lines, NOSAVE_FUSED)
    assert count(backend, TRAIN_FUSED) == c0 + 1


# ---- the table of DESIGN.md ---------------------------------------------------------------------------------------------------------
def forms(no, uni):
    """launch forms beyond the plain and the per-line no-save launch, which every size has (F: fused forward and its no-save twin;
    B1 / B2: overlapped backward as one launch / as two; the x.d form behind it)"""
    out = []
    if fused_forward([no], uni, 83, len(T_ORACLE), 2, "hip"):
        out.append("F")
    if overlapped(no, 2):
        out.append("B1 + x.d producers" if geometry(no)[2] >= 4 else "B2 + x.d prologue")
    return ", ".join(out) or "-"


def table(log=None):
    worst = {}
    if log:
        for m in re.finditer(r"^\W*SWEEP .* class=\((\d+), (\d+), (\d+)\) moved=.* worst=([0-9.]+|inf)", open(log).read(), re.M):
            k = tuple(int(x) for x in m.groups()[:3])
            worst[k] = max(worst.get(k, 0.0), float(m.group(4)))
    rows = ["| cells | NK4 / KU | waves | group-B waves | bidirectional | one direction | worst error / bar (MI355X) |", "|---|---|---|---|---|---|---|"]
    runs = []
    for no in range(1, 129):
        key = (geometry(no)[:4], forms(no, False), forms(no, True))
        if runs and runs[-1][0] == key:
            runs[-1][2] = no
        else:
            runs.append([key, no, no])
    for (g, bi, un), lo, hi in runs:
        w = worst.get(g[:3])
        rows.append("| %s | %d / %d | %d | %d | %s | %s | %s |" % ("%d" % lo if lo == hi else "%d..%d" % (lo, hi), g[0], g[1], g[2], g[3], bi, un,
                                                                   "%.2f" % w if w is not None else "-"))
    return "\n".join(rows)


if __name__ == "__main__":
    import sys
    print(table(sys.argv[1] if len(sys.argv) > 1 else None))
