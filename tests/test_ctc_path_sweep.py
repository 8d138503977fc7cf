"""CTC alignment sweep over every edge of the kernel's path rule, the path asserted (ctc.h: ctc_align_kernel).

Which path a line takes is decided in ctc.h by ctc_batch_plan (host, once per minibatch: tile, smax, ncp), ctc_line_plan and
ctc_scores_in_lds (every workgroup, from its line and the batch plan).  clstm_debug_ctc_plan answers with the same functions on the host;
every claim below about a path is an assertion on its answer, never a comment.

CASES is the literal list of minibatches (one launch each); EDGES names, for every decision of the plan, two listed lines that differ by
one in a single quantity (T, S, nc or the number of distinct classes) and sit on the two sides of the decision -- so the first is AT the
bound and the second one past it, whatever the constants in ctc.h are.  A later change to CTC_CCACHE, to the carve or to a predicate
that moves a bound fails test_the_sweep_covers_every_decision_on_both_sides with the name of the side that lost its line.

Parity (test_parity, test_companions): every line of every minibatch against the f32 oracle (oracle.ctc_align_classes), under two bars.
  project bar  the suite's: rtol 1e-4, atol 1e-6 on the posteriors, atol 2e-6 on the deltas.
  tight bar    |aligned - oracle| <= N(k) * 2^-23 * m_t for every class of frame t, m_t the frame's largest oracle posterior and k the most
               occurrences of one label in the line's target.  N follows from the error budget ctc.h states for itself, in units of
               eps = 2^-23 (one float32 ulp, relative), every quantity being a sum of positive terms so that relative errors carry over:
                 recursion (alpha, reversed alpha)     0: cr_math.h reproduces every float rounding of the reference's log_add
                 epath = limexp(both - max)            3: ctc_limexp <= 2 ulp including v_exp_f32, the reference's expf <= 1 ulp
                 per-state total (double)              3: a sum of such cells
                 cell / total                          7 = 3 + 3 + 1: each side rounds its quotient to float once (the kernel's
                                                          reciprocal multiply in double is exact to 2^-52 before that rounding)
                 class column                          8 + (k - 1) / 2 for k >= 3, else 8: one rounding of the sum on each side; labels
                                                          that occur three times or more are added in float, k - 1 additions of
                                                          half an ulp each (blank and k <= 2: the reference's double accumulator)
                 frame total (double)                  as the columns
                 aligned = column / total              N = 2 * column + 1: the second reciprocal multiply and its rounding
               N = 17 for k <= 2 and 16 + k beyond: 2.0e-6 m_t at k <= 2 against the project bar's 1e-4 m_t + 1e-6 there.  Every listed target
               keeps k <= 25, so N * 2^-23 <= 4.9e-6 <= 1e-5: at a frame's significant posteriors the tight bar is twenty times tighter than the
               project bar or more (asserted per line); at posteriors near zero the project bar's absolute 1e-6 stays the tighter one, which is
               why both are asserted.
               The deltas carry no bar of their own: d = aligned - p is ONE float subtraction of the kernel's own posterior (clstmhl.h:211-212),
               asserted bit for bit.
Two input regimes: the suite's noise (random ** 4, normalised, one exact zero for the 1e-5 floor) and peaked posteriors (one class per
frame at 0.98 along a monotone walk over the line's states, one other class with the remainder, the rest below the 1e-5 floor; a share
0 / 0.1 / 0.5 of the frames on a wrong class, so that log_add's cut-off at 10 and limexp's clamp at -30 are reached).

Each test prints `SWEEP ctc <case> <regime> <backend> line=<i> plan=<record> worst=<largest error / tight bar>` per line.
`python tests/test_ctc_path_sweep.py [pytest output ...]` prints the tables of DESIGN.md 4.5 from the plan entry and those lines."""
import re
import sys
import zlib

import numpy as np
import pytest

from common import ROOT, assert_close
if ROOT not in sys.path:          # (run as a script for the table: no conftest.py has put the package on the path)
    sys.path.insert(0, ROOT)
from clstm_amd.abi import ptr
from test_ops_parity import ctc_via_abi

FIELDS = ("T", "S", "nu", "form", "rec", "flat", "lds_lat", "lm_lds", "lanemap", "flat_stage", "c_in_regs", "d_per_state", "ntiles")
SHORT, TILED, HUGE, NONE = 0, 1, 2, 3                   # form (include/clstm_abi.h: clstm_debug_ctc_plan)
WAVE, PAIR, RM2, RM8, ROUNDS = 0, 1, 2, 3, 4            # rec
FORM_NAMES = ("short", "tiled", "huge", "none")
REC_NAMES = ("one wave", "two per lane", "RM 2", "RM 8", "rounds")
EPS = 2.0 ** -23
KMAX = 25                                               # most occurrences of one label in a listed target (see N above)

# ---- the case list: {minibatch: (nc, [(T, kind, n, m)])} ----------------------------------------------------------------------------
# kind "mk": n labels, blank-interleaved (mktargets): S = 2 n + 1.  "cl": a plain class list of n states without blanks (the Classes
# overload), so S can be even.  m: distinct labels, taken in turn (label i of the target is label i mod m): repeats at distance m.
X = (200, "mk", 25, 24)                                 # the companion tests' line: the OCR bench shape
CASES = {
    # S = 1, 2, a full wave and its neighbours, a full two-per-lane wave and its neighbours (all short lines, scores from memory for S > 64)
    "waves": (78, [(20, "cl", 1, 1), (20, "cl", 2, 2), (20, "mk", 31, 31), (20, "cl", 64, 64), (20, "mk", 32, 32), (20, "mk", 63, 63),
                   (20, "cl", 128, 77), (20, "mk", 64, 64)]),
    # R = ceil(S / 256) switching, the last short line / RM 2 -> 8 at 512 | 513, R = 3 | 4
    "wide": (78, [(5, "cl", 256, 77), (5, "mk", 128, 77), (5, "mk", 255, 77), (5, "cl", 512, 77), (5, "mk", 256, 77), (5, "cl", 768, 77),
                  (5, "mk", 384, 77)]),
    # the last register-resident line and the first that walks the label axis in rounds
    "huge-edge": (205, [(3, "mk", 1023, 204), (3, "cl", 2048, 204), (3, "mk", 1024, 204)]),
    # S <= 64, the carve sized by a 63-state companion: both lattices fit LDS | do not (52 | 53 states); the scores behind them fit |
    # do not (40 states of 25 | 26 distinct classes)
    "lds-cap": (40, [(40, "cl", 52, 39), (40, "cl", 53, 39), (40, "cl", 40, 25), (40, "cl", 40, 26), (10, "mk", 31, 31)]),
    # (and a tiled line of 81 states: the two-per-lane recursion from the tiled path's call site)
    "lanemap-edge": (83, [(256, "mk", 12, 12), (257, "mk", 12, 12), (257, "mk", 40, 40)]),
    # T S = 13312 | 13364 on a short line (the second goes tiled for that term alone, and streams phase C)
    "cells-short": (11, [(256, "cl", 52, 10), (257, "cl", 52, 10)]),
    # T S = 13312 | 14144 on a tiled line (832 states: tiled whatever T is); 500 states over 30 frames: RM 2 from the tiled path's call site;
    # 512 | 513 states over 27 frames (13824 cells and more: tiled both): the last line of the generic phase D and of RM 2 from that call
    # site, and the first with one thread per state
    "cells-tiled": (78, [(16, "cl", 832, 77), (17, "cl", 832, 77), (30, "cl", 500, 77), (27, "cl", 512, 77), (27, "mk", 256, 77)]),
    # T nc = 17347 | 17430 around CTC_PREG x 512 = 17408 with odd nc; 17384 | 17466 with even nc (never flat)
    "flat-odd": (83, [(209, "mk", 12, 12), (210, "mk", 12, 12)]),
    "flat-even": (82, [(212, "mk", 12, 12), (213, "mk", 12, 12)]),
    "nc511": (511, [(4, "mk", 3, 3), (9, "cl", 6, 5)]),
    "nc512": (512, [(4, "mk", 3, 3), (9, "cl", 6, 5)]),
    "nc513": (513, [(4, "mk", 3, 3), (9, "cl", 6, 5)]),
    # a carve of 7 frames per tile: T = tile, tile + 1, 2 tile, 2 tile + 1, staged class by class (even nc) and flat (odd nc)
    "tiles-even": (4000, [(7, "mk", 3, 3), (8, "mk", 3, 3), (14, "mk", 3, 3), (15, "mk", 3, 3), (9, "cl", 6, 3)]),
    "tiles-odd": (4001, [(7, "mk", 3, 3), (8, "mk", 3, 3), (14, "mk", 3, 3), (15, "mk", 3, 3), (9, "cl", 6, 3)]),
    # the CTC_PD = 8 register ring of the one-wave recursions: lines around the ring size and twice it, scores from LDS / two per lane
    "ring": (30, [(T, "mk", 10, 10) for T in (7, 8, 9, 15, 16, 17)]),
    "ring-pair": (30, [(T, "cl", 70, 29) for T in (7, 8, 9, 15, 16, 17)]),
    # the capacity terms of the short-line rule deciding alone: T (ncp + nub) against a carve-limited tile (74 | 75 frames of 401
    # classes); T ((S | 1) + nub) beside a line of 2049 states, which collapses the tile to a few frames (23 | 24 frames of 401 states).
    # Those 401 states are a plain class list of 300 distinct classes -- more than the (S + 1) / 2 a blank-interleaved target can have:
    # nub is the line's own count there.  (The rule used to reserve (S + 1) / 2 columns for every target; it then kept this line short
    # up to 27 frames, and the class columns ran over the region into the per-state arrays behind it: the 27-frame line is listed too.)
    "cap-classes": (401, [(74, "mk", 3, 3), (75, "mk", 3, 3)]),
    "cap-states": (301, [(23, "cl", 401, 300), (24, "cl", 401, 300), (2, "cl", 2049, 300), (27, "cl", 401, 300)]),
    # T <= 512 deciding: only beside a companion whose states enlarge the region (alone, a 512-frame line never fits it) -- and only
    # with few classes: the 201-state companion makes the carve, not tmax, the limit of the tile (122 frames at 41 classes), and from 45
    # classes on the 512-frame line no longer fits.  At 83 classes both lines are tiled (tile = 104): listed, and asserted as that
    "mixed512-41": (41, [(512, "mk", 12, 12), (513, "mk", 12, 12), (20, "mk", 100, 40)]),
    "mixed512": (83, [(512, "mk", 12, 12), (513, "mk", 12, 12), (20, "mk", 100, 60)]),
    # the same line alone, beside a long line, beside a many-state line, beside a line of more than 2048 states, beside an empty line
    "x-alone": (83, [X]),
    "x-long": (83, [X, (300, "mk", 2, 2)]),
    "x-201": (83, [X, (20, "mk", 100, 60)]),
    "x-huge": (83, [X, (2, "cl", 2049, 82)]),
    "x-empty": (83, [X, (0, "mk", 2, 2)]),
}
COMPANIONS = ("x-alone", "x-long", "x-201", "x-huge", "x-empty")

# ---- the decisions: (what, field, value at the bound, (case, line), value one past it, (case, line), the quantity that steps by one) ---
EDGES = [
    ("short line: S <= 512", "form", SHORT, ("wide", 3), TILED, ("wide", 4), "S"),
    ("short line: nc <= 512", "form", SHORT, ("nc512", 0), TILED, ("nc513", 0), "nc"),
    ("short line: T <= 512 (mixed minibatch only)", "form", SHORT, ("mixed512-41", 0), TILED, ("mixed512-41", 1), "T"),
    ("short line: T S <= 512 CTC_CCACHE", "form", SHORT, ("cells-short", 0), TILED, ("cells-short", 1), "T"),
    ("short line: T (ncp + nub) <= cap", "form", SHORT, ("cap-classes", 0), TILED, ("cap-classes", 1), "T"),
    ("short line: T ((S | 1) + nub) <= cap", "form", SHORT, ("cap-states", 0), TILED, ("cap-states", 1), "T"),
    ("huge: S > CTC_SMAX_LDS", "form", TILED, ("huge-edge", 1), HUGE, ("huge-edge", 2), "S"),
    ("recursion: one wave, S <= 64", "rec", WAVE, ("waves", 3), PAIR, ("waves", 4), "S"),
    ("recursion: two per lane, S <= 128", "rec", PAIR, ("waves", 6), RM2, ("waves", 7), "S"),
    ("recursion: RM 2, ceil(S / 256) <= 2", "rec", RM2, ("wide", 3), RM8, ("wide", 4), "S"),
    ("recursion: rounds beyond CTC_SMAX_LDS", "rec", RM8, ("huge-edge", 1), ROUNDS, ("huge-edge", 2), "S"),
    ("flat: T nc <= CTC_PREG 512 (odd nc)", "flat", 1, ("flat-odd", 0), 0, ("flat-odd", 1), "T"),
    ("flat: ncp == nc", "flat", 1, ("nc511", 0), 0, ("nc512", 0), "nc"),
    ("lds_lat: S <= 64", "lds_lat", 1, ("waves", 3), 0, ("waves", 4), "S"),
    ("lds_lat: 2 T S <= cap", "lds_lat", 1, ("lds-cap", 0), 0, ("lds-cap", 1), "S"),
    ("lm_lds: scores fit behind the lattices", "lm_lds", 1, ("lds-cap", 2), 0, ("lds-cap", 3), "nu"),
    ("lanemap: S <= 64", "lanemap", 1, ("waves", 3), 0, ("waves", 4), "S"),
    ("lanemap: T <= 256", "lanemap", 1, ("lanemap-edge", 0), 0, ("lanemap-edge", 1), "T"),
    ("tiled: flat staging, ncp == nc", "flat_stage", 0, ("tiles-even", 1), 1, ("tiles-odd", 1), "nc"),
    ("tiled: phase C in registers, T S <= 512 CTC_CCACHE", "c_in_regs", 1, ("cells-tiled", 0), 0, ("cells-tiled", 1), "T"),
    ("tiled: phase D one thread per state, S > 512", "d_per_state", 0, ("cells-tiled", 3), 1, ("cells-tiled", 4), "S"),
    ("tiled: recursion RM 2, ceil(S / 256) <= 2", "rec", RM2, ("cells-tiled", 3), RM8, ("cells-tiled", 4), "S"),
    ("tiled: one tile | two", "ntiles", 1, ("tiles-even", 0), 2, ("tiles-even", 1), "T"),
    ("tiled: two tiles | three", "ntiles", 2, ("tiles-even", 2), 3, ("tiles-even", 3), "T"),
]


def targets(nc, kind, n, m):
    """the target states of a listed line: label i is 1 + (i mod m) * stride, the m labels spread over the classes"""
    assert 1 <= m <= nc - 1
    lab = 1 + (np.arange(n) % m) * max(1, (nc - 1) // m)
    if kind == "cl":
        return lab.astype(np.int32)
    st = np.zeros(2 * n + 1, np.int32)
    st[1::2] = lab
    return st


def most_repeats(st):
    lab = st[st != 0]
    return int(np.bincount(lab).max()) if lab.size else 0


def case_states(name):
    nc, lines = CASES[name]
    return [targets(nc, kind, n, m) for (_, kind, n, m) in lines]


_plans = {}


def plan_of(lib, name):
    """(batch plan, [record per line]) of a listed minibatch, from the library's own rule"""
    if name not in _plans:
        nc, lines = CASES[name]
        sts = case_states(name)
        loff = np.concatenate([[0], np.cumsum([ln[0] for ln in lines])]).astype(np.int32)
        soff = np.concatenate([[0], np.cumsum([len(s) for s in sts])]).astype(np.int32)
        states = np.concatenate(sts).astype(np.int32)
        bp = np.zeros(4, np.int32)
        lp = np.zeros((len(lines), len(FIELDS)), np.int32)
        lib.call("clstm_debug_ctc_plan", nc, ptr(loff), ptr(states), ptr(soff), len(lines), ptr(bp), ptr(lp))
        batch = dict(zip(("tile", "smax", "ncp", "smem"), (int(v) for v in bp)))
        _plans[name] = (batch, [dict(zip(FIELDS, (int(v) for v in row))) for row in lp])
    return _plans[name]


@pytest.fixture(scope="module")
def planlib():
    """the plan entry is host arithmetic: no device is needed to ask it"""
    from common import emu_lib
    return emu_lib()


def fmt(rec):
    return "%s/%s" % (FORM_NAMES[rec["form"]], REC_NAMES[rec["rec"]]) + "".join(
        " %s" % f for f in ("flat", "lds_lat", "lm_lds", "lanemap", "flat_stage", "c_in_regs", "d_per_state") if rec[f]) + (
        " ntiles=%d" % rec["ntiles"] if rec["form"] in (TILED, HUGE) else "")


# ---- a. coverage: no kernel runs --------------------------------------------------------------------------------------------------------
def test_the_sweep_covers_every_decision_on_both_sides(planlib):
    every = [(name, i, rec) for name in CASES for i, rec in enumerate(plan_of(planlib, name)[1])]
    for rec in (r for _, _, r in every):
        assert (rec["form"] == NONE) == (rec["T"] == 0 or rec["S"] == 0)
    # every value of every decision is taken by a listed line
    have = lambda form, field, value: [n for n, _, r in every if r["form"] in form and r[field] == value]
    for value, what in enumerate(FORM_NAMES):
        assert have((SHORT, TILED, HUGE, NONE), "form", value), "no listed line takes the %s form" % what
    for value, what in enumerate(REC_NAMES):
        assert have((SHORT, TILED, HUGE), "rec", value), "no listed line runs the recursion '%s'" % what
    for rec_class in (WAVE, PAIR, RM2):                       # the short-line path and the tiled path share ctc_lattice: both call sites
        for form in (SHORT, TILED):
            assert [1 for _, _, r in every if r["form"] == form and r["rec"] == rec_class], "no listed %s line runs the recursion '%s'" % (
                FORM_NAMES[form], REC_NAMES[rec_class])
    for field in ("flat", "lds_lat", "lm_lds", "lanemap"):
        for value in (0, 1):
            assert have((SHORT,), field, value), "no short line with %s = %d" % (field, value)
    assert [1 for _, _, r in every if r["lds_lat"] and not r["lm_lds"]] and [1 for _, _, r in every if r["S"] <= 64 and r["form"] == SHORT and not r["lds_lat"]]
    for field in ("flat_stage", "c_in_regs", "d_per_state"):
        for value in (0, 1):
            assert have((TILED, HUGE), field, value), "no tiled line with %s = %d" % (field, value)
    assert have((HUGE,), "flat_stage", 1) and [1 for _, _, r in every if r["form"] == HUGE and r["ntiles"] >= 1]
    # every bound: one listed line AT it, one listed line one past it
    for what, field, at, (ca, ia), past, (cb, ib), step in EDGES:
        a, b = plan_of(planlib, ca)[1][ia], plan_of(planlib, cb)[1][ib]
        assert a[field] == at, "%s: the line at the bound (%s[%d], %r) has %s = %d, not %d" % (what, ca, ia, fmt(a), field, a[field], at)
        assert b[field] == past, "%s: the line past the bound (%s[%d], %r) has %s = %d, not %d" % (what, cb, ib, fmt(b), field, b[field], past)
        qa = dict(T=a["T"], S=a["S"], nu=a["nu"], nc=CASES[ca][0])
        qb = dict(T=b["T"], S=b["S"], nu=b["nu"], nc=CASES[cb][0])
        assert qb[step] == qa[step] + 1, (what, step, qa, qb)
        fixed = {"T": ("S", "nc"), "S": ("T", "nc"), "nc": ("T", "S"), "nu": ("T", "S", "nc")}[step]
        assert all(qa[q] == qb[q] for q in fixed), (what, qa, qb)
    # the widths, ring lengths, tile multiples and products the sweep is about, present as such
    s_listed = {r["S"] for _, _, r in every}
    assert {1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 511, 512, 513, 768, 769, 2047, 2048, 2049} <= s_listed
    for name in ("ring", "ring-pair"):
        recs = plan_of(planlib, name)[1]
        assert [r["T"] for r in recs] == [7, 8, 9, 15, 16, 17] and {r["rec"] for r in recs} == {WAVE if name == "ring" else PAIR}
    assert all(r["lm_lds"] for r in plan_of(planlib, "ring")[1])
    for name in ("tiles-even", "tiles-odd"):                   # T = tile, tile + 1, 2 tile, 2 tile + 1 at the carve's own tile
        batch, recs = plan_of(planlib, name)
        tile = batch["tile"]
        assert tile < 16 and [r["T"] for r in recs[:4]] == [tile, tile + 1, 2 * tile, 2 * tile + 1] and [r["ntiles"] for r in recs[:4]] == [1, 2, 2, 3]
    for name, nc in (("flat-odd", 83), ("flat-even", 82)):     # T nc on both sides of the flat bound, whatever the parity of nc decides
        recs = plan_of(planlib, name)[1]
        assert recs[0]["T"] * nc <= 34 * 512 < recs[1]["T"] * nc and all(r["form"] == SHORT for r in recs)
    assert plan_of(planlib, "cells-short")[1][0]["T"] * 52 == 13312 and plan_of(planlib, "cells-tiled")[1][0]["T"] * 832 == 13312
    assert [CASES[n][0] for n in ("nc511", "nc512", "nc513")] == [511, 512, 513]
    # the mixed minibatches of the T <= 512 edge: the 201-state companion is what lets a 512-frame line fit the region at all
    for name, forms in (("mixed512-41", [SHORT, TILED]), ("mixed512", [TILED, TILED])):
        batch, recs = plan_of(planlib, name)
        assert batch["smax"] == 201 and batch["tile"] < 256 and (recs[2]["T"], recs[2]["S"]) == (20, 201)
        assert [(r["T"], r["S"], r["form"]) for r in recs[:2]] == [(512, 25, forms[0]), (513, 25, forms[1])]
    # the tight bar's premise: no listed target repeats a label more than KMAX times
    assert max(most_repeats(st) for name in CASES for st in case_states(name)) <= KMAX


def test_companions_change_the_plan_of_the_same_line(planlib):
    """tile and smax come from the whole minibatch: the same line's record differs between its minibatches"""
    recs = {name: plan_of(planlib, name)[1][0] for name in COMPANIONS}
    batches = {name: plan_of(planlib, name)[0] for name in COMPANIONS}
    assert len({tuple(r.values()) for r in recs.values()}) >= 2, recs
    assert recs["x-alone"]["form"] == SHORT and recs["x-alone"]["lm_lds"] and recs["x-huge"]["form"] == TILED and recs["x-huge"]["ntiles"] > 1
    assert batches["x-201"]["smax"] == 201 and batches["x-huge"]["smax"] == 2048 and batches["x-huge"]["tile"] < 16
    assert batches["x-long"]["tile"] > batches["x-alone"]["tile"] == 200
    assert plan_of(planlib, "x-empty")[1][1]["form"] == NONE and plan_of(planlib, "x-huge")[1][1]["form"] == HUGE


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
REGIMES = ("noise", "peaked0", "peaked10", "peaked50")


def posteriors(nc, line, st, regime):
    """a listed line's posteriors: a function of the line and the regime alone, so the same line has the same inputs in every minibatch"""
    T = line[0]
    rng = np.random.default_rng(zlib.crc32(repr((nc, line, regime)).encode()))
    if regime == "noise":
        p = rng.random((T, nc)).astype(np.float32) ** 4
        p /= p.sum(1, keepdims=True)
        if T:
            p[0, 1] = 0.0                                     # exercises the 1e-5 floor (ctc.cc:68)
        return p.astype(np.float32)
    share = {"peaked0": 0.0, "peaked10": 0.1, "peaked50": 0.5}[regime]
    p = (rng.random((T, nc)) * 5e-6).astype(np.float32)      # below the floor
    for t in range(T):
        c = int(st[min(len(st) - 1, t * len(st) // T)])       # a monotone walk over the line's states
        if rng.random() < share:
            c = int((c + 1 + rng.integers(0, nc - 1)) % nc)  # a wrong class
        other = int((c + 1 + rng.integers(0, nc - 1)) % nc)
        p[t, c] = 0.0
        p[t, other] = 0.0
        p[t, other] = max(0.0, 0.02 - float(p[t].sum()))
        p[t, c] = 0.98
    return p


def lattice_extremes(p, st):
    """(largest |x - y| a log_add of the forward recursion sees, smallest both - max that limexp sees) of a line, restated in float64
    from ctc.cc:24-55, 66-82: what the peaked regimes are for is checked on the inputs, not assumed"""
    out = np.maximum(1e-5, p.astype(np.float64))
    lm = np.log(out / out.sum(1, keepdims=True))[:, st]

    def forward(lm):
        T, S = lm.shape
        v, gap, rows = -5.0 * np.arange(S), 0.0, []
        for i in range(T):
            w = np.concatenate([[-5.0 * i], v[:-1]])
            same, nxt = v + lm[i], w + lm[i]
            gap = max(gap, float(np.abs(same - nxt).max()))
            v = np.where(np.abs(same - nxt) > 10, np.maximum(same, nxt), np.logaddexp(same, nxt))
            rows.append(v)
        return np.array(rows), gap
    al, gap = forward(lm)
    be = forward(lm[::-1, ::-1])[0][::-1, ::-1]
    both = al + be
    return gap, float((both - both.max()).min())


def test_the_peaked_regimes_reach_the_cutoffs():
    """log_add's cut-off at |x - y| > 10 and limexp's clamp at -30: reached by every peaked regime on lines of every recursion class"""
    for name, i in (("ring", 5), ("ring-pair", 5), ("waves", 7), ("cells-tiled", 3)):
        nc, lines = CASES[name]
        st = targets(nc, *lines[i][1:])
        for regime in ("peaked0", "peaked10", "peaked50"):
            gap, low = lattice_extremes(posteriors(nc, lines[i], st, regime), st)
            assert gap > 10 and low < -30, (name, i, regime, gap, low)


_oracle = {}


def oracle_line(ora32, nc, line, regime):
    """(posteriors, states, oracle alignment) of a listed line, computed once"""
    key = (nc, line, regime)
    if key not in _oracle:
        st = targets(nc, *line[1:])
        p = posteriors(nc, line, st, regime)
        want = ora32.ctc_align_classes(p, st) if line[0] else np.zeros((0, nc), np.float32)
        _oracle[key] = (p, st, want)
    return _oracle[key]


def tight_n(st):
    k = most_repeats(st)
    return 17 + (k - 1 if k >= 3 else 0)


def check_minibatch(backend, ora32, name, regime):
    nc, lines = CASES[name]
    data = [oracle_line(ora32, nc, line, regime) for line in lines]
    recs = plan_of(backend.lib, name)[1]                       # (host arithmetic in either library: the same ctc.h)
    al, dz, loff = ctc_via_abi(backend, [d[0] for d in data], [d[1] for d in data])
    failures = []
    for i, (p, st, want) in enumerate(data):
        a, d = al[loff[i]:loff[i + 1]], dz[loff[i]:loff[i + 1]]
        if not len(p):
            print("SWEEP ctc %s %s %s line=%d plan=%r worst=0.000" % (name, regime, backend.kind, i, fmt(recs[i])))
            continue
        n = tight_n(st)
        assert n * EPS <= 1e-5                                 # ten times tighter than rtol 1e-4 where a frame's posteriors are significant
        bar = n * EPS * want.max(1, keepdims=True).astype(np.float64)
        frac = float((np.abs(a.astype(np.float64) - want) / bar).max())
        print("SWEEP ctc %s %s %s line=%d plan=%r worst=%.3f" % (name, regime, backend.kind, i, fmt(recs[i]), frac))
        what = "%s %s line %d (%s)" % (name, regime, i, fmt(recs[i]))
        assert_close(a, want, rtol=1e-4, atol=1e-6, what="project bar, aligned, " + what)
        assert_close(d, want - p, rtol=1e-4, atol=2e-6, what="project bar, delta, " + what)
        assert np.array_equal(d, a - p), "delta is not aligned - p as one float subtraction: " + what
        if frac > 1.0:
            failures.append("tight bar, %s: %.2f x N = %d ulp of the frame's largest posterior" % (what, frac, n))
    assert not failures, "\n".join(failures)


# ---- b. companions, c. parity of every listed minibatch -------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ("noise", "peaked10"))
def test_companions(backend, ora32, regime):
    """the same line -- same posteriors, same targets -- meets the oracle in every minibatch (its path differs between them:
    test_companions_change_the_plan_of_the_same_line)"""
    nc = CASES["x-alone"][0]
    for name in COMPANIONS:
        assert CASES[name][1][0] == X and CASES[name][0] == nc
        check_minibatch(backend, ora32, name, regime)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", [n for n in CASES if n not in COMPANIONS])
def test_parity(backend, ora32, name, regime):
    check_minibatch(backend, ora32, name, regime)


# ---- d. the tables of DESIGN.md ---------------------------------------------------------------------------------------------------------
def table(logs=()):
    from common import emu_lib
    lib = emu_lib()
    worst = {}
    for log in logs:
        for m in re.finditer(r"^\W*SWEEP ctc (\S+) (\S+) (\S+) line=(\d+) plan='([^']*)' worst=([0-9.]+|inf|nan)", open(log).read(), re.M):
            name, _, kind, i, path, frac = m.groups()
            for key in ((kind, path), (kind, name, int(i))):
                worst[key] = max(worst.get(key, 0.0), float(frac))
    w = lambda key: "%.2f" % worst[key] if key in worst else "-"
    rows = ["| decision | at the bound | one past it | worst error / tight bar: emulator | MI355X |", "|---|---|---|---|---|"]
    for what, field, at, (ca, ia), past, (cb, ib), _ in EDGES:
        a, b = plan_of(lib, ca)[1][ia], plan_of(lib, cb)[1][ib]
        side = lambda c, i, r: "%s[%d]: T = %d, S = %d, nc = %d (%s)" % (c, i, r["T"], r["S"], CASES[c][0], fmt(r))
        rows.append("| %s | %s | %s | %s | %s |" % (what, side(ca, ia, a), side(cb, ib, b),
                                                    " / ".join(w(("emu", c, i)) for c, i in ((ca, ia), (cb, ib))),
                                                    " / ".join(w(("hip", c, i)) for c, i in ((ca, ia), (cb, ib)))))
    paths = {}
    for name in CASES:
        for i, rec in enumerate(plan_of(lib, name)[1]):
            paths.setdefault(fmt(rec), []).append("%s[%d]" % (name, i))
    rows += ["", "| path | listed lines | worst error / tight bar: emulator | MI355X |", "|---|---|---|---|"]
    for path in sorted(paths):
        rows.append("| %s | %s | %s | %s |" % (path, ", ".join(paths[path]), w(("emu", path)), w(("hip", path))))
    return "\n".join(rows)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print(table(sys.argv[1:]))
