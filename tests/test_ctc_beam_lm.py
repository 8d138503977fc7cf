"""clstm_ctc_beam_lm_batch / clstm_net_beam_lm (clstm_amd/csrc/ctc_beam.h, second part): CTC prefix beam search with a character
n-gram language model inside the extension step.

The referee is test_ctc_beam.py's beam_ref extended by the model exactly as the header states it, written out here: the acoustic
recursion unchanged, a candidate's key logadd(lb', lnb') + lm(its prefix), lm(l + c) = lm(l) + (weight lm[ctx(l)][c] + bonus) kept
per prefix, EVERY class 1 .. nc-1 a candidate of every entry, the final ranking by (tot + lm(l)) + weight end[ctx(l)].  A float64
form and a float32 form (one rounding per operation; a gauge only).  test_referee_is_exact_without_pruning pins the float64 form to
the sum over every path plus the labelling's LM value where the beam cannot prune.

Bars, the project's (test_ctc_beam.py).  Both scores of a hypothesis -- the total that was ranked and the acoustic tot -- against
the FLOAT64 referee: |s - s64| <= 1e-4 max(1, |s64|); the float32 referee is asserted within half of it.  Labels exact on DECIDED
lines: with D = the largest |s32 - s64| over both scores of a line's reported hypotheses, a line is decided when every pruning
margin of the float64 run and every gap between adjacent totals of the final ranking (down to the first hypothesis NOT reported)
exceeds 8 D; there the scores also lie within max(8 D, 16 f32 ulps).  Any other line: labels in range, lengths <= T, totals
descending, every acoustic score <= the labelling's exact CTC log-likelihood + bar, total - acoustic score = the labelling's LM
value within the bar, top total >= the referee's - bar.  At most a quarter of a case's lines undecided, asserted for every case
from the referee alone (test_the_inputs_are_adequate).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_ctc_beam import (NC, bar, call_beam, enumerate_paths, exact_loglik, exhaustive_case, line_bytes, logadd, lp_ref,
                           peaked_probs, split, sweep_case, tiny_batch, tiny_net)

F32, F64 = np.float32, np.float64
EXHAUSTIVE = [(4, 3), (5, 2), (6, 2)]


# ---- the model and the referee ---------------------------------------------------------------------------------------------
class Lm:
    """a table, an optional end table, weight and bonus; the device copies are made once per backend"""

    def __init__(self, order, nc, table, end=None, weight=1.0, bonus=0.0):
        self.order, self.nc, self.weight, self.bonus = order, nc, float(F32(weight)), float(F32(bonus))
        self.table = np.ascontiguousarray(table, F32).reshape(nc ** (order - 1), nc)
        self.end = None if end is None else np.ascontiguousarray(end, F32).reshape(nc ** (order - 1))
        self.dev = {}

    def but(self, **kw):
        d = dict(order=self.order, nc=self.nc, table=self.table, end=self.end, weight=self.weight, bonus=self.bonus)
        d.update(kw)
        return Lm(**d)

    def ctx(self, l):
        last = l[-1] if l else 0
        return last if self.order == 2 else self.nc * (l[-2] if len(l) >= 2 else 0) + last

    def value(self, l, dt, with_end=True):
        """lm(l) (+ weight end[ctx(l)]) left to right in dt, one rounding per operation"""
        w, b, v = dt(self.weight), dt(self.bonus), dt(0)
        for j, c in enumerate(l):
            v = dt(v + dt(dt(w * dt(self.table[self.ctx(l[:j]), c])) + b))
        if with_end and self.end is not None:
            v = dt(v + dt(w * dt(self.end[self.ctx(l)])))
        return v

    def handle(self, backend):
        from clstm_amd.lm import CharLM
        if backend.kind not in self.dev:
            self.dev[backend.kind] = CharLM(self.order, self.nc, self.table, self.end, lib=backend.lib)
        return self.dev[backend.kind].handle(backend.lib)


class Run:
    """hyps [(labels, total, acoustic tot)] in the final ranking (all live entries), the smallest pruning margin, the re-extension
    trap count, whether the final ranking moved an entry"""


def beam_ref_lm(lp, beam, dt, lm):
    T, nc = lp.shape
    NEG = dt(-np.inf)
    w, bonus, tab = dt(lm.weight), dt(lm.bonus), lm.table.astype(dt)
    ent, order = {(): (dt(0), NEG)}, [()]
    lmv = {(): dt(0)}   # the trie: a prefix's LM value, made once
    ever, margin, trap = {()}, np.inf, 0
    for t in range(T):
        row = lp[t]
        tot = {l: logadd(*ent[l], dt) for l in order}
        cands = []
        for i, l in enumerate(order):
            lb, lnb = ent[l]
            e = l[-1] if l else 0
            lbn, lnbn = dt(tot[l] + row[0]), NEG
            if l:
                lnbn, par = dt(lnb + row[e]), l[:-1]
                if par in ent:
                    pe = par[-1] if par else 0
                    lnbn = logadd(lnbn, dt(row[e] + (ent[par][0] if pe == e else tot[par])), dt)
            cands.append((dt(logadd(lbn, lnbn, dt) + lmv[l]), i, l, lbn, lnbn, lmv[l]))
            v = (row + tot[l]).astype(dt)
            if e:
                v[e] = dt(row[e] + lb)
            v[0] = NEG
            for k in ent:   # l + c is itself an entry
                if len(k) == len(l) + 1 and k[:-1] == l:
                    v[k[-1]] = NEG
            term = ((w * tab[lm.ctx(l)]).astype(dt) + bonus).astype(dt)
            lnew = (lmv[l] + term).astype(dt)
            key = (v + lnew).astype(dt)
            for c in np.argsort(-key, kind="stable")[:beam + 1]:   # (an entry's own best beam + 1 hold every winner and the first loser)
                if key[c] > NEG:
                    cands.append((key[c], beam + i * nc + int(c), l + (int(c),), NEG, v[c], lnew[c]))
        cands = [c for c in cands if c[0] > NEG or c[0] != c[0]]
        cands.sort(key=lambda c: (-c[0], c[1]))
        keep = cands[:beam]
        if len(cands) > beam:
            margin = min(margin, float(keep[-1][0]) - float(cands[beam][0]))
        new = {c[2] for c in keep}
        for c in keep:
            x = c[2]
            if c[1] >= beam and x in ever and any(len(y) > len(x) and y[:len(x)] == x and y in ent for y in new):
                trap += 1
            assert lmv.setdefault(x, c[5]) == c[5], "a prefix has one LM value"
        ent = {c[2]: (c[3], c[4]) for c in keep}
        order = [c[2] for c in keep]
        ever |= new
    fin = []
    for i, l in enumerate(order):
        am = logadd(*ent[l], dt)
        total = dt(am + lmv[l])
        if lm.end is not None:
            total = dt(total + dt(w * dt(lm.end[lm.ctx(l)])))
        fin.append((total, i, l, am))
    fin.sort(key=lambda c: (-c[0], c[1]))
    r = Run()
    r.hyps = [(l, total, am) for total, _, l, am in fin]
    r.margin, r.trap, r.reordered = margin, trap, [c[1] for c in fin] != list(range(len(fin)))
    return r


class Line:
    """one line and its referee figures for one beam width and model (computed once, shared by backends and tests)"""

    def __init__(self, probs, beam, lm, what):
        self.probs, self.beam, self.lm, self.what, self.T = np.ascontiguousarray(probs, F32), beam, lm, what, len(probs)
        if self.T == 0:
            return
        self.lp64 = lp_ref(probs, F64)
        self.r64, self.r32 = beam_ref_lm(self.lp64, beam, F64, lm), beam_ref_lm(lp_ref(probs, F32), beam, F32, lm)

    def gauge(self, nbest):
        """-> (decided, D) from the referee alone"""
        h64, h32 = self.r64.hyps[:nbest], self.r32.hyps[:nbest]
        if [h[0] for h in h64] != [h[0] for h in h32]:
            return False, None
        D = 0.0
        for a, b in zip(h64, h32):
            for k in (1, 2):
                assert abs(float(b[k]) - float(a[k])) <= 0.5 * bar(a[k]), (self.what, "referee", b[k], a[k])
                D = max(D, abs(float(b[k]) - float(a[k])))
        ranked = self.r64.hyps[:nbest + 1]   # (the first hypothesis not reported decides the last one that is)
        gaps = [float(a[1]) - float(b[1]) for a, b in zip(ranked, ranked[1:])]
        return min([self.r64.margin] + gaps) > 8 * D, D

    def check(self, nbest, nc, hyps):
        """hyps: the device's [(labels, score, am_score)] for this line -> decided"""
        if self.T == 0:
            assert hyps == [], self.what
            return True
        h64 = self.r64.hyps[:nbest]
        assert len(hyps) == len(h64), (self.what, "nhyp", len(hyps), len(h64))
        decided, D = self.gauge(nbest)
        sc = [h[1] for h in hyps]
        for lab, s, am in hyps:
            assert len(lab) <= self.T and ((lab >= 1) & (lab < nc)).all(), (self.what, lab)
        assert all(a >= b for a, b in zip(sc, sc[1:])), (self.what, "not descending", sc)
        if decided:
            for k, ((lab, s, am), (l64, s64, am64)) in enumerate(zip(hyps, h64)):
                assert tuple(int(c) for c in lab) == l64, (self.what, k, lab, l64)
                for name, x, x64 in (("total", s, s64), ("acoustic", am, am64)):
                    err = abs(x - float(x64))
                    print("%-34s k=%d %-8s %+.7e f64 %+.7e err %.3g D %.3g" % (self.what, k, name, x, x64, err, D))
                    assert err <= bar(x64), (self.what, k, name, x, x64)
                    assert err <= max(8 * D, 16 * float(np.spacing(F32(abs(float(x64)))))), (self.what, k, name, x, x64, D)
        else:
            for lab, s, am in hyps:
                l = tuple(int(c) for c in lab)
                ex = exact_loglik(self.lp64, l)
                assert am <= ex + bar(ex), (self.what, "above the labelling's likelihood", lab, am, ex)
                v = float(self.lm.value(l, F64))
                assert abs((s - am) - v) <= bar(s) + bar(am) + bar(v), (self.what, "total - acoustic is not the LM value", lab, s, am, v)
            assert sc[0] >= float(h64[0][1]) - bar(h64[0][1]), (self.what, "top total", sc[0], h64[0][1])
        return decided


def adequate(lines, nbest):
    und = [ln.what for ln in lines if ln.T and not ln.gauge(nbest)[0]]
    n = sum(1 for ln in lines if ln.T)
    assert 4 * len(und) <= n, ("the case proves too little: undecided by the referee alone", und)


def call_beam_lm(backend, lines, nc, beam, nbest, lm, want_am=True, handle=None, weight=None, bonus=None):
    """lines: list of [T_b, nc] arrays -> per line [(labels, score, am_score)], and the raw arrays"""
    from clstm_amd.abi import i32, ptr
    from clstm_amd.net import unpack_beam
    T = [len(p) for p in lines]
    N = int(sum(T))
    flat = np.concatenate([np.asarray(p, F32).reshape(-1, nc) for p in lines], 0) if N else np.zeros((1, nc), F32)
    pd = backend.up(flat)
    lo = i32(np.concatenate([[0], np.cumsum(T)]))
    nhyp = np.full(len(T), -3, np.int32)
    ln = np.full(max(1, len(T) * nbest), -3, np.int32)
    sc = np.full(max(1, len(T) * nbest), 123.0, F32)
    am = np.full(max(1, len(T) * nbest), 123.0, F32)
    lab = np.full(max(1, nbest * N), -3, np.int32)
    backend.lib.call("clstm_ctc_beam_lm_batch", ptr(pd), nc, ptr(lo), len(T), beam, nbest,
                     lm.handle(backend) if handle is None else handle, lm.weight if weight is None else weight,
                     lm.bonus if bonus is None else bonus, ptr(nhyp), ptr(ln), ptr(sc), ptr(am) if want_am else None, ptr(lab))
    return unpack_beam(T, nbest, nhyp, ln, sc, lab, am), (nhyp, ln, sc, lab, am)


def lm_line_bytes(T, nbest, raw, b):
    nhyp, ln, sc, lab, am = raw
    return line_bytes(T, nbest, (nhyp, ln, sc, lab), b) + am[b * nbest:(b + 1) * nbest].tobytes()


def random_lm(seed, order, nc, end=True, weight=0.7, bonus=0.3, scale=1.0):
    """column 0 holds 1e30: a search that read it would show"""
    rng = np.random.default_rng(seed)
    table = rng.normal(-1.0, scale, (nc ** (order - 1), nc)).astype(F32)
    table[:, 0] = 1e30
    return Lm(order, nc, table, rng.normal(-1.0, scale, nc ** (order - 1)).astype(F32) if end else None, weight, bonus)


# ---- 1. the referee, pinned by exhaustive enumeration ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pinned_lm(nc, order):
    return random_lm(100 + 10 * nc + order, order, nc)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("T,nc", EXHAUSTIVE)
def test_referee_is_exact_without_pruning(T, nc, order):
    lm = pinned_lm(nc, order)
    for seed in range(20):
        p, exact = exhaustive_case(T, nc, seed)
        r = beam_ref_lm(lp_ref(p, F64), 32, F64, lm)
        assert r.margin == np.inf, "a 32-wide beam must not prune here"
        assert {h[0] for h in r.hyps} == set(exact)
        for l, s, am in r.hyps:
            want = exact[l] + float(lm.value(l, F64))
            assert abs(float(am) - exact[l]) <= 1e-13 * max(1.0, abs(exact[l])), (l, am, exact[l])
            assert abs(float(s) - want) <= 1e-13 * max(1.0, abs(want)), (l, s, want)
        assert [h[1] for h in r.hyps] == sorted((h[1] for h in r.hyps), reverse=True)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("T,nc", EXHAUSTIVE)
def test_every_labelling_where_nothing_is_pruned(backend, T, nc, order):
    lm = pinned_lm(nc, order)
    cases = [exhaustive_case(T, nc, seed) for seed in range(8)]
    got, _ = call_beam_lm(backend, [p for p, _ in cases], nc, 32, 32, lm)
    for (p, exact), hyps in zip(cases, got):
        assert {tuple(int(c) for c in h[0]) for h in hyps} == set(exact) and len(hyps) == len(exact)
        sc = [h[1] for h in hyps]
        assert all(a >= b for a, b in zip(sc, sc[1:]))
        for lab, s, am in hyps:
            l = tuple(int(c) for c in lab)
            want = exact[l] + float(lm.value(l, F64))
            assert abs(am - exact[l]) <= bar(exact[l]), (lab, am, exact[l])
            assert abs(s - want) <= bar(want), (lab, s, want)


# ---- 2. zero weight is the search without a model --------------------------------------------------------------------------
ZERO = [(1, 2, 1, 1, 0.9), (7, 5, 4, 2, 0.9), (64, 12, 32, 20, 0.8)]   # test_shape_sweep's small cases


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("T,nc,beam,L,peak", ZERO)
def test_zero_weight_is_the_old_search(backend, T, nc, beam, L, peak, order):
    lines = [ln.probs for ln in sweep_case(T, nc, beam, L, peak)]
    lm = random_lm(7, order, nc, end=False, weight=0.0, bonus=0.0)
    for nbest in sorted({beam, max(1, beam // 2)}):
        _, (nhyp, ln, sc, lab) = call_beam(backend, lines, nc, beam, nbest)
        _, (nhyp2, ln2, sc2, lab2, am2) = call_beam_lm(backend, lines, nc, beam, nbest, lm)
        assert nhyp2.tobytes() == nhyp.tobytes() and ln2.tobytes() == ln.tobytes() and lab2.tobytes() == lab.tobytes()
        assert (sc2 == sc).all() and (am2 == sc).all()
        assert nhyp.max() >= 1


# ---- 3. the class list is lossless -----------------------------------------------------------------------------------------
def background(T, nc):
    """small posteriors, no two alike: no exact ties among the candidates nobody cares about"""
    return (0.02 + 0.001 * np.arange(nc)[None, :] + 0.0003 * np.arange(T)[:, None]).astype(F32)


def lifted_line():
    """beam 1, nc 6, T 5.  Frame 2: labels 2 (0.4) and 3 (0.3) lead, label 4 (0.15) is third -- outside the 2 beam = 2 classes
    an acoustic list keeps"""
    p = background(5, 6)
    p[0, 1], p[1, 0], p[3, 0], p[4, 0] = 0.9, 0.9, 0.9, 0.9
    p[2] = [0.05, 0.05, 0.40, 0.30, 0.15, 0.05]
    return p


@functools.lru_cache(maxsize=None)
def lifted_cases():
    wide = np.full((6, 6), -5.0, F32)
    wide[0, 1:] = 0.0      # the first label is free
    wide[1, 4] = 0.0       # 1 4 is cheap, 1 anything else dear
    wide[:, 0] = 1e30
    tiny = (np.random.default_rng(3).normal(0, 1e-4, (6, 6))).astype(F32)   # L = weight (max - min) ~ 1e-3: a bound-based list cuts
    return (Line(lifted_line(), 1, Lm(2, 6, wide, None, 4.0, 0.0), "lifted, wide table"),
            Line(lifted_line(), 1, Lm(2, 6, tiny, None, 4.0, 0.0), "lifted, tiny table"))


def test_the_class_list_is_lossless(backend):
    wide, tiny = lifted_cases()
    lp = lp_ref(wide.probs, F64)[2]
    assert sorted(range(1, 6), key=lambda c: -lp[c]).index(4) == 2, "label 4 must be third by posterior on frame 2"
    assert wide.r64.hyps[0][0] == (1, 4) and tiny.r64.hyps[0][0] == (1, 2)
    for ln in (wide, tiny):
        assert ln.gauge(1)[0], ln.what
        got, _ = call_beam_lm(backend, [ln.probs], 6, 1, 1, ln.lm)
        assert ln.check(1, 6, got[0])
        assert tuple(got[0][0][0].tolist()) == ln.r64.hyps[0][0]
    got, _ = call_beam_lm(backend, [wide.probs], 6, 1, 1, wide.lm)
    assert 4 in got[0][0][0].tolist()


# ---- 4. the model decides --------------------------------------------------------------------------------------------------
def even_line():
    """T 6, nc 4: frames 2 and 3 near 0.5 / 0.5 between labels 1 and 2, label 1 a little ahead"""
    p = background(6, 4)
    p[0, 1], p[1, 0], p[4, 0], p[5, 0] = 0.94, 0.94, 0.94, 0.94
    p[2] = [0.03, 0.48, 0.46, 0.03]
    p[3] = [0.03, 0.49, 0.45, 0.03]   # (not the same twice: 1 1 2 and 1 2 1 would tie)
    return p


@functools.lru_cache(maxsize=None)
def decide_cases():
    t = np.full((4, 4), -1.0, F32)
    t[1, 2], t[1, 1] = 0.0, -3.0   # 1 2 cheap, 1 1 dear
    lm = Lm(2, 4, t, None, 1.0, 0.0)
    flat = Lm(2, 4, np.zeros((4, 4), F32), None, 0.0, 0.0)
    # a constructed line for the bonus: label 1 clear, label 2 likelier than not (0.61), label 3 less likely than not (0.41):
    # 1 2 wins by posterior, a bonus of 2 buys 3 as well, a bonus of -2 sells 2
    q = background(6, 4)
    q[0, 1] = 0.94
    q[1] = [0.35, 0.02, 0.61, 0.02]
    q[2] = [0.90, 0.04, 0.03, 0.03]
    q[3] = [0.55, 0.02, 0.02, 0.41]
    q[4] = [0.90, 0.04, 0.03, 0.03]
    q[5] = [0.90, 0.04, 0.03, 0.03]
    return (Line(even_line(), 4, flat, "even, no model"), Line(even_line(), 4, lm, "even, bigram"),
            [Line(q, 4, flat.but(weight=1.0, bonus=b), "bonus %+g" % b) for b in (-2.0, 0.0, 2.0)])


def test_the_model_decides(backend):
    plain, with_lm, bonus = decide_cases()
    assert plain.r64.hyps[0][0] == (1, 1) and with_lm.r64.hyps[0][0] == (1, 2)
    for ln in (plain, with_lm):
        got, _ = call_beam_lm(backend, [ln.probs], 4, 4, 4, ln.lm)
        assert ln.check(4, 4, got[0]), ln.what
        assert tuple(got[0][0][0].tolist()) == ln.r64.hyps[0][0]
    old, _ = call_beam(backend, [plain.probs], 4, 4, 4)
    assert tuple(old[0][0][0].tolist()) == (1, 1)
    lens = []
    for ln in bonus:
        got, _ = call_beam_lm(backend, [ln.probs], 4, 4, 4, ln.lm)
        assert ln.check(4, 4, got[0]), ln.what
        lens.append(len(got[0][0][0]))
    assert lens[0] < lens[1] < lens[2], lens


# ---- 5. order 3 contexts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def before_last_lm(nc, seed=5):
    """a table that depends on the label BEFORE last (and the class) only: an order 2 context would not see it"""
    g = np.random.default_rng(seed).normal(-1.0, 1.0, (nc, nc)).astype(F32)
    table = np.repeat(g, nc, axis=0)   # row nc a + b = g[a]
    table[:, 0] = 1e30
    return Lm(3, nc, table, None, 0.8, 0.1)


@functools.lru_cache(maxsize=None)
def order3_lines():
    """the trap of test_ctc_beam.py's trap_lines under the model (4 decided lines in which a prefix that had left the beam is
    extended into it again), and a line that repeats a label through a blank"""
    lm = before_last_lm(3)
    out = []
    for seed in range(600):
        p = np.random.default_rng(9000 + seed).dirichlet(np.full(3, 0.5), 10).astype(F32)
        if beam_ref_lm(lp_ref(p, F64), 3, F64, lm).trap:
            ln = Line(p, 3, lm, "trap seed %d" % seed)
            if ln.gauge(3)[0]:
                out.append(ln)
        if len(out) == 4:
            break
    rep = peaked_probs(np.random.default_rng(1), 12, [1, 1, 2, 2, 1], 3, 0.9)
    out.append(Line(rep, 3, lm, "a a through a blank"))
    return out


def test_order3_contexts_and_the_reextended_prefix(backend):
    lines = order3_lines()
    lm = lines[0].lm
    assert len(lines) == 5 and all(ln.r64.trap > 0 for ln in lines[:4]), "the trap does not occur"
    assert lines[4].r64.hyps[0][0] == (1, 1, 2, 2, 1)
    got, _ = call_beam_lm(backend, [ln.probs for ln in lines], 3, 3, 3, lm)
    seen = set()
    for ln, hyps in zip(lines, got):
        assert ln.check(3, 3, hyps), ln.what
        for lab, s, am in hyps:   # the start contexts (0, 0) and (0, a), and every later one, by the labelling's value
            l = tuple(int(c) for c in lab)
            v = float(lm.value(l, F64))
            assert abs((s - am) - v) <= bar(s) + bar(am), (ln.what, l, s, am, v)
            seen |= {(l[j - 2] if j >= 2 else 0, l[j - 1] if j >= 1 else 0) for j in range(len(l))}
    assert (0, 0) in seen and {(0, 1), (0, 2)} & seen and {(1, 1), (2, 2)} & seen


# ---- 6. the end table ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def end_lines():
    """random small lines whose final ranking the end table changes, decided"""
    rng = np.random.default_rng(21)
    lm = Lm(2, 3, np.zeros((3, 3), F32), np.asarray([0.0, -4.0, 3.0], F32), 1.0, 0.0)
    out = []
    for seed in range(200):
        p = np.random.default_rng(3000 + seed).dirichlet(np.full(3, 0.5), 4).astype(F32)
        ln = Line(p, 4, lm, "end seed %d" % seed)
        if ln.r64.reordered and ln.gauge(3)[0] and ln.r64.hyps[0][0] != Line(p, 4, lm.but(end=None), "").r64.hyps[0][0]:
            out.append(ln)
        if len(out) == 4:
            break
    return out


def test_the_end_table_reorders_the_last_beam(backend):
    lines = end_lines()
    assert len(lines) == 4
    got, _ = call_beam_lm(backend, [ln.probs for ln in lines], 3, 4, 3, lines[0].lm)
    for ln, hyps in zip(lines, got):
        assert ln.check(3, 3, hyps), ln.what
    bare, _ = call_beam_lm(backend, [ln.probs for ln in lines], 3, 4, 3, lines[0].lm.but(end=None))
    assert all(tuple(a[0][0].tolist()) != tuple(b[0][0].tolist()) for a, b in zip(got, bare))


# ---- 7. shapes -------------------------------------------------------------------------------------------------------------
#        T, nc, beam, order, labels, lines
SHAPES = [(200, 83, 8, 3, 40, 4), (40, 600, 4, 2, 8, 3), (1, 5, 4, 2, 1, 3)]


@functools.lru_cache(maxsize=None)
def shape_case(T, nc, beam, order, L, nlines):
    """ragged lines (the first of T frames), an empty line among them"""
    rng = np.random.default_rng(1000 * T + nc)
    lm = random_lm(T + nc, order, nc, weight=0.5, bonus=0.2)
    lines = []
    for b in range(nlines):
        Tb = max(1, T - (b * T) // 8)
        Lb = max(1, min(L, (L * Tb) // T)) if Tb >= 3 else 0
        lines.append(Line(peaked_probs(rng, Tb, rng.integers(1, nc, Lb), nc, 0.9), beam, lm, "T=%d nc=%d beam=%d line %d" % (Tb, nc, beam, b)))
    lines.insert(1, Line(np.zeros((0, nc), F32), beam, lm, "empty line"))
    return lines


@pytest.mark.parametrize("T,nc,beam,order,L,nlines", SHAPES)
def test_shapes(backend, T, nc, beam, order, L, nlines):
    lines = shape_case(T, nc, beam, order, L, nlines)
    nbest = max(1, beam // 2)
    adequate(lines, nbest)
    got, (nhyp, lens, sc, _, am) = call_beam_lm(backend, [ln.probs for ln in lines], nc, beam, nbest, lines[0].lm)
    for b, (ln, hyps) in enumerate(zip(lines, got)):
        ln.check(nbest, nc, hyps)
        for k in range(len(hyps), nbest):   # unused slots
            assert lens[b * nbest + k] == 0 and sc[b * nbest + k] == -np.inf and am[b * nbest + k] == -np.inf
    if T == 1:   # fewer entries alive than asked for
        assert all(len(h) == min(nbest, nc) for h, ln in zip(got, lines) if ln.T)


@functools.lru_cache(maxsize=None)
def long_case():
    nc, beam = 12, 8
    rng = np.random.default_rng(21)   # (a seed whose long line the referee decides)
    Ts = [30, 700, 9]
    lm = random_lm(12, 2, nc, weight=0.5, bonus=0.2)
    lines = [peaked_probs(rng, T, rng.integers(1, nc, max(1, T // 5)), nc, 0.9) for T in Ts]
    return Ts, lines, lm, Line(lines[1], beam, lm, "T=700 (workspace)")


def test_a_line_too_long_for_lds_beside_short_ones(backend):
    nc, beam, nbest = 12, 8, 4
    Ts, lines, lm, long_line = long_case()
    assert long_line.gauge(nbest)[0], "the long line proves too little: undecided by the referee alone"
    got, mixed = call_beam_lm(backend, lines, nc, beam, nbest, lm)
    _, short = call_beam_lm(backend, [lines[0], lines[2]], nc, beam, nbest, lm)
    _, alone = call_beam_lm(backend, [lines[1]], nc, beam, nbest, lm)
    assert lm_line_bytes(Ts, nbest, mixed, 0) == lm_line_bytes([30, 9], nbest, short, 0)
    assert lm_line_bytes(Ts, nbest, mixed, 2) == lm_line_bytes([30, 9], nbest, short, 1)
    assert lm_line_bytes(Ts, nbest, mixed, 1) == lm_line_bytes([700], nbest, alone, 0)
    assert long_line.check(nbest, nc, got[1])


def test_a_line_depends_on_nothing_but_itself(backend):
    nc, beam, nbest = 12, 8, 5
    rng = np.random.default_rng(13)
    Ts = [30, 1, 17, 64, 9]
    lm = random_lm(13, 3, nc, weight=0.5, bonus=0.0)
    # flat-ish posteriors on a coarse grid: plenty of near and exact ties
    lines = [(np.round(rng.dirichlet(np.ones(nc), T) * 16 + 1) / (16 + nc)).astype(F32) for T in Ts]
    _, base = call_beam_lm(backend, lines, nc, beam, nbest, lm)
    ref = [lm_line_bytes(Ts, nbest, base, b) for b in range(len(Ts))]
    _, again = call_beam_lm(backend, lines, nc, beam, nbest, lm)
    assert [lm_line_bytes(Ts, nbest, again, b) for b in range(len(Ts))] == ref, "the same call twice"
    for b in range(len(Ts)):
        _, alone = call_beam_lm(backend, [lines[b]], nc, beam, nbest, lm)
        assert lm_line_bytes([Ts[b]], nbest, alone, 0) == ref[b], ("line alone", b)
    perm = [3, 0, 4, 2, 1]
    _, other = call_beam_lm(backend, [lines[b] for b in perm], nc, beam, nbest, lm)
    for i, b in enumerate(perm):
        assert lm_line_bytes([Ts[q] for q in perm], nbest, other, i) == ref[b], ("another order", b)
    _, bare = call_beam_lm(backend, lines, nc, beam, nbest, lm, want_am=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(bare[:4], base[:4])) and (bare[4] == 123.0).all()


def test_the_inputs_are_adequate():
    """every case's lines are decided by the referee alone, up to a quarter (no library here)"""
    for ln in lifted_cases():
        assert ln.gauge(1)[0], ln.what
    plain, with_lm, bonus = decide_cases()
    adequate([plain, with_lm] + bonus, 4)
    assert plain.r64.hyps[0][0] != with_lm.r64.hyps[0][0]
    assert len(bonus[0].r64.hyps[0][0]) < len(bonus[1].r64.hyps[0][0]) < len(bonus[2].r64.hyps[0][0])
    adequate(order3_lines(), 3)
    adequate(end_lines(), 3)
    for shape in SHAPES:
        adequate(shape_case(*shape), max(1, shape[2] // 2))
    assert long_case()[3].gauge(4)[0]


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def count(backend, which=30):
    n = C.c_longlong()
    backend.lib.call("clstm_debug_path_count", which, C.byref(n))
    return n.value


def test_refusals_are_named_and_touch_nothing(backend):
    from clstm_amd.abi import ClstmError, ptr
    from clstm_amd.lm import CharLM
    lines = [ln.probs for ln in sweep_case(7, 5, 4, 2, 0.9)]
    lm = random_lm(1, 2, 5)
    n0 = count(backend)
    _, good = call_beam_lm(backend, lines, 5, 4, 3, lm)
    assert count(backend) == n0 + 1 and count(backend, 29) >= 0
    other = random_lm(2, 2, 6)
    for kw, text in ((dict(handle=other.handle(backend)), "another class count"), (dict(weight=-0.5), "weight"),
                     (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"),
                     (dict(bonus=float("nan")), "bonus"), (dict(bonus=float("-inf")), "bonus"), (dict(handle=0), "language model")):
        with pytest.raises(ClstmError, match=text):
            call_beam_lm(backend, lines, 5, 4, 3, lm, **kw)
    for beam, nbest in ((0, 1), (33, 1), (4, 5), (4, 0)):
        with pytest.raises(ClstmError, match="must lie in"):
            call_beam_lm(backend, lines, 5, beam, nbest, lm)
    assert count(backend) == n0 + 1
    # outputs of a refused call keep the caller's bytes
    from clstm_amd.abi import i32
    pd, lo = backend.up(np.concatenate([p for p in lines if len(p)], 0)), i32(np.concatenate([[0], np.cumsum([len(p) for p in lines])]))
    nhyp, sc, am = np.full(len(lines), -3, np.int32), np.full(len(lines) * 3, 123.0, F32), np.full(len(lines) * 3, 123.0, F32)
    with pytest.raises(ClstmError, match="weight"):
        backend.lib.call("clstm_ctc_beam_lm_batch", ptr(pd), 5, ptr(lo), len(lines), 4, 3, lm.handle(backend), -1.0, 0.0,
                         ptr(nhyp), None, ptr(sc), ptr(am), None)
    assert (nhyp == -3).all() and (sc == 123.0).all() and (am == 123.0).all()
    # creation
    tab = np.zeros((5, 5), F32)
    h = C.c_void_p()
    for order in (1, 4, 0):
        with pytest.raises(ClstmError, match="order must be 2 or 3"):
            backend.lib.call("clstm_charlm_create", C.byref(h), order, 5, ptr(tab), None)
    with pytest.raises(ClstmError, match="2\\^26"):
        backend.lib.call("clstm_charlm_create", C.byref(h), 3, 407, ptr(tab), None)   # (refused before the table is read)
    for bad in (np.nan, np.inf, -np.inf):
        t = tab.copy()
        t[3, 2] = bad
        with pytest.raises(ClstmError, match="not finite"):
            backend.lib.call("clstm_charlm_create", C.byref(h), 2, 5, ptr(t), None)
        e = np.zeros(5, F32)
        e[4] = bad
        with pytest.raises(ClstmError, match="end table entry is not finite"):
            backend.lib.call("clstm_charlm_create", C.byref(h), 2, 5, ptr(tab), ptr(e))
        with pytest.raises(ValueError):
            CharLM(2, 5, t)
    assert h.value is None
    _, again = call_beam_lm(backend, lines, 5, 4, 3, lm)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again))


def test_the_largest_key_set_admitted_runs_and_one_more_is_refused(backend):
    from clstm_amd.abi import ClstmError
    rng = np.random.default_rng(5)
    for nc, ok in ((513, True), (514, False)):   # beam 8: 8 * 512 = 4096 extension keys
        lm = Lm(2, nc, rng.normal(-1, 1, (nc, nc)).astype(F32), None, 0.5, 0.0)
        labels = rng.integers(1, nc, 2)
        ln = Line(peaked_probs(rng, 6, labels, nc, 0.9), 8, lm, "nc=%d beam=8" % nc)
        if ok:
            assert ln.gauge(2)[0]
            got, _ = call_beam_lm(backend, [ln.probs], nc, 8, 2, lm)
            assert ln.check(2, nc, got[0])
        else:
            n0 = count(backend)
            with pytest.raises(ClstmError, match="exceeds 4096"):
                call_beam_lm(backend, [ln.probs], nc, 8, 2, lm)
            assert count(backend) == n0
            call_beam(backend, [ln.probs], nc, 8, 2)   # (the search without a model has no such limit)


# ---- 9. net level ----------------------------------------------------------------------------------------------------------
def net_lm(backend, order=3):
    from clstm_amd.lm import CharLM
    rng = np.random.default_rng(77)
    table = rng.normal(-1, 1, (NC ** (order - 1), NC)).astype(F32)
    return CharLM(order, NC, table, rng.normal(-1, 1, NC ** (order - 1)).astype(F32), lib=backend.lib)


def as_test_lm(clm, weight, bonus):
    lm = Lm(clm.order, clm.nc, clm.table, clm.end, weight, bonus)
    return lm


def same_hyps(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(
        p[0].tobytes() == q[0].tobytes() and F32(p[1]).tobytes() == F32(q[1]).tobytes() and F32(p[2]).tobytes() == F32(q[2]).tobytes()
        for p, q in zip(x, y)) for x, y in zip(a, b))


def standalone(backend, net, clm, weight, bonus, beam, nbest):
    return call_beam_lm(backend, split(net.outputs(), net.T), NC, beam, nbest, as_test_lm(clm, weight, bonus),
                        handle=clm.handle(backend.lib))[0]


def test_net_beam_lm_equals_standalone_and_counts(backend):
    net, clm = tiny_net(backend), net_lm(backend)
    lines, _ = tiny_batch(31)
    net.set_inputs(lines)
    net.forward()
    n0, p0 = count(backend), count(backend, 29)
    got = net.beam_lm(clm, 0.6, 0.2, beam=4, nbest=3)
    assert count(backend) == n0 + 1 and count(backend, 29) == p0
    assert same_hyps(got, standalone(backend, net, clm, 0.6, 0.2, 4, 3))
    assert all(len(h) == 3 and np.isfinite(h[0][1]) and np.isfinite(h[0][2]) for h in got)
    assert same_hyps(net.beam_lm(clm, 0.6, beam=4), standalone(backend, net, clm, 0.6, 0.0, 4, 4))   # nbest defaults to beam
    for hyps in got:
        for lab, s, am in hyps:
            v = clm.value(lab.tolist(), float(F32(0.6)), float(F32(0.2)))
            assert abs((s - am) - v) <= bar(s) + bar(am)


def test_beam_lm_after_predict_while_ctc_refuses(backend):
    from clstm_amd.abi import ClstmError
    net, clm = tiny_net(backend), net_lm(backend, 2)
    lines, trs = tiny_batch(41)
    net.predict(lines)
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)
    got = net.beam_lm(clm, 0.5, beam=4, nbest=2)
    assert same_hyps(got, standalone(backend, net, clm, 0.5, 0.0, 4, 2))
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)


def test_beam_lm_leaves_the_training_state_alone(backend):
    from test_ctc_score import read_dz
    lines, trs = tiny_batch(43)
    got = []
    for with_beam in (False, True):
        net, clm = tiny_net(backend), net_lm(backend)
        net.enable_input_deltas(True)
        net.set_inputs(lines)
        net.forward()
        if with_beam:
            net.beam_lm(clm, 0.5, 0.1, beam=8, nbest=3)
        al = net.ctc(trs, want_aligned=True)
        dz = read_dz(backend, net)
        net.backward()
        g, dx = net.get_grads(), net.input_deltas()
        net.update()
        if with_beam:
            net.beam_lm(clm, 0.5, beam=2)
        backend.sync()
        got.append((al, dz, g, dx, net.get_params(), net.get_derivs()))
    for name, a, b in zip(("aligned", "Dz", "grads", "input deltas", "params", "derivs"), *got):
        assert a.tobytes() == b.tobytes(), name
    assert np.abs(got[0][1]).max() > 0


def test_beam_lm_between_training_steps_and_without_a_current_minibatch(backend):
    from clstm_amd.abi import ClstmError
    from clstm_amd.net import Network
    from common import synth_lines
    from test_ctc_beam import NI
    rng = np.random.default_rng(47)
    batches = []
    for k in range(3):
        T = [int(t) for t in rng.integers(3, 12, 3)]
        trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
        x = backend.up(np.ascontiguousarray(np.concatenate(synth_lines(rng, T, NI), 0), F32))
        batches.append((Network.prepare_step(T, trs), x, trs))
    res = []
    for disturbed in (False, True):
        net, clm = tiny_net(backend), net_lm(backend)
        net.train_step_prepared(batches[0][0], batches[0][1], batches[1][0], batches[1][1])
        if disturbed:
            p = net.get_params()
            with pytest.raises(ClstmError, match="no current minibatch"):
                net.beam_lm(clm, 0.5, beam=4)
            assert net.get_params().tobytes() == p.tobytes()
        net.train_step_prepared(batches[1][0], batches[1][1])
        if disturbed:
            assert all(len(h) >= 1 for h in net.beam_lm(clm, 0.5, beam=4, nbest=2))
        net.train_step_prepared(batches[2][0], batches[2][1])
        if disturbed:
            net.beam_lm(clm, 0.5, beam=8)
        backend.sync()
        res.append((net.get_params(), net.get_derivs()))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()


def test_net_bad_arguments_leave_the_net_alone(backend):
    from clstm_amd.abi import ClstmError, ptr
    net, clm = tiny_net(backend), net_lm(backend)
    lines, trs = tiny_batch(53)
    net.set_inputs(lines)
    net.forward()
    z = net.outputs()
    h = clm.handle(backend.lib)
    nhyp, sc = np.zeros(3, np.int32), np.zeros(3 * 32, F32)
    for beam, nbest in ((0, 1), (33, 1), (4, 5)):
        with pytest.raises(ClstmError, match="nbest <= beam"):
            backend.lib.call("clstm_net_beam_lm", net.h, beam, nbest, h, 0.5, 0.0, ptr(nhyp), None, ptr(sc), None, None)
    with pytest.raises(ClstmError, match="required"):
        backend.lib.call("clstm_net_beam_lm", net.h, 4, 2, h, 0.5, 0.0, ptr(nhyp), None, None, None, None)
    with pytest.raises(ClstmError, match="language model"):
        backend.lib.call("clstm_net_beam_lm", net.h, 4, 2, None, 0.5, 0.0, ptr(nhyp), None, ptr(sc), None, None)
    with pytest.raises(ClstmError, match="weight"):
        backend.lib.call("clstm_net_beam_lm", net.h, 4, 2, h, -1.0, 0.0, ptr(nhyp), None, ptr(sc), None, None)
    with pytest.raises(ClstmError, match="bonus"):
        backend.lib.call("clstm_net_beam_lm", net.h, 4, 2, h, 1.0, float("nan"), ptr(nhyp), None, ptr(sc), None, None)
    wrong = random_lm(3, 2, NC + 1)
    with pytest.raises(ClstmError, match="another class count"):
        backend.lib.call("clstm_net_beam_lm", net.h, 4, 2, wrong.handle(backend), 0.5, 0.0, ptr(nhyp), None, ptr(sc), None, None)
    fresh = tiny_net(backend)
    with pytest.raises(ClstmError, match="set_batch first"):
        backend.lib.call("clstm_net_beam_lm", fresh.h, 4, 2, h, 0.5, 0.0, ptr(nhyp), None, ptr(sc), None, None)
    assert net.outputs().tobytes() == z.tobytes() and (nhyp == 0).all() and (sc == 0).all()
    net.ctc(trs)
    net.backward()
    backend.sync()
