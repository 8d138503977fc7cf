"""clstm_ctc_beam_lex_batch / clstm_net_beam_lex / clstm_lexicon_* (clstm_amd/csrc/ctc_beam.h, third part): CTC prefix beam search
constrained to a lexicon.

The referee is test_ctc_beam_lm.py's beam_ref_lm with the two changes the header states, written out here: a prefix's disallowed
extensions are set to -inf BEFORE the per-entry top-(beam + 1) cut, and the final list is filtered to the prefixes whose last run of
word classes is empty or a word.  The lexicon of the referee is a Python set of words (Lex below): the state of a prefix is its last
run, an extension by a word class is allowed when the longer run is a prefix of a word, by a separator when the run is empty or a
word.  Float64 and float32 forms.  test_referee_is_exact_without_pruning pins the float64 form to the sum over every path of every
ADMISSIBLE labelling plus its LM value where the beam cannot prune.

Bars: the project's, unchanged (test_ctc_beam_lm.py: Line.gauge / Line.check are used as they stand).  Both scores against float64
within 1e-4 max(1, |s64|); labels exact on decided lines (every pruning margin and every gap of the final ranking > 8 D), there
the scores also within max(8 D, 16 ulp); on the other lines validity, the likelihood bound, total - acoustic = the LM value -- and
on EVERY line admissibility of every reported labelling.  Adequacy (test_the_inputs_are_adequate, from the referee alone): at most a
quarter of a case's lines undecided, at least half of a case's lines report a hypothesis.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_ctc_beam as tb
import test_ctc_beam_lm as tl
from test_ctc_beam import (NC, bar, call_beam, exhaustive_case, line_bytes, logadd, lp_ref, peaked_probs, split, sweep_case,
                           tiny_batch, tiny_net)
from test_ctc_beam_lm import Lm, Run, lm_line_bytes, random_lm

F32, F64 = np.float32, np.float64
PC_LEX = 32


# ---- the lexicon and the referee -------------------------------------------------------------------------------------------
class Lex:
    """word classes, words (a Python set) and the device copies, one per backend"""

    def __init__(self, nc, word_classes, words):
        self.nc, self.wc = nc, np.zeros(nc, bool)
        self.wc[list(word_classes)] = True
        self.words = {tuple(int(c) for c in w) for w in words}
        self.word_list = [tuple(int(c) for c in w) for w in words]   # (with the duplicates: the library merges them)
        self.prefixes = {w[:k] for w in self.words for k in range(len(w) + 1)} | {()}
        self.dev = {}

    def run(self, l):
        k = len(l)
        while k > 0 and self.wc[l[k - 1]]:
            k -= 1
        return tuple(l[k:])

    def allow_row(self, l):
        """[nc] bool: the classes prefix l may be extended by"""
        r = self.run(l)
        out = np.zeros(self.nc, bool)
        done = (not r) or r in self.words
        for c in range(1, self.nc):
            out[c] = (r + (c,)) in self.prefixes if self.wc[c] else done
        return out

    def finished(self, l):
        r = self.run(l)
        return (not r) or r in self.words

    def admits(self, l):
        """0 / 1 / 2 as clstm_lexicon_admits"""
        for k, c in enumerate(l):
            if c < 1 or c >= self.nc or not self.allow_row(tuple(l[:k]))[c]:
                return 0
        return 2 if self.finished(tuple(l)) else 1

    def obj(self, backend):
        from clstm_amd.lexicon import Lexicon
        if backend.kind not in self.dev:
            self.dev[backend.kind] = Lexicon(self.nc, self.wc.astype(np.uint8), self.word_list, lib=backend.lib)
        return self.dev[backend.kind]

    def handle(self, backend):
        return self.obj(backend).handle(backend.lib)


def no_lm(nc, bonus=0.0, weight=0.0):
    """lm == NULL: the table term of an all-zero table"""
    return Lm(2, nc, np.zeros((nc, nc), F32), None, weight, bonus)


def beam_ref_lex(lp, beam, dt, lm, lex):
    """beam_ref_lm (test_ctc_beam_lm.py), statement for statement, with the lexicon's two changes (marked)"""
    T, nc = lp.shape
    NEG = dt(-np.inf)
    w, bonus, tab = dt(lm.weight), dt(lm.bonus), lm.table.astype(dt)
    ent, order = {(): (dt(0), NEG)}, [()]
    lmv = {(): dt(0)}
    ever, margin, trap = {()}, np.inf, 0
    rows = {}
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
            for k in ent:
                if len(k) == len(l) + 1 and k[:-1] == l:
                    v[k[-1]] = NEG
            if l not in rows:
                rows[l] = lex.allow_row(l)
            v[~rows[l]] = NEG                                   # (the lexicon: a disallowed extension is no candidate)
            term = ((w * tab[lm.ctx(l)]).astype(dt) + bonus).astype(dt)
            lnew = (lmv[l] + term).astype(dt)
            key = (v + lnew).astype(dt)
            for c in np.argsort(-key, kind="stable")[:beam + 1]:
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
        if not lex.finished(l):                                 # (the lexicon: only finished runs are ranked)
            continue
        am = logadd(*ent[l], dt)
        total = dt(am + lmv[l])
        if lm.end is not None:
            total = dt(total + dt(w * dt(lm.end[lm.ctx(l)])))
        fin.append((total, i, l, am))
    fin.sort(key=lambda c: (-c[0], c[1]))
    r = Run()
    r.hyps = [(l, total, am) for total, _, l, am in fin]
    r.margin, r.trap, r.live = margin, trap, len(order)
    return r


class Line(tl.Line):
    """test_ctc_beam_lm.py's Line with the lexicon referee: gauge and check are its own"""

    def __init__(self, probs, beam, lm, lex, what):
        self.probs, self.beam, self.lm, self.lex, self.what, self.T = np.ascontiguousarray(probs, F32), beam, lm, lex, what, len(probs)
        if self.T == 0:
            return
        self.lp64 = lp_ref(probs, F64)
        self.r64, self.r32 = beam_ref_lex(self.lp64, beam, F64, lm, lex), beam_ref_lex(lp_ref(probs, F32), beam, F32, lm, lex)

    def check(self, nbest, nc, hyps):
        for lab, s, am in hyps:
            assert self.lex.admits(tuple(int(c) for c in lab)) == 2, (self.what, "not admissible", lab)
        if self.T and not self.r64.hyps:   # nothing admissible survived: a line of this kind is decided when no margin is in doubt
            assert hyps == [], (self.what, hyps)
            return self.gauge(nbest)[0]
        return super().check(nbest, nc, hyps)


def adequate(lines, nbest):
    tl.adequate(lines, nbest)
    n = sum(1 for ln in lines if ln.T)
    assert 2 * sum(1 for ln in lines if ln.T and ln.r64.hyps) >= n, "the case proves too little: most lines report no hypothesis"


def call_beam_lex(backend, lines, nc, beam, nbest, lex, lm=None, weight=None, bonus=None, want_am=True, lex_handle=None, lm_handle=None):
    """lines: list of [T_b, nc] arrays; lm: an Lm of test_ctc_beam_lm.py or None (then weight / bonus default to 0)
    -> per line [(labels, score, am_score)], and the raw arrays"""
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
    if weight is None:
        weight = lm.weight if lm is not None else 0.0
    if bonus is None:
        bonus = lm.bonus if lm is not None else 0.0
    if lm_handle is None:
        lm_handle = lm.handle(backend) if lm is not None else None
    backend.lib.call("clstm_ctc_beam_lex_batch", ptr(pd), nc, ptr(lo), len(T), beam, nbest,
                     lex.handle(backend) if lex_handle is None else lex_handle, lm_handle, weight, bonus,
                     ptr(nhyp), ptr(ln), ptr(sc), ptr(am) if want_am else None, ptr(lab))
    return unpack_beam(T, nbest, nhyp, ln, sc, lab, am), (nhyp, ln, sc, lab, am)


def count(backend, which=PC_LEX):
    n = C.c_longlong()
    backend.lib.call("clstm_debug_path_count", which, C.byref(n))
    return n.value


# ---- 1. the referee, pinned by exhaustive enumeration -----------------------------------------------------------------------
PIN_NC = 4                                  # two word classes (1, 2), one separator (3)
PIN_T = [3, 4]                              # (at T = 5 more than 32 admissible prefixes are alive: a 32-wide beam prunes)


@functools.lru_cache(maxsize=None)
def pin_lex():
    return Lex(PIN_NC, (1, 2), [(1,), (1, 2), (2, 1)])


@functools.lru_cache(maxsize=None)
def pin_lm(order):
    return no_lm(PIN_NC, bonus=0.25) if order == 0 else tl.pinned_lm(PIN_NC, order)


@pytest.mark.parametrize("order", [0, 2, 3])
@pytest.mark.parametrize("T", PIN_T)
def test_referee_is_exact_without_pruning(T, order):
    lex, lm = pin_lex(), pin_lm(order)
    for seed in range(8):
        p, exact = exhaustive_case(T, PIN_NC, seed)
        adm = {l: s for l, s in exact.items() if lex.admits(l) == 2}
        assert () in adm and (1, 2) in adm and (1, 1) not in adm and (2,) not in adm and (1, 3, 1) in adm
        r = beam_ref_lex(lp_ref(p, F64), 32, F64, lm, lex)
        assert r.margin == np.inf, "a 32-wide beam must not prune here"
        assert {h[0] for h in r.hyps} == set(adm)
        for l, s, am in r.hyps:
            want = adm[l] + float(lm.value(l, F64))
            assert abs(float(am) - adm[l]) <= 1e-13 * max(1.0, abs(adm[l])), (l, am, adm[l])
            assert abs(float(s) - want) <= 1e-13 * max(1.0, abs(want)), (l, s, want)
        assert [h[1] for h in r.hyps] == sorted((h[1] for h in r.hyps), reverse=True)


@pytest.mark.parametrize("order", [0, 2, 3])
@pytest.mark.parametrize("T", PIN_T)
def test_every_admissible_labelling_where_nothing_is_pruned(backend, T, order):
    lex, lm = pin_lex(), pin_lm(order)
    cases = [exhaustive_case(T, PIN_NC, seed) for seed in range(8)]
    got, _ = call_beam_lex(backend, [p for p, _ in cases], PIN_NC, 32, 32, lex, None if order == 0 else lm, bonus=lm.bonus, weight=lm.weight)
    for (p, exact), hyps in zip(cases, got):
        adm = {l: s for l, s in exact.items() if lex.admits(l) == 2}
        assert {tuple(int(c) for c in h[0]) for h in hyps} == set(adm) and len(hyps) == len(adm)
        sc = [h[1] for h in hyps]
        assert all(a >= b for a, b in zip(sc, sc[1:]))
        for lab, s, am in hyps:
            l = tuple(int(c) for c in lab)
            want = adm[l] + float(lm.value(l, F64))
            assert abs(am - adm[l]) <= bar(adm[l]), (lab, am, adm[l])
            assert abs(s - want) <= bar(want), (lab, s, want)


# ---- 2. a lexicon that admits everything changes nothing --------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("T,nc,beam,L,peak", tl.ZERO)
def test_a_lexicon_that_admits_everything_changes_nothing(backend, T, nc, beam, L, peak, order):
    lines = [ln.probs for ln in sweep_case(T, nc, beam, L, peak)]
    lex = Lex(nc, (), [])   # no word classes: every class is a separator, the root takes them all
    lm = random_lm(7, order, nc, end=True, weight=0.6, bonus=0.2)
    for nbest in sorted({beam, max(1, beam // 2)}):
        _, want = tl.call_beam_lm(backend, lines, nc, beam, nbest, lm)
        _, got = call_beam_lex(backend, lines, nc, beam, nbest, lex, lm)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), "the LM form's bytes"
        _, (nhyp, ln, sc, lab) = call_beam(backend, lines, nc, beam, nbest)
        _, (nhyp2, ln2, sc2, lab2, am2) = call_beam_lex(backend, lines, nc, beam, nbest, lex, None, weight=0.7, bonus=0.0)
        assert nhyp2.tobytes() == nhyp.tobytes() and ln2.tobytes() == ln.tobytes() and lab2.tobytes() == lab.tobytes()
        assert sc2.tobytes() == sc.tobytes() and am2.tobytes() == sc.tobytes(), "the plain search's bytes"
        assert nhyp.max() >= 1


# ---- 3. the lexicon decides ------------------------------------------------------------------------------------------------
def framed(nc, frames):
    """one frame per entry: {class: posterior}, the rest spread unevenly (no exact ties) over the other classes"""
    p = tl.background(len(frames), nc).astype(F64)
    for t, f in enumerate(frames):
        rest = [c for c in range(nc) if c not in f]
        p[t, rest] *= (1.0 - sum(f.values())) / p[t, rest].sum()
        for c, x in f.items():
            p[t, c] = x
    return p.astype(F32)


@functools.lru_cache(maxsize=None)
def decide_cases():
    """-> [(Line, the labelling the constrained search must report first, the labelling the plain search reports)]"""
    B = {0: 0.9}
    out = []
    # "c0t" -> "cat": classes c a t 0 = 1 2 3 4 (all word classes), 5 a separator; the line is peaked on c 0 t, a is the runner-up of 0
    lex = Lex(6, (1, 2, 3, 4), [(1, 2, 3)])
    p = framed(6, [{1: 0.9}, B, {4: 0.55, 2: 0.35}, B, {3: 0.9}, B])
    out.append((Line(p, 4, no_lm(6), lex, "c0t -> cat"), (1, 2, 3), (1, 4, 3)))
    # a word allowed only after a separator: words "a", "b"; "ab" is none.  The frame between them: blank 0.5, the separator 0.4
    lex = Lex(4, (1, 2), [(1,), (2,)])
    p = framed(4, [{1: 0.9}, {0: 0.5, 3: 0.4}, {2: 0.9}, B])
    out.append((Line(p, 4, no_lm(4), lex, "a b, not ab"), (1, 3, 2), (1, 2)))
    # a terminal node with children: "a", "ab"
    lex = Lex(4, (1, 2), [(1,), (1, 2)])
    out.append((Line(framed(4, [{1: 0.9}, B, {2: 0.9}, B]), 4, no_lm(4), lex, "ab of {a, ab}"), (1, 2), (1, 2)))
    out.append((Line(framed(4, [{1: 0.9}, B, {0: 0.8, 2: 0.1}, B]), 4, no_lm(4), lex, "a of {a, ab}"), (1,), (1,)))
    out.append((Line(framed(4, [{2: 0.6, 1: 0.3}, B, {2: 0.9}, B]), 4, no_lm(4), lex, "b is no word start"), (1, 2), (2, 2)))
    # the double letter: "aa" against {"a"} (2 a separator); through a blank it is an extension and the lexicon refuses it
    lex = Lex(3, (1,), [(1,)])
    out.append((Line(framed(3, [{1: 0.9}, {0: 0.9}, {1: 0.9}, {0: 0.9}]), 4, no_lm(3), lex, "aa against {a}"), None, (1, 1)))
    return out


def test_the_lexicon_decides(backend):
    for ln, want, plain in decide_cases():
        nc = ln.probs.shape[1]
        got, _ = call_beam_lex(backend, [ln.probs], nc, 4, 4, ln.lex)
        assert ln.check(4, nc, got[0]), ln.what
        top = tuple(got[0][0][0].tolist())
        assert top == ln.r64.hyps[0][0] and (want is None or top == want), (ln.what, top)
        old, _ = call_beam(backend, [ln.probs], nc, 4, 4)
        assert tuple(old[0][0][0].tolist()) == plain, (ln.what, old[0][0][0])
        if want is None:
            assert all(tuple(h[0].tolist()) != (1, 1) for h in got[0]) and any(tuple(h[0].tolist()) == (1, 1) for h in old[0])


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------
#        T, nc, beam, nbest, words, max word length, lines, peak
SHAPES = [(24, 12, 4, 2, 6, 3, 8, 0.8), (40, 40, 8, 3, 30, 4, 8, 0.8), (64, 83, 8, 3, 200, 5, 8, 0.85), (30, 83, 32, 4, 200, 5, 8, 0.7)]


@functools.lru_cache(maxsize=None)
def shape_lexicon(nc, nwords, maxlen, seed):
    """separators: the last max(1, nc // 6) classes.  Beside the random words: the first and the last word class as children of one
    node (the root), a node with one child, a word that ends at the largest word class"""
    rng = np.random.default_rng(seed)
    nsep = max(1, nc // 6)
    first, last = 1, nc - 1 - nsep
    words = [tuple(int(c) for c in rng.integers(first, last + 1, int(rng.integers(1, maxlen + 1)))) for _ in range(nwords)]
    words += [(first, last), (last, first, last)][:2 if maxlen >= 3 else 1]
    return Lex(nc, range(first, last + 1), words), list(range(last + 1, nc))


@functools.lru_cache(maxsize=None)
def shape_case(T, nc, beam, nbest, nwords, maxlen, nlines, peak):
    """truths: random lexicon words joined by separators, cut at a word boundary near T / 3 labels; half of the words carry one
    replaced character (a misprint the lexicon has to repair or to refuse)"""
    rng = np.random.default_rng(1000 * T + nc)
    lex, seps = shape_lexicon(nc, nwords, maxlen, 1000 * T + nc)
    wl = sorted(lex.words)
    lm = random_lm(T + nc, 2, nc, weight=0.3, bonus=0.1) if nc != 40 else None
    lines = []
    for b in range(nlines):
        Tb = max(3, T - (b * T) // 16)
        truth = []
        while True:
            w = list(wl[int(rng.integers(len(wl)))])
            if rng.random() < 0.5:
                w[int(rng.integers(len(w)))] = int(rng.integers(1, nc - len(seps)))
            more = truth + ([int(seps[int(rng.integers(len(seps)))])] if truth else []) + w
            if len(more) > max(1, Tb // 3):
                break
            truth = more
        truth = truth or w[:max(1, Tb // 3)]
        lines.append(Line(peaked_probs(rng, Tb, truth, nc, peak), beam, lm if lm is not None else no_lm(nc, 0.1), lex,
                          "T=%d nc=%d beam=%d line %d" % (Tb, nc, beam, b)))
    return lines, lex, lm


@pytest.mark.parametrize("T,nc,beam,nbest,nwords,maxlen,nlines,peak", SHAPES)
def test_shapes(backend, T, nc, beam, nbest, nwords, maxlen, nlines, peak):
    lines, lex, lm = shape_case(T, nc, beam, nbest, nwords, maxlen, nlines, peak)
    adequate(lines, nbest)
    got, (nhyp, lens, sc, _, am) = call_beam_lex(backend, [ln.probs for ln in lines], nc, beam, nbest, lex, lm, weight=lines[0].lm.weight,
                                                 bonus=lines[0].lm.bonus)
    und = 0
    for b, (ln, hyps) in enumerate(zip(lines, got)):
        und += 0 if ln.check(nbest, nc, hyps) else 1
        for k in range(len(hyps), nbest):   # unused slots
            assert lens[b * nbest + k] == 0 and sc[b * nbest + k] == -np.inf and am[b * nbest + k] == -np.inf
    print("T=%d nc=%d beam=%d: %d of %d undecided, %d without a hypothesis" % (T, nc, beam, und, nlines, sum(1 for h in got if not h)))


# ---- 5. no admissible hypothesis ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def empty_case():
    """beam 1, words {"ab"}: a line peaked on a alone ends in an unfinished run"""
    lex = Lex(4, (1, 2), [(1, 2)])
    B = {0: 0.9}
    miss = Line(framed(4, [{1: 0.9}, B, B, B]), 1, no_lm(4), lex, "a of {ab}")
    rng = np.random.default_rng(3)
    left = Line(peaked_probs(rng, 9, [1, 2, 3, 1, 2], 4, 0.9), 1, no_lm(4), lex, "ab ab")
    right = Line(peaked_probs(rng, 5, [3], 4, 0.9), 1, no_lm(4), lex, "a separator")
    return lex, left, miss, right


def test_no_admissible_hypothesis(backend):
    lex, left, miss, right = empty_case()
    assert miss.r64.hyps == [] and miss.r64.live == 1 and left.r64.hyps and right.r64.hyps
    three = [left.probs, miss.probs, right.probs]
    got, raw = call_beam_lex(backend, three, 4, 1, 1, lex)
    nhyp, ln, sc, lab, am = raw
    assert nhyp[1] == 0 and ln[1] == 0 and sc[1] == -np.inf and am[1] == -np.inf and (lab[9:13] == 0).all()
    for line, hyps in zip((left, miss, right), got):
        assert line.check(1, 4, hyps), line.what
    T3 = [9, 4, 5]
    _, two = call_beam_lex(backend, [left.probs, right.probs], 4, 1, 1, lex)
    assert lm_line_bytes(T3, 1, raw, 0) == lm_line_bytes([9, 5], 1, two, 0) and lm_line_bytes(T3, 1, raw, 2) == lm_line_bytes([9, 5], 1, two, 1)
    _, alone = call_beam_lex(backend, [miss.probs], 4, 1, 1, lex)
    assert lm_line_bytes(T3, 1, raw, 1) == lm_line_bytes([4], 1, alone, 0)
    _, other = call_beam_lex(backend, [miss.probs, left.probs], 4, 1, 1, lex)
    assert lm_line_bytes(T3, 1, raw, 1) == lm_line_bytes([4, 9], 1, other, 0)
    # a wider beam keeps admissible prefixes alive beside it: the same line reports hypotheses
    wide, _ = call_beam_lex(backend, [miss.probs], 4, 4, 4, lex)
    assert Line(miss.probs, 4, no_lm(4), lex, "a of {ab}, beam 4").check(4, 4, wide[0]) and len(wide[0]) >= 1


# ---- 6. a prefix that leaves the beam and is extended again ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trap_case():
    """test_ctc_beam.py's trap lines (nc 3, beam 3, T 10) under a lexicon that admits every labelling of them while the state moves
    with every label: class 1 a word class with the words 1, 11, .. (ten of them), class 2 a separator"""
    lex = Lex(3, (1,), [(1,) * k for k in range(1, 11)])
    return lex, [Line(ln.probs, 3, no_lm(3), lex, ln.what) for ln in tb.trap_lines()]


def test_a_reextended_prefix_keeps_its_node_and_state(backend):
    lex, lines = trap_case()
    assert len(lines) == 4 and all(ln.r64.trap > 0 and ln.gauge(3)[0] for ln in lines), "the trap does not occur"
    got, raw = call_beam_lex(backend, [ln.probs for ln in lines], 3, 3, 3, lex)
    for ln, hyps in zip(lines, got):
        assert ln.check(3, 3, hyps), ln.what
    _, plain = call_beam(backend, [ln.probs for ln in lines], 3, 3, 3)   # nothing is refused here: the plain search's bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(raw[:4], plain)) and raw[4].tobytes() == plain[2].tobytes()


# ---- 7. both instantiations; the LDS ceiling -------------------------------------------------------------------------------
BEAM_LDS_WORDS, BEAM_MAX = 36 * 1024, 32   # ctc_beam.h


def beam_lds_words(T, nc, beam):
    """(LDS words of a lexicon-form launch with this one line, whether every section that may lies in LDS): beam_lds_layout and
    plan_ctc_beam restated (test_lds_ceiling.py does it for the other forms): the LM form's fixed part + beam * ceil(nc / 32) words
    of allowed classes, and six node arrays"""
    K = nc - 1
    fixed = 4 * (beam + beam * K) + 2 * 7 * BEAM_MAX + 2 * BEAM_MAX + 2 * (2 * K + 2) + 4 + 5 * BEAM_MAX + beam * ((nc + 31) // 32)
    fixed += fixed & 1
    nn = 1 + T * beam
    H = 64
    while H < 2 * nn:
        H *= 2
    used, all_lds = 0, True
    for need in (H, 6 * nn, T * nc):
        if used + need <= BEAM_LDS_WORDS - fixed:
            used += need
        else:
            all_lds = False
    return fixed + used, all_lds


@functools.lru_cache(maxsize=None)
def lds_line(T, nc, beam):
    lex, seps = shape_lexicon(nc, 40, 3, nc)
    rng = np.random.default_rng(1000 * T + nc)
    wl = sorted(lex.words)
    truth = []
    while len(truth) < max(1, T // 4):
        truth += ([seps[0]] if truth else []) + list(wl[int(rng.integers(len(wl)))])
    lm = tl.random_lm(7 + nc, 2, nc, weight=0.5, bonus=0.2)
    return Line(peaked_probs(rng, T, truth[:max(1, T // 3)], nc, 0.9), beam, lm, lex, "T=%d nc=%d beam=%d lex" % (T, nc, beam))


#            all in LDS, (T, nc, beam) of the first call, of the larger one
LDS_CASES = [(True, (6, 5, 4), (8, 101, 32)), (False, (64, 101, 32), (70, 101, 32))]


@pytest.mark.parametrize("all_lds,first,larger", LDS_CASES)
def test_lds_ceiling(backend, all_lds, first, larger):
    """a first carve, a larger one above 64 KiB, the first again (tests/test_lds_ceiling.py states the rule under test)"""
    nbest = 4
    w0, w1 = beam_lds_words(*first), beam_lds_words(*larger)
    print("beam carves: %d, %d bytes" % (4 * w0[0], 4 * w1[0]))
    assert w0[1] == w1[1] == all_lds and w0[0] < w1[0] and 4 * w1[0] > 65536, (w0, w1)
    assert (4 * w0[0] <= 65536) == all_lds, w0
    for T, nc, beam in (first, larger, first):
        ln = lds_line(T, nc, beam)
        got, _ = call_beam_lex(backend, [ln.probs], nc, beam, nbest, ln.lex, ln.lm)
        ln.check(nbest, nc, got[0])


def test_a_line_too_long_for_lds_beside_short_ones(backend):
    """the long line's posteriors do not fit beside its trie (ctc_beam_kernel<false, true, true> for the whole batch); the short
    lines alone run in <true, true, true>: the same bytes"""
    nc, beam, nbest = 101, 32, 4
    assert not beam_lds_words(64, nc, beam)[1] and beam_lds_words(9, nc, beam)[1] and beam_lds_words(6, nc, beam)[1]
    long_line = lds_line(64, nc, beam)
    shorts = [lds_line(9, nc, beam), lds_line(6, nc, beam)]
    lines, Ts = [shorts[0].probs, long_line.probs, shorts[1].probs], [9, 64, 6]
    got, mixed = call_beam_lex(backend, lines, nc, beam, nbest, long_line.lex, long_line.lm)
    _, short = call_beam_lex(backend, [lines[0], lines[2]], nc, beam, nbest, long_line.lex, long_line.lm)
    _, alone = call_beam_lex(backend, [lines[1]], nc, beam, nbest, long_line.lex, long_line.lm)
    assert lm_line_bytes(Ts, nbest, mixed, 0) == lm_line_bytes([9, 6], nbest, short, 0)
    assert lm_line_bytes(Ts, nbest, mixed, 2) == lm_line_bytes([9, 6], nbest, short, 1)
    assert lm_line_bytes(Ts, nbest, mixed, 1) == lm_line_bytes([64], nbest, alone, 0)
    for ln, hyps in zip((shorts[0], long_line, shorts[1]), got):
        ln.check(nbest, nc, hyps)


def test_the_inputs_are_adequate():
    """from the referee alone (no library here): decided lines, reported hypotheses, the trie shapes the sweep is to contain"""
    for ln, want, plain in decide_cases():
        assert ln.gauge(4)[0], ln.what
        assert ln.r64.hyps and (want is None or ln.r64.hyps[0][0] == want), (ln.what, ln.r64.hyps[:1])
    for shape in SHAPES:
        lines, lex, _ = shape_case(*shape)
        adequate(lines, shape[3])
        nc, nsep = shape[1], max(1, shape[1] // 6)
        first, last = 1, nc - 1 - nsep
        kids = {}
        for p in lex.prefixes:
            if p:
                kids.setdefault(p[:-1], set()).add(p[-1])
        assert {first, last} <= kids[()] and any(len(k) == 1 for k in kids.values()) and any(w[-1] == last for w in lex.words)
    lex, left, miss, right = empty_case()
    assert miss.gauge(1)[0] and left.gauge(1)[0] and right.gauge(1)[0]
    adequate(trap_case()[1], 3)
    for _, first, larger in LDS_CASES:
        for shape in (first, larger):
            assert lds_line(*shape).gauge(4)[0], shape
    adequate([lds_line(64, 101, 32), lds_line(9, 101, 32), lds_line(6, 101, 32)], 4)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_are_named_and_touch_nothing(backend):
    from clstm_amd.abi import ClstmError, i32, ptr
    lines = [ln.probs for ln in sweep_case(7, 5, 4, 2, 0.9)]
    lex = Lex(5, (1, 2), [(1,), (1, 2), (2, 2)])
    lm = random_lm(1, 2, 5)
    n0 = count(backend)
    _, good = call_beam_lex(backend, lines, 5, 4, 3, lex, lm)
    assert count(backend) == n0 + 1
    p29, p30 = count(backend, 29), count(backend, 30)
    other_lm, other_lex = random_lm(2, 2, 6), Lex(6, (1,), [(1,)])
    for kw, text in ((dict(lm_handle=other_lm.handle(backend)), "language model was made for another class count"),
                     (dict(lex_handle=other_lex.handle(backend)), "lexicon was made for another class count"),
                     (dict(lex_handle=0), "lexicon is required"), (dict(weight=-0.5), "weight"), (dict(weight=float("nan")), "weight"),
                     (dict(weight=float("inf")), "weight"), (dict(bonus=float("nan")), "bonus"), (dict(bonus=float("-inf")), "bonus")):
        with pytest.raises(ClstmError, match="clstm_ctc_beam_lex: .*" + text):
            call_beam_lex(backend, lines, 5, 4, 3, lex, lm, **kw)
    with pytest.raises(ClstmError, match="weight"):   # (checked without a model too)
        call_beam_lex(backend, lines, 5, 4, 3, lex, None, weight=-1.0)
    for beam, nbest in ((0, 1), (33, 1), (4, 5), (4, 0)):
        with pytest.raises(ClstmError, match="must lie in"):
            call_beam_lex(backend, lines, 5, beam, nbest, lex, lm)
    pd = backend.up(np.concatenate([p for p in lines if len(p)], 0))
    lo = i32(np.concatenate([[0], np.cumsum([len(p) for p in lines])]))
    bad = lo.copy()
    bad[2] = bad[1] - 1
    nhyp, sc, am = np.full(len(lines), -3, np.int32), np.full(len(lines) * 3, 123.0, F32), np.full(len(lines) * 3, 123.0, F32)
    for off, weight, text in ((bad, 0.5, "bad offsets"), (lo, -1.0, "weight")):
        with pytest.raises(ClstmError, match=text):
            backend.lib.call("clstm_ctc_beam_lex_batch", ptr(pd), 5, ptr(off), len(lines), 4, 3, lex.handle(backend), lm.handle(backend),
                             weight, 0.0, ptr(nhyp), None, ptr(sc), ptr(am), None)
    assert (nhyp == -3).all() and (sc == 123.0).all() and (am == 123.0).all()
    assert count(backend) == n0 + 1 and count(backend, 29) == p29 and count(backend, 30) == p30
    # creation: each refusal by name, nothing made
    h = C.c_void_p()
    wc = np.asarray([0, 1, 1, 0, 0], np.uint8)

    def create(wc, words, nc=5):
        flat = i32([c for w in words for c in w] or [0])
        off = i32(np.concatenate([[0], np.cumsum([len(w) for w in words])]))
        backend.lib.call("clstm_lexicon_create", C.byref(h), nc, ptr(wc), ptr(flat), ptr(off), len(words))
    for a, words, text in ((np.asarray([1, 1, 1, 0, 0], np.uint8), [(1,)], "class 0 .blank. cannot be a word class"),
                           (wc, [(1,), (2, 5)], "word 1 holds a label outside 1 .. nc-1"), (wc, [(0,)], "word 0 holds a label outside"),
                           (wc, [(1, 3)], "word 0 holds a label that is not a word class"), (wc, [(1,), (), (2,)], "word 1 is empty")):
        with pytest.raises(ClstmError, match="clstm_lexicon_create: " + text):
            create(a, words)
    with pytest.raises(ClstmError, match="2\\^28 bytes"):   # 2^21 + 1 nodes of 32 words each (the words are read, nothing is uploaded)
        create(np.concatenate([[0], np.ones(1023, np.uint8)]).astype(np.uint8), [tuple([1] * (1 << 21))], nc=1024)
    assert h.value is None
    from clstm_amd.lexicon import Lexicon
    for args in ((5, [1, 1, 0, 0, 0], []), (5, wc, [()]), (5, wc, [(3,)]), (5, wc, [(7,)]), (1, [0], [])):
        with pytest.raises(ValueError):
            Lexicon(*args)
    create(wc, [])   # no words: legal, only separators can be written
    info = np.zeros(4, np.int64)
    backend.lib.call("clstm_lexicon_info", h, ptr(info))
    assert info.tolist()[:3] == [0, 1, 0]
    backend.lib.call("clstm_lexicon_destroy", h)
    _, again = call_beam_lex(backend, lines, 5, 4, 3, lex, lm)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again))


def test_the_largest_key_set_admitted_runs_and_one_more_is_refused(backend):
    from clstm_amd.abi import ClstmError
    rng = np.random.default_rng(5)
    for nc, ok in ((513, True), (514, False)):   # beam 8: 8 * 512 = 4096 extension keys; 17 words of allowed classes per node
        lex = Lex(nc, range(1, nc - 1), [(1, 2), (nc - 2, 1), (3,)])
        ln = Line(peaked_probs(rng, 6, [nc - 2, 1], nc, 0.9), 8, no_lm(nc, 0.1), lex, "nc=%d beam=8" % nc)
        if ok:
            assert ln.gauge(2)[0] and ln.r64.hyps[0][0] == (nc - 2, 1)
            got, _ = call_beam_lex(backend, [ln.probs], nc, 8, 2, lex, bonus=ln.lm.bonus)
            assert ln.check(2, nc, got[0])
        else:
            n0 = count(backend)
            with pytest.raises(ClstmError, match="clstm_ctc_beam_lex: .*exceeds 4096"):
                call_beam_lex(backend, [ln.probs], nc, 8, 2, lex)
            assert count(backend) == n0


# ---- 9. the trie builder ---------------------------------------------------------------------------------------------------
def test_admits_and_info_against_a_set(backend):
    rng = np.random.default_rng(17)
    nc = 9   # word classes 1 .. 6, separators 7, 8
    words = [tuple(int(c) for c in rng.integers(1, 7, int(rng.integers(1, 5)))) for _ in range(200)]
    words += words[:40]   # duplicates: counted once
    lex = Lex(nc, range(1, 7), words)
    info = lex.obj(backend).info(backend.lib)
    edges = len(lex.prefixes) - 1
    assert info["words"] == len(lex.words) and info["nodes"] == edges + 1 and info["edges"] == edges
    assert info["device_bytes"] == 4 * (4 + (edges + 1) * 1 + (edges + 2) + 2 * edges)
    seen = set()
    probes = [()] + [w for w in sorted(lex.words)[:30]] + [w[:-1] for w in sorted(lex.words)[:30]]
    for _ in range(600):
        L = int(rng.integers(0, 9))
        l = []
        for _k in range(L):   # mostly allowed continuations, so that long sequences stay admissible
            row = np.flatnonzero(lex.allow_row(tuple(l)))
            l.append(int(row[rng.integers(len(row))]) if len(row) and rng.random() < 0.85 else int(rng.integers(1, nc)))
        probes.append(tuple(l))
    for l in probes:
        want = lex.admits(l)
        assert lex.obj(backend).admits(l, backend.lib) == want, (l, want)
        seen.add(want)
    assert seen == {0, 1, 2}
    assert lex.obj(backend).admits((0,)) == 0 and lex.obj(backend).admits((nc,)) == 0 and lex.obj(backend).admits((-1,)) == 0


# ---- 10. net level ---------------------------------------------------------------------------------------------------------
def net_lex(backend):
    """NC = 5: word classes 1 .. 3, separator 4"""
    rng = np.random.default_rng(9)
    words = [tuple(int(c) for c in rng.integers(1, 4, int(rng.integers(1, 4)))) for _ in range(12)] + [(1,), (2,), (3,)]
    return Lex(NC, (1, 2, 3), words)


def standalone(backend, net, lex, clm, weight, bonus, beam, nbest):
    lm = None if clm is None else tl.as_test_lm(clm, weight, bonus)
    return call_beam_lex(backend, split(net.outputs(), net.T), NC, beam, nbest, lex, lm, weight=weight, bonus=bonus,
                         lm_handle=None if clm is None else clm.handle(backend.lib))[0]


def test_net_beam_lex_equals_standalone_and_counts(backend):
    net, clm, lex = tiny_net(backend), tl.net_lm(backend), net_lex(backend)
    lines, _ = tiny_batch(31)
    net.set_inputs(lines)
    net.forward()
    n0, p29, p30 = count(backend), count(backend, 29), count(backend, 30)
    got = net.beam_lex(lex.obj(backend), beam=4, nbest=3, lm=clm, weight=0.6, bonus=0.2)
    assert count(backend) == n0 + 1 and count(backend, 29) == p29 and count(backend, 30) == p30
    assert tl.same_hyps(got, standalone(backend, net, lex, clm, 0.6, 0.2, 4, 3))
    assert all(len(h) >= 1 and np.isfinite(h[0][1]) and np.isfinite(h[0][2]) for h in got)
    bare = net.beam_lex(lex.obj(backend), beam=4)   # nbest defaults to beam, no model
    assert tl.same_hyps(bare, standalone(backend, net, lex, None, 0.0, 0.0, 4, 4))
    for hyps in got + bare:
        for lab, s, am in hyps:
            assert lex.admits(tuple(lab.tolist())) == 2
    for hyps in bare:
        for lab, s, am in hyps:
            assert s == am


def test_beam_lex_after_predict_while_ctc_refuses(backend):
    from clstm_amd.abi import ClstmError
    net, clm, lex = tiny_net(backend), tl.net_lm(backend, 2), net_lex(backend)
    lines, trs = tiny_batch(41)
    net.predict(lines)
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)
    got = net.beam_lex(lex.obj(backend), beam=4, nbest=2, lm=clm, weight=0.5)
    assert tl.same_hyps(got, standalone(backend, net, lex, clm, 0.5, 0.0, 4, 2))
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)


def test_beam_lex_leaves_the_training_state_alone(backend):
    from test_ctc_score import read_dz
    lines, trs = tiny_batch(43)
    got = []
    for with_beam in (False, True):
        net, clm, lex = tiny_net(backend), tl.net_lm(backend), net_lex(backend)
        net.enable_input_deltas(True)
        net.set_inputs(lines)
        net.forward()
        if with_beam:
            net.beam_lex(lex.obj(backend), beam=8, nbest=3, lm=clm, weight=0.5, bonus=0.1)
        al = net.ctc(trs, want_aligned=True)
        dz = read_dz(backend, net)
        net.backward()
        g, dx = net.get_grads(), net.input_deltas()
        net.update()
        if with_beam:
            net.beam_lex(lex.obj(backend), beam=2)
        backend.sync()
        got.append((al, dz, g, dx, net.get_params(), net.get_derivs()))
    for name, a, b in zip(("aligned", "Dz", "grads", "input deltas", "params", "derivs"), *got):
        assert a.tobytes() == b.tobytes(), name
    assert np.abs(got[0][1]).max() > 0


def test_beam_lex_between_training_steps_and_without_a_current_minibatch(backend):
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
        net, lex = tiny_net(backend), net_lex(backend)
        net.train_step_prepared(batches[0][0], batches[0][1], batches[1][0], batches[1][1])
        if disturbed:
            p = net.get_params()
            with pytest.raises(ClstmError, match="no current minibatch"):
                net.beam_lex(lex.obj(backend), beam=4)
            assert net.get_params().tobytes() == p.tobytes()
        net.train_step_prepared(batches[1][0], batches[1][1])
        if disturbed:
            assert len(net.beam_lex(lex.obj(backend), beam=4, nbest=2)) == 3
        net.train_step_prepared(batches[2][0], batches[2][1])
        if disturbed:
            net.beam_lex(lex.obj(backend), beam=8, bonus=0.3)
        backend.sync()
        res.append((net.get_params(), net.get_derivs()))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()


def test_net_bad_arguments_leave_the_net_alone(backend):
    from clstm_amd.abi import ClstmError, ptr
    net, clm, lex = tiny_net(backend), tl.net_lm(backend), net_lex(backend)
    lines, trs = tiny_batch(53)
    net.set_inputs(lines)
    net.forward()
    z = net.outputs()
    h, x = clm.handle(backend.lib), lex.handle(backend)
    nhyp, sc = np.zeros(3, np.int32), np.zeros(3 * 32, F32)
    n0 = count(backend)

    def call(n, beam, nbest, x, h, weight, bonus, sc=sc):
        backend.lib.call("clstm_net_beam_lex", n.h, beam, nbest, x, h, weight, bonus, ptr(nhyp), None, ptr(sc), None, None)
    for beam, nbest in ((0, 1), (33, 1), (4, 5)):
        with pytest.raises(ClstmError, match="clstm_net_beam_lex: 1 <= nbest <= beam"):
            call(net, beam, nbest, x, h, 0.5, 0.0)
    with pytest.raises(ClstmError, match="required"):
        call(net, 4, 2, x, h, 0.5, 0.0, sc=None)
    with pytest.raises(ClstmError, match="lexicon is required"):
        call(net, 4, 2, None, h, 0.5, 0.0)
    with pytest.raises(ClstmError, match="weight"):
        call(net, 4, 2, x, h, -1.0, 0.0)
    with pytest.raises(ClstmError, match="bonus"):
        call(net, 4, 2, x, None, 1.0, float("nan"))
    with pytest.raises(ClstmError, match="language model was made for another class count"):
        call(net, 4, 2, x, random_lm(3, 2, NC + 1).handle(backend), 0.5, 0.0)
    with pytest.raises(ClstmError, match="lexicon was made for another class count"):
        call(net, 4, 2, Lex(NC + 1, (1,), [(1,)]).handle(backend), h, 0.5, 0.0)
    fresh = tiny_net(backend)
    with pytest.raises(ClstmError, match="set_batch first"):
        call(fresh, 4, 2, x, h, 0.5, 0.0)
    assert net.outputs().tobytes() == z.tobytes() and (nhyp == 0).all() and (sc == 0).all() and count(backend) == n0
    net.ctc(trs)
    net.backward()
    backend.sync()
