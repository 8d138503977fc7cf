"""clstm_ctc_beam_batch / clstm_net_beam (clstm_amd/csrc/ctc_beam.h): the n best labellings of a line by CTC prefix beam search.

The referee is a numpy restatement of the algorithm in the header of ctc_beam.h with prefixes as tuples in a dict, in a float64
form and a float32 form (one rounding per operation; a gauge only).  test_referee_is_exact_without_pruning pins the float64 form
to the sum over every path where the beam cannot prune.

Bars.  Scores against the FLOAT64 referee on the posteriors the device was given: |s - s64| <= 1e-4 max(1, |s64|)
(test_ctc_score.py's form); every case asserts the float32 referee within half of it.  Label identity only where no near tie
decides: with D = the largest |s32 - s64| of a line's reported hypotheses, a line is DECIDED when every pruning margin of the
float64 run (last kept minus first dropped candidate, every frame) and every gap between adjacent reported hypotheses exceeds 8 D;
a decided line must match the referee's sequences and order exactly, its scores within max(8 D, 16 f32 ulps of |s64|): the device
may round an operation differently from numpy, not by another order of magnitude.  Any other line: labels in range, lengths <= T,
scores descending, every score <= the labelling's exact CTC log-likelihood (float64 forward recursion) + bar, top score >= the
referee's - bar.  A case may leave at most a quarter of its lines undecided, asserted from the referee alone.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from common import RTOL, synth_lines

F32, F64 = np.float32, np.float64


# ---- the referee -------------------------------------------------------------------------------------------------------------
def lp_ref(probs, dt):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(np.fmax(np.asarray(probs, F32).astype(dt), dt(F32(1e-30)))).astype(dt)


def logadd(a, b, dt):
    m = a if a > b else b
    if m == -np.inf:
        return dt(-np.inf)
    return dt(m + dt(np.log1p(dt(np.exp(dt(-abs(dt(a - b))))))))


class Run:
    """result of one referee run: hyps [(labels tuple, tot)] best first, the smallest pruning margin, whether the re-extension
    trap occurred (a prefix that had left the beam is extended into it again while a descendant of it is an entry)"""


def beam_ref(lp, beam, dt):
    T, nc = lp.shape
    NEG = dt(-np.inf)
    ent, order = {(): (dt(0), NEG)}, [()]
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
            cands.append((logadd(lbn, lnbn, dt), i, l, lbn, lnbn))
            v = (row + tot[l]).astype(dt)
            if e:
                v[e] = dt(row[e] + lb)
            v[0] = NEG
            for k in ent:   # l + c is itself an entry
                if len(k) == len(l) + 1 and k[:-1] == l:
                    v[k[-1]] = NEG
            for c in np.argsort(-v, kind="stable")[:beam + 1]:   # (an entry's own best beam + 1 hold every winner and the first loser)
                if v[c] > NEG:
                    cands.append((v[c], beam + i * nc + int(c), l + (int(c),), NEG, v[c]))
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
        ent = {c[2]: (c[3], c[4]) for c in keep}
        order = [c[2] for c in keep]
        ever |= new
    r = Run()
    r.hyps = [(l, logadd(*ent[l], dt)) for l in order]
    r.margin, r.trap = margin, trap
    return r


def exact_loglik(lp64, labels):
    """log p(labels | line): the textbook CTC forward recursion in float64"""
    T = len(lp64)
    st = [0]
    for c in labels:
        st += [int(c), 0]
    S = len(st)
    a = np.full(S, -np.inf)
    a[0] = lp64[0, 0]
    if S > 1:
        a[1] = lp64[0, st[1]]
    for t in range(1, T):
        b = a.copy()
        b[1:] = np.logaddexp(b[1:], a[:-1])
        for s in range(2, S):
            if st[s] != 0 and st[s] != st[s - 2]:
                b[s] = np.logaddexp(b[s], a[s - 2])
        a = b + lp64[t, st]
    return float(np.logaddexp(a[-1], a[-2]) if S > 1 else a[-1])


def bar(s64):
    return RTOL * max(1.0, abs(float(s64)))


class Line:
    """one line and its referee figures for one beam width (computed once, shared by backends and tests)"""

    def __init__(self, probs, beam, what):
        self.probs, self.beam, self.what, self.T = np.ascontiguousarray(probs, F32), beam, what, len(probs)
        if self.T == 0:
            return
        self.lp64 = lp_ref(probs, F64)
        self.r64, self.r32 = beam_ref(self.lp64, beam, F64), beam_ref(lp_ref(probs, F32), beam, F32)

    def gauge(self, nbest):
        """-> (decided, D) from the referee alone"""
        h64, h32 = self.r64.hyps[:nbest], self.r32.hyps[:nbest]
        if [l for l, _ in h64] != [l for l, _ in h32]:
            return False, None
        for (_, s64), (_, s32) in zip(h64, h32):
            assert abs(float(s32) - float(s64)) <= 0.5 * bar(s64), (self.what, "referee", s32, s64)
        D = max(abs(float(s32) - float(s64)) for (_, s64), (_, s32) in zip(h64, h32))
        gaps = [float(a[1]) - float(b[1]) for a, b in zip(h64, h64[1:])]
        return min([self.r64.margin] + gaps) > 8 * D, D

    def check(self, nbest, nc, hyps):
        """hyps: the device's [(labels, score)] for this line -> (decided, worst device error / D)"""
        if self.T == 0:
            assert hyps == [], self.what
            return True, 0.0
        h64 = self.r64.hyps[:nbest]
        assert len(hyps) == len(h64), (self.what, "nhyp", len(hyps), len(h64))
        decided, D = self.gauge(nbest)
        sc = [s for _, s in hyps]
        for lab, s in hyps:
            assert len(lab) <= self.T and ((lab >= 1) & (lab < nc)).all(), (self.what, lab)
        assert all(a >= b for a, b in zip(sc, sc[1:])), (self.what, "not descending", sc)
        worst = 0.0
        if decided:
            for k, ((lab, s), (l64, s64)) in enumerate(zip(hyps, h64)):
                assert tuple(int(c) for c in lab) == l64, (self.what, k, lab, l64)
                err = abs(s - float(s64))
                print("%-30s k=%d score %+.7e f64 %+.7e err %.3g D %.3g err/D %.2f" % (self.what, k, s, s64, err, D, err / D if D else 0))
                assert err <= bar(s64), (self.what, k, s, s64)
                assert err <= max(8 * D, 16 * float(np.spacing(F32(abs(float(s64)))))), (self.what, k, s, s64, D)
                worst = max(worst, err / D if D else 0.0)
        else:
            for lab, s in hyps:
                ex = exact_loglik(self.lp64, lab)
                assert s <= ex + bar(ex), (self.what, "above the labelling's likelihood", lab, s, ex)
            assert sc[0] >= float(h64[0][1]) - bar(h64[0][1]), (self.what, "top score", sc[0], h64[0][1])
        return decided, worst


# ---- inputs and the call -----------------------------------------------------------------------------------------------------
def peaked_probs(rng, T, labels, nc, peak):
    """posteriors peaked along a linear alignment of blank-interleaved `labels` over the frames"""
    st = [0]
    for c in labels:
        st += [int(c), 0]
    st = np.asarray(st)
    pos = np.minimum(len(st) - 1, ((np.arange(T) + 0.5) * len(st) / T).astype(int))
    p = rng.dirichlet(np.ones(nc), T) * (1.0 - peak)
    p[np.arange(T), st[pos]] += peak
    return p.astype(F32)


def call_beam(backend, lines, nc, beam, nbest, want_labels=True, want_len=True):
    """lines: list of [T_b, nc] arrays -> per line [(labels, score)], and the raw arrays"""
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
    lab = np.full(max(1, nbest * N), -3, np.int32)
    backend.lib.call("clstm_ctc_beam_batch", ptr(pd), nc, ptr(lo), len(T), beam, nbest, ptr(nhyp),
                     ptr(ln) if want_len else None, ptr(sc), ptr(lab) if want_labels else None)
    return unpack_beam(T, nbest, nhyp, ln, sc, lab), (nhyp, ln, sc, lab)


def line_bytes(T, nbest, raw, b):
    """every result byte of line b"""
    nhyp, ln, sc, lab = raw
    off = int(sum(T[:b]))
    return nhyp[b:b + 1].tobytes() + ln[b * nbest:(b + 1) * nbest].tobytes() + sc[b * nbest:(b + 1) * nbest].tobytes() + \
        lab[nbest * off:nbest * (off + T[b])].tobytes()


# ---- 1. the referee, pinned by exhaustive enumeration ------------------------------------------------------------------------
EXHAUSTIVE = [(4, 3), (5, 2), (6, 2)]


def enumerate_paths(p64):
    """{labelling: log of the summed probability of every path that collapses to it}"""
    T, nc = p64.shape
    acc = {}
    for idx in np.ndindex(*([nc] * T)):
        lab, prev = [], 0
        for c in idx:
            if c != 0 and c != prev:
                lab.append(c)
            prev = c
        acc[tuple(lab)] = acc.get(tuple(lab), 0.0) + float(np.prod(p64[np.arange(T), list(idx)]))
    return {l: np.log(v) for l, v in acc.items()}


@functools.lru_cache(maxsize=None)
def exhaustive_case(T, nc, seed):
    p = np.random.default_rng(seed).dirichlet(np.full(nc, 0.5), T).astype(F32)
    return p, enumerate_paths(p.astype(F64))


@pytest.mark.parametrize("T,nc", EXHAUSTIVE)
def test_referee_is_exact_without_pruning(T, nc):
    for seed in range(20):
        p, exact = exhaustive_case(T, nc, seed)
        r = beam_ref(lp_ref(p, F64), 32, F64)
        assert r.margin == np.inf, "a 32-wide beam must not prune here"
        assert {l for l, _ in r.hyps} == set(exact)
        for l, s in r.hyps:
            assert abs(float(s) - exact[l]) <= 1e-13 * max(1.0, abs(exact[l])), (l, s, exact[l])


@pytest.mark.parametrize("T,nc", EXHAUSTIVE)
def test_every_labelling_where_nothing_is_pruned(backend, T, nc):
    cases = [exhaustive_case(T, nc, seed) for seed in range(8)]
    got, _ = call_beam(backend, [p for p, _ in cases], nc, 32, 32)
    for (p, exact), hyps in zip(cases, got):
        assert {tuple(int(c) for c in lab) for lab, _ in hyps} == set(exact) and len(hyps) == len(exact)
        sc = [s for _, s in hyps]
        assert all(a >= b for a, b in zip(sc, sc[1:]))   # (with every score inside the bar: the right order wherever the gaps allow)
        for lab, s in hyps:
            ex = exact[tuple(int(c) for c in lab)]
            assert abs(s - ex) <= bar(ex), (lab, s, ex)


# ---- 2. shape sweep ----------------------------------------------------------------------------------------------------------
#        T, nc, beam, labels, peak
SWEEP = [(1, 2, 1, 1, 0.9), (7, 5, 4, 2, 0.9), (64, 12, 32, 20, 0.8), (200, 83, 8, 40, 0.9), (40, 600, 4, 8, 0.9), (300, 5, 16, 60, 0.9)]


@functools.lru_cache(maxsize=None)
def sweep_case(T, nc, beam, L, peak):
    """8 lines of ragged length (the first of T frames), an empty line among them"""
    rng = np.random.default_rng(1000 * T + nc)
    lines = []
    for b in range(8):
        Tb = max(1, T - (b * T) // 16)
        Lb = max(1, min(L, (L * Tb) // T)) if Tb >= 3 else 0
        labels = rng.integers(1, nc, Lb)
        lines.append(Line(peaked_probs(rng, Tb, labels, nc, peak), beam, "T=%d nc=%d beam=%d line %d" % (Tb, nc, beam, b)))
    lines.insert(3, Line(np.zeros((0, nc), F32), beam, "empty line"))
    return lines


@pytest.mark.parametrize("T,nc,beam,L,peak", SWEEP)
def test_shape_sweep(backend, T, nc, beam, L, peak):
    lines = sweep_case(T, nc, beam, L, peak)
    for nbest in sorted({beam, max(1, beam // 2)}):
        undecided = [ln.what for ln in lines if ln.T and not ln.gauge(nbest)[0]]
        assert 4 * len(undecided) <= len(lines) - 1, ("the case proves too little: undecided by the referee alone", undecided)
        got, (nhyp, lens, sc, _) = call_beam(backend, [ln.probs for ln in lines], nc, beam, nbest)
        worst = 0.0
        for b, (ln, hyps) in enumerate(zip(lines, got)):
            worst = max(worst, ln.check(nbest, nc, hyps)[1])
            for k in range(len(hyps), nbest):   # unused slots
                assert lens[b * nbest + k] == 0 and sc[b * nbest + k] == -np.inf
        print("T=%d nc=%d beam=%d nbest=%d: %d of 8 undecided, worst device error / D = %.2f" % (T, nc, beam, nbest, len(undecided), worst))
    if T == 1:   # fewer entries alive than asked for
        assert all(len(h) == min(beam, nc) for h, ln in zip(got, lines) if ln.T)


def test_optional_outputs_and_counter(backend):
    from clstm_amd.abi import ClstmError
    lines = sweep_case(7, 5, 4, 2, 0.9)

    def count():
        n = C.c_longlong()
        backend.lib.call("clstm_debug_path_count", 29, C.byref(n))
        return n.value
    n0 = count()
    full = call_beam(backend, [ln.probs for ln in lines], 5, 4, 3)[1]
    bare = call_beam(backend, [ln.probs for ln in lines], 5, 4, 3, want_labels=False, want_len=False)[1]
    assert count() == n0 + 2
    assert full[0].tobytes() == bare[0].tobytes() and full[2].tobytes() == bare[2].tobytes()
    assert (bare[1] == -3).all() and (bare[3] == -3).all()
    for beam, nbest in ((0, 1), (33, 1), (4, 5), (4, 0)):
        with pytest.raises(ClstmError, match="must lie in"):
            call_beam(backend, [ln.probs for ln in lines], 5, beam, nbest)
    with pytest.raises(ClstmError, match="class count"):
        call_beam(backend, [np.ones((3, 1), F32)], 1, 2, 2)
    assert count() == n0 + 2
    call_beam(backend, [np.zeros((0, 5), F32)], 5, 4, 3)   # nothing to launch
    assert count() == n0 + 2


# ---- 3. a prefix that leaves the beam and is extended again ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trap_lines():
    """random small lines in which the referee sees the trap and which it decides"""
    out = []
    for seed in range(400):
        p = np.random.default_rng(7000 + seed).dirichlet(np.full(3, 0.5), 10).astype(F32)
        if beam_ref(lp_ref(p, F64), 3, F64).trap:
            ln = Line(p, 3, "trap seed %d" % seed)
            if ln.gauge(3)[0]:
                out.append(ln)
        if len(out) == 4:
            break
    return out


def test_reextended_prefix_is_the_same_node(backend):
    lines = trap_lines()
    assert len(lines) == 4 and all(ln.r64.trap > 0 for ln in lines), "the trap does not occur"
    got, _ = call_beam(backend, [ln.probs for ln in lines], 3, 3, 3)
    for ln, hyps in zip(lines, got):
        assert ln.check(3, 3, hyps)[0]


# ---- 4. planted truth ------------------------------------------------------------------------------------------------------
def test_planted_truth_equals_trivial_decode(backend):
    from clstm_amd.abi import i32, ptr
    nc, rng = 20, np.random.default_rng(11)
    truth = [rng.integers(1, nc, L) for L in (5, 1, 12, 8)]
    Ts = [40, 9, 90, 33]
    lines = [peaked_probs(rng, T, lab, nc, 0.99) for T, lab in zip(Ts, truth)]
    got, _ = call_beam(backend, lines, nc, 8, 2)
    lo = i32(np.concatenate([[0], np.cumsum(Ts)]))
    cls, cnt = np.zeros(sum(Ts), np.int32), np.zeros(len(Ts), np.int32)
    pd = backend.up(np.concatenate(lines, 0))
    backend.lib.call("clstm_trivial_decode_batch", ptr(pd), nc, ptr(lo), len(Ts), ptr(cls), None, ptr(cnt))
    for b, (lab, hyps) in enumerate(zip(truth, got)):
        assert hyps[0][0].tolist() == lab.tolist(), b
        assert cls[lo[b]:lo[b] + cnt[b]].tolist() == lab.tolist(), b
        assert len(hyps) == 2 and hyps[0][1] > hyps[1][1]


# ---- 5. determinism ------------------------------------------------------------------------------------------------------
def test_a_line_depends_on_nothing_but_itself(backend):
    nc, beam, nbest = 12, 8, 5
    rng = np.random.default_rng(13)
    Ts = [30, 1, 17, 64, 9]
    # flat-ish posteriors on a coarse grid: plenty of near and exact ties
    lines = [(np.round(rng.dirichlet(np.ones(nc), T) * 16 + 1) / (16 + nc)).astype(F32) for T in Ts]
    _, base = call_beam(backend, lines, nc, beam, nbest)
    ref = [line_bytes(Ts, nbest, base, b) for b in range(len(Ts))]
    _, again = call_beam(backend, lines, nc, beam, nbest)
    assert [line_bytes(Ts, nbest, again, b) for b in range(len(Ts))] == ref, "the same call twice"
    for b in range(len(Ts)):
        _, alone = call_beam(backend, [lines[b]], nc, beam, nbest)
        assert line_bytes([Ts[b]], nbest, alone, 0) == ref[b], ("line alone", b)
    perm = [3, 0, 4, 2, 1]
    _, other = call_beam(backend, [lines[b] for b in perm], nc, beam, nbest)
    for i, b in enumerate(perm):
        assert line_bytes([Ts[q] for q in perm], nbest, other, i) == ref[b], ("another order", b)
    dirty = [p.copy() for p in lines]
    dirty[2][5, 3] = np.nan
    dirty[2][6, 0] = np.inf
    got, bad = call_beam(backend, dirty, nc, beam, nbest)
    for b in range(len(Ts)):
        if b != 2:
            assert line_bytes(Ts, nbest, bad, b) == ref[b], ("beside a NaN line", b)
    for lab, _ in got[2]:
        assert len(lab) <= Ts[2] and ((lab >= 1) & (lab < nc)).all()


def test_a_line_too_long_for_lds_beside_short_ones(backend):
    """a line whose trie and class lists go to the workspace puts the launch on the kernel's other instantiation: the short
    lines' bytes are those of a launch of their own, the long line agrees with the referee"""
    nc, beam, nbest = 12, 8, 4
    rng = np.random.default_rng(17)
    Ts = [30, 700, 9]
    lines = [peaked_probs(rng, T, rng.integers(1, nc, max(1, T // 5)), nc, 0.9) for T in Ts]
    long_line = Line(lines[1], beam, "T=700 (workspace)")
    assert long_line.gauge(nbest)[0], "the long line proves too little: undecided by the referee alone"
    got, mixed = call_beam(backend, lines, nc, beam, nbest)
    _, short = call_beam(backend, [lines[0], lines[2]], nc, beam, nbest)
    assert line_bytes(Ts, nbest, mixed, 0) == line_bytes([30, 9], nbest, short, 0)
    assert line_bytes(Ts, nbest, mixed, 2) == line_bytes([30, 9], nbest, short, 1)
    assert long_line.check(nbest, nc, got[1])[0]


# ---- 6. net level ----------------------------------------------------------------------------------------------------------
NI, NH, NC = 8, [4], 5


def tiny_net(backend, seed=0.222):
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    net = Network(NI, NH, NC, lib=backend.lib)
    net.set_params(init_params(NI, NH, NC, seed=seed) * 20.0)
    net.setLearningRate(1e-2, 0.9)
    return net


def tiny_batch(seed, T=(9, 4, 13)):
    rng = np.random.default_rng(seed)
    lines = synth_lines(rng, list(T), NI)
    trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
    return lines, trs


def split(z, T):
    o = np.concatenate([[0], np.cumsum(T)])
    return [z[o[b]:o[b + 1]] for b in range(len(T))]


def same_hyps(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(
        p[0].tobytes() == q[0].tobytes() and F32(p[1]).tobytes() == F32(q[1]).tobytes() for p, q in zip(x, y)) for x, y in zip(a, b))


def test_net_beam_equals_standalone_and_counts(backend):
    net = tiny_net(backend)
    lines, _ = tiny_batch(31)
    net.set_inputs(lines)
    net.forward()
    n = C.c_longlong()
    backend.lib.call("clstm_debug_path_count", 29, C.byref(n))
    n0 = n.value
    got = net.beam(4, 3)
    backend.lib.call("clstm_debug_path_count", 29, C.byref(n))
    assert n.value == n0 + 1
    alone, _ = call_beam(backend, split(net.outputs(), net.T), NC, 4, 3)
    assert same_hyps(got, alone)
    assert all(len(h) == 3 and np.isfinite(h[0][1]) for h in got)
    assert same_hyps(net.beam(4), call_beam(backend, split(net.outputs(), net.T), NC, 4, 4)[0])   # nbest defaults to beam


def test_beam_after_predict_while_ctc_refuses(backend):
    from clstm_amd.abi import ClstmError
    net = tiny_net(backend)
    lines, trs = tiny_batch(41)
    net.predict(lines)
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)
    got = net.beam(4, 2)
    assert same_hyps(got, call_beam(backend, split(net.outputs(), net.T), NC, 4, 2)[0])
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)


def test_beam_leaves_the_training_state_alone(backend):
    from test_ctc_score import read_dz
    lines, trs = tiny_batch(43)
    got = []
    for with_beam in (False, True):
        net = tiny_net(backend)
        net.enable_input_deltas(True)
        net.set_inputs(lines)
        net.forward()
        if with_beam:
            net.beam(8, 3)
        al = net.ctc(trs, want_aligned=True)
        dz = read_dz(backend, net)
        net.backward()
        g, dx = net.get_grads(), net.input_deltas()
        net.update()
        if with_beam:
            net.beam(2)
        backend.sync()
        got.append((al, dz, g, dx, net.get_params(), net.get_derivs()))
    for name, a, b in zip(("aligned", "Dz", "grads", "input deltas", "params", "derivs"), *got):
        assert a.tobytes() == b.tobytes(), name
    assert np.abs(got[0][1]).max() > 0


def test_beam_between_training_steps_and_without_a_current_minibatch(backend):
    """a training trajectory with beam calls between the steps is bit-identical to one without; after
    clstm_net_train_step_next there is no current minibatch and the call refuses by the text of the one guard (Net::require)"""
    from clstm_amd.abi import ClstmError
    from clstm_amd.net import Network
    rng = np.random.default_rng(47)
    batches = []
    for k in range(3):
        T = [int(t) for t in rng.integers(3, 12, 3)]
        trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
        x = backend.up(np.ascontiguousarray(np.concatenate(synth_lines(rng, T, NI), 0), F32))
        batches.append((Network.prepare_step(T, trs), x, trs))
    res = []
    for disturbed in (False, True):
        net = tiny_net(backend)
        net.train_step_prepared(batches[0][0], batches[0][1], batches[1][0], batches[1][1])
        if disturbed:
            p = net.get_params()
            with pytest.raises(ClstmError, match="no current minibatch"):
                net.beam(4)
            assert net.get_params().tobytes() == p.tobytes()
        net.train_step_prepared(batches[1][0], batches[1][1])
        if disturbed:
            assert all(len(h) >= 1 for h in net.beam(4, 2))
        net.train_step_prepared(batches[2][0], batches[2][1])
        if disturbed:
            net.beam(8)
        backend.sync()
        res.append((net.get_params(), net.get_derivs()))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()


def test_net_bad_arguments_leave_the_net_alone(backend):
    from clstm_amd.abi import ClstmError, ptr
    net = tiny_net(backend)
    lines, trs = tiny_batch(53)
    net.set_inputs(lines)
    net.forward()
    z = net.outputs()
    nhyp, sc = np.zeros(3, np.int32), np.zeros(3 * 32, F32)
    for beam, nbest in ((0, 1), (33, 1), (4, 5)):
        with pytest.raises(ClstmError, match="nbest <= beam"):
            backend.lib.call("clstm_net_beam", net.h, beam, nbest, ptr(nhyp), None, ptr(sc), None)
    with pytest.raises(ClstmError, match="required"):
        backend.lib.call("clstm_net_beam", net.h, 4, 2, ptr(nhyp), None, None, None)
    fresh = tiny_net(backend)
    with pytest.raises(ClstmError, match="set_batch first"):
        backend.lib.call("clstm_net_beam", fresh.h, 4, 2, ptr(nhyp), None, ptr(sc), None)
    assert net.outputs().tobytes() == z.tobytes()
    net.ctc(trs)
    net.backward()
    backend.sync()


def test_hypotheses_feed_score_and_align(backend):
    net = tiny_net(backend)
    lines, _ = tiny_batch(61, T=(12, 7, 20))
    net.set_inputs(lines)
    net.forward()
    hyps = net.beam(4, 3)
    flat = [lab for h in hyps for lab, _ in h]
    cl = [b for b, h in enumerate(hyps) for _ in h]
    s = net.score(flat, lines=cl)
    assert np.isfinite(s).all()
    for lab, b, path in zip(flat, cl, net.align(flat, lines=cl)):
        S = 2 * len(lab) + 1
        assert len(path) == net.T[b] and path[-1] == S - 1 and ((path >= -1) & (path < S)).all()
        seen = path[path >= 0]
        assert ((np.diff(seen) == 0) | (np.diff(seen) == 1)).all()
