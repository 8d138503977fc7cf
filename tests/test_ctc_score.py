"""clstm_ctc_score_batch / clstm_net_score (clstm_amd/csrc/ctc_score.h): per-candidate scores and forced alignments.

The referee is a numpy restatement of forward_algorithm (ctc.cc:24-40) over the match scores of ctc_align_targets
(ctc.cc:66-77), in a float32 form (one rounding per operation) and a float64 form; test_referee_pin ties it to the oracle that
test_oracle_ctc.py pins to the reference's own test-ctc.cc.

Bars.  Scores are compared with the FLOAT64 referee fed the very posteriors the device was given:
    |score - s64| <= 1e-4 * max(1, |s64|)       (the same for vscore)
1e-4 relative is the project's bar (common.RTOL); the floor of 1 is there because this score passes through zero (frame 0 of
state 0 counts `same` and `next` both: a well-fitting transcript scores slightly above 0).  Every case also asserts that the
float32 REFEREE is within half that bar, so the inputs prove themselves adequate.
Paths are checked for validity, not identity: a last-bit difference in a match score may legitimately flip a near-tie.
"""
import ctypes as C

import numpy as np
import pytest

from common import RTOL, synth_lines

SKIP = -5.0
F32, F64 = np.float32, np.float64


# ---- the referee -------------------------------------------------------------------------------------------------------------
def lmatch_ref(probs, classes, dt):
    """log(out_t[class_s]), out_t = max(1e-5, p_t) / sum (sequential sum in class order, as asum1)"""
    p = np.asarray(probs, F32).astype(dt)
    with np.errstate(invalid="ignore"):
        x = np.maximum(dt(1e-5), p)                      # (np.maximum keeps a NaN)
        tot = np.cumsum(x, axis=1, dtype=dt)[:, -1:]     # cumsum accumulates sequentially in dt
        out = (x / tot).astype(dt)
        return np.log(out.astype(F64)).astype(dt)[:, np.asarray(classes, np.int64)]


def log_add(x, y, dt):
    """tensor.h:86-89: |x - y| > 10 -> max, else log(exp(x - y) + 1) + y, every operation rounded to dt"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - y).astype(dt)
        e = np.exp(np.clip(d, -20, 20).astype(F64)).astype(dt)
        lg = (np.log((e + dt(1)).astype(dt).astype(F64)).astype(dt) + y).astype(dt)
        return np.where(np.abs(d) > 10, np.maximum(x, y), lg).astype(dt)


def forward_ref(lm, dt, maxplus=False, lattice=False):
    """forward_algorithm: -> last cell (and the whole lattice / the back-pointers when asked)"""
    T, S = lm.shape
    v = (dt(SKIP) * np.arange(S)).astype(dt)
    lr = np.zeros((T, S), dt)
    for i in range(T):
        w = np.concatenate([[dt(SKIP * i)], v[:-1]]).astype(dt)
        same, nxt = (v + lm[i]).astype(dt), (w + lm[i]).astype(dt)
        v = np.where(nxt > same, nxt, same).astype(dt) if maxplus else log_add(same, nxt, dt)
        lr[i] = v
    return (v[-1], lr) if lattice else v[-1]


def path_score(path, lm64):
    """the score of a path by the rule of the header: its match scores + one boundary term; asserts its validity"""
    T, S = lm64.shape
    path = np.asarray(path)
    assert path.shape == (T,)
    assert ((path >= -1) & (path < S)).all(), "entries outside [-1, S)"
    i0 = int((path == -1).sum())
    assert (path[:i0] == -1).all() and (path[i0:] >= 0).all(), "-1 is not a prefix"
    assert i0 < T
    if i0 > 0:
        assert path[i0] == 0, "a late start must enter state 0"
    st = np.diff(path[i0:])
    assert ((st == 0) | (st == 1)).all(), "steps are 0 or 1"
    assert path[-1] == S - 1, "the path ends in the last state"
    body = lm64[np.arange(i0, T), path[i0:]].sum()
    return body + (SKIP * i0 if i0 > 0 else SKIP * max(int(path[0]) - 1, 0))


def bar(s64):
    return RTOL * max(1.0, abs(float(s64)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def states_for(rng, S, nc):
    """blank on the even states, a label on the odd ones (mktargets' shape; an even S ends on a label)"""
    cls = np.zeros(S, np.int32)
    cls[1::2] = rng.integers(1, nc, len(cls[1::2]))
    return cls


def peaked_probs(rng, T, classes, nc, peak=0.9):
    """posteriors peaked along a plausible (linear) alignment of the states over the frames"""
    S = len(classes)
    st = np.minimum(S - 1, ((np.arange(T) + 0.5) * S / T).astype(int))
    p = rng.dirichlet(np.ones(nc), T) * (1.0 - peak)
    p[np.arange(T), np.asarray(classes)[st]] += peak
    return p.astype(F32)


def call_score(backend, probs, nc, line_off, states, state_off, cand_line, ncand, want=(True, True, True), npath=None):
    from clstm_amd.abi import i32, ptr
    pd = backend.up(probs if len(probs) else np.zeros((1, nc), F32))
    lo, so = i32(line_off), i32(state_off)
    T = np.diff(lo)
    if npath is None:
        npath = int(sum(T[b] for b in (cand_line if cand_line is not None else range(ncand))))
    score = np.full(ncand, 123.0, F32) if want[0] else None
    vscore = np.full(ncand, 123.0, F32) if want[1] else None
    path = np.full(max(1, npath), -7, np.int32) if want[2] else None
    backend.lib.call("clstm_ctc_score_batch", ptr(pd), nc, ptr(lo), len(lo) - 1, ptr(i32(states)), ptr(so),
                     ptr(i32(cand_line)) if cand_line is not None else None, ncand, ptr(score), ptr(vscore), ptr(path))
    return score, vscore, path


class Case:
    """one (line, candidate) item and its referee figures (computed once, shared by the backends)"""

    def __init__(self, probs, classes, what):
        self.probs, self.classes, self.what = probs, np.asarray(classes, np.int32), what
        self.T, self.S = len(probs), len(classes)
        if self.T:
            self.lm64 = lmatch_ref(probs, classes, F64)
            lm32 = lmatch_ref(probs, classes, F32)
            self.s64, self.v64 = forward_ref(self.lm64, F64), forward_ref(self.lm64, F64, maxplus=True)
            self.s32, self.v32 = forward_ref(lm32, F32), forward_ref(lm32, F32, maxplus=True)

    def check(self, score, vscore, path):
        w = self.what
        if self.T == 0:
            assert score == -np.inf and vscore == -np.inf, w
            return 0.0
        # the inputs prove themselves adequate: the float32 referee sits within half the bar
        assert abs(float(self.s32) - self.s64) <= 0.5 * bar(self.s64), (w, "referee", self.s32, self.s64)
        assert abs(float(self.v32) - self.v64) <= 0.5 * bar(self.v64), (w, "referee (max-plus)", self.v32, self.v64)
        ds, dv = abs(float(score) - self.s64), abs(float(vscore) - self.v64)
        print("%-28s score %+.6e (f64 %+.6e, dev %.3g = %.3f bar)  vscore dev %.3g = %.3f bar" % (
            w, score, self.s64, ds, ds / bar(self.s64), dv, dv / bar(self.v64)))
        assert ds <= bar(self.s64), (w, "score", score, self.s64)
        assert dv <= bar(self.v64), (w, "vscore", vscore, self.v64)
        ps = path_score(path, self.lm64)
        assert abs(ps - self.v64) <= bar(self.v64), (w, "path score vs optimum", ps, self.v64)
        assert abs(ps - float(vscore)) <= bar(self.v64), (w, "path score vs vscore", ps, vscore)
        return max(ds / bar(self.s64), dv / bar(self.v64))


def run_cases(backend, cases, nc, cand_line=None, lines=None):
    """cases as ONE call; lines: the distinct lines' posteriors when several candidates share one (cand_line)"""
    if lines is None:
        lines = [c.probs for c in cases]
    line_off = np.concatenate([[0], np.cumsum([len(p) for p in lines])])
    state_off = np.concatenate([[0], np.cumsum([c.S for c in cases])])
    probs = np.concatenate([p.reshape(-1, nc) for p in lines], 0)
    states = np.concatenate([c.classes for c in cases])
    score, vscore, path = call_score(backend, probs, nc, line_off, states, state_off, cand_line, len(cases))
    worst, o = 0.0, 0
    for k, c in enumerate(cases):
        worst = max(worst, c.check(score[k], vscore[k], path[o:o + c.T]))
        o += c.T
    assert o == 0 or (path[o:] == -7).all()
    return worst


# ---- 1. the referee is the oracle's recursion ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L,nc", [(40, 3, 5), (64, 32, 12), (7, 3, 5)])
def test_referee_pin(ora32, T, L, nc):
    """float32 referee: forward lattice + reversed lattice, pushed through steps C-E of ctc_align_targets (ctc.cc:82-109) in numpy,
    against ora32.ctc_align_classes"""
    rng = np.random.default_rng(100 + T)
    classes = np.zeros(2 * L + 1, np.int32)
    classes[1::2] = rng.integers(1, nc, L)
    probs = peaked_probs(rng, T, classes, nc, peak=0.7)
    lm = lmatch_ref(probs, classes, F32)
    lr = forward_ref(lm, F32, lattice=True)[1]
    rl = forward_ref(lm[::-1, ::-1], F32, lattice=True)[1][::-1, ::-1]
    both = (lr + rl).astype(F32)
    epath = np.exp(np.clip((both - both.max()).astype(F32), -30, 30).astype(F64)).astype(F32)
    epath = (epath / np.maximum(1e-9, epath.astype(F64).sum(0))).astype(F32)
    aligned = np.zeros((T, nc), F64)
    for s, c in enumerate(classes):
        aligned[:, c] += epath[:, s]
    aligned = aligned.astype(F32)
    aligned = (aligned / np.maximum(aligned.astype(F64).sum(1, keepdims=True), 1e-9)).astype(F32)
    want = ora32.ctc_align_classes(probs, classes)
    dev = np.abs(aligned - want).max()
    print("referee vs oracle at (T, L, nc) = (%d, %d, %d): %.3g" % (T, L, nc, dev))
    assert dev <= 1e-5


# ---- 2. the reference's identity case ---------------------------------------------------------------------------------------
def test_known_answer(backend):
    """test-ctc.cc:47-74: T = 4, nc = 3, frames one-hot 0, 1, 2, 2, states [0, 1, 2]"""
    probs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]], F32)
    c = Case(probs, [0, 1, 2], "identity")
    score, vscore, path = call_score(backend, probs, 3, [0, 4], c.classes, [0, 3], None, 1)
    assert path.tolist() == [0, 1, 2, 2]
    c.check(score[0], vscore[0], path)


# ---- 3. the shape sweep ----------------------------------------------------------------------------------------------------
SWEEP_S = [1, 2, 7, 63, 64, 65, 128, 129, 512, 513, 2048, 2049]
SWEEP_T = [1, 3, 40]
_sweep_cache = {}


def sweep_cases(nc):
    if nc not in _sweep_cache:
        rng = np.random.default_rng(1000 + nc)
        cases = []
        for S in SWEEP_S:
            for T in SWEEP_T:
                cls = states_for(rng, S, nc)
                cases.append(Case(peaked_probs(rng, T, cls, nc), cls, "S=%d T=%d nc=%d" % (S, T, nc)))
        if nc == 101:   # the bench line's lattice
            cls = states_for(rng, 51, nc)
            cases.append(Case(peaked_probs(rng, 200, cls, nc), cls, "S=51 T=200 nc=101"))
        _sweep_cache[nc] = cases
    return _sweep_cache[nc]


@pytest.mark.parametrize("nc", [2, 5, 101, 600])
def test_shape_sweep(backend, nc):
    """every S class edge x T in {1, 3, 40} (T < S: the path must start at j0 > 0), one item per line, one call per class count"""
    cases = sweep_cases(nc)
    worst = run_cases(backend, cases, nc)
    print("nc = %d: largest deviation %.3f of the bar over %d items" % (nc, worst, len(cases)))
    # each item alone gives the bytes it gave in the batch (grouping and sorting do not reach the arithmetic)
    for c in (cases[0], cases[17], cases[-2]):
        s1, v1, p1 = call_score(backend, c.probs, nc, [0, c.T], c.classes, [0, c.S], None, 1)
        c.check(s1[0], v1[0], p1)


def test_late_start_and_other_paths_of_the_code(backend):
    """a line whose first frames fit no state of the transcript: the best path enters state 0 late (a prefix of -1) -- on each
    form; more classes than the LDS tile of the normalisers holds (sums straight from memory); more frames than the one-wave
    form's LDS carve holds (a short transcript on the register form); a one-wave item too large for the LDS table of match scores"""
    nc = 6
    rng = np.random.default_rng(11)
    for S in (3, 70, 2100):
        T = S + 12
        cls = states_for(rng, S, nc - 1)            # class nc - 1 is in no transcript
        probs = peaked_probs(rng, T - 5, cls, nc, peak=0.99)
        junk = np.full((5, nc), 1e-6, F32)
        junk[:, nc - 1] = 1.0
        probs = np.concatenate([junk, probs], 0)
        c = Case(probs, cls, "late start S=%d" % S)
        s, v, p = call_score(backend, probs, nc, [0, T], cls, [0, S], None, 1)
        c.check(s[0], v[0], p)
        assert p[0] == -1 and (p == -1).sum() == 5, p[:8]
    nc = 8300
    cls = states_for(rng, 7, nc)
    c = Case(peaked_probs(rng, 5, cls, nc), cls, "nc=8300")
    c.check(*[x[0] if k < 2 else x for k, x in enumerate(call_score(backend, c.probs, nc, [0, 5], cls, [0, 7], None, 1))])
    nc = 4
    cls = states_for(rng, 30, nc)   # T S floats beyond the LDS table of match scores: one-wave form, logarithm in the step
    c = Case(peaked_probs(rng, 1000, cls, nc), cls, "T=1000 S=30")
    c.check(*[x[0] if k < 2 else x for k, x in enumerate(call_score(backend, c.probs, nc, [0, 1000], cls, [0, 30], None, 1))])
    cls = states_for(rng, 9, nc)
    c = Case(peaked_probs(rng, 1030, cls, nc), cls, "T=1030")
    c.check(*[x[0] if k < 2 else x for k, x in enumerate(call_score(backend, c.probs, nc, [0, 1030], cls, [0, 9], None, 1))])


def test_mixed_call(backend):
    """a ragged batch of 3 lines, one of them without frames; 7 candidates in shuffled line order; 5 / 65 / 300 states on one line,
    the empty transcript (S = 1) among them"""
    nc = 12
    rng = np.random.default_rng(7)
    Ts = [40, 0, 25]
    spec = [(0, 65), (2, 7), (1, 3), (0, 300), (2, 129), (0, 1), (0, 5)]   # (line, S)
    lines = [None] * 3
    cases = []
    for b, S in spec:
        cls = states_for(rng, S, nc)
        if lines[b] is None:
            lines[b] = peaked_probs(rng, Ts[b], cls if S > 3 else states_for(rng, 9, nc), nc, peak=0.6) if Ts[b] else np.zeros((0, nc), F32)
        cases.append(Case(lines[b], cls, "line %d S=%d" % (b, S)))
    worst = run_cases(backend, cases, nc, cand_line=[b for b, _ in spec], lines=lines)
    print("mixed call: largest deviation %.3f of the bar" % worst)
    # the outputs are optional one by one
    line_off = np.concatenate([[0], np.cumsum(Ts)])
    state_off = np.concatenate([[0], np.cumsum([c.S for c in cases])])
    args = (np.concatenate(lines, 0), nc, line_off, np.concatenate([c.classes for c in cases]), state_off, [b for b, _ in spec], 7)
    full = call_score(backend, *args)
    s_only = call_score(backend, *args, want=(True, False, False))
    v_only = call_score(backend, *args, want=(False, True, False))
    p_only = call_score(backend, *args, want=(False, False, True))
    assert s_only[0].tobytes() == full[0].tobytes() and s_only[1] is None and s_only[2] is None
    assert v_only[1].tobytes() == full[1].tobytes()
    assert p_only[2].tobytes() == full[2].tobytes()


def test_counter_and_refusals_standalone(backend):
    from clstm_amd.abi import ClstmError
    nc = 5
    rng = np.random.default_rng(3)
    cls = states_for(rng, 7, nc)
    probs = peaked_probs(rng, 9, cls, nc)

    def count():
        n = C.c_longlong()
        backend.lib.call("clstm_debug_path_count", 28, C.byref(n))
        return n.value
    n0 = count()
    call_score(backend, probs, nc, [0, 9], cls, [0, 7], None, 1, want=(True, False, False))
    assert count() == n0 + 1
    call_score(backend, probs, nc, [0, 9], cls, [0, 7], None, 1)
    assert count() == n0 + 3
    with pytest.raises(ClstmError, match="all NULL"):
        call_score(backend, probs, nc, [0, 9], cls, [0, 7], None, 1, want=(False, False, False))
    with pytest.raises(ClstmError, match="cand_line out of range"):
        call_score(backend, probs, nc, [0, 9], cls, [0, 7], [1], 1, npath=9)
    with pytest.raises(ClstmError, match="class out of range"):
        call_score(backend, probs, nc, [0, 9], [0, 5, 0], [0, 3], None, 1)
    assert count() == n0 + 3


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


class _DevArray:
    def __init__(self, address, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (address, False), "version": 2}


def read_dz(backend, net):
    """the bytes of the net's output-delta block"""
    n = net.N * net.nclasses
    _, d = net.device_outputs()
    backend.sync()
    if backend.kind == "emu":
        return np.array((C.c_float * n).from_address(d), F32)
    return backend.torch.as_tensor(_DevArray(d, n), device="cuda").cpu().numpy().copy()


def mk_states(tr):
    """mktargets (ctc.cc:148-157)"""
    st = np.zeros(2 * len(tr) + 1, np.int32)
    st[1::2] = tr
    return st


def standalone_on(backend, z, T, trs, cand_line=None):
    st = [mk_states(t) for t in trs]
    so = np.concatenate([[0], np.cumsum([len(s) for s in st])])
    lo = np.concatenate([[0], np.cumsum(T)])
    return call_score(backend, z, z.shape[1], lo, np.concatenate(st), so, cand_line, len(trs))


def test_net_score_equals_standalone(backend):
    from clstm_amd.net import spans
    net = tiny_net(backend)
    lines, trs = tiny_batch(31)
    net.set_inputs(lines)
    net.forward()
    z = net.outputs()
    s, v = net.score(trs, viterbi=True)
    paths = net.align(trs)
    s1, v1, p1 = standalone_on(backend, z, net.T, trs)
    assert s.tobytes() == s1.tobytes() and v.tobytes() == v1.tobytes()
    assert np.concatenate(paths).tobytes() == p1.tobytes()
    assert np.isfinite(s).all() and np.isfinite(v).all()
    for b, tr in enumerate(trs):
        Case(z[sum(net.T[:b]):sum(net.T[:b + 1])], mk_states(tr), "net line %d" % b).check(
            s[b], v[b], paths[b])
        sp = spans(paths[b], len(tr))
        assert len(sp) == len(tr)
        seen = [x for x in sp if x != (-1, -1)]
        assert all(0 <= f <= l < net.T[b] for f, l in seen)
        assert all(a[1] < b_[0] for a, b_ in zip(seen, seen[1:])), "labels occupy disjoint, ordered frame ranges"
    assert spans([0, 0, 1, 1, 2, 4, 4], 3) == [(2, 3), (-1, -1), (-1, -1)]
    assert spans([-1, 0, 1, 2, 3, 3, 4], 2) == [(2, 2), (4, 5)]


def test_k_candidates_equal_single_calls(backend):
    net = tiny_net(backend)
    lines, _ = tiny_batch(37)
    net.set_inputs(lines)
    net.forward()
    rng = np.random.default_rng(5)
    K = 4
    cands = [[rng.integers(1, NC, int(rng.integers(0, 4))).astype(np.int32) for _ in range(K)] for _ in net.T]
    flat = [c for per in cands for c in per]
    cl = [b for b in range(len(net.T)) for _ in range(K)]
    s, v = net.score(flat, lines=cl, viterbi=True)
    paths = net.align(flat, lines=cl)
    for k in range(K):
        s1, v1 = net.score([cands[b][k] for b in range(len(net.T))], viterbi=True)
        p1 = net.align([cands[b][k] for b in range(len(net.T))])
        for b in range(len(net.T)):
            i = b * K + k
            assert s[i].tobytes() == s1[b].tobytes() and v[i].tobytes() == v1[b].tobytes(), (b, k)
            assert paths[i].tobytes() == p1[b].tobytes(), (b, k)


def test_score_after_predict_while_ctc_refuses(backend):
    from clstm_amd.abi import ClstmError
    net = tiny_net(backend)
    lines, trs = tiny_batch(41)
    net.predict(lines)
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)
    s = net.score(trs)
    s1 = standalone_on(backend, net.outputs(), net.T, trs)[0]
    assert np.isfinite(s).all() and s.tobytes() == s1.tobytes()
    with pytest.raises(ClstmError, match="clstm_net_ctc"):
        net.ctc(trs)


def test_score_leaves_the_training_state_alone(backend):
    lines, trs = tiny_batch(43)
    got = []
    for with_score in (False, True):
        net = tiny_net(backend)
        net.enable_input_deltas(True)
        net.set_inputs(lines)
        net.forward()
        if with_score:
            net.score([trs[2], trs[0], trs[0]], lines=[0, 1, 2], viterbi=True)
            net.align(trs)
        al = net.ctc(trs, want_aligned=True)
        dz = read_dz(backend, net)
        net.backward()
        g, dx = net.get_grads(), net.input_deltas()
        net.update()
        backend.sync()
        got.append((al, dz, g, dx, net.get_params(), net.get_derivs()))
    for name, a, b in zip(("aligned", "Dz", "grads", "input deltas", "params", "derivs"), *got):
        assert a.tobytes() == b.tobytes(), name
    assert np.abs(got[0][1]).max() > 0


def test_score_refuses_without_a_current_minibatch_and_training_goes_on(backend):
    """clstm_net_train_step_next leaves no current minibatch: score refuses by the text of the one guard (Net::require); a bad call after a forward is
    refused too, a good one accepted; the training step that follows gives the parameters of an undisturbed run"""
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
                net.score(batches[0][2])
            assert net.get_params().tobytes() == p.tobytes()
        # the declared minibatch is consumed by the next step (its prepared alignment must have survived)
        net.train_step_prepared(batches[1][0], batches[1][1])
        if disturbed:
            with pytest.raises(ClstmError, match="cand_line out of range"):
                net.score(batches[1][2], lines=[0, 1, 3])
            assert np.isfinite(net.score(batches[1][2])).all()
        net.train_step_prepared(batches[2][0], batches[2][1])
        backend.sync()
        res.append((net.get_params(), net.get_derivs()))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()


def test_net_bad_arguments_leave_the_net_alone(backend):
    from clstm_amd.abi import ClstmError, i32, ptr
    net = tiny_net(backend)
    lines, trs = tiny_batch(53)
    net.set_inputs(lines)
    net.forward()
    z = net.outputs()
    L, lab = i32([len(t) for t in trs]), i32(np.concatenate(trs))
    out = np.zeros(3, F32)
    with pytest.raises(ClstmError, match="all NULL"):
        backend.lib.call("clstm_net_score", net.h, ptr(lab), ptr(L), None, 3, None, None, None)
    with pytest.raises(ClstmError, match="cand_line out of range"):
        backend.lib.call("clstm_net_score", net.h, ptr(lab), ptr(L), ptr(i32([0, -1, 2])), 3, ptr(out), None, None)
    bad = lab.copy()
    bad[0] = NC
    with pytest.raises(ClstmError, match="class out of range"):
        backend.lib.call("clstm_net_score", net.h, ptr(bad), ptr(L), None, 3, ptr(out), None, None)
    assert net.outputs().tobytes() == z.tobytes()
    net.ctc(trs)
    net.backward()
    backend.sync()


# ---- 7. non-finite posteriors ------------------------------------------------------------------------------------------------
def test_nan_posterior_stays_in_its_line(backend):
    nc = 12
    rng = np.random.default_rng(59)
    Ts = [30, 20, 40]
    spec = [(0, 7), (1, 65), (1, 9), (2, 11), (0, 130), (1, 1), (2, 2100)]
    lines = [peaked_probs(rng, T, states_for(rng, 9, nc), nc, peak=0.6) for T in Ts]
    cls = [states_for(rng, S, nc) for _, S in spec]
    line_off = np.concatenate([[0], np.cumsum(Ts)])
    state_off = np.concatenate([[0], np.cumsum([len(c) for c in cls])])
    cl = [b for b, _ in spec]
    clean = call_score(backend, np.concatenate(lines, 0), nc, line_off, np.concatenate(cls), state_off, cl, len(spec))
    dirty_lines = [p.copy() for p in lines]
    dirty_lines[1][11, 4] = np.nan
    dirty = call_score(backend, np.concatenate(dirty_lines, 0), nc, line_off, np.concatenate(cls), state_off, cl, len(spec))
    o = 0
    for k, (b, S) in enumerate(spec):
        T = Ts[b]
        if b == 1:
            assert not np.isfinite(dirty[0][k]) and not np.isfinite(dirty[1][k]), (k, dirty[0][k], dirty[1][k])
        else:
            assert np.isfinite(clean[0][k])
            assert dirty[0][k].tobytes() == clean[0][k].tobytes() and dirty[1][k].tobytes() == clean[1][k].tobytes(), k
            assert dirty[2][o:o + T].tobytes() == clean[2][o:o + T].tobytes(), k
        assert ((dirty[2][o:o + T] >= -1) & (dirty[2][o:o + T] < S)).all(), k
        o += T
