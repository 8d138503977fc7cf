"""clstm_edit_distance_batch / clstm_net_errors (clstm_amd/csrc/edit_distance.h): unit-cost Levenshtein distance, the canonical
edit script, its counts and the confusion table, batched on the device.

The referee is the full table in numpy with the tie rule of the header: from (la, lb), diagonal if it explains D[i][j], else up (an
insertion: a hypothesis symbol), else left (a deletion: a reference symbol).  Every comparison is of exact integers: there is no
tolerance anywhere.  Shapes are the smallest that reach a path -- strip edges at 63 / 64 / 65 / 127 / 128 / 129, the thresholds of
the LDS carve asked from clstm_debug_edit_plan -- because the emulator runs one fiber per GPU thread.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from common import synth_lines

SENTINEL = -7


# ---- the referee -------------------------------------------------------------------------------------------------------------
def levenshtein(a, b):
    """the form of tests/test_corpus_decode.py (the reference's clstm.h:329-351)"""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def ref_edit(h, r):
    """-> (distance, script codes in forward order): 0 match, 1 substitution, 2 insertion, 3 deletion"""
    h, r = np.asarray(h, np.int64), np.asarray(r, np.int64)
    la, lb = len(h), len(r)
    ar = np.arange(lb + 1)
    D = np.zeros((la + 1, lb + 1), np.int64)
    D[0] = ar
    for i in range(1, la + 1):
        t = np.minimum(D[i - 1, :-1] + (r != h[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(np.concatenate([[i], t]) - ar) + ar   # D[i][j] = min(t[j], D[i][j-1] + 1), unrolled
    ops, i, j = [], la, lb
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1, j - 1] + (h[i - 1] != r[j - 1]) == D[i, j]:
            ops.append(int(h[i - 1] != r[j - 1]))
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1, j] + 1 == D[i, j]:
            ops.append(2)
            i -= 1
        else:
            assert j > 0 and D[i, j - 1] + 1 == D[i, j]
            ops.append(3)
            j -= 1
    return int(D[la, lb]), ops[::-1]


def ref_counts(ops):
    return [ops.count(1), ops.count(2), ops.count(3)]


def ref_confusion(pairs, nsym):
    """pairs: [(h, r, ops)]"""
    conf = np.zeros((nsym, nsym), np.int64)
    for h, r, ops in pairs:
        i = j = 0
        for op in ops:
            if op <= 1:
                conf[r[j], h[i]] += 1
                i, j = i + 1, j + 1
            elif op == 2:
                conf[0, h[i]] += 1
                i += 1
            else:
                conf[r[j], 0] += 1
                j += 1
        assert i == len(h) and j == len(r)
    return conf


def test_referee_is_the_reference_distance():
    rng = np.random.default_rng(1)
    pairs = [([], []), ([1], []), ([], [2, 2]), ([1, 2, 1], [2, 1, 2]), ([3, 1, 4, 1, 5], [3, 1, 4, 1, 5])]
    pairs += [(rng.integers(1, 4, rng.integers(0, 40)).tolist(), rng.integers(1, 4, rng.integers(0, 40)).tolist()) for _ in range(20)]
    for h, r in pairs:
        d, ops = ref_edit(h, r)
        assert d == levenshtein(h, r) == levenshtein(r, h) == sum(ref_counts(ops))
        assert len(ops) - ops.count(3) == len(h) and len(ops) - ops.count(2) == len(r)


# ---- the call ----------------------------------------------------------------------------------------------------------------
def pack(seqs):
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int32)
    flat = np.asarray([c for x in seqs for c in x] or [0], np.int32)
    return flat, off


def plan_of(backend, la, lb, script):
    """clstm_debug_edit_plan: [strips, directions 0 none / 1 LDS / 2 workspace, edge 0 / 1 / 2, words per column, LDS words]"""
    p = (C.c_int * 5)()
    backend.lib.call("clstm_debug_edit_plan", int(la), int(lb), int(script), p)
    return list(p)


def path_count(backend, which):
    n = C.c_longlong()
    backend.lib.call("clstm_debug_path_count", which, C.byref(n))
    return n.value


def counter(backend):
    return path_count(backend, 31)


class Result:
    pass


def call_edit(backend, hyps, refs, ref_of=None, nsym=4, want=("dist", "counts", "nops", "ops", "conf"), raw_args=None, keep=None):
    """-> Result with the raw arrays (SENTINEL where not asked for) and per pair the script"""
    from clstm_amd.abi import i32, ptr
    hyp, hoff = pack(hyps)
    ref, roff = pack(refs)
    n = len(hyps)
    ro = None if ref_of is None else i32(ref_of)
    lb = [len(refs[q]) for q in (range(n) if ref_of is None else ref_of)] if raw_args is None else [0] * n
    res = Result()
    res.dist = np.full(max(1, n), SENTINEL, np.int32)
    res.counts = np.full(max(1, 3 * n), SENTINEL, np.int32)
    res.nops = np.full(max(1, n), SENTINEL, np.int32)
    res.ops = np.full(max(1, int(hoff[-1]) + sum(lb)), SENTINEL, np.int32)
    res.conf = np.full(nsym * nsym if 0 < nsym < 4096 else 1, SENTINEL, np.int32)
    out = [ptr(getattr(res, k)) if k in want else None for k in ("dist", "counts", "nops", "ops", "conf")]
    args = dict(hyp=ptr(hyp), hoff=ptr(hoff), n=n, ref=ptr(ref), roff=ptr(roff), nref=len(refs), ro=ptr(ro), nsym=nsym)
    args.update(raw_args or {})
    if keep is not None:
        keep.append(res)   # (a refused call: the arrays stay in sight)
    backend.lib.call("clstm_edit_distance_batch", args["hyp"], args["hoff"], args["n"], args["ref"], args["roff"], args["nref"],
                     args["ro"], args["nsym"], *out)
    res.starts = (hoff[:-1].astype(np.int64) + np.concatenate([[0], np.cumsum(lb)[:-1]])).astype(np.int64) if n else []
    res.lb = lb
    return res


def scripts_of(res):
    return [res.ops[int(s):int(s) + int(k)].tolist() for s, k in zip(res.starts, res.nops)]


def check_against_referee(res, hyps, refs, ref_of=None, nsym=None, what=""):
    n = len(hyps)
    got = scripts_of(res)
    done = []
    for p in range(n):
        r = refs[p if ref_of is None else ref_of[p]]
        d, ops = cached_ref(tuple(hyps[p]), tuple(r))
        assert res.dist[p] == d, (what, p, len(hyps[p]), len(r), res.dist[p], d)
        assert res.counts[3 * p:3 * p + 3].tolist() == ref_counts(ops), (what, p, res.counts[3 * p:3 * p + 3], ref_counts(ops))
        assert res.nops[p] == len(ops) and got[p] == ops, (what, p, "script", len(hyps[p]), len(r))
        # the slots of the pair beyond its script are the caller's
        s, cap = int(res.starts[p]), len(hyps[p]) + len(r)
        assert (res.ops[s + len(ops):s + cap] == SENTINEL).all(), (what, p, "slots beyond the script")
        done.append((hyps[p], r, ops))
    if nsym is not None:
        assert np.array_equal(res.conf.reshape(nsym, nsym), ref_confusion(done, nsym)), (what, "confusion")


@functools.lru_cache(maxsize=None)
def cached_ref(h, r):
    return ref_edit(h, r)


# ---- 1. exhaustive over {1, 2}, lengths 0 .. 4 ---------------------------------------------------------------------------------
def test_exhaustive_two_symbols(backend):
    seqs = [list(s) for L in range(5) for s in itertools.product((1, 2), repeat=L)]
    assert len(seqs) == 31
    hyps = [h for h in seqs for _ in seqs]
    refs = [r for _ in seqs for r in seqs]
    res = call_edit(backend, hyps, refs, nsym=3)
    check_against_referee(res, hyps, refs, nsym=3, what="exhaustive")


# ---- 2. strip edges --------------------------------------------------------------------------------------------------------
EDGES = (0, 1, 63, 64, 65, 127, 128, 129)


def planted(rng, ref, la, nsym):
    """a hypothesis of la symbols made from `ref` by a few edits: small distances against long equal runs"""
    h = list(ref)
    for _ in range(3):
        if h:
            h[int(rng.integers(len(h)))] = int(rng.integers(1, nsym))
    while len(h) > la:
        del h[int(rng.integers(len(h)))]
    while len(h) < la:
        h.insert(int(rng.integers(len(h) + 1)), int(rng.integers(1, nsym)))
    return h


@functools.lru_cache(maxsize=None)
def strip_case(nsym):
    rng = np.random.default_rng(100 + nsym)
    hyps, refs = [], []
    for la in EDGES:
        for lb in EDGES:
            r = rng.integers(1, nsym, lb).tolist()
            hyps += [rng.integers(1, nsym, la).tolist(), planted(rng, r, la, nsym)]
            refs += [r, r]
    return hyps, refs


@pytest.mark.parametrize("nsym", [4, 81])   # 3 and 80 symbols
def test_strip_edges(backend, nsym):
    hyps, refs = strip_case(nsym)
    strips = {plan_of(backend, len(h), len(r), 1)[0] for h, r in zip(hyps, refs)}
    assert {1, 2, 3} <= strips, strips
    assert any(plan_of(backend, len(h), len(r), 1)[1:3] == [1, 1] for h, r in zip(hyps, refs))   # directions and edge column in LDS
    res = call_edit(backend, hyps, refs, nsym=nsym)
    check_against_referee(res, hyps, refs, nsym=nsym, what="strip edges, %d symbols" % (nsym - 1))
    small = [p for p, (h, r) in enumerate(zip(hyps, refs)) if p % 2 == 1 and len(h) == len(r) >= 63]
    assert small and all(res.dist[p] <= 3 for p in small)   # the planted pairs of equal length: long equal runs


# ---- 3. beyond the LDS carve -------------------------------------------------------------------------------------------------
def first_workspace_square(backend):
    """the smallest la = lb whose directions the plan sends to the workspace"""
    n = 1
    while plan_of(backend, n, n, 1)[1] != 2:
        n += 1
        assert n < 4096
    return n


def first_workspace_edge(backend):
    """the smallest la whose edge column (two strips: lb = 65) the plan sends to the workspace"""
    la = 1
    while plan_of(backend, la, 65, 0)[2] != 2:
        la *= 2
        assert la < (1 << 20)
    lo = la // 2
    while lo + 1 < la:   # (the rule is monotone in la)
        mid = (lo + la) // 2
        lo, la = (lo, mid) if plan_of(backend, mid, 65, 0)[2] == 2 else (mid, la)
    return la


@functools.lru_cache(maxsize=None)
def long_pairs(n_dirs, la_edge):
    rng = np.random.default_rng(7)
    r1 = rng.integers(1, 4, n_dirs).tolist()
    r2 = rng.integers(1, 4, 65).tolist()
    hyps = [[1, 2, 3], planted(rng, r1, n_dirs, 4), [], rng.integers(1, 4, la_edge).tolist(), [2, 2]]
    refs = [[1, 3], r1, [3], r2, [2, 1, 2]]
    return hyps, refs


def test_beyond_the_lds_carve(backend):
    n, la = first_workspace_square(backend), first_workspace_edge(backend)
    assert plan_of(backend, n - 1, n - 1, 1)[1] == 1 and plan_of(backend, n, n, 1)[1] == 2
    assert plan_of(backend, la - 1, 65, 1)[2] == 1 and plan_of(backend, la, 65, 1)[2] == 2
    assert plan_of(backend, n, n, 0)[1] == 0 and plan_of(backend, n, n, 0)[4] <= 4096
    hyps, refs = long_pairs(n, la)
    res = call_edit(backend, hyps, refs, nsym=4)
    check_against_referee(res, hyps, refs, nsym=4, what="workspace directions / edge")
    bare = call_edit(backend, hyps, refs, nsym=4, want=("dist",))
    assert np.array_equal(bare.dist, res.dist)
    for k in ("counts", "nops", "ops", "conf"):
        assert (getattr(bare, k) == SENTINEL).all(), k


# ---- 4. the ref_of form ------------------------------------------------------------------------------------------------------
def test_ref_of_form(backend):
    from clstm_amd.abi import ClstmError
    rng = np.random.default_rng(11)
    refs = [rng.integers(1, 6, int(L)).tolist() for L in (12, 0, 70, 5, 33, 64, 1, 20)]
    ref_of = [int(q) for q in rng.permutation(np.repeat(np.arange(8), 5))]
    assert any(a > b for a, b in zip(ref_of, ref_of[1:]))
    hyps = [planted(rng, refs[q], max(0, len(refs[q]) + int(rng.integers(-2, 3))), 6) for q in ref_of]
    res = call_edit(backend, hyps, refs, ref_of=ref_of, nsym=6)
    check_against_referee(res, hyps, refs, ref_of=ref_of, nsym=6, what="ref_of")
    one = call_edit(backend, hyps, [refs[q] for q in ref_of], nsym=6)   # pair by pair
    for k in ("dist", "counts", "nops", "ops", "conf"):
        assert np.array_equal(getattr(one, k), getattr(res, k)), k
    with pytest.raises(ClstmError, match="clstm_edit_distance_batch.*ref_of_h is NULL"):
        call_edit(backend, hyps, refs, nsym=6, raw_args={})


# ---- 5. a pair depends on nothing but itself -----------------------------------------------------------------------------------
def pair_bytes(res, p):
    s = int(res.starts[p])
    return res.dist[p:p + 1].tobytes() + res.counts[3 * p:3 * p + 3].tobytes() + res.nops[p:p + 1].tobytes() + \
        res.ops[s:s + int(res.nops[p])].tobytes()


def test_a_pair_depends_on_nothing_but_itself(backend):
    rng = np.random.default_rng(13)
    shapes = [(30, 28), (1, 64), (70, 3), (65, 130), (0, 9)]
    refs = [rng.integers(1, 3, lb).tolist() for _, lb in shapes]
    hyps = [rng.integers(1, 3, la).tolist() for la, _ in shapes]
    base = call_edit(backend, hyps, refs, nsym=3)
    want = [pair_bytes(base, p) for p in range(len(hyps))]
    for p in range(len(hyps)):
        alone = call_edit(backend, [hyps[p]], [refs[p]], nsym=3)
        assert pair_bytes(alone, 0) == want[p], ("alone", p)
    perm = [3, 0, 4, 2, 1]
    other = call_edit(backend, [hyps[p] for p in perm], [refs[p] for p in perm], nsym=3)
    for i, p in enumerate(perm):
        assert pair_bytes(other, i) == want[p], ("another order", p)
    beside = call_edit(backend, [[]] + hyps, [[]] + refs, nsym=3)
    assert beside.dist[0] == 0 and beside.nops[0] == 0
    lh, lr = long_pairs(first_workspace_square(backend), first_workspace_edge(backend))
    big = call_edit(backend, hyps + [lh[1]], refs + [lr[1]], nsym=4)
    for p in range(len(hyps)):
        assert pair_bytes(beside, p + 1) == want[p], ("beside an empty pair", p)
        assert pair_bytes(big, p) == want[p], ("beside the long pair", p)


# ---- 6. optional outputs, the plan without directions, the counter -------------------------------------------------------------
def test_optional_outputs_and_counter(backend):
    rng = np.random.default_rng(17)
    hyps = [rng.integers(1, 4, int(L)).tolist() for L in (5, 0, 66, 20)]
    refs = [rng.integers(1, 4, int(L)).tolist() for L in (7, 3, 64, 0)]
    n0 = counter(backend)
    full = call_edit(backend, hyps, refs, nsym=4)
    assert counter(backend) == n0 + 1
    names = ("dist", "counts", "nops", "ops", "conf")
    ncalls = 0
    for k in range(1, 5):
        for want in itertools.combinations(names, k):
            res = call_edit(backend, hyps, refs, nsym=4, want=want)
            ncalls += 1
            for name in names:
                if name == "ops" and "ops" in want and "nops" not in want:
                    res.nops = full.nops
                    assert scripts_of(res) == scripts_of(full), want
                elif name in want:
                    assert np.array_equal(getattr(res, name), getattr(full, name)), (want, name)
                else:
                    assert (getattr(res, name) == SENTINEL).all(), (want, name, "written though not asked for")
    assert counter(backend) == n0 + 1 + ncalls
    assert all(plan_of(backend, len(h), len(r), 0)[1] == 0 for h, r in zip(hyps, refs))   # distances alone: no directions
    assert plan_of(backend, 66, 64, 1)[1] == 1
    res = call_edit(backend, [], [], nsym=4)   # nothing to launch
    assert counter(backend) == n0 + 1 + ncalls
    assert (res.conf == 0).all()


# ---- 7. confusion identities ---------------------------------------------------------------------------------------------------
def test_confusion_identities(backend):
    rng = np.random.default_rng(19)
    nsym = 9
    refs = [rng.integers(1, nsym, int(L)).tolist() for L in rng.integers(0, 90, 24)]
    hyps = [planted(rng, r, max(0, len(r) + int(rng.integers(-6, 7))), nsym) for r in refs]
    res = call_edit(backend, hyps, refs, nsym=nsym)
    check_against_referee(res, hyps, refs, nsym=nsym, what="confusions")
    conf = res.conf.reshape(nsym, nsym).astype(np.int64)
    cnt = res.counts.reshape(-1, 3).astype(np.int64)
    assert conf.sum() - np.trace(conf) == res.dist.sum() == cnt.sum()
    assert conf[0].sum() == cnt[:, 1].sum() and conf[:, 0].sum() == cnt[:, 2].sum() and conf[0, 0] == 0
    assert conf[1:, 1:].sum() - np.trace(conf) == cnt[:, 0].sum()
    assert conf[:, 1:].sum() == sum(len(h) for h in hyps) and conf[1:, :].sum() == sum(len(r) for r in refs)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(backend):
    from clstm_amd.abi import ClstmError, i32, ptr
    hyps, refs = [[1, 2], [3], [2, 2, 1]], [[1], [3, 3], [2]]
    n0 = counter(backend)
    E = "clstm_edit_distance_batch"

    def refused(match, **kw):
        kept = []
        with pytest.raises(ClstmError, match=match):
            call_edit(backend, kw.pop("hyps", hyps), kw.pop("refs", refs), keep=kept, **kw)
        for k in ("dist", "counts", "nops", "ops", "conf"):   # ... and no output array is written
            assert (getattr(kept[0], k) == SENTINEL).all(), (match, k)

    bad_off = i32([0, 2, 1, 4])
    refused(E + ".*hyp_off_h\\[2\\]", raw_args={"hoff": ptr(bad_off)})
    neg_off = i32([-1, 1, 2, 3])
    refused(E + ".*ref_off_h\\[0\\] is negative", raw_args={"roff": ptr(neg_off)})
    refused(E + ".*hypothesis label 0 at index 3", hyps=[[1, 2], [3], [0, 2, 1]])
    refused(E + ".*reference label 4 at index 1", refs=[[1], [4, 3], [2]])
    refused(E + ".*reference label -2 at index 0", refs=[[-2], [3, 3], [2]])
    refused(E + ".*ref_of_h\\[1\\] is out of range", ref_of=[0, 3, 2], raw_args={})
    refused(E + ".*ref_of_h\\[2\\] is out of range", ref_of=[0, 1, -1], raw_args={})
    refused(E + ".*nsym must be at least 2", nsym=1, hyps=[[], [], []], refs=[[], [], []])
    refused(E + ".*confusion table exceeds 2\\^26", nsym=8193)
    refused(E + ".*every output is NULL", want=())
    refused(E + ".*ref_of_h is NULL", refs=refs[:2], raw_args={})
    assert counter(backend) == n0


# ---- 9. net level --------------------------------------------------------------------------------------------------------------
NI, NH, NC = 8, [4], 5


def tiny_net(backend):
    """(large random weights and noisy frames, tiny_batch: a net that decodes something else than blanks)"""
    from clstm_amd.net import Network
    net = Network(NI, NH, NC, lib=backend.lib)
    net.set_params(np.random.default_rng(1).normal(0, 2.0, net.nparams).astype(np.float32))
    net.setLearningRate(1e-2, 0.9)
    return net


def tiny_batch(seed, T=(9, 4, 13, 30)):
    rng = np.random.default_rng(seed)
    lines = [rng.normal(0, 2.0, (t, NI)).astype(np.float32) for t in T]
    trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
    return lines, trs


def check_net_errors(net, trs, what):
    dec = [d.tolist() for d in net.decode()]
    dist, cnt, conf = net.errors(trs, counts=True, confusion=True)
    done = []
    for b, (h, r) in enumerate(zip(dec, trs)):
        d, ops = ref_edit(h, list(r))
        assert dist[b] == d and cnt[b].tolist() == ref_counts(ops), (what, b, h, list(r), dist[b], d)
        done.append((h, [int(c) for c in r], ops))
    assert np.array_equal(conf, ref_confusion(done, NC + 1)), what
    assert np.array_equal(net.errors(trs), dist), what
    return dec, dist


def test_net_errors_after_forward_step_and_predict(backend):
    from clstm_amd.net import Network, cer
    net = tiny_net(backend)
    lines, trs = tiny_batch(31)
    net.set_inputs(lines)
    net.forward()
    n0 = counter(backend)
    dec, dist = check_net_errors(net, trs, "after forward")
    assert counter(backend) == n0 + 2
    assert sum(len(d) for d in dec) > 0, "the net decodes nothing: the case proves too little"
    assert cer(dist, trs) == dist.sum() / sum(len(t) for t in trs)
    # label nclasses in a reference: a character outside the codec, it matches nothing
    outside = [np.asarray(list(t) + [NC], np.int32) for t in trs]
    assert np.array_equal(net.errors(outside), dist + 1)
    T = [len(x) for x in lines]
    x = backend.up(np.ascontiguousarray(np.concatenate(lines, 0), np.float32))
    net.train_step_prepared(Network.prepare_step(T, trs), x)
    check_net_errors(net, trs, "after a training step")
    lines2, trs2 = tiny_batch(37, T=(21, 2, 70))
    net.predict(lines2)
    check_net_errors(net, trs2, "after predict")
    check_net_errors(net, [[], [1], []], "short references")


def test_net_errors_leaves_the_training_state_alone(backend):
    from clstm_amd.abi import ClstmError
    from clstm_amd.net import Network
    rng = np.random.default_rng(47)
    batches = []
    for k in range(3):
        T = [int(t) for t in rng.integers(3, 12, 3)]
        trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
        x = backend.up(np.ascontiguousarray(np.concatenate(synth_lines(rng, T, NI), 0), np.float32))
        batches.append((Network.prepare_step(T, trs), x, trs))
    res = []
    for disturbed in (False, True):
        net = tiny_net(backend)
        net.train_step_prepared(batches[0][0], batches[0][1], batches[1][0], batches[1][1])
        if disturbed:   # a declared next minibatch: no current one, refused by the one guard; the declaration survives
            with pytest.raises(ClstmError, match="no current minibatch"):
                net.errors(batches[0][2])
        n20 = path_count(backend, 20)
        net.train_step_prepared(batches[1][0], batches[1][1])
        res.append(path_count(backend, 20) - n20)   # the step found its minibatch declared
        if disturbed:
            backend.sync()
            p, d, g = net.get_params(), net.get_derivs(), net.get_grads()
            net.errors(batches[1][2], counts=True, confusion=True)
            assert net.get_params().tobytes() == p.tobytes() and net.get_derivs().tobytes() == d.tobytes()
            assert net.get_grads().tobytes() == g.tobytes()
        net.train_step_prepared(batches[2][0], batches[2][1])
        if disturbed:
            net.errors(batches[2][2])
        backend.sync()
        res.append((net.get_params(), net.get_derivs()))
    assert res[0] == res[2], "a refused call must leave the declared minibatch declared"
    assert res[1][0].tobytes() == res[3][0].tobytes() and res[1][1].tobytes() == res[3][1].tobytes()


def test_net_errors_refusals(backend):
    from clstm_amd.abi import ClstmError, i32, ptr
    fresh = tiny_net(backend)
    dist = np.full(4, SENTINEL, np.int32)
    lab, L = i32([1, 2, 3, 4]), i32([1, 1, 1, 1])
    with pytest.raises(ClstmError, match="set_batch first"):
        backend.lib.call("clstm_net_errors", fresh.h, ptr(lab), ptr(L), ptr(dist), None, None)
    net = tiny_net(backend)
    lines, trs = tiny_batch(53)
    net.set_inputs(lines)
    net.forward()
    with pytest.raises(ClstmError, match="clstm_net_errors.*every output is NULL"):
        backend.lib.call("clstm_net_errors", net.h, ptr(lab), ptr(L), None, None, None)
    bad = i32([1, 2, NC + 1, 4])
    with pytest.raises(ClstmError, match="clstm_net_errors.*reference label %d at index 2" % (NC + 1)):
        backend.lib.call("clstm_net_errors", net.h, ptr(bad), ptr(L), ptr(dist), None, None)
    with pytest.raises(ClstmError, match="clstm_net_errors.*reference label 0 at index 0"):
        backend.lib.call("clstm_net_errors", net.h, ptr(i32([0, 2, 1, 4])), ptr(L), ptr(dist), None, None)
    with pytest.raises(ClstmError, match="clstm_net_errors.*L_h\\[1\\] is negative"):
        backend.lib.call("clstm_net_errors", net.h, ptr(lab), ptr(i32([1, -1, 1, 1])), ptr(dist), None, None)
    assert (dist == SENTINEL).all()
    net.ctc(trs)   # the net is still in the middle of an ordinary step
    net.backward()
    backend.sync()


def test_module_level_wrapper(backend):
    from clstm_amd.net import edit_distance
    hyps, refs = [[1, 2, 3], [], [2, 2]], [[1, 3], [4]]
    dist, cnt, scripts, conf = edit_distance(hyps, refs, ref_of=[0, 1, 0], script=True, confusion=True, lib=backend.lib)
    for p, q in enumerate([0, 1, 0]):
        d, ops = ref_edit(hyps[p], refs[q])
        assert dist[p] == d and scripts[p].tolist() == ops and cnt[p].tolist() == ref_counts(ops)
    assert conf.shape == (5, 5) and conf.sum() - np.trace(conf) == dist.sum()
    assert np.array_equal(edit_distance(hyps[:2], refs, lib=backend.lib), dist[:2])
