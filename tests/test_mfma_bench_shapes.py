"""The batched-MFMA recurrences (clstm_amd/csrc/lstm_mfma.h, lstm_mfma_bwd.h, lstm_mfma_bwd_dw.h) at the sizes they are the DEFAULT for
-- 640 lines per GPU and more, 200 frames, the `large_minibatch` leg of the bench line -- in the trained regime, through the one-call
training step, across the 640-line rule inside one trajectory, on inputs of any magnitude, and under clstm_net_set_strict_f32.

-m gpu only (the host emulator compiles these kernels out).  tests/test_mfma_recurrence.py keeps the small forced geometries (every
line checked); here minibatches are too large for that and `run_sampled` checks every line's outputs, CTC posteriors and decode,
>= 32 kept lines in full, and the whole gradient / update.  Every test asserts through clstm_debug_path_count which kernels ran:
16 batched forward launched, 17 batched backward, 18 backward as one launch with the weight-gradient items, and 21 -- counted on
the device -- minibatches whose forward pass the batched kernel handed to the per-line kernels because an input left
[-255, 255] (lstm_mfma.h "Input range"): it moves in the input-range tests and nowhere else."""
import ctypes
import os
import time

import numpy as np
import pytest

from common import assert_close, synth_lines
from oracle.oracle import Oracle, OracleNet
from test_net_parity import DELTAS, STATES, run_case, set_opt, _forget_debug_options  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

NI, NC = 48, 83
NTHREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def backend():
    from common import Backend
    return Backend("hip")


def _count(backend, which):
    out = ctypes.c_longlong(0)
    backend.lib.call("clstm_debug_path_count", which, ctypes.byref(out))
    return out.value


def _counts(backend):
    return [_count(backend, i) for i in (16, 17, 18, 21)]


def routes(n):
    """the decorated test hands n minibatches to the per-line kernels (a parametrised test says so per case: parameter `routed`)"""
    def mark(f):
        f.routes = n
        return f
    return mark


@pytest.fixture(autouse=True)
def _routed_only_where_a_test_says_so(request, backend):
    """no test passes by silently taking the per-line path: counter 21 stays unless the test says how far it moves"""
    before = _count(backend, 21)
    yield
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    assert _count(backend, 21) == before + params.get("routed", getattr(request.function, "routes", 0))


def _force(backend):
    set_opt(backend, "fwd_mfma", 2)
    set_opt(backend, "bwd_mfma", 2)


def kept_lines(T, nkeep=32, seed=0):
    """>= nkeep lines: the longest and the shortest, one of the first and one of the last full 16-line workgroup of the library's
    longest-first order (Net::set_batch: stable sort by decreasing length), one of the partial last group if there is one, the
    rest drawn at random"""
    bs = len(T)
    order = sorted(range(bs), key=lambda b: -T[b])          # (Python's sort is stable, like std::stable_sort)
    keep = {order[0], order[-1], order[min(7, bs - 1)]}
    nfull = bs // 16
    if nfull:
        keep.add(order[16 * (nfull - 1) + 5])
    if bs % 16:
        keep.add(order[16 * nfull + (bs % 16) // 2])
    rng = np.random.default_rng(seed)
    while len(keep) < min(nkeep, bs):
        keep.add(int(rng.integers(0, bs)))
    return sorted(keep)


def _kept_state(view, d, which):
    plane = 1 if which.startswith("d_") else 0
    s = view.state(0, d, which[2:] if plane else which, plane)[:, 0, :]
    return s[::-1] if d == 1 else s          # the NPLSTM inside Reversed runs on reversed frames


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def run_sampled(backend, ora32, nh, params, lines, trs, what, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3, referee=False, rule=True):
    """`run_case` (tests/test_net_parity.py) for minibatches too large to keep every line's states: one-layer bidirectional net,
    sequence of calls forward / ctc / backward / update against OracleNet.minibatch (OpenMP over lines).

    every line: softmax outputs (1e-4 / 2e-6), CTC posteriors (ctc_rtol), decode (bit-exact);
    kept_lines(): every saved activation of both directions (1e-4 / 2e-6) and every gate delta (grad_tol of the line's largest);
    the minibatch gradient, the parameters after update() and the momentum buffer with run_case's bars;
    rule: the path counters moved as the library's own rule says (16, 17; 18 exactly below 900 lines).

    referee (the trained regime, as test_gpu_e2e.py::test_full_bench_shape_trained_weights_real_line_crops): the float64 oracle
    sets, at run time, the absolute floor of every state array (max(1e-5, 3 x max |oracle32 - oracle64|)) and of the softmax
    outputs (max(2e-6, 3 x ...)), the delta / gradient bars (max(1e-3, 3 x rel(oracle32, oracle64))), and the explicit check
    max |hip - f64| <= 3 x max |oracle32 - f64| + 1e-6 per state array; a line whose smallest top-2 posterior gap under the
    float64 oracle is below 16 x max |outputs32 - outputs64| is NEAR A TIE and may decode differently -- every other line
    bit-exact, and near-tie lines at most 1 % of the minibatch, else the case is badly chosen and fails.
    Returns the figures printed."""
    from clstm_amd.net import Network
    T = [len(x) for x in lines]
    bs = len(T)
    keep = kept_lines(T)
    assert len(keep) >= min(32, bs)
    dirs = (0, 1)
    t0 = time.time()
    ref = OracleNet(ora32, NI, nh, NC, init=False)
    ref.set_params(params)
    ref.set_lr(lr, 0.9)
    want = ref.minibatch(lines, trs, nthreads=NTHREADS, keep=keep)
    t_ora = time.time() - t0
    skeys = [(d, w) for d in dirs for w in STATES]
    dkeys = [(d, w) for d in dirs for w in DELTAS]
    w_state = {k: {b: _kept_state(want["kept"][b], *k) for b in keep} for k in skeys + dkeys}
    out_atol, act_atol, d_tol, g_tol = 2e-6, {k: 2e-6 for k in skeys}, {k: grad_tol for k in dkeys}, grad_tol
    fig = {}
    near = set()
    if referee:
        t0 = time.time()
        ora64 = Oracle("f64")
        r64 = OracleNet(ora64, NI, nh, NC, init=False)
        r64.set_params(params.astype(np.float64))
        ex = r64.minibatch(lines, trs, nthreads=NTHREADS, keep=keep)
        t_ora += time.time() - t0
        x_state = {k: {b: _kept_state(ex["kept"][b], *k) for b in keep} for k in skeys + dkeys}
        e_ora = {k: max(float(np.abs(w_state[k][b] - x_state[k][b]).max()) for b in keep) for k in skeys}
        act_atol = {k: max(1e-5, 3.0 * e_ora[k]) for k in skeys}
        d_rel = {k: max(_rel(w_state[k][b], x_state[k][b]) for b in keep) for k in dkeys}
        d_tol = {k: max(1e-3, 3.0 * d_rel[k]) for k in dkeys}
        g_rel = _rel(want["derivs"], ex["derivs"])
        g_tol = max(1e-3, 3.0 * g_rel)
        e_out = max(float(np.abs(want["outputs"][b] - ex["outputs"][b]).max()) for b in range(bs))
        out_atol = max(2e-6, 3.0 * e_out)
        for b in range(bs):
            top = np.sort(ex["outputs"][b], axis=1)
            if float((top[:, -1] - top[:, -2]).min()) < 16.0 * e_out:
                near.add(b)
        o_mism = sum(want["decode"][b].tolist() != ex["decode"][b].tolist() for b in range(bs))
        print("%s: oracle32 vs oracle64: gradient %.3g of max, softmax outputs %.3g, gate deltas up to %.3g of a line's max; %d / %d "
              "lines near a tie; %d decode mismatches between the two oracles" % (what, g_rel, e_out, max(d_rel.values()), len(near), bs, o_mism))
        assert len(near) <= 0.01 * bs, "badly chosen case: %d of %d lines near a tie" % (len(near), bs)
        assert sum(len(t) > 1 for t in trs) >= 0.9 * bs                      # the trained net reads the crops
        fig.update(g_ora=g_rel, e_out_ora=e_out, near=len(near))
    before = _counts(backend)
    net = Network(NI, nh, NC, lib=backend.lib)
    net.set_params(params)
    net.setLearningRate(lr, 0.9)
    t0 = time.time()
    net.set_inputs(lines)
    net.forward()
    got = net.split(net.outputs())
    for b in range(bs):
        assert_close(got[b], want["outputs"][b], atol=out_atol, what="%s: softmax outputs line %d" % (what, b))
    for k in skeys:
        s = net.split(net.state(0, k[0], k[1]))
        for b in keep:
            assert_close(s[b], w_state[k][b], atol=act_atol[k], what="%s: state %s line %d" % (what, k, b))
        if referee:
            e_hip = max(float(np.abs(s[b] - x_state[k][b]).max()) for b in keep)
            print("%s %s: max |hip - f64| %.3g, max |oracle32 - f64| %.3g" % (what, k, e_hip, e_ora[k]))
            assert e_hip <= 3.0 * e_ora[k] + 1e-6, (k, e_hip, e_ora[k])
            fig[k] = (e_hip, e_ora[k])
    dec = net.decode()
    mism = [b for b in range(bs) if dec[b].tolist() != want["decode"][b].tolist()]
    print("%s: %d decode mismatches vs the float32 oracle (lines %s), %d near-tie lines" % (what, len(mism), mism[:8], len(near)))
    assert all(b in near for b in mism), ("decodes differ on lines that are not near a tie", [b for b in mism if b not in near])
    al = net.split(net.ctc(trs, want_aligned=True))
    for b in range(bs):
        assert_close(al[b], want["aligned"][b], rtol=ctc_rtol, atol=1e-6, what="%s: aligned line %d" % (what, b))
    net.backward()
    for k in dkeys:
        s = net.split(net.state(0, k[0], k[1]))
        for b in keep:
            assert_close(s[b], w_state[k][b], rtol=d_tol[k], atol=1e-9, scale_atol=d_tol[k], what="%s: delta %s line %d" % (what, k, b))
    g = net.get_grads()
    fig["g_hip_vs_ora32"] = _rel(g, want["derivs"])
    if referee:
        fig["g_hip"] = _rel(g, ex["derivs"])
        print("%s: minibatch gradient, of max: |hip - f64| %.3g, |oracle32 - f64| %.3g" % (what, fig["g_hip"], fig["g_ora"]))
    print("%s: minibatch gradient |hip - oracle32| %.3g of max" % (what, fig["g_hip_vs_ora32"]))
    assert_close(g, want["derivs"], rtol=g_tol, atol=1e-9, scale_atol=g_tol, what="%s: minibatch gradient" % what)
    net.update()
    ref.update()
    upd_atol = 1e-7 + lr * g_tol * float(np.abs(want["derivs"]).max())
    assert_close(net.get_params(), ref.get_params(), rtol=1e-5, atol=upd_atol, what="%s: params after update" % what)
    assert_close(net.get_derivs(), ref.get_derivs(), rtol=g_tol, atol=1e-9, scale_atol=g_tol, what="%s: momentum buffer" % what)
    after = _counts(backend)
    if rule:
        assert bs >= 640
        assert after[0] == before[0] + 1, "the batched forward recurrence did not run"
        assert after[1] == before[1] + 1, "the batched backward recurrence did not run"
        assert (after[2] > before[2]) == (bs < 900), "one-launch form of the backward pass: %d lines" % bs
        assert after[3] == before[3], "the batched forward kernel handed the minibatch to the per-line kernels"
    print("%s: oracle %.1f s, library calls and checks %.1f s" % (what, t_ora, time.time() - t0))
    return fig


# ---- B.1: the shape `large_minibatch` times ---------------------------------------------------------------------------------
def _noise_case(ora32, T, seed):
    rng = np.random.default_rng(seed)
    params = OracleNet(ora32, NI, 100, NC, seed=0.222).get_params() * 10.0
    lines = synth_lines(rng, T, NI)
    trs = [rng.integers(1, NC, min(25, max(1, t // 3))).astype(np.int32) for t in T]
    return params, lines, trs


def test_large_minibatch_2048_lines_of_200_frames(backend, ora32):
    """2048 lines x 200 frames, init x 10, smoothed noise, 25 labels per line: what the `large_minibatch` leg of the bench line runs,
    by the library's own rule (batched forward, batched backward with the weight-gradient items BEHIND it: >= 900 lines)"""
    params, lines, trs = _noise_case(ora32, [200] * 2048, 41)
    run_sampled(backend, ora32, 100, params, lines, trs, "2048 x 200")


def test_ragged_650_lines_with_a_one_frame_line(backend, ora32):
    """650 ragged lines T ~ U{150..250} with a one-frame line: 40 full 16-line groups and a partial one of 10 lines that holds the
    one-frame line (longest first), the backward recurrence and the weight-gradient items as ONE launch (< 900 lines)"""
    rng = np.random.default_rng(42)
    T = [int(t) for t in rng.integers(150, 251, 649)]
    T.insert(321, 1)
    params, lines, trs = _noise_case(ora32, T, 43)
    run_sampled(backend, ora32, 100, params, lines, trs, "650 ragged")


# ---- B.2: the trained regime through the batched kernels, float64 as referee --------------------------------------------------
@pytest.mark.parametrize("shape,seed", [("fixed", 31), ("ragged", 32)])
def test_trained_weights_640_real_line_crops(backend, ora32, shape, seed):
    """The trained weight set (tests/trained_weights.py: |w| up to 8, the recurrence not contractive) on 640 jittered crops of the
    fixture line, each with the transcript the oracle decodes on it, by the library's own rule: the f16 x 2 forward products
    (2^-22) and the bf16 x 2 R^T.delta (2^-16) amplified over 200 steps.  No bar is fixed here: run_sampled(referee=True) derives
    all of them from the distance of the float32 oracle to the float64 oracle and prints both sides."""
    from trained_weights import NC as TNC, NH, fixture_crops, trained_like_params
    assert TNC == NC
    params, reads_fixture = trained_like_params(ora32)
    assert reads_fixture
    dec_net = OracleNet(ora32, NI, NH, NC, init=False)
    dec_net.set_params(params)
    rng = np.random.default_rng(seed)
    T = [200] * 640 if shape == "fixed" else [int(t) for t in rng.integers(150, 251, 640)]
    lines, trs = fixture_crops(rng, T, dec_net)
    run_sampled(backend, ora32, NH, params, lines, trs, "trained 640 %s" % shape, referee=True)


# ---- B.3: the bench's call at the bench's size --------------------------------------------------------------------------------
def test_one_call_step_at_2048_lines_and_its_prepared_next_form(backend, ora32):
    """clstm_net_train_step at 2048 x 200, three updates against the oracle (test_gpu_e2e._trajectory: decodes of all lines
    identical at every step, parameters and momentum within the derived tolerance), and the same three minibatches through
    clstm_net_train_step_next (each step's tail ingests the next minibatch): parameters and momentum BIT FOR BIT those of the
    plain calls.  The batched kernels ran in every step of both."""
    import torch
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    from test_gpu_e2e import _trajectory
    Ts, L, nsteps = [200] * 2048, 25, 3
    seen = []

    def moved(step, net):
        now = _counts(backend)
        assert now[0] > seen[-1][0] and now[1] > seen[-1][1], "step %d did not take the batched kernels" % step
        seen.append(now)
    seen.append(_counts(backend))
    a = _trajectory(ora32, NI, 100, NC, Ts, L, 10.0, nsteps, 1e-4, 0.9, True, nthreads=NTHREADS, on_step=moved)
    assert len(seen) == nsteps + 1
    rng = np.random.default_rng(70)                       # _trajectory's own minibatches (seed 70: lines, then transcripts, per step)
    batches = []
    for _ in range(nsteps):
        lines = synth_lines(rng, Ts, NI)
        trs = [rng.integers(1, NC, L).astype(np.int32) for _ in Ts]
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate(lines, 0), np.float32)).cuda()
        batches.append((Network.prepare_step(Ts, trs), x))
    b = Network(NI, 100, NC, lib=backend.lib)
    b.set_params(init_params(NI, 100, NC, seed=0.222) * 10.0)
    b.setLearningRate(1e-4, 0.9)
    used0 = _count(backend, 20)
    for k in range(nsteps):
        before = _counts(backend)
        if k + 1 < nsteps:
            b.train_step_prepared(batches[k][0], batches[k][1], batches[k + 1][0], batches[k + 1][1])
        else:
            b.train_step_prepared(batches[k][0], batches[k][1])
        after = _counts(backend)
        assert after[0] == before[0] + 1 and after[1] == before[1] + 1, "step %d of the prepared form: %s -> %s" % (k + 1, before, after)
    assert _count(backend, 20) == used0 + nsteps - 1, "the declared minibatches were not the ones used"
    assert np.array_equal(a.get_params(), b.get_params())
    assert np.array_equal(a.get_derivs(), b.get_derivs())


# ---- B.4: crossing the 640-line rule inside one trajectory --------------------------------------------------------------------
def test_trajectory_across_the_640_line_rule(backend, ora32):
    """Minibatches of 64, 704, 64, 704, 640, 639 lines (T ~ U{20..64}, one line of 64 frames: the overlap rule holds) on ONE net:
    the kernel family -- and with it the weight packs in use, the source-row handling of layer 0, the line order table --
    changes between consecutive steps.  clstm_net_train_step_next against the same sequence of plain clstm_net_train_step calls
    bit for bit after every step, the plain sequence against the oracle at every step with _trajectory's derived bars (decodes
    identical; parameters within sum_j sum_i mom^(j-i) x lr x grad_tol x max |d|; momentum within grad_tol x that geometric
    factor), and counters 16 / 17 move in exactly the steps of >= 640 lines."""
    import torch
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    sizes, lr, mom, grad_tol = [64, 704, 64, 704, 640, 639], 1e-4, 0.9, 1e-3
    rng = np.random.default_rng(77)
    p0 = init_params(NI, 100, NC, seed=0.222) * 10.0
    ref = OracleNet(ora32, NI, 100, NC, init=False)
    ref.set_params(p0); ref.set_lr(lr, mom)
    a, b = Network(NI, 100, NC, lib=backend.lib), Network(NI, 100, NC, lib=backend.lib)
    for n in (a, b):
        n.set_params(p0); n.setLearningRate(lr, mom)
    batches = []
    for bs in sizes:
        T = [64] + [int(t) for t in rng.integers(20, 65, bs - 1)]
        lines = synth_lines(rng, T, NI)
        trs = [rng.integers(1, NC, max(1, t // 4)).astype(np.int32) for t in T]
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate(lines, 0), np.float32)).cuda()
        batches.append((Network.prepare_step(T, trs), x, lines, trs))
    d_fac = v_fac = 0.0
    for k, bs in enumerate(sizes):
        prep, x, lines, trs = batches[k]
        want = ref.minibatch(lines, trs, nthreads=NTHREADS)
        gmax = float(np.abs(want["derivs"]).max())
        ref.update()
        before = _counts(backend)
        a.train_step_prepared(prep, x)
        mid = _counts(backend)
        if k + 1 < len(sizes):
            b.train_step_prepared(prep, x, batches[k + 1][0], batches[k + 1][1])
        else:
            b.train_step_prepared(prep, x)
        after = _counts(backend)
        batched = 1 if bs >= 640 else 0
        assert [mid[i] - before[i] for i in (0, 1)] == [batched, batched], (k, bs, before, mid)
        assert [after[i] - mid[i] for i in (0, 1)] == [batched, batched], (k, bs, mid, after)
        assert np.array_equal(a.get_params(), b.get_params()), "step %d (%d lines): parameters differ" % (k + 1, bs)
        assert np.array_equal(a.get_derivs(), b.get_derivs()), "step %d (%d lines): momentum differs" % (k + 1, bs)
        dec = a.decode()
        mism = [i for i in range(bs) if dec[i].tolist() != want["decode"][i].tolist()]
        assert not mism, "step %d (%d lines): decodes differ on lines %s" % (k + 1, bs, mism)
        d_fac = mom * d_fac + 1.0
        v_fac += d_fac
        assert_close(a.get_params(), ref.get_params(), rtol=1e-5, atol=1e-7 + v_fac * lr * grad_tol * gmax, what="parameters after step %d" % (k + 1))
        assert_close(a.get_derivs(), ref.get_derivs(), rtol=grad_tol, atol=1e-9, scale_atol=d_fac * grad_tol, what="momentum buffer after step %d" % (k + 1))


# ---- B.5: variants the host code accepts, forced onto small minibatches -------------------------------------------------------
def test_forced_unidirectional(backend, ora32):
    """`lstm1` (ndir = 1) through both batched kernels: one workgroup column instead of two, no reversed direction"""
    _force(backend)
    before = _counts(backend)
    run_case(backend, ora32, NI, 100, NC, [70, 33, 1, 52, 70, 18], uni=True, scale=10.0)
    after = _counts(backend)
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1, (before, after)


def test_forced_with_input_deltas(backend, ora32):
    """enable_input_deltas: the first layer's dx = W_x^T . delta, summed over both directions (Parallel::backward,
    clstm.cc:538-541), formed from the gate deltas the batched backward recurrence wrote -- against the oracle's per line"""
    _force(backend)
    T = [64, 40, 23, 1, 57]
    rng = np.random.default_rng(9)
    params = OracleNet(ora32, NI, 100, NC, seed=0.222).get_params() * 10.0
    lines = synth_lines(rng, T, NI)
    trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
    before = _counts(backend)
    net, _ = run_case(backend, ora32, NI, 100, NC, T, check_dx=True, params=params, lines=lines, trs=trs)
    after = _counts(backend)
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1, (before, after)
    dx = net.split(net.input_deltas())                    # (left by the backward pass; the update does not touch them)
    ref = OracleNet(ora32, NI, 100, NC, init=False)
    ref.set_params(params)
    for b, (x, tr) in enumerate(zip(lines, trs)):
        ref.set_inputs(x); ref.forward(); ref.ctc_deltas(tr); ref.backward()
        assert_close(dx[b], ref.input_deltas()[:, 0, :], rtol=1e-4, atol=1e-9, scale_atol=1e-4, what="input deltas line %d" % b)


def test_forced_stacked_100_over_64(backend, ora32):
    """nh = [100, 64]: layer 0 (48 inputs, 100 cells) takes the batched forward kernel -- exactly ONE launch per forward pass --,
    layer 1 (200 inputs: not an instantiated geometry) the hoisted W_x GEMM and the per-line forward kernel on the h rows the
    batched kernel left.  The batched BACKWARD kernel has no condition on the inputs: forced, both layers take it (two launches),
    layer 1's input deltas handed down as layer 0's dH."""
    _force(backend)
    before = _counts(backend)
    run_case(backend, ora32, NI, [100, 64], NC, [60, 44, 1, 60, 27], scale=10.0)
    after = _counts(backend)
    assert after[0] == before[0] + 1, (before, after)
    assert after[1] == before[1] + 2, (before, after)


@pytest.mark.parametrize("nh", [64, 128])
def test_forced_64_and_128_cells_at_200_frames(backend, ora32, nh):
    """the 64- and the 128-cell instantiation over 200 steps, a shorter line and a one-frame line beside them (128 cells: the
    batched forward only -- the backward's LDS image does not fit -- so counter 17 must NOT move there)"""
    _force(backend)
    before = _counts(backend)
    run_case(backend, ora32, NI, nh, NC, [200, 173, 200, 1], scale=10.0, lr=1e-4, ctc_rtol=1e-3, grad_tol=1e-3)
    after = _counts(backend)
    assert after[0] == before[0] + 1, (before, after)
    assert after[1] == before[1] + (1 if nh == 64 else 0), (before, after)


# ---- C: inputs of any magnitude ----------------------------------------------------------------------------------------------
MAGS = [255.0, 256.0, 300.0, -300.0, 1000.0, 1e4, 30.0, 1.0]


def _spiked_lines(rng, mags, T=60):
    """smoothed noise in which 5 % of the pixels of line b are mag_b x U(0, 1) and one pixel is exactly mag_b"""
    lines = synth_lines(rng, [T] * len(mags), NI)
    for x, mag in zip(lines, mags):
        hit = rng.random(x.shape) < 0.05
        x[hit] = (mag * rng.random(int(hit.sum()))).astype(np.float32)
        x[int(rng.integers(0, T)), int(rng.integers(0, NI))] = mag
    return lines


def _init_params(ora32):
    return OracleNet(ora32, NI, 100, NC, seed=0.222).get_params() * 1.0


@routes(1)
def test_forced_inputs_far_outside_0_1(backend, ora32):
    """The contract of include/clstm_abi.h (set_inputs): inputs of any magnitude.  Eight lines with pixels up to 255, 256, 300,
    -300, 1000, 1e4, 30, 1 in ONE forced minibatch: every activation, delta, the gradient and the update meet run_case's bars.
    Which path ran: the batched forward kernel is launched (counter 16) and declines the minibatch on the device -- counter 21
    moves by one: the routed per-line twins computed the forward pass (lstm_mfma.h "Input range") --, the backward pass is the
    batched kernel's (counter 17; it reads no inputs).  (The oracle alone on these lines: all finite, at most 76 % of a
    line's gate activations saturated.)"""
    _force(backend)
    rng = np.random.default_rng(101)
    lines = _spiked_lines(rng, MAGS)
    trs = [rng.integers(1, NC, 20).astype(np.int32) for _ in MAGS]
    before = _counts(backend)
    run_case(backend, ora32, NI, 100, NC, [60] * len(MAGS), params=_init_params(ora32), lines=lines, trs=trs)
    after = _counts(backend)
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[3] == before[3] + 1, (before, after)


@routes(1)
def test_result_class_does_not_depend_on_the_minibatch_size(backend, ora32):
    """the same eight lines as lines 0..7 of a 640-line minibatch (the other 632 in [0, 1]; the library's own rule launches the
    batched kernel, which hands the minibatch to the routed per-line twins: counters 16 and 21) and as a minibatch of their
    own (per-line kernels by the rule: neither counter moves): in both, their softmax outputs within 1e-4 / 2e-6 of the oracle
    and their decodes the oracle's"""
    from clstm_amd.net import Network
    rng = np.random.default_rng(101)
    lines8 = _spiked_lines(rng, MAGS)
    lines = lines8 + synth_lines(rng, [60] * 632, NI)
    params = _init_params(ora32)
    ref = OracleNet(ora32, NI, 100, NC, init=False)
    ref.set_params(params)
    net = Network(NI, 100, NC, lib=backend.lib)
    net.set_params(params)
    for name, batch, batched in (("640 lines", lines, 1), ("8 lines", lines8, 0)):
        before = _counts(backend)
        net.set_inputs(batch)
        net.forward()
        now = _counts(backend)
        assert now[0] == before[0] + batched and now[3] == before[3] + batched, (name, before, now)
        got, dec = net.split(net.outputs()), net.decode()
        for b in range(8):
            ref.set_inputs(lines8[b])
            want = ref.forward()[:, 0, :]
            assert np.isfinite(got[b]).all(), "%s: non-finite outputs on line %d (max |x| %g)" % (name, b, MAGS[b])
            assert_close(got[b], want, what="%s: softmax outputs line %d (max |x| %g)" % (name, b, MAGS[b]))
            assert dec[b].tolist() == ref.decode().tolist(), (name, b)


@pytest.mark.parametrize("top,routed", [(255.0, 0), (255.95, 1)])
def test_forced_inputs_at_the_edge_of_the_f16_range(backend, ora32, top, routed):
    """255.0 is the last input the 2^8 operand scale represents (255 x 256 = 65280 < 65504): the batched kernel computes that
    minibatch (counter 21 stays); 255.95 x 256 rounds to the f16 infinity: handed to the per-line twins (counter 21 moves).
    Both minibatches meet run_case's bars."""
    _force(backend)
    rng = np.random.default_rng(102)
    T = [60] * 8
    lines = synth_lines(rng, T, NI)
    lines[3][17, 5] = top
    trs = [rng.integers(1, NC, 20).astype(np.int32) for _ in T]
    before = _counts(backend)
    run_case(backend, ora32, NI, 100, NC, T, params=_init_params(ora32), lines=lines, trs=trs)
    after = _counts(backend)
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[3] == before[3] + routed, (before, after)


@routes(1)
@pytest.mark.parametrize("fused", [False, True], ids=["sequence_of_calls", "clstm_net_train_step"])
def test_forced_non_finite_gradient_is_never_applied(backend, ora32, fused):
    """test_states_and_step.py::test_non_finite_gradient_is_never_applied with the batched kernels forced: a NaN pixel makes the
    minibatch's max |x| non-finite -- that one forward pass is the per-line twins' (counter 21: once in four steps), where a
    NaN stays a NaN --, the batched backward kernel carries it into the gradient, which is not applied; later updates are
    skipped until the host has reported the step, training resumes afterwards"""
    from clstm_amd.net import Network
    _force(backend)
    rng = np.random.default_rng(5)
    T = [30, 21, 12]
    params = OracleNet(ora32, NI, 100, NC, seed=0.222).get_params() * 10.0
    lines = synth_lines(rng, T, NI)
    trs = [rng.integers(1, NC, 4).astype(np.int32) for _ in T]
    net = Network(NI, 100, NC, lib=backend.lib)
    net.set_params(params)
    net.setLearningRate(1e-2, 0.9)
    prep = Network.prepare_step(T, trs)

    def step(ls):
        x = np.ascontiguousarray(np.concatenate(ls, 0), np.float32)
        if fused:
            net.train_step_prepared(prep, backend.up(x))
        else:
            net.set_inputs(ls); net.forward(); net.ctc(trs); net.backward(); net.update()
    before = _counts(backend)
    step(lines)
    backend.sync()
    after = _counts(backend)
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1, (before, after)
    p1, d1 = net.get_params(), net.get_derivs()
    assert np.isfinite(p1).all() and not np.array_equal(p1, params.astype(np.float32))
    poisoned = [l.copy() for l in lines]
    poisoned[1][2, 3] = np.nan
    step(poisoned)
    step(lines)
    with pytest.raises(Exception, match="non-finite value .* training step 2"):
        backend.sync()
    assert np.array_equal(net.get_params(), p1) and np.array_equal(net.get_derivs(), d1)
    step(lines)
    backend.sync()
    p4 = net.get_params()
    assert np.isfinite(p4).all() and not np.array_equal(p4, p1)
    end = _counts(backend)
    assert end[0] == before[0] + 4 and end[1] == before[1] + 4 and end[3] == before[3] + 1, (before, end)


# ---- D: strict_f32 means strict ----------------------------------------------------------------------------------------------
def test_strict_f32_keeps_the_per_line_kernels_at_640_lines(backend, ora32):
    """clstm_net_set_strict_f32 promises every product of the step on the f32 MFMA (include/clstm_abi.h): a strict net of 640
    lines does not take the f16 x 2 / bf16 x 2 split-product recurrences by the library's own rule -- counters 16, 17, 18, 21 stay --
    and meets run_case's bars.  (Forced with fwd_mfma = 2 / bwd_mfma = 2 the option wins:
    test_gpu_e2e.py::test_full_bench_shape_trained_weights_forced_batched_kernels, strict cases.)"""
    bs = 640
    rng = np.random.default_rng(bs)
    Ts = [64] * 8 + [int(t) for t in rng.integers(1, 25, bs - 8)]
    before = _counts(backend)
    run_case(backend, ora32, NI, 100, NC, Ts, scale=10.0, seed=bs, strict_f32=True)
    assert _counts(backend) == before, "a strict net took a split-product recurrence: counters 16 / 17 / 18 / 21 %s -> %s" % (before, _counts(backend))
