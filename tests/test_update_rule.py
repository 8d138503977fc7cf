"""The SGD update where the gradient clip SATURATES, on every path that implements it.

The rule (sgd_update, clstm.cc:201-217 with clip_gradient / sgd_update of clstm_compute.cc:553-563 on the flat buffers):

    d += g ; d = clip(d, +-gclip) ; v += lr * d ; d *= mom

is written four times in the library: k_update (the sequence of calls, and behind an all-reduce), reduce_scatter_one under
UpdateFuse (clstm_net_train_step without a communicator; for a single narrow layer it also rewrites the packed parameter copies
through PackDst), the same code deferred into k_reduce_scatter_ingest (clstm_net_train_step_next) and k_peer_allreduce_update
(several ranks: tests/test_distributed.py).  At the default gclip = 100 and gradients of order 10 the clamp is the identity, so
the path-equality tests compare four identities.  Here every path is held against a plain numpy float32 statement of the rule, one
operation per rounding, with inputs that drive a large share of the entries of d + g beyond +-gclip.

Acceptance, everywhere in this file: d' bit for bit; v' bit for bit either the unfused value f32(v0 + f32(di * lr)) or the
single-rounding fused multiply-add of di * lr + v0 (the compilers may contract `v += di * lr`; `fma_f32` in tests/common.py states
that value exactly and is checked against rational arithmetic below).  No wider tolerance -- except test (d), a four-step trajectory against the oracle whose GRADIENTS differ by summation
order: it uses the tolerances of test_net_parity.py::test_second_step_momentum."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from common import (F32, assert_close, assert_every_entry_once, assert_update_bits, bits, fma_f32, pm200, synth_lines,
                    update_of_clamped)
from oracle.oracle import OracleNet


# ---- the statement of the rule (its arithmetic after the clamp, and the bit comparison, are shared through tests/common.py) ------
def expected_update(v0, d0, g, lr, mom, clip):
    """(d', v' unfused, v' fused) of one update in numpy float32, one operation per rounding"""
    d0, g, clip = np.asarray(d0, F32), np.asarray(g, F32), F32(clip)
    di = (d0 + g).astype(F32)
    if clip < 1e6:
        di = np.maximum(-clip, np.minimum(clip, di)).astype(F32)
    return update_of_clamped(v0, di, lr, mom)


def assert_rule(v0, d0, g, v1, d1, lr, mom, clip, what):
    """the acceptance rule of this file; returns the share of entries whose d0 + g lies beyond +-clip"""
    assert np.isfinite(g).all(), what
    assert_update_bits(v1, d1, expected_update(v0, d0, g, lr, mom, clip), what, v0=v0, d0=d0, g=g)
    return float((np.abs((np.asarray(d0, F32) + np.asarray(g, F32)).astype(F32)) > F32(clip)).mean())


def _round_fraction_f32(x):
    """nearest-even float32 of an exact rational (normal range only)"""
    if x == 0:
        return F32(0)
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = 0
    while x >= 2 ** 24:
        x /= 2; e += 1
    while x < 2 ** 23:
        x *= 2; e -= 1
    n = int(x)                                            # floor
    rem = x - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F32(sign * float(n) * 2.0 ** e)


def test_fma_statement_is_exact():
    """fma_f32 against exact rational arithmetic: random operands of the update's magnitudes, and operands built so that
    a * b + c falls on / next to a float32 rounding tie (where rounding through float64 first goes wrong)."""
    rng = np.random.default_rng(1)
    a = rng.uniform(-150, 150, 4000).astype(F32)
    b = np.full(4000, 1e-2, F32)
    c = (rng.normal(0, 0.3, 4000)).astype(F32)
    # ties: c = 2^10 (1 + 2^-23 k), whose half ulp is 2^-14.  a * b = +-2^-14 exactly (a true tie), or +-2^-14 (1 - 2^-46) =
    # 2^-14 (1 + 2^-23)(1 - 2^-23): short of the tie by 2^-60, far below the float64 ulp of c (2^-42) -- float64 rounds the sum
    # ONTO the tie and the second rounding goes to even, where the exact sum rounds back to c
    k = rng.integers(0, 1000, 300)
    ct = (2.0 ** 10 * (1.0 + k * 2.0 ** -23)).astype(F32)
    at = np.where(np.arange(300) % 2 == 0, 1.0, 1.0 + 2.0 ** -23).astype(F32)
    bt = np.where(np.arange(300) % 2 == 0, 2.0 ** -14, 2.0 ** -14 * (1.0 - 2.0 ** -23)).astype(F32)
    bt[::3] *= -1
    a, b, c = np.concatenate([a, at]), np.concatenate([b, bt]), np.concatenate([c, ct])
    got = fma_f32(a, b, c)
    want = np.array([_round_fraction_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(bits(got), bits(want))
    through_f64 = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert not np.array_equal(through_f64, want), "the tie cases do not exercise the double rounding"


# ---- nets, regimes, paths -------------------------------------------------------------------------------------------------------
NI, NC = 6, 7
T_SMALL = ([9, 5, 12], [7, 11, 4, 6])                     # the two minibatches of a case (changing geometry)
#            nhidden      unidirectional  gemm precision  init x  lr
NETS = {
    "h10": ([10], False, 0, 20.0, 1e-2),
    "h7_5": ([7, 5], False, 0, 20.0, 1e-2),
    "h10_uni": ([10], True, 0, 20.0, 1e-2),
    "h136_wide": ([136], False, 0, 1.0, 1e-4),
    "h136_132_bf16": ([136, 132], False, 2, 1.0, 1e-4),
}
#               clip   preloaded derivs   momentum  lr (None: the net's)
REGIMES = {
    "clip100_u150": (100.0, "u150", 0.9, None),
    "clip0.01_zero_derivs": (0.01, "zero", 0.9, None),
    "clip_off_u150_and_2e6": (1e6, "u150_2e6", 0.9, None),
    "mom0": (100.0, "u150", 0.0, None),
    "lr0": (100.0, "u150", 0.9, 0.0),
}
PATHS = ["calls", "train_step", "train_step_next", "train_step_host"]
CASES_A = [(n, r) for n in ("h10", "h7_5") for r in REGIMES] + [(n, "clip100_u150") for n in ("h10_uni", "h136_wide", "h136_132_bf16")]


def count(backend, i):
    out = ctypes.c_longlong(0)
    backend.lib.call("clstm_debug_path_count", i, ctypes.byref(out))
    return out.value


def make_derivs(kind, rng, n):
    if kind == "zero":
        return np.zeros(n, F32)
    if kind == "pm200":
        return pm200(n)
    d = rng.uniform(-150, 150, n).astype(F32)
    if kind == "u150_2e6":                                 # a few entries far beyond 1e6: a switched-off clamp must let them through
        at = rng.choice(n, 6, replace=False)
        d[at] = np.array([2e6, -2e6, 2e6, -2e6, 2e6, -2e6], F32)
    return d


def make_net(backend, ni, nh, nc, uni, precision, scale):
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    net = Network(ni, nh, nc, unidirectional=uni, lib=backend.lib)
    net.set_params(init_params(ni, nh, nc, unidirectional=uni, seed=0.222) * scale)
    if precision:
        net.set_gemm_precision(precision)
    return net


def make_batch(backend, rng, ni, nc, T, L=None):
    from clstm_amd.net import Network
    lines = synth_lines(rng, T, ni)
    trs = [rng.integers(1, nc, max(1, t // 3) if L is None else L).astype(np.int32) for t in T]
    x = np.ascontiguousarray(np.concatenate(lines, 0), F32)
    return {"T": list(T), "trs": trs, "x": x, "xd": backend.up(x), "prep": Network.prepare_step(T, trs)}


def run_step(net, path, batch, nxt=None):
    """one training step of `net` on `batch` along `path`; nxt: the minibatch a train_step_next call declares"""
    if path == "calls":
        net.set_batch(batch["T"]); net.set_inputs_device(batch["xd"])
        net.forward(); net.ctc(batch["trs"]); net.backward(); net.update()
    elif path == "train_step":
        net.train_step_prepared(batch["prep"], batch["xd"])
    elif path == "train_step_next":
        if nxt is not None:
            net.train_step_prepared(batch["prep"], batch["xd"], nxt["prep"], nxt["xd"])
        else:
            net.train_step_prepared(batch["prep"], batch["xd"])
    elif path == "train_step_host":
        net.train_step_host(batch["prep"], batch["x"].copy())
    else:
        raise ValueError(path)


def drive(backend, net, path, batches, derivs_kind, rng, check, what):
    """`len(batches)` steps along `path`.  Before every step the derivs are preloaded and the parameters read; after it
    check(v0, d0, g, v1, d1, what) judges the step.  train_step_next: every step but the last declares the next minibatch (its
    last reduction -- the update -- rides that minibatch's ingest launch), and the step after a deferring one starts from what
    that launch left; both kinds are judged."""
    tails0, used0 = count(backend, 19), count(backend, 20)
    out = []
    for k, batch in enumerate(batches):
        d0 = make_derivs(derivs_kind, rng, net.nparams)
        net.set_derivs(d0)
        v0 = net.get_params()
        nxt = batches[k + 1] if k + 1 < len(batches) else None
        run_step(net, path, batch, nxt)
        backend.sync()
        out.append(check(v0, d0, net.get_grads(), net.get_params(), net.get_derivs(), "%s step %d" % (what, k)))
    if path == "train_step_next":
        assert count(backend, 19) - tails0 == len(batches) - 1, "the update did not ride the next minibatch's ingest launch"
        assert count(backend, 20) - used0 == len(batches) - 1, "the step after a deferring one did not start from the declared minibatch"
    return out


# ---- (a) the rule, path by path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("netkey,regime", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_update_rule_where_the_clip_saturates(backend, netkey, regime, path):
    """Every path against the numpy statement.  The share of saturated entries is computed from the statement's own d0 + g and
    ASSERTED: the clip-100 regimes need 20..80 % of the entries beyond +-100 (U(-150, 150) puts a third there), the clip-0.01
    regime at least one entry clamped and one not; a case outside these bounds fails as inconclusive."""
    nh, uni, precision, scale, lr_net = NETS[netkey]
    clip, derivs_kind, mom, lr = REGIMES[regime]
    lr = lr_net if lr is None else lr
    rng = np.random.default_rng(41)
    net = make_net(backend, NI, nh, NC, uni, precision, scale)
    net.setLearningRate(lr, mom)
    if clip != 100.0:                                      # (the clip-100 regimes run on the library's default)
        net.set_gradient_clip(clip)
    batches = [make_batch(backend, rng, NI, NC, T) for T in T_SMALL]
    what = "%s %s %s" % (netkey, regime, path)
    shares = drive(backend, net, path, batches, derivs_kind, rng,
                   lambda v0, d0, g, v1, d1, w: assert_rule(v0, d0, g, v1, d1, lr, mom, clip, w), what)
    print("saturated share, %s: %s" % (what, ["%.3f" % s for s in shares]))
    for s in shares:
        if clip == 100.0:
            assert 0.2 <= s <= 0.8, "inconclusive: %.3f of the entries beyond the clip (%s)" % (s, what)
        elif clip < 1.0:
            assert 0.0 < s < 1.0, "inconclusive: %.3f of the entries beyond the clip (%s)" % (s, what)
        else:                                              # only the planted +-2e6 entries, which the statement lets through
            assert s == 6.0 / net.nparams


# ---- (b) every parameter exactly once -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("netkey", list(NETS))
def test_every_parameter_is_updated_exactly_once(backend, netkey, path):
    nh, uni, precision, scale, lr = NETS[netkey]
    rng = np.random.default_rng(43)
    net = make_net(backend, NI, nh, NC, uni, precision, scale)
    net.setLearningRate(lr, 0.9)
    batches = [make_batch(backend, rng, NI, NC, T) for T in T_SMALL]
    what = "%s %s" % (netkey, path)
    gmax = drive(backend, net, path, batches, "pm200", rng,
                 lambda v0, d0, g, v1, d1, w: assert_every_entry_once(v0, d0, g, v1, d1, lr, 0.9, w), what)
    print("max |g|, %s: %s" % (what, ["%.3g" % x for x in gmax]))


# The bench-shaped net of the batched-MFMA recurrences (ni 48, nh 100, nc 83).  The minibatch gradient is a SUM over thousands of
# frames and has to stay below 100 in every entry for the +-200 argument: the weights stay at the scale they are drawn with (the
# hidden activations, and with them every weight gradient, are small), and the softmax bias of the blank class -- whose gradient is
# (frames the alignment gives to blank) - (sum of the blank outputs) -- is set so that the net emits blank about as often as a
# CTC alignment of L labels on T frames with near-uniform label scores asks for.  max |g| < 100 is asserted, not assumed.
# The two shares below belong to THIS seed, geometry, synth_lines and init_params; a change to any of them can move the alignment's
# blank share, and the cases then fail as inconclusive (max |g| >= 100) rather than pass.  To derive them again: run the case with
# any share b and print g at the blank bias (index p.size - nsm in mfma_case).  The weights are small, so the net emits blank on a
# share b of the N = nlines * T frames whatever the input, and that entry is N * (alignment's blank share - b): the share to put
# here is b + g / N.  (Found that way on the emulator: 0.533 for 5 labels on 12 frames, 0.502 for 83 labels on 200 frames; the
# largest entry left is then a softmax bias of about 25 at both sizes, a quarter of the bound.)
MFMA_NI, MFMA_NH, MFMA_NC = 48, [100], 83
MFMA_BLANK_SHARE_12, MFMA_BLANK_SHARE_200 = 0.532, 0.5


def mfma_case(backend, path, nlines, T, L, blank_share, steps):
    nh = MFMA_NH
    rng = np.random.default_rng(nlines)
    net = make_net(backend, MFMA_NI, nh, MFMA_NC, False, 0, 1.0)
    p = net.get_params()
    nsm = MFMA_NC * (2 * nh[-1] + 1)                       # the softmax layer closes the flat layout; its first entry is the blank bias
    p[p.size - nsm] = np.log(blank_share / (1.0 - blank_share) * (MFMA_NC - 1))
    net.set_params(p)
    # every parameter moves by 100 lr per step: 1e-4 against weights of order 1e-2, so the second step (train_step_next) still finds
    # the small activations and the calibrated blank output that keep its gradient below 100.  (lr 1e-4 is too large: a step of
    # 1e-2 on every weight left a second-step gradient entry of 143 on the emulator.  Should max |g| of the SECOND step alone reach
    # 100 after a change to the inputs, lower lr: the expected values scale with it and stay exact.)
    lr = 1e-6
    net.setLearningRate(lr, 0.9)
    batches = [make_batch(backend, rng, MFMA_NI, MFMA_NC, [T] * nlines, L=L) for _ in range(steps)]
    f0, b0 = count(backend, 16), count(backend, 17)
    what = "%d lines x %d frames %s" % (nlines, T, path)
    gmax = drive(backend, net, path, batches, "pm200", rng,
                 lambda v0, d0, g, v1, d1, w: assert_every_entry_once(v0, d0, g, v1, d1, lr, 0.9, w), what)
    if backend.kind == "hip" and nlines >= 640:            # (the emulator build has no MFMA kernels: it runs the per-line ones)
        assert count(backend, 16) - f0 == steps and count(backend, 17) - b0 == steps, "the batched-MFMA recurrences did not run"
    print("max |g|, %s: %s" % (what, ["%.3g" % x for x in gmax]))


@pytest.mark.parametrize("path", PATHS)
def test_every_parameter_once_batched_mfma_640_lines(backend, path):
    """640 lines of 12 frames: on the GPU the library's own rule sends them through the batched-MFMA recurrences (the geometry of
    test_mfma_recurrence.py::test_mfma_default_rule_at_chip_filling_minibatches), whose weight-gradient slabs feed the reductions"""
    mfma_case(backend, path, 640, 12, 5, MFMA_BLANK_SHARE_12, 2 if path == "train_step_next" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_every_parameter_once_batched_mfma_64_long_lines(path):
    """64 lines of 200 frames, the per-line recurrences at bench length (GPU only: minutes on the emulator)"""
    from common import Backend
    mfma_case(Backend("hip"), path, 64, 200, 83, MFMA_BLANK_SHARE_200, 2)


# ---- (c) packed copies follow the clipped value ---------------------------------------------------------------------------------
@pytest.mark.parametrize("uni", [False, True], ids=["bidi", "lstm1"])
def test_packed_copies_take_the_clipped_value(backend, uni):
    """A single narrow layer under clstm_net_train_step: the thread that moves v[o] also rewrites the packed copies of parameter
    o that the next forward pass reads (ops.h: PackDst), and nothing repacks them.  In the saturated regime those copies must
    hold the CLIPPED update: the forward pass of the stepped net on a fresh minibatch equals, bit for bit, that of a new net
    given set_params(get_params()) -- which packs from the flat parameters."""
    from clstm_amd.net import Network
    nh, lr, mom, clip = [10], 1e-2, 0.9, 100.0
    rng = np.random.default_rng(47)
    net = make_net(backend, NI, nh, NC, uni, 0, 20.0)
    net.setLearningRate(lr, mom)
    for k, T in enumerate(T_SMALL):
        batch = make_batch(backend, rng, NI, NC, T)
        d0 = make_derivs("u150", rng, net.nparams)
        net.set_derivs(d0)
        v0 = net.get_params()
        kept = count(backend, 10)
        run_step(net, "train_step", batch)
        backend.sync()
        assert count(backend, 10) - kept == 1, "the fused update did not rewrite the packed copies"
        v1 = net.get_params()
        share = assert_rule(v0, d0, net.get_grads(), v1, net.get_derivs(), lr, mom, clip, "step %d" % k)
        assert 0.2 <= share <= 0.8, "inconclusive: %.3f of the entries beyond the clip" % share
        fresh = synth_lines(rng, [8, 3, 10], NI)
        net.set_inputs(fresh)
        net.forward()
        got = net.outputs()
        other = Network(NI, nh, NC, unidirectional=uni, lib=backend.lib)
        other.set_params(v1)
        other.set_inputs(fresh)
        other.forward()
        assert np.array_equal(bits(got), bits(other.outputs())), "step %d: the packed copies are not the clipped parameters" % k


# ---- (d) saturated trajectory against the oracle --------------------------------------------------------------------------------
TRAJ_SEED, TRAJ_SCALE = 53, 30.0


def oracle_trajectory(ora32, nh, nsteps=4, lr=5e-2, mom=0.9):
    """The oracle's own saturated run: the clip is the median of |derivs| it holds before its FIRST update (d + g accumulated, not
    yet clipped).  Returns clip, the minibatches, the parameters / derivs after every step and the share of pre-clip entries
    beyond the clip at every step."""
    rng = np.random.default_rng(TRAJ_SEED)
    ref = OracleNet(ora32, NI, nh, NC, seed=0.222)
    p0 = ref.get_params() * TRAJ_SCALE
    ref.set_params(p0)
    ref.set_lr(lr, mom)
    clip, data, after, shares = None, [], [], []
    for step in range(nsteps):
        T = [int(t) for t in rng.integers(4, 12, 3)]
        lines = synth_lines(rng, T, NI)
        trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
        for x, tr in zip(lines, trs):
            ref.set_inputs(x); ref.forward(); ref.ctc_deltas(tr); ref.backward()
        pre = np.abs(ref.get_derivs())
        if clip is None:
            clip = float(np.median(pre))
            ref.set_gradient_clip(clip)
        shares.append(float((pre > clip).mean()))
        ref.update()
        data.append((T, lines, trs))
        after.append((ref.get_params(), ref.get_derivs()))
    return p0, clip, data, after, shares


@pytest.mark.parametrize("nh", [[10], [7, 5]], ids=["h10", "h7_5"])
def test_oracle_saturated_trajectory_is_conclusive(ora32, nh):
    """the condition of the trajectory test on the oracle alone (CPU): at every step 10..90 % of its pre-clip entries exceed the clip"""
    _, clip, _, _, shares = oracle_trajectory(ora32, nh)
    print("clip %g, shares beyond it per step: %s" % (clip, ["%.3f" % s for s in shares]))
    assert clip > 0 and all(0.1 <= s <= 0.9 for s in shares), (clip, shares)


@pytest.mark.parametrize("path", ["calls", "train_step"])
@pytest.mark.parametrize("nh", [[10], [7, 5]], ids=["h10", "h7_5"])
def test_saturated_trajectory_matches_the_oracle(backend, ora32, nh, path):
    """Four steps with momentum 0.9 under a clip that bites at every step, against the oracle with the same clip.  Tolerances of
    test_net_parity.py::test_second_step_momentum: the clamp is continuous, entries near the threshold need no allowance."""
    from clstm_amd.net import Network
    lr, mom = 5e-2, 0.9
    p0, clip, data, after, shares = oracle_trajectory(ora32, nh)
    assert all(0.1 <= s <= 0.9 for s in shares), "inconclusive: %r" % (shares,)
    net = Network(NI, nh, NC, lib=backend.lib)
    net.set_params(p0)
    net.setLearningRate(lr, mom)
    net.set_gradient_clip(clip)
    for step, (T, lines, trs) in enumerate(data):
        x = np.ascontiguousarray(np.concatenate(lines, 0), F32)
        run_step(net, path, {"T": T, "trs": trs, "x": x, "xd": backend.up(x), "prep": Network.prepare_step(T, trs)})
        backend.sync()
        assert_close(net.get_params(), after[step][0], rtol=2e-5, atol=2e-7, what="params step %d" % step)
        assert_close(net.get_derivs(), after[step][1], rtol=1e-4, atol=1e-9, scale_atol=2e-4, what="derivs step %d" % step)


# ---- (e) the setter, and the per-operator entry points --------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["calls", "train_step"])
def test_refused_clip_leaves_the_previous_one(backend, path):
    """clstm_net_set_gradient_clip refuses 0, a negative value and NaN with a message in clstm_last_error; the clip set before
    still governs the next step."""
    nh, uni, precision, scale, lr = NETS["h10"]
    rng = np.random.default_rng(59)
    net = make_net(backend, NI, nh, NC, uni, precision, scale)
    net.setLearningRate(lr, 0.9)
    net.set_gradient_clip(40.0)
    for bad in (0.0, -3.0, float("nan")):
        rc = backend.lib.dll.clstm_net_set_gradient_clip(net.h, bad)
        assert rc != 0, bad
        assert b"clip must be positive" in backend.lib.dll.clstm_last_error(), bad
        with pytest.raises(Exception, match="clip must be positive"):
            net.set_gradient_clip(bad)
    batches = [make_batch(backend, rng, NI, NC, T_SMALL[0])]
    shares = drive(backend, net, path, batches, "u150", rng,
                   lambda v0, d0, g, v1, d1, w: assert_rule(v0, d0, g, v1, d1, lr, 0.9, 40.0, w), "clip 40 " + path)
    assert 0.6 <= shares[0] <= 0.85          # U(-150, 150) against +-40: 73 % beyond


GRID_THREADS = 4096 * 256                                 # runtime.inc: nblocks() caps a launch at 4096 workgroups of 256 threads


def test_clip_and_sgd_operators_beyond_one_grid(backend, ora32):
    """clstm_clip_gradient / clstm_sgd_update against the oracle's clip_gradient / sgd_update (clstm_compute.cc:553-563) on
    4096 * 256 + 259 entries.  The launch is capped at 4096 workgroups of 256 threads, so entries from index 1 048 576 on are
    reached only by the second turn of the grid-stride loop (1 000 003 entries would still fit one turn: 3907 workgroups), and the
    length is no multiple of the workgroup size.  Entries at exactly +-clip, one float32 beyond +-clip and +-inf are planted on
    both sides of that index.  Clip: bit for bit.  Update: d' bit for bit, v' the unfused or the fused value (the oracle's own
    compiler makes the same choice one way or the other)."""
    from clstm_amd.abi import ptr
    G = GRID_THREADS
    n, clip, lr, mom = G + 259, F32(100.0), F32(1e-2), F32(0.9)
    rng = np.random.default_rng(61)
    d0 = rng.uniform(-300, 300, n).astype(F32)
    above = np.nextafter(clip, F32(np.inf))
    #            first turn of the loop               second turn
    planted = {
        clip:    [0, 255, 256, 1000, G - 1,           G, G + 100, n - 1],
        -clip:   [1, 257, 1001, G - 2,                G + 1, G + 101, n - 2],
        np.inf:  [2, 1002, G - 3,                     G + 2, G + 102, n - 3],
        -np.inf: [3, 1003, G - 4,                     G + 3, G + 103, n - 4],
        above:   [4, G - 5,                           G + 4, n - 5],
        -above:  [5, G - 6,                           G + 5, n - 6],
    }
    at = np.concatenate([np.asarray(i) for i in planted.values()])
    assert at.size == np.unique(at).size and at.max() == n - 1 and n > G and n % 256
    for value, idx in planted.items():
        d0[idx] = value
    v0 = rng.normal(0, 0.3, n).astype(F32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d_ref = d0.copy()
    ora32.lib.ora_clip_gradient(P(d_ref), n, clip)
    assert np.array_equal(d_ref, np.clip(d0, -clip, clip)) and np.abs(d_ref).max() == clip
    d = backend.up(d0)
    backend.lib.call("clstm_clip_gradient", ptr(d), n, 1e6)                 # switched off: +-inf stay
    assert np.array_equal(bits(backend.down(d)), bits(d0))
    backend.lib.call("clstm_clip_gradient", ptr(d), n, float(clip))
    got = backend.down(d)
    bad = np.flatnonzero(bits(got) != bits(d_ref))
    assert bad.size == 0, "clip differs at %d entries, first %d (second turn from %d): got %r want %r" % (bad.size, bad[0], G, got[bad[0]], d_ref[bad[0]])
    with pytest.raises(Exception, match="clip must be positive"):
        backend.lib.call("clstm_clip_gradient", ptr(d), n, 0.0)
    v_ref = v0.copy()
    d_ref2 = d_ref.copy()
    ora32.lib.ora_sgd_update(P(v_ref), P(d_ref2), n, lr, mom)
    want = update_of_clamped(v0, d_ref, lr, mom)
    assert_update_bits(v_ref, d_ref2, want, "the oracle's sgd_update against the statement", v0=v0, di=d_ref)
    v = backend.up(v0)
    backend.lib.call("clstm_sgd_update", ptr(v), ptr(d), n, float(lr), float(mom))
    assert_update_bits(backend.down(v), backend.down(d), want, "clstm_sgd_update (second turn from index %d)" % G, v0=v0, di=d_ref)
