"""What one training step leaves behind when a call fails: nothing.  The plan of a step (update fused into the reductions, gradient
into the peer slot, last reduction held back for the next minibatch's ingest, host-fed step word) is a value of that call; a call
that fails on the next minibatch, on its own transcripts, or in a host-fed step must leave the following calls -- one-call steps and
the sequence of separate calls alike -- equal, byte for byte, to a twin net that only ever ran plain clstm_net_train_step."""
import ctypes

import numpy as np
import pytest

from common import synth_lines

NI, NC = 8, 7
pytestmark = pytest.mark.parametrize("nh", [[10], [7, 5]])


def _twins(backend, nh):
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    p0 = init_params(NI, nh, NC, seed=0.222) * 20
    a, b = Network(NI, nh, NC, lib=backend.lib), Network(NI, nh, NC, lib=backend.lib)
    for n in (a, b):
        n.set_params(p0)
        n.setLearningRate(1e-2, 0.9)
    return a, b


def _batch(backend, rng, nlines, bad=False):
    """(prep, frames on the device, frames on the host, T, transcripts); bad: one label past the last class, or ("size") a negative
    line length"""
    from clstm_amd.net import Network
    T = [int(t) for t in rng.integers(3, 12, nlines)]
    trs = [rng.integers(1, NC, max(1, t // 3)).astype(np.int32) for t in T]
    x = np.ascontiguousarray(np.concatenate(synth_lines(rng, T, NI), 0), np.float32)
    if bad == "size":
        T[-1] = -T[-1]
    elif bad:
        trs[-1][0] = NC + 3
    return Network.prepare_step(T, trs), backend.up(x), x, T, trs


def _with_bad_label(batch):
    from clstm_amd.net import Network
    prep, xd, x, T, trs = batch
    bad = [t.copy() for t in trs]
    bad[0][0] = NC + 3
    return Network.prepare_step(T, bad), xd, x, T, bad


def _count(backend, i):
    out = ctypes.c_longlong(0)
    backend.lib.call("clstm_debug_path_count", i, ctypes.byref(out))
    return out.value


def _same(a, b, what):
    assert a.get_params().tobytes() == b.get_params().tobytes(), what
    assert a.get_derivs().tobytes() == b.get_derivs().tobytes(), what


def _separate_calls(net, batch):
    prep, xd, x, T, trs = batch
    net.set_batch(T)
    net.set_inputs_device(xd)
    net.forward()
    net.ctc(trs)
    net.backward()
    net.update()


def _bad_next_minibatch(backend, nh, how, text):
    rng = np.random.default_rng(31)
    a, b = _twins(backend, nh)
    g0, bad, g1 = _batch(backend, rng, 3), _batch(backend, rng, 2, bad=how), _batch(backend, rng, 4)
    a.train_step_prepared(g0[0], g0[1])
    tails = _count(backend, 19)
    b.train_step_prepared(g0[0], g0[1], bad[0], bad[1])
    assert _count(backend, 19) == tails
    _same(a, b, "the step that declared a bad next minibatch")
    # the refused minibatch touched nothing: step k's minibatch is the current one and its outputs are addressable
    assert b.holds() == [3, sum(g0[3]), 1, 1, 1, 2, 1, 0]
    assert b.outputs().tobytes() == a.outputs().tobytes()
    assert [d.tolist() for d in b.decode()] == [d.tolist() for d in a.decode()]
    with pytest.raises(Exception, match=text):
        b.train_step_prepared(bad[0], bad[1])
    a.train_step_prepared(g1[0], g1[1])
    b.train_step_prepared(g1[0], g1[1])
    _same(a, b, "a good step after the refused one")


def test_bad_next_minibatch_does_not_fail_the_step_that_declared_it(backend, nh):
    """A step declares a next minibatch with a label out of range: the step itself completes (no ingest tail is launched for
    it: counter 19 stays) and still holds its own minibatch -- outputs and decode equal the twin's --, the call that brings the bad
    minibatch as its current one reports the error, and a good step afterwards equals the twin again."""
    _bad_next_minibatch(backend, nh, True, "out of range")


def test_next_minibatch_bad_by_size_does_not_fail_the_step_that_declared_it(backend, nh):
    """The same with a next minibatch that is bad by size: a negative line length."""
    _bad_next_minibatch(backend, nh, "size", "negative line length")


def test_failed_step_after_a_good_declaration_leaves_no_plan_behind(backend, nh):
    """Step k declares k+1; the k+1 call arrives with a bad label in its own transcripts: it does not match the declaration, takes
    the ordinary path and raises.  The sequence of separate calls on the good minibatch then equals the twin."""
    rng = np.random.default_rng(37)
    a, b = _twins(backend, nh)
    g0, g1, g2 = _batch(backend, rng, 2), _batch(backend, rng, 3), _batch(backend, rng, 4)
    a.train_step_prepared(g0[0], g0[1])
    b.train_step_prepared(g0[0], g0[1], g1[0], g1[1])
    _same(a, b, "step k, which declared k+1")
    bad1 = _with_bad_label(g1)
    with pytest.raises(Exception, match="out of range"):
        b.train_step_prepared(bad1[0], bad1[1], g2[0], g2[1])
    a.train_step_prepared(g1[0], g1[1])
    _separate_calls(b, g1)
    _same(a, b, "the sequence of calls after the failed step")
    a.train_step_prepared(g2[0], g2[1])
    b.train_step_prepared(g2[0], g2[1])
    _same(a, b, "a one-call step after that")


def test_host_fed_steps_after_a_failed_one(backend, nh):
    """A failing clstm_net_train_step_h, then the sequence of separate calls, then good host-fed steps (enough of them that a
    step waits for the word of the step two before it): every good step equals the twin's.  A committed host-fed step whose
    kernels had not taken the step word raises; none of these does."""
    rng = np.random.default_rng(41)
    a, b = _twins(backend, nh)
    g = [_batch(backend, rng, 2 + k % 3) for k in range(4)]
    bad0 = _with_bad_label(g[0])
    with pytest.raises(Exception, match="out of range"):
        b.train_step_host(bad0[0], bad0[2])
    a.train_step_prepared(g[0][0], g[0][1])
    _separate_calls(b, g[0])
    _same(a, b, "the sequence of calls after a failed host-fed step")
    for k in (1, 2, 3):
        a.train_step_prepared(g[k][0], g[k][1])
        b.train_step_host(g[k][0], g[k][2])
        _same(a, b, "host-fed step %d" % k)
