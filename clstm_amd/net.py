"""Host-side mirror of the reference's network interface for the hot path.

Names follow the reference: `make_net("bidi"|"bidi2"|"lstm1", ...)` (clstm_prefab.cc:163-173),
`INetwork.forward()/backward()`, `sgd_update(net)` (clstm.cc:201-217), `set_inputs`,
`ctc_align_targets`, `trivial_decode` (clstm.h:310-320), `get_params/set_params/get_derivs`
(clstm.cc:872-917) and `CLSTMOCR` (clstmhl.h:146-272).  All arithmetic happens in
libclstm_hip.so; this file only moves pointers and small host arrays.
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import NetDesc, f32, i32, ptr

STATE_CODES = {"gi": 0, "gf": 1, "go": 2, "ci": 3, "state": 4, "outputs": 5,
               "d_gi": 6, "d_gf": 7, "d_go": 8, "d_ci": 9}


class Network:
    """Stacked{Parallel{NPLSTM, Reversed{NPLSTM}} x L, SoftmaxLayer} on one MI355X.

    A minibatch is a list of text lines (line b has T_b frames of `ninput` features);
    frames are packed line after line ("frame-major", feature contiguous).
    """

    def __init__(self, ninput, nhidden, nclasses, unidirectional=False, lib=None,
                 params=None, derivs=None, grads=None):
        self.lib = lib or abi.load()
        self.nhidden = list(nhidden) if isinstance(nhidden, (list, tuple)) else [int(nhidden)]
        self.ninput, self.nclasses, self.unidirectional = int(ninput), int(nclasses), bool(unidirectional)
        d = NetDesc()
        d.nlayers = len(self.nhidden)
        d.unidirectional = int(self.unidirectional)
        d.ninput = self.ninput
        d.nclasses = self.nclasses
        for i, h in enumerate(self.nhidden):
            d.nhidden[i] = int(h)
        self.desc = d
        self.nparams = self.lib.call("clstm_net_nparams_for", C.byref(d))
        for buf in (params, derivs, grads):
            if buf is not None:
                assert buf.numel() == self.nparams and buf.is_contiguous()
        self._keep = (params, derivs, grads)    # caller-owned device buffers stay alive
        h = C.c_void_p()
        self.lib.call("clstm_net_create", C.byref(h), C.byref(d), ptr(params), ptr(derivs), ptr(grads))
        self.h = h
        self._holds = (C.c_int * 8)()
        self.T = []
        self.N = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.call("clstm_net_destroy", self.h)
                self.h = None
        except Exception:
            pass

    # -- parameters: get_params / set_params / get_derivs (clstm.cc:872-917) -------------
    def set_params(self, a):
        a = f32(a)
        assert a.size == self.nparams
        self.lib.call("clstm_net_set_params_h", self.h, ptr(a))

    def get_params(self):
        a = np.empty(self.nparams, np.float32)
        self.lib.call("clstm_net_get_params_h", self.h, ptr(a))
        return a

    def set_derivs(self, a):
        a = f32(a)
        assert a.size == self.nparams
        self.lib.call("clstm_net_set_derivs_h", self.h, ptr(a))

    def get_derivs(self):
        a = np.empty(self.nparams, np.float32)
        self.lib.call("clstm_net_get_derivs_h", self.h, ptr(a))
        return a

    def get_grads(self):
        a = np.empty(self.nparams, np.float32)
        self.lib.call("clstm_net_get_grads_h", self.h, ptr(a))
        return a

    def params_changed(self):
        self.lib.call("clstm_net_params_changed", self.h)

    def setLearningRate(self, lr, momentum):          # INetwork::setLearningRate clstm.cc:158
        self.lib.call("clstm_net_set_learning_rate", self.h, float(lr), float(momentum))

    def set_gemm_precision(self, mode):
        """0: exact f32 MFMA (default, the parity path); 1: bf16 inputs / f32 accumulation for the hoisted
        gate GEMMs (BASELINE config '2 x BiLSTM(512), bf16 MFMA')."""
        self.lib.call("clstm_net_set_gemm_precision", self.h, int(mode))

    def set_gradient_clip(self, clip):
        self.lib.call("clstm_net_set_gradient_clip", self.h, float(clip))

    # -- data ------------------------------------------------------------------------------
    def holds(self):
        """What the library says the net holds (clstm_debug_net_holds): [bs, N, batch, training_buffers, forward, frames,
        offsets_sent, dx0] -- the record is the library's; this class keeps no copy of it."""
        self.lib.call("clstm_debug_net_holds", self.h, self._holds)
        return list(self._holds)

    def _held(self, T, holds=None):
        """T / N of the minibatch the library holds; T, the caller's line lengths of that minibatch, only splits N by lines."""
        bs, N = (holds or self.holds())[:2]
        assert len(T) == bs and sum(T) == N, "the library holds another minibatch"
        self.T, self.N = list(T), N

    def set_batch(self, T):
        self.T = [int(t) for t in T]
        self.N = int(sum(self.T))
        t = i32(self.T)
        self.lib.call("clstm_net_set_batch", self.h, ptr(t), len(self.T))

    def set_inputs(self, lines):
        """lines: list of [T_b, ninput] arrays (set_inputs, clstm.cc:684-690), or a packed [N, ninput]
        array after an explicit set_batch()."""
        if isinstance(lines, (list, tuple)):
            self.set_batch([len(x) for x in lines])
            x = f32(np.concatenate([f32(x).reshape(-1, self.ninput) for x in lines], 0))
        else:
            x = f32(lines)
        assert x.shape == (self.holds()[1], self.ninput)    # (the library's N: a declared next minibatch is adopted by this call)
        self.lib.call("clstm_net_set_inputs_h", self.h, ptr(x))

    def set_inputs_device(self, x_dev):
        self.lib.call("clstm_net_set_inputs_d", self.h, ptr(x_dev))

    def forward(self):
        self.lib.call("clstm_net_forward", self.h)
        self._held(self.T)                        # (a minibatch declared by the last train step has become the current one)

    def outputs(self):
        p = np.empty((self.N, self.nclasses), np.float32)
        self.lib.call("clstm_net_get_outputs_h", self.h, ptr(p))
        return p

    def split(self, packed):
        out, o = [], 0
        for t in self.T:
            out.append(packed[o:o + t])
            o += t
        return out

    def set_output_deltas(self, d):
        d = f32(d)
        assert d.shape == (self.N, self.nclasses)
        self.lib.call("clstm_net_set_output_deltas_h", self.h, ptr(d))

    def ctc(self, transcripts, want_aligned=False):
        """mktargets + ctc_align_targets + `outputs.d = aligned - outputs.v` for every line
        (clstmhl.h:207-212)."""
        assert len(transcripts) == len(self.T)
        L = i32([len(t) for t in transcripts])
        flat = [int(c) for t in transcripts for c in t]
        labels = i32(flat if flat else [0])
        al = np.empty((self.N, self.nclasses), np.float32) if want_aligned else None
        self.lib.call("clstm_net_ctc", self.h, ptr(labels), ptr(L), ptr(al))
        return al

    def _score(self, transcripts, lines, want_score, want_vscore, want_path):
        """clstm_net_score: candidate k is scored against line lines[k] of the current minibatch (None: one per line)."""
        if lines is None:
            assert len(transcripts) == len(self.T)
            cl = None
            T = self.T
        else:
            assert len(lines) == len(transcripts)
            cl = i32(lines)
            T = [self.T[b] if 0 <= b < len(self.T) else 0 for b in cl.tolist()]   # (the library refuses a bad index)
        n = len(transcripts)
        L = i32([len(t) for t in transcripts])
        flat = [int(c) for t in transcripts for c in t]
        labels = i32(flat if flat else [0])
        score = np.empty(n, np.float32) if want_score else None
        vscore = np.empty(n, np.float32) if want_vscore else None
        path = np.empty(max(1, int(sum(T))), np.int32) if want_path else None
        self.lib.call("clstm_net_score", self.h, ptr(labels), ptr(L), ptr(cl), n, ptr(score), ptr(vscore), ptr(path))
        paths = None
        if want_path:
            paths, o = [], 0
            for t in T:
                paths.append(path[o:o + t].copy())
                o += t
        return score, vscore, paths

    def score(self, transcripts, lines=None, viterbi=False):
        """Per-candidate CTC score of `transcripts` against the current minibatch's outputs: the last cell of the reference's
        forward_algorithm (ctc.cc:24-40; unnormalised, see include/clstm_abi.h).  lines: the line of each candidate (None: one
        transcript per line).  viterbi=True: -> (score, vscore), vscore the best single path's score."""
        s, v, _ = self._score(transcripts, lines, True, viterbi, False)
        return (s, v) if viterbi else s

    def align(self, transcripts, lines=None):
        """Forced alignment: per candidate the state index occupied at every frame of its line on a best path (label k is
        state 2k + 1, blanks the even states; -1 on frames before a late start).  See spans()."""
        return self._score(transcripts, lines, False, False, True)[2]

    def beam(self, beam=8, nbest=None):
        """The n best transcripts of every line of the current minibatch by CTC prefix beam search (clstm_net_beam; the algorithm
        in clstm_amd/csrc/ctc_beam.h).  Per line a list of (labels array, score), best first; score is the log-probability the
        beam gathered for that labelling -- not on the scale of score().  nbest defaults to beam."""
        nbest = beam if nbest is None else nbest
        bs = len(self.T)
        nhyp = np.zeros(bs, np.int32)
        ln = np.zeros(max(1, bs * nbest), np.int32)
        sc = np.zeros(max(1, bs * nbest), np.float32)
        lab = np.zeros(max(1, nbest * self.N), np.int32)
        self.lib.call("clstm_net_beam", self.h, int(beam), int(nbest), ptr(nhyp), ptr(ln), ptr(sc), ptr(lab))
        return unpack_beam(self.T, nbest, nhyp, ln, sc, lab)

    def beam_lm(self, lm, weight, bonus=0.0, beam=8, nbest=None):
        """beam() with a character n-gram language model (clstm_amd.lm.CharLM) inside the search (clstm_net_beam_lm; the algorithm
        in clstm_amd/csrc/ctc_beam.h, second part).  Per line a list of (labels array, score, am_score), best first: score is
        what was ranked -- am_score plus the labelling's weighted LM value, bonus and end term --, am_score the acoustic
        log-probability beam() reports."""
        nbest = beam if nbest is None else nbest
        bs = len(self.T)
        nhyp = np.zeros(bs, np.int32)
        ln = np.zeros(max(1, bs * nbest), np.int32)
        sc = np.zeros(max(1, bs * nbest), np.float32)
        am = np.zeros(max(1, bs * nbest), np.float32)
        lab = np.zeros(max(1, nbest * self.N), np.int32)
        self.lib.call("clstm_net_beam_lm", self.h, int(beam), int(nbest), lm.handle(self.lib), float(weight), float(bonus),
                      ptr(nhyp), ptr(ln), ptr(sc), ptr(am), ptr(lab))
        return unpack_beam(self.T, nbest, nhyp, ln, sc, lab, am)

    def beam_lex(self, lexicon, beam=8, nbest=None, lm=None, weight=0.0, bonus=0.0):
        """beam_lm() constrained to a lexicon (clstm_amd.lexicon.Lexicon; clstm_net_beam_lex; the algorithm in
        clstm_amd/csrc/ctc_beam.h, third part): every run of word classes of a transcript is a word of the lexicon.  lm (a CharLM)
        is optional; without one score = am_score + bonus * length.  Returns what beam_lm() returns; a line on which no admissible
        labelling survived has an empty list."""
        nbest = beam if nbest is None else nbest
        bs = len(self.T)
        nhyp = np.zeros(bs, np.int32)
        ln = np.zeros(max(1, bs * nbest), np.int32)
        sc = np.zeros(max(1, bs * nbest), np.float32)
        am = np.zeros(max(1, bs * nbest), np.float32)
        lab = np.zeros(max(1, nbest * self.N), np.int32)
        self.lib.call("clstm_net_beam_lex", self.h, int(beam), int(nbest), lexicon.handle(self.lib),
                      None if lm is None else lm.handle(self.lib), float(weight), float(bonus),
                      ptr(nhyp), ptr(ln), ptr(sc), ptr(am), ptr(lab))
        return unpack_beam(self.T, nbest, nhyp, ln, sc, lab, am)

    def errors(self, transcripts, counts=False, confusion=False):
        """Edit distance of every line's trivial_decode against its transcript, computed where the decoded classes lie on the
        device (clstm_net_errors).  transcripts: one label sequence per line; label `nclasses` stands for a character outside the
        codec and matches nothing.  -> dist [bs]; with counts / confusion: (dist[, counts [bs, 3] = substitutions, insertions,
        deletions][, confusion [nclasses + 1, nclasses + 1], rows = reference label, columns = output label, row / column 0 =
        insertions / deletions])."""
        assert len(transcripts) == len(self.T)
        bs, nsym = len(self.T), self.nclasses + 1
        L = i32([len(t) for t in transcripts])
        flat = [int(c) for t in transcripts for c in t]
        labels = i32(flat if flat else [0])
        dist = np.zeros(bs, np.int32)
        cnt = np.zeros((bs, 3), np.int32) if counts else None
        conf = np.zeros((nsym, nsym), np.int32) if confusion else None
        self.lib.call("clstm_net_errors", self.h, ptr(labels), ptr(L), ptr(dist), ptr(cnt), ptr(conf))
        out = (dist,) + ((cnt,) if counts else ()) + ((conf,) if confusion else ())
        return out if len(out) > 1 else dist

    def backward(self):
        self.lib.call("clstm_net_backward", self.h)

    def enable_input_deltas(self, on=True):
        self.lib.call("clstm_net_enable_input_deltas", self.h, int(on))

    def input_deltas(self):
        d = np.empty((self.N, self.ninput), np.float32)
        self.lib.call("clstm_net_get_input_deltas_h", self.h, ptr(d))
        return d

    def update(self):                                   # sgd_update(Network) clstm.cc:201-217
        self.lib.call("clstm_net_update", self.h)

    def train_step(self, T, x_dev, transcripts):
        """CLSTMOCR::train (clstmhl.h:201-223) for a minibatch resident in HBM, ONE library call:
        set_batch + set_inputs + forward + CTC + backward + [all-reduce] + update, no host sync."""
        self.train_step_prepared(self.prepare_step(T, transcripts), x_dev)

    @staticmethod
    def prepare_step(T, transcripts):
        """Host arrays of one minibatch in the form the C ABI takes (line lengths, packed transcripts, their
        lengths) -- build once per minibatch, outside any timed loop."""
        Tl = [int(t) for t in T]
        assert len(transcripts) == len(Tl)
        L = i32([len(tr) for tr in transcripts])
        flat = np.concatenate([i32(tr).reshape(-1) for tr in transcripts]) if len(transcripts) else i32([])
        return Tl, i32(Tl), i32(flat if flat.size else [0]), L

    def train_step_prepared(self, prep, x_dev, next_prep=None, next_x_dev=None):
        """clstm_net_train_step; with the NEXT minibatch given (same forms), clstm_net_train_step_next: its ingest rides this
        step's last launch and the next call -- which must pass that very minibatch -- starts with its forward launch."""
        Tl, t, labels, L = prep
        self.T, self.N = Tl, int(sum(Tl))
        if next_prep is None:
            self.lib.call("clstm_net_train_step", self.h, ptr(t), len(Tl), ptr(x_dev), ptr(labels), ptr(L))
        else:
            nTl, nt, nlabels, nL = next_prep
            self.lib.call("clstm_net_train_step_next", self.h, ptr(t), len(Tl), ptr(x_dev), ptr(labels), ptr(L),
                          ptr(nt), len(nTl), ptr(next_x_dev), ptr(nlabels), ptr(nL))
            # the geometry is the declared next minibatch's now -- unless the library refused it, or had no tail to declare it with
            holds = self.holds()
            self._held(nTl if holds[2] == 2 else Tl, holds)

    def train_step_host(self, prep, x_host):
        """The same step fed from host memory (numpy array or pinned torch tensor [sum T, ninput]): the frames travel on a
        copy stream while the previous step computes (clstm_net_train_step_h)."""
        Tl, t, labels, L = prep
        self.T, self.N = Tl, int(sum(Tl))
        self.lib.call("clstm_net_train_step_h", self.h, ptr(t), len(Tl), ptr(x_host), ptr(labels), ptr(L))

    def replica_check(self):
        """Enqueue the replica-consistency check (parameter checksum all-reduced over the attached communicator; collective).
        A mismatch surfaces at the next synchronisation point as 'replicas diverged'.  The library also runs it by itself
        every CLSTM_REPLICA_CHECK_EVERY updates.  Reference: distribute_weights (clstm.cc:718-729) re-syncs instead."""
        self.lib.call("clstm_net_replica_check", self.h)

    def set_training(self, on):
        """False: forward passes of this net belong to no training step (predict): a non-finite logit does not arm the
        device NaN flag that blocks updates (the reference asserts in backward only, clstm.cc:630-649)."""
        self.lib.call("clstm_net_set_training", self.h, int(bool(on)))

    def set_comm(self, comm):
        """Attach a `Comm` (RCCL): update()/train_step() all-reduce the fresh gradient first."""
        self._comm = comm
        self.lib.call("clstm_net_set_comm", self.h, comm.h if comm is not None else None)

    # -- state externalisation: n_states / get_states / set_states (clstm.cc:762-811) --------
    def n_states(self):
        n = C.c_longlong()
        self.lib.call("clstm_net_n_states", self.h, C.byref(n))
        return n.value

    def get_states(self):
        a = np.empty(self.n_states(), np.float32)
        self.lib.call("clstm_net_get_states_h", self.h, ptr(a), a.size)
        return a

    def set_states(self, a):
        a = f32(a)
        self.lib.call("clstm_net_set_states_h", self.h, ptr(a), a.size)
        self.T = [int(a[1])] * int(a[3])
        self.N = sum(self.T)

    def decode(self):
        """trivial_decode (ctc.cc:159-190) of every line -> list of int arrays."""
        cls = np.zeros(self.N, np.int32)
        loc = np.zeros(self.N, np.int32)
        cnt = np.zeros(len(self.T), np.int32)
        self.lib.call("clstm_net_decode", self.h, ptr(cls), ptr(loc), ptr(cnt))
        out, o = [], 0
        for b, t in enumerate(self.T):
            out.append(cls[o:o + cnt[b]].copy())
            o += t
        return out

    def predict(self, lines):
        """CLSTMOCR::predict (clstmhl.h:225-262) for a whole minibatch in one call (clstm_net_predict_h): the forward pass in
        its no-save form + trivial_decode.  lines: list of [T_b, ninput] arrays.  Returns (decodes, locs, confs), one array per
        line each: the classes, their frames, and the softmax output at (frame, class).  The minibatch is the current one
        afterwards (outputs(), decode(), state(.., 'outputs')); nothing was saved for a backward pass."""
        self.T = [len(x) for x in lines]
        self.N = int(sum(self.T))
        x = f32(np.concatenate([f32(x).reshape(-1, self.ninput) for x in lines], 0))
        t = i32(self.T)
        cls, loc = np.zeros(self.N, np.int32), np.zeros(self.N, np.int32)
        conf, cnt = np.zeros(self.N, np.float32), np.zeros(len(self.T), np.int32)
        self.lib.call("clstm_net_predict_h", self.h, ptr(t), len(self.T), ptr(x), ptr(cls), ptr(loc), ptr(conf), ptr(cnt))
        dec, locs, confs, o = [], [], [], 0
        for b, tb in enumerate(self.T):
            dec.append(cls[o:o + cnt[b]].copy())
            locs.append(loc[o:o + cnt[b]].copy())
            confs.append(conf[o:o + cnt[b]].copy())
            o += tb
        return dec, locs, confs

    def predict_images(self, images, normalizer):
        """predict() for RAW line images (ink = 1, [w, h] arrays): normalised on the device by `normalizer` (Normalizer.run_device),
        the frames handed to clstm_net_predict where they lie.  Returns what predict() returns."""
        T, _, frames_d = normalizer.run_device(images)
        self.T = [int(t) for t in T]
        self.N = int(sum(self.T))
        cls, loc = np.zeros(self.N, np.int32), np.zeros(self.N, np.int32)
        conf, cnt = np.zeros(self.N, np.float32), np.zeros(len(self.T), np.int32)
        t = i32(self.T)
        self.lib.call("clstm_net_predict", self.h, ptr(t), len(self.T), frames_d, ptr(cls), ptr(loc), ptr(conf), ptr(cnt))
        dec, locs, confs, o = [], [], [], 0
        for b, tb in enumerate(self.T):
            dec.append(cls[o:o + cnt[b]].copy())
            locs.append(loc[o:o + cnt[b]].copy())
            confs.append(conf[o:o + cnt[b]].copy())
            o += tb
        return dec, locs, confs

    def device_bytes(self):
        """sum of this net's device allocations in bytes (clstm_net_device_bytes)"""
        n = C.c_longlong()
        self.lib.call("clstm_net_device_bytes", self.h, C.byref(n))
        return n.value

    def state(self, layer, direction, which):
        a = np.empty((self.N, self.nhidden[layer]), np.float32)
        self.lib.call("clstm_net_get_state_h", self.h, layer, direction, STATE_CODES[which], ptr(a))
        return a

    def device_buffers(self):
        v, d, g = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.lib.call("clstm_net_buffers", self.h, C.byref(v), C.byref(d), C.byref(g))
        return v.value, d.value, g.value

    def device_outputs(self):
        p, d = C.c_void_p(), C.c_void_p()
        self.lib.call("clstm_net_outputs", self.h, C.byref(p), C.byref(d))
        return p.value, d.value

    def set_overlap(self, mode):
        """0: weight-gradient GEMM after the backward recurrence; 1: beside it where it pays (default); 2: always."""
        self.lib.call("clstm_net_set_overlap", self.h, int(mode))

    def set_strict_f32(self, on=True):
        """every product of the step on the exact f32 MFMA (the default computes the backward weight-gradient / softmax-backward
        products as f32-grade bf16 x 3 split products)"""
        self.lib.call("clstm_net_set_strict_f32", self.h, int(bool(on)))

    def overlap_stats(self):
        n, t = C.c_longlong(), C.c_int()
        self.lib.call("clstm_net_overlap_stats", self.h, C.byref(n), C.byref(t))
        return n.value, t.value

    # -- timing (bench.py) ---------------------------------------------------------------------
    def enable_timing(self, on=True):
        self.lib.call("clstm_net_enable_timing", self.h, int(on))

    def kernel_time_ms(self, name):
        ms, n = C.c_double(), C.c_int()
        self.lib.call("clstm_net_kernel_time_ms", self.h, name.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def reset_timing(self):
        self.lib.call("clstm_net_reset_timing", self.h)


class Normalizer:
    """CenterNormalizer (extras.cc:227-285) on the device (clstm_normalizer_*, csrc/normalize.h): raw line images in, input
    frames out, bit for bit the host normaliser's.  images: [w, h] float arrays with ink = 1 -- image[x, y], the host Image
    layout -- of any sizes."""

    def __init__(self, target_height=48, smooth2d=1.0, smooth1d=0.3, range=4.0, lib=None):
        self.lib = lib or abi.load()
        self.target_height = int(target_height)
        h = C.c_void_p()
        self.lib.call("clstm_normalizer_create", C.byref(h), self.target_height, float(smooth2d), float(smooth1d), float(range))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            try:
                self.lib.call("clstm_normalizer_destroy", self.h)
            except Exception:
                pass
            self.h = None

    @staticmethod
    def pack(images):
        images = [f32(a) for a in images]
        for a in images:
            if a.ndim != 2:
                raise ValueError("a line image is a [w, h] array")
        w, h = i32([a.shape[0] for a in images]), i32([a.shape[1] for a in images])
        pix = f32(np.concatenate([a.reshape(-1) for a in images])) if images else f32([])
        return pix, w, h

    def _run(self, name, pix, w, h):
        bs = len(w)
        T, r = np.zeros(bs, np.int32), np.zeros(bs, np.float32)
        frames_d = C.c_void_p()
        self.lib.call(name, self.h, ptr(pix), ptr(w), ptr(h), bs, ptr(T), ptr(r), C.byref(frames_d))
        self.nframes = int(T.sum())
        return T, r, frames_d.value

    def run_device(self, images):
        """-> (T, r, address of the DEVICE frames [sum T][target_height], valid until the next call on this normalizer)"""
        return self._run("clstm_normalizer_run_h", *self.pack(images))

    def run_device_pixels(self, pix_d, w, h):
        """the same for pixels already on the device (packed back to back; a torch tensor or an address)"""
        return self._run("clstm_normalizer_run_d", pix_d, i32(w), i32(h))

    def frames(self):
        """the last call's frames as a host array [sum T][target_height] (blocking)"""
        out = np.empty((self.nframes, self.target_height), np.float32)
        self.lib.call("clstm_normalizer_get_frames_h", self.h, ptr(out))
        return out

    def run(self, images):
        """-> (T, r, frames ndarray [sum T][target_height])"""
        T, r, _ = self.run_device(images)
        return T, r, self.frames()

    def device_bytes(self):
        n = C.c_longlong()
        self.lib.call("clstm_normalizer_device_bytes", self.h, C.byref(n))
        return n.value


def degrade_line(m=(1.0, 0.0, 0.0, 1.0), tx=0.0, ty=0.0, sigma=0.0, maxdelta=0.0, blur=0.0, seed=0):
    """one line's degradation parameters (clstm_degrade_line); the defaults are the identity"""
    return abi.DegradeLine((C.c_float * 4)(*m), tx, ty, sigma, maxdelta, blur, seed)


def default_ranges(lib=None):
    rg = abi.DegradeRanges()
    (lib or abi.load()).call("clstm_degrade_default_ranges", C.byref(rg))
    return rg


def draw(seed, key, visit, w, h, ranges=None, lib=None):
    """clstm_degrade_draw: the parameters of line `key` (the caller's name for it, not its place in a minibatch) on its `visit`-th
    visit, drawn within `ranges` (default: clstm_degrade_default_ranges)"""
    lib = lib or abi.load()
    out = abi.DegradeLine()
    lib.call("clstm_degrade_draw", int(seed), int(key), int(visit), C.byref(ranges if ranges is not None else default_ranges(lib)),
             int(w), int(h), C.byref(out))
    return out


class Degrader:
    """Training-time degradation of raw line images on the device (clstm_degrader_*, csrc/degrade.h): a small elastic distortion, an
    affine jitter, a little blur, bit for bit degrade_line of clstm_amd/host/degrade.h.  images: [w, h] float arrays with ink = 1, as
    Normalizer takes them; lines: one abi.DegradeLine (degrade_line(...), draw(...)) per image.  The output is packed the way
    Normalizer.run_device_pixels takes it."""

    def __init__(self, lib=None):
        self.lib = lib or abi.load()
        h = C.c_void_p()
        self.lib.call("clstm_degrader_create", C.byref(h))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            try:
                self.lib.call("clstm_degrader_destroy", self.h)
            except Exception:
                pass
            self.h = None

    def _run(self, name, pix, w, h, lines):
        w, h = i32(w), i32(h)
        arr = (abi.DegradeLine * max(len(lines), 1))(*lines)
        out_d = C.c_void_p()
        self.lib.call(name, self.h, ptr(pix), ptr(w), ptr(h), len(w), C.cast(arr, C.c_void_p), C.byref(out_d))
        self.shapes = list(zip(w.tolist(), h.tolist()))
        return out_d.value

    def run_device(self, images, lines):
        """-> address of the DEVICE pixels, the degraded lines packed back to back, valid until the next call on this degrader"""
        return self._run("clstm_degrader_run_h", *Normalizer.pack(images), lines)

    def run_device_pixels(self, pix_d, w, h, lines):
        """the same for pixels already on the device (packed back to back; a torch tensor or an address); no host synchronisation"""
        return self._run("clstm_degrader_run_d", pix_d, w, h, lines)

    def pixels(self):
        """the last call's output as a list of host arrays [w, h] (blocking)"""
        out = np.empty(sum(w * h for w, h in self.shapes), np.float32)
        self.lib.call("clstm_degrader_get_pixels_h", self.h, ptr(out))
        res, o = [], 0
        for w, h in self.shapes:
            res.append(out[o:o + w * h].reshape(w, h))
            o += w * h
        return res

    def run(self, images, lines):
        """-> the degraded images, a list of host arrays [w, h]"""
        self.run_device(images, lines)
        return self.pixels()

    def device_bytes(self):
        n = C.c_longlong()
        self.lib.call("clstm_degrader_device_bytes", self.h, C.byref(n))
        return n.value


class Comm:
    """RCCL communicator of the data-parallel ranks (clstm_comm_*): one per process / GPU.
    `exchange(id_bytes_or_None) -> id_bytes` ships rank 0's 128-byte id to every rank."""

    ID_BYTES = 128

    def __init__(self, rank, nranks, exchange, lib=None):
        self.lib = lib or abi.load()
        buf = C.create_string_buffer(self.ID_BYTES)
        if rank == 0:
            self.lib.call("clstm_comm_unique_id", buf)
        ident = exchange(bytes(buf.raw) if rank == 0 else None)
        assert len(ident) == self.ID_BYTES
        h = C.c_void_p()
        self.lib.call("clstm_comm_create", C.byref(h), C.create_string_buffer(ident, self.ID_BYTES), int(rank), int(nranks))
        self.h = h
        self.rank, self.nranks = int(rank), int(nranks)

    def allreduce(self, buf, n):
        self.lib.call("clstm_allreduce_flat", self.h, ptr(buf), int(n))

    def peer_capacity(self):
        """floats one exchange buffer of the peer path holds at present; 0 before its set-up or after a fallback"""
        n = C.c_longlong(0)
        self.lib.call("clstm_comm_peer_capacity", self.h, C.byref(n))
        return int(n.value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.call("clstm_comm_destroy", self.h)
            self.h = None


def make_net(kind, ninput, noutput, nhidden, nhidden2=None, lib=None, **bufs):
    """make_net(kind, {ninput, noutput, nhidden[, nhidden2]}) -- clstm_prefab.cc:151-173."""
    if kind == "bidi":
        return Network(ninput, [nhidden], noutput, lib=lib, **bufs)
    if kind == "bidi2":
        return Network(ninput, [nhidden, nhidden2], noutput, lib=lib, **bufs)
    if kind == "lstm1":
        return Network(ninput, [nhidden], noutput, unidirectional=True, lib=lib, **bufs)
    raise ValueError("no such network or layer: %s (on the MI355X path: bidi, bidi2, lstm1)" % kind)


def sgd_update(net):
    net.update()


def unpack_beam(T, nbest, nhyp, ln, sc, lab, am=None):
    """the arrays of clstm_ctc_beam_batch / clstm_net_beam (include/clstm_abi.h) as a list per line of (labels, score); with the
    am_score array of the language model calls: of (labels, score, am_score)"""
    out, off = [], 0
    for b, t in enumerate(T):
        hyps = []
        for k in range(int(nhyp[b])):
            s = nbest * off + k * t
            hyp = (lab[s:s + ln[b * nbest + k]].copy(), float(sc[b * nbest + k]))
            hyps.append(hyp if am is None else hyp + (float(am[b * nbest + k]),))
        out.append(hyps)
        off += t
    return out


def _pack(seqs):
    off = i32(np.concatenate([[0], np.cumsum([len(x) for x in seqs])]))
    flat = [int(c) for x in seqs for c in x]
    return i32(flat if flat else [0]), off


def edit_distance(hyps, refs, ref_of=None, nsym=None, script=False, confusion=False, lib=None):
    """Levenshtein distance of hypothesis k against reference ref_of[k] (None: one reference per hypothesis) on the device
    (clstm_edit_distance_batch; the algorithm and the canonical script rule in clstm_amd/csrc/edit_distance.h).  Sequences of
    labels in [1, nsym); nsym defaults to the largest label + 1.  -> dist [n]; with script: (dist, counts [n, 3] =
    substitutions, insertions, deletions, scripts = per pair an array of codes 0 match, 1 substitution, 2 insertion, 3 deletion);
    with confusion a [nsym, nsym] table (rows = reference label, columns = hypothesis label, row / column 0 = insertions /
    deletions) is appended."""
    lib = lib or abi.load()
    hyps, refs = [list(x) for x in hyps], [list(x) for x in refs]
    n = len(hyps)
    hyp, hoff = _pack(hyps)
    ref, roff = _pack(refs)
    ro = None if ref_of is None else i32(ref_of)
    assert ro is None or len(ro) == n
    if nsym is None:
        nsym = max(2, 1 + max([int(c) for x in hyps + refs for c in x], default=1))
    lb = [len(refs[q]) if 0 <= q < len(refs) else 0 for q in (range(n) if ro is None else ro.tolist())]   # (the library refuses a bad index)
    dist = np.zeros(n, np.int32)
    cnt = np.zeros((n, 3), np.int32) if script else None
    nops = np.zeros(n, np.int32) if script else None
    ops = np.zeros(max(1, int(hoff[-1]) + int(sum(lb))), np.int32) if script else None
    conf = np.zeros((nsym, nsym), np.int32) if confusion else None
    lib.call("clstm_edit_distance_batch", ptr(hyp), ptr(hoff), n, ptr(ref), ptr(roff), len(refs), ptr(ro), int(nsym),
             ptr(dist), ptr(cnt), ptr(nops), ptr(ops), ptr(conf))
    out = (dist,)
    if script:
        starts = np.asarray(hoff[:-1], np.int64) + np.concatenate([[0], np.cumsum(lb)[:-1]]).astype(np.int64) if n else []
        out += (cnt, [ops[int(s):int(s) + int(k)].copy() for s, k in zip(starts, nops)])
    if confusion:
        out += (conf,)
    return out if len(out) > 1 else dist


def cer(dist, transcripts):
    """character error rate: summed distances over summed transcript lengths (0 for no reference character at all)"""
    n = sum(len(t) for t in transcripts)
    return float(np.sum(dist)) / n if n else 0.0


def spans(path, L):
    """Per label k < L of a transcript the (first_frame, last_frame) it occupies on `path` (Network.align): label k is state
    2k + 1.  A label the path never visits gives (-1, -1)."""
    path = np.asarray(path)
    out = []
    for k in range(int(L)):
        f = np.flatnonzero(path == 2 * k + 1)
        out.append((int(f[0]), int(f[-1])) if f.size else (-1, -1))
    return out


def mktargets(transcript):
    """ctc.cc:148-157 as a list of state classes."""
    lib = abi.load()
    tr = i32(transcript)
    st = np.zeros(2 * len(tr) + 1, np.int32)
    lib.call("clstm_mktargets", ptr(st), ptr(tr), len(tr))
    return st
