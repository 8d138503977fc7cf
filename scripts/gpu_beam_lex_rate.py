#!/usr/bin/env python3
"""Rate of the beam search launch constrained to a lexicon (clstm_net_beam_lex, csrc/ctc_beam.h, third part).
Writes profiles/beam_lex_rate.txt.  Needs a GPU.

Shape: gpu_beam_lm_rate.py's -- 64 lines x T = 200, 83 classes, on the outputs of a BiLSTM(100) forward pass; then 1024 lines.
beam = nbest = 4 / 8 / 16 (1024 lines: 8).  Two lexicons of random words of 2 .. 8 characters over the first 69 classes (the last
13 are separators): 500 words and 50,000 words; each without a model (bonus 0) and with a random order-3 table with an end table,
weight 0.5.  Beside each width, alternating in the same process (so drift hits all alike): the launch with the same order-3 model
and no lexicon (clstm_net_beam_lm) -- the SAME key count per frame, beam * nc: the comparison that matters -- and the plain launch
(clstm_net_beam).
Per configuration the median kernel time of REPEATS alternating repeats (the launch's own pair of events) and the host wall clock
of the whole call, as gpu_beam_lm_rate.py takes them; for the 64-line launches also the time per frame; and the share of lines
that reported a hypothesis (the posteriors of an untrained net spell no words: most lines end inside a word).
No threshold: the first measurement of this form."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NI, NH, NC, T = 48, 100, 83, 200
NSEP = NC // 6
REPEATS = 15
WEIGHT = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_lex_rate.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_beam_lex_rate.py needs a GPU")
    from clstm_amd import abi
    from clstm_amd.init import init_params
    from clstm_amd.lexicon import Lexicon
    from clstm_amd.lm import CharLM
    from clstm_amd.net import Network
    lib = abi.load()
    rng = np.random.default_rng(0)
    lm3 = CharLM(3, NC, rng.normal(-3.0, 1.5, (NC * NC, NC)).astype(np.float32), rng.normal(-3.0, 1.5, NC * NC).astype(np.float32), lib=lib)
    flags = np.zeros(NC, np.uint8)
    flags[1:NC - NSEP] = 1
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    lex = {}
    for nw in (500, 50000):
        words = [rng.integers(1, NC - NSEP, int(rng.integers(2, 9))).tolist() for _ in range(nw)]
        lex[nw] = Lexicon(NC, flags, words, lib=lib)
        say("# lexicon of %d words: %s" % (nw, lex[nw].info(lib)))

    def measure(nlines, beams, repeats):
        net = Network(NI, [NH], NC, lib=lib)
        net.set_params(init_params(NI, NH, NC, seed=0.222) * 10.0)
        net.set_inputs([np.clip(rng.normal(0.2, 0.3, (T, NI)), 0, 1).astype(np.float32) for _ in range(nlines)])
        net.forward()
        cfg = {}
        for w in beams:
            cfg["beam %d" % w] = ("ctc_beam", w * (1 + min(NC - 1, 2 * w)), lambda w=w: net.beam(w))
            cfg["beam %d order 3" % w] = ("ctc_beam_lm", w * NC, lambda w=w: net.beam_lm(lm3, WEIGHT, beam=w))
            for nw in lex:
                cfg["beam %d lex %d" % (w, nw)] = ("ctc_beam_lex", w * NC, lambda w=w, nw=nw: net.beam_lex(lex[nw], beam=w))
                cfg["beam %d lex %d order 3" % (w, nw)] = ("ctc_beam_lex", w * NC,
                                                            lambda w=w, nw=nw: net.beam_lex(lex[nw], beam=w, lm=lm3, weight=WEIGHT))
        found = {}
        for name, (_, _, fn) in cfg.items():      # warm every configuration (allocations, LDS attribute, code upload)
            fn()
            found[name] = sum(1 for h in fn() if h) / nlines
        kern, call = {name: [] for name in cfg}, {name: [] for name in cfg}
        for timed in (True, False):
            net.enable_timing(timed)
            for _ in range(repeats):
                for name, (kname, _, fn) in cfg.items():
                    if timed:
                        net.reset_timing()
                        fn()
                        lib.call("clstm_synchronize")
                        ms, n = net.kernel_time_ms(kname)
                        assert n == 1, (name, n)
                        kern[name].append(ms * 1e3)
                    else:
                        lib.call("clstm_synchronize")
                        t0 = time.perf_counter()
                        fn()
                        lib.call("clstm_synchronize")
                        call[name].append((time.perf_counter() - t0) * 1e6)
        for name, (_, keys, _) in cfg.items():
            k, c = np.array(kern[name]), np.array(call[name])
            frame = "%6.2f us/frame" % (np.median(k) / T) if nlines <= 64 else "%15s" % ""
            say("%5d lines  %-26s %5d keys/frame  kernel %9.1f us  (spread %4.1f %%)  %s  %9.0f lines/s   call %9.1f us   %3.0f %% of lines with a hypothesis"
                % (nlines, name, keys, np.median(k), 100 * (k.max() - k.min()) / np.median(k), frame, nlines / (np.median(k) * 1e-6), np.median(c),
                   100 * found[name]))

    say("# beam search launch: plain, with an order-3 character model, and constrained to a lexicon (without / with that model); nbest = beam, "
        "weight %.1f; T = %d, %d classes; %s; medians of %d alternating repeats" % (WEIGHT, T, NC, torch.cuda.get_device_name(0), REPEATS))
    measure(64, (4, 8, 16), REPEATS)
    say("# 1024 lines")
    measure(1024, (8,), 7)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
