#!/usr/bin/env python3
"""Rates of the edit-distance launch (clstm_edit_distance_batch / clstm_net_errors, csrc/edit_distance.h).  Writes
profiles/errors_rate.txt.  Needs a GPU.

1. clstm_edit_distance_batch at 64, 1024 and 16384 pairs of about 50 labels (references of 40 .. 60 labels over 82 symbols, each
   hypothesis its reference with a few edits): host wall clock of the whole call, results on the host, for distances alone and for
   distances + counts + scripts + confusion table; medians of REPEATS alternating repeats.
2. clstm_net_errors on 64 lines x T = 200 of a BiLSTM(100): the launch's own time (clstm_net_kernel_time_ms "edit_distance") and the
   call's wall clock (it decodes on the device first), beside clstm_net_decode's call -- what the host loop needs before it can start.
3. The test pass of `clstmocrtrain test_batch=64` on the 512-line rendered corpus (scripts/make_corpus.py) with gpu_errors=1 and with
   the host's levenshtein loop (gpu_errors=0: the code of the commit before this option).  A process runs K test passes between K
   updates of 64 lines; the time of one pass is the slope between K = 2 and K = 42 minus the same slope of runs that never test.
   A pass reads and normalises its 512 PNGs again: that is part of it, as it is for a user.
No threshold: the first measurement of this kernel."""
import argparse
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NI, NH, NC, T, L = 48, 100, 83, 200, 25
REPEATS = 15


def planted(rng, ref, nsym):
    h = list(ref)
    for _ in range(int(rng.integers(0, 6))):
        k = int(rng.integers(3))
        i = int(rng.integers(len(h)))
        if k == 0:
            h[i] = int(rng.integers(1, nsym))
        elif k == 1:
            del h[i]
        else:
            h.insert(i, int(rng.integers(1, nsym)))
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errors_rate.txt"))
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_errors_rate.py needs a GPU")
    from clstm_amd import abi
    from clstm_amd.abi import i32, ptr
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    lib = abi.load()
    rng = np.random.default_rng(0)
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    say("# edit distance on the device; %s; medians of %d alternating repeats" % (torch.cuda.get_device_name(0), REPEATS))
    say("# 1. clstm_edit_distance_batch, pairs of ~50 labels, 82 symbols: wall clock of the call")
    for npairs in (64, 1024, 16384):
        refs = [rng.integers(1, NC, int(rng.integers(40, 61))).tolist() for _ in range(npairs)]
        hyps = [planted(rng, r, NC) for r in refs]
        hoff = i32(np.concatenate([[0], np.cumsum([len(h) for h in hyps])]))
        roff = i32(np.concatenate([[0], np.cumsum([len(r) for r in refs])]))
        hyp, ref = i32([c for h in hyps for c in h]), i32([c for r in refs for c in r])
        dist, cnt, nops = np.zeros(npairs, np.int32), np.zeros(3 * npairs, np.int32), np.zeros(npairs, np.int32)
        ops, conf = np.zeros(int(hoff[-1]) + int(roff[-1]), np.int32), np.zeros(NC * NC, np.int32)
        forms = {"distances": (ptr(dist), None, None, None, None),
                 "distances + counts + scripts + confusions": (ptr(dist), ptr(cnt), ptr(nops), ptr(ops), ptr(conf))}

        def call(o):
            lib.call("clstm_edit_distance_batch", ptr(hyp), ptr(hoff), npairs, ptr(ref), ptr(roff), npairs, None, NC, *o)
        times = {name: [] for name in forms}
        for o in forms.values():
            call(o); call(o)
        for _ in range(REPEATS):
            for name, o in forms.items():
                lib.call("clstm_synchronize")
                t0 = time.perf_counter()
                call(o)
                times[name].append((time.perf_counter() - t0) * 1e6)
        for name in forms:
            t = np.array(times[name])
            say("%6d pairs  %-42s call %9.1f us  (spread %5.1f %%)  %11.0f pairs/s" % (
                npairs, name, np.median(t), 100 * (t.max() - t.min()) / np.median(t), npairs / (np.median(t) * 1e-6)))

    say("# 2. clstm_net_errors, 64 lines x T = %d, transcripts of %d labels" % (T, L))
    net = Network(NI, [NH], NC, lib=lib)
    net.set_params(init_params(NI, NH, NC, seed=0.222) * 10.0)
    net.set_inputs([np.clip(rng.normal(0.2, 0.3, (T, NI)), 0, 1).astype(np.float32) for _ in range(64)])
    net.forward()
    # (the library calls themselves, arrays packed beforehand: Network.errors / Network.decode add their Python list handling)
    labels, Ls = i32(rng.integers(1, NC, 64 * L)), i32([L] * 64)
    dist, cnt, conf = np.zeros(64, np.int32), np.zeros(3 * 64, np.int32), np.zeros((NC + 1) ** 2, np.int32)
    cls, loc, num = np.zeros(64 * T, np.int32), np.zeros(64 * T, np.int32), np.zeros(64, np.int32)
    cfg = {"errors (distances)": ("edit_distance", lambda: lib.call("clstm_net_errors", net.h, ptr(labels), ptr(Ls), ptr(dist), None, None)),
           "errors (+ counts + confusions)": ("edit_distance", lambda: lib.call("clstm_net_errors", net.h, ptr(labels), ptr(Ls), ptr(dist),
                                                                                ptr(cnt), ptr(conf))),
           "trivial decode": (None, lambda: lib.call("clstm_net_decode", net.h, ptr(cls), ptr(loc), ptr(num)))}
    for _, fn in cfg.values():
        fn(); fn()
    kern, wall = {name: [] for name in cfg}, {name: [] for name in cfg}
    for timed in (True, False):
        net.enable_timing(timed)
        for _ in range(REPEATS):
            for name, (kname, fn) in cfg.items():
                if timed and kname:
                    net.reset_timing()
                    fn()
                    lib.call("clstm_synchronize")
                    ms, n = net.kernel_time_ms(kname)
                    assert n == 1, (name, n)
                    kern[name].append(ms * 1e3)
                elif not timed:
                    lib.call("clstm_synchronize")
                    t0 = time.perf_counter()
                    fn()
                    wall[name].append((time.perf_counter() - t0) * 1e6)
    for name in cfg:
        k, c = np.array(kern[name]), np.array(wall[name])
        ks = "kernel %8.1f us  (spread %5.1f %%)" % (np.median(k), 100 * (k.max() - k.min()) / np.median(k)) if len(k) else "%37s" % "-"
        say("   64 lines  %-32s %s   call %9.1f us" % (name, ks, np.median(c)))
    if not args.no_cli:
        cli_rates(say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


def cli_rates(say):
    from make_corpus import make_corpus
    bin_dir = os.path.join(ROOT, "clstm_amd", "bin")
    d = tempfile.mkdtemp(prefix="errors_cli_")
    names, _ = make_corpus(d, n=512, seed=0)
    lst = os.path.join(d, "list.txt")
    env = dict(os.environ, batch="64", ntrain="64", lrate="1e-4", nhidden="100", seed="0.222", save_name=os.path.join(d, "_m"),
               save_every="64", report_every="1000000", test_every="100000000")
    subprocess.run([os.path.join(bin_dir, "clstmocrtrain"), lst], env=env, check=True, capture_output=True, timeout=600)
    model = sorted(glob.glob(os.path.join(d, "_m-*.clstm")))[-1]
    K1, K2 = 2, 42

    def run(k, test, gpu_errors):
        e = dict(os.environ, load=model, batch="64", test_batch="64", gpu_errors=str(gpu_errors), ntrain=str(64 + 64 * k),
                 save_name=os.path.join(d, "_r"), save_every="100000000", report_every="100000000",
                 test_every="64" if test else "100000000")
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(bin_dir, "clstmocrtrain"), lst, lst], env=e, check=True, capture_output=True, text=True, timeout=600)
        dt = time.perf_counter() - t0
        assert r.stdout.count("ERROR ") == (k if test else 0), r.stdout[-1000:]
        return dt
    slopes = {"no test pass": [], "gpu_errors=0": [], "gpu_errors=1": []}
    for _ in range(5):
        for name, (test, ge) in (("no test pass", (False, 0)), ("gpu_errors=0", (True, 0)), ("gpu_errors=1", (True, 1))):
            slopes[name].append((run(K2, test, ge) - run(K1, test, ge)) / (K2 - K1))
    base = float(np.median(slopes["no test pass"]))
    say("# 3. clstmocrtrain test_batch=64 on the 512-line rendered corpus: seconds per (update of 64 lines + test pass), slope between "
        "%d and %d passes, 5 alternating repeats" % (K1, K2))
    say("update alone        %s   median %.4f s" % (" ".join("%.4f" % s for s in slopes["no test pass"]), base))
    for name in ("gpu_errors=0", "gpu_errors=1"):
        s = np.array(slopes[name])
        per = float(np.median(s)) - base
        say("%-19s %s   median %.4f s   test pass %.4f s = %.0f lines/s" % (name, " ".join("%.4f" % x for x in s), np.median(s), per, len(names) / per))


if __name__ == "__main__":
    main()
