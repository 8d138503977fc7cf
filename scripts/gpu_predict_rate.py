#!/usr/bin/env python3
"""Recognition rate on one MI355X: (A) clstm_net_set_batch + set_inputs_d + forward + decode -- the way before clstm_net_predict, still
in the library -- against (B) clstm_net_predict, alternating in one process.  Writes profiles/predict_rate.txt.  Needs a GPU.

Per size: both shapes warmed, then ALTERNATIONS x (window A, window B); a window runs whole calls until MIN_WINDOW_S have passed and
ends with a synchronise (both ways are blocking calls anyway: they return decodes); the rate of a window is lines / wall time.
Reported: the median rate of each way, the spread (max - min over the windows, relative to the median) and B / A.
Also: bytes the recurrence moves per cell-step in either form (from the shapes), and the 256- / 640-line rates of predict with the
per-line and the batched-MFMA family forced (the crossover is inherited from training).

--profile-run: a few calls of each way at 64 / 256 / 640 lines and nothing else -- the workload for
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gpu_predict_rate.py --profile-run
whose kernel table gives the save / no-save times of the three recurrence families.

--cli: wall time of `clstmocr batch=1` against `batch=64` on the 512-line rendered corpus (scripts/make_corpus.py), PNG decoding and
normalisation included, as lines/s; three alternations; appended to the output file.  The model is the uw3 architecture after one
update (the time does not depend on what the weights are)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NI, NH, NC = 48, 100, 83
MIN_WINDOW_S, ALTERNATIONS = 1.0, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_rate.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_predict_rate.py needs a GPU")
    from clstm_amd import abi
    from clstm_amd.abi import i32, ptr
    from clstm_amd.init import init_params
    from clstm_amd.net import Network
    if args.cli:
        return cli_rates(args.out)
    lib = abi.load()
    rng = np.random.default_rng(0)
    params = init_params(NI, NH, NC, seed=0.222) * 10.0

    def count(which):
        c = ctypes.c_longlong(0)
        lib.call("clstm_debug_path_count", which, ctypes.byref(c))
        return c.value

    class Case:
        def __init__(self, T):
            self.T = [int(t) for t in T]
            self.t = i32(self.T)
            self.N = sum(self.T)
            x = np.clip(rng.normal(0.2, 0.3, (self.N, NI)), 0, 1).astype(np.float32)
            self.x = torch.from_numpy(x).cuda()
            self.cls, self.loc = np.zeros(self.N, np.int32), np.zeros(self.N, np.int32)
            self.conf, self.cnt = np.zeros(self.N, np.float32), np.zeros(len(self.T), np.int32)

    def way_a(net, c):
        lib.call("clstm_net_set_batch", net.h, ptr(c.t), len(c.T))
        lib.call("clstm_net_set_inputs_d", net.h, ptr(c.x))
        lib.call("clstm_net_forward", net.h)
        lib.call("clstm_net_decode", net.h, ptr(c.cls), ptr(c.loc), ptr(c.cnt))

    def way_b(net, c):
        lib.call("clstm_net_predict", net.h, ptr(c.t), len(c.T), ptr(c.x), ptr(c.cls), ptr(c.loc), ptr(c.conf), ptr(c.cnt))

    def window(fn, net, c, min_s=MIN_WINDOW_S):
        lib.call("clstm_synchronize")
        t0, n = time.perf_counter(), 0
        while True:
            fn(net, c)
            n += 1
            if time.perf_counter() - t0 >= min_s:
                break
        lib.call("clstm_synchronize")
        return n * len(c.T) / (time.perf_counter() - t0)

    def nets():
        a, b = Network(NI, [NH], NC, lib=lib), Network(NI, [NH], NC, lib=lib)
        a.set_params(params); b.set_params(params)
        a.set_training(False)          # (way A as CLSTMOCR::predict runs it)
        return a, b

    if args.profile_run:
        for nl in (64, 256, 640):
            c = Case([200] * nl)
            a, b = nets()
            for _ in range(6):
                way_a(a, c)
                way_b(b, c)
        lib.call("clstm_synchronize")
        return

    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)
    say("# recognition rate, lines/s: A = set_batch + set_inputs_d + forward + decode, B = clstm_net_predict; BiLSTM(%d), %d inputs, %d classes"
        % (NH, NI, NC))
    say("# %s; %d alternations of windows >= %.1f s, each ended by a synchronise; spread = (max - min) / median over the windows"
        % (torch.cuda.get_device_name(0), ALTERNATIONS, MIN_WINDOW_S))
    sizes = [("1 x 200", [200]), ("64 x 200", [200] * 64), ("256 x 200", [200] * 256), ("640 x 200", [200] * 640),
             ("2048 x 200", [200] * 2048), ("512 ragged U{150..250}", rng.integers(150, 251, 512))]
    worst = None
    for name, T in sizes:
        c = Case(T)
        a, b = nets()
        k0 = [count(k) for k in (22, 23, 15)]
        for _ in range(3):
            way_a(a, c); way_b(b, c)
        fam = [n for n, k, v in zip(("per-line", "fused", "batched MFMA"), (22, 23, 15), k0) if count(k) != v]
        ra, rb = [], []
        for _ in range(ALTERNATIONS):
            ra.append(window(way_a, a, c))
            rb.append(window(way_b, b, c))
        ma, mb = float(np.median(ra)), float(np.median(rb))
        sa, sb = (max(ra) - min(ra)) / ma, (max(rb) - min(rb)) / mb
        say("%-24s family %-13s A %10.0f (spread %4.1f %%)  B %10.0f (spread %4.1f %%)  B/A %.3f   device bytes A %d  B %d"
            % (name, "+".join(fam), ma, 100 * sa, mb, 100 * sb, mb / ma, a.device_bytes(), b.device_bytes()))
        slower = 1.0 - mb / ma
        if slower > max(sa, sb) and (worst is None or slower > worst[1]):
            worst = (name, 100 * slower)
        del a, b, c
        torch.cuda.empty_cache()
    say("# crossover (inherited from training: batched MFMA from 640 lines on): predict with either family forced")
    for nl in (256, 640):
        c = Case([200] * nl)
        for mode, fam in ((0, "per-line"), (2, "batched MFMA")):
            lib.call("clstm_debug_set_option", b"fwd_mfma", mode)
            _, b = nets()
            for _ in range(3):
                way_b(b, c)
            r = [window(way_b, b, c) for _ in range(3)]
            say("%4d x 200  predict, %-13s %10.0f lines/s (spread %4.1f %%)" % (nl, fam, np.median(r), 100 * (max(r) - min(r)) / np.median(r)))
            del b
        lib.call("clstm_debug_set_option", None, 0)
    say("# bytes per cell-step of the recurrence's global traffic (f32): training form = 4 B pre-activation in (per-line / fused) + 16 B "
        "activations + 4 B c + 4 B h + 4 B source row out; no-save = 4 B in + 4 B h out.  Per-line / fused: 32 -> 8 B; batched MFMA "
        "(no pre-activation array): 28 -> 4 B")
    say("# acceptance: B slower than A by more than the spread at: %s" % ("none" if worst is None else "%s (%.1f %%)" % worst))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    if worst is not None:
        sys.exit(1)


def cli_rates(out_path):
    import glob
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from make_corpus import make_corpus
    bin_dir = os.path.join(ROOT, "clstm_amd", "bin")
    d = tempfile.mkdtemp(prefix="predict_cli_")
    names, _ = make_corpus(d, n=512, seed=0)
    env = dict(os.environ, batch="64", ntrain="64", lrate="1e-4", nhidden="100", seed="0.222", save_name=os.path.join(d, "_m"),
               save_every="64", report_every="1000000", test_every="100000000")
    subprocess.run([os.path.join(bin_dir, "clstmocrtrain"), os.path.join(d, "list.txt")], env=env, check=True, capture_output=True, timeout=600)
    model = sorted(glob.glob(os.path.join(d, "_m-*.clstm")))[-1]
    rates = {1: [], 64: []}
    for _ in range(3):
        for b in (1, 64):
            t0 = time.perf_counter()
            subprocess.run([os.path.join(bin_dir, "clstmocr"), os.path.join(d, "list.txt")], env=dict(os.environ, load=model, batch=str(b), save_text="0"),
                           check=True, capture_output=True, timeout=600)
            rates[b].append(len(names) / (time.perf_counter() - t0))
    lines = ["# clstmocr on the 512-line rendered corpus, wall time of the whole process (start-up, PNG decoding, normalisation included), lines/s"]
    for b in (1, 64):
        lines.append("clstmocr batch=%-3d %s   median %.0f" % (b, " ".join("%.0f" % r for r in rates[b]), float(np.median(rates[b]))))
    lines.append("batch=64 / batch=1: %.2f" % (float(np.median(rates[64])) / float(np.median(rates[1]))))
    print("\n".join(lines), flush=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
