#!/usr/bin/env python3
"""Line normalisation on one MI355X against the host CenterNormalizer.  Writes profiles/prep_rate.txt.  Needs a GPU.

(1) The normaliser alone on 64 and 256 crops of the fixture line (tests/golden/textline.bin.png, 819 x 88; crop k drops 16 * (k % 8)
    columns): device lines/s of clstm_normalizer_run_d (pixels resident) and clstm_normalizer_run_h, alternating windows -- a window
    runs whole calls until MIN_WINDOW_S have passed; every call is blocking for r / T and the window ends with a synchronise, so the
    warp kernel is inside -- with the spread (max - min over the windows, relative to the median); the host CenterNormalizer on the
    same lines on 1 and on 16 threads (`clstm_hosttool normalize-bench`) on the same box.
(2) `clstmocr batch=64` on the 512-line rendered corpus (scripts/make_corpus.py), gpu_prep=0 against gpu_prep=1, three alternations,
    whole-process wall time (start-up, PNG decoding included), lines/s, and whether gpu_prep=1 is faster by more than the spread.

--profile-run: a few run_d calls on 64 crops and nothing else -- the workload for
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gpu_prep_rate.py --profile-run
--kernel-table DIR: append the k_nz_* rows of that run's kernel statistics, with each kernel's share, to the output file."""
import argparse
import csv
import glob
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "clstm_amd", "bin")
FIXTURE = os.path.join(ROOT, "tests", "golden", "textline.bin.png")
MIN_WINDOW_S, ALTERNATIONS = 1.0, 3
PROFILE_CALLS = 10


def fixture_crops(n, tmp):
    raw = os.path.join(tmp, "fixture.raw")
    subprocess.run([os.path.join(BIN, "clstm_hosttool"), "png2raw", FIXTURE, raw], check=True)
    data = open(raw, "rb").read()
    w, h = struct.unpack("<ii", data[:8])
    img = np.float32(1.0) - np.frombuffer(data[8:], np.float32).reshape(w, h)
    return [np.ascontiguousarray(img[:w - 16 * (k % 8)]) for k in range(n)]


def spread(r):
    return (max(r) - min(r)) / float(np.median(r))


def normaliser_rates(say, tmp):
    import torch
    from clstm_amd import abi
    from clstm_amd.net import Normalizer
    lib = abi.load()
    for n in (64, 256):
        images = fixture_crops(n, tmp)
        pix, w, h = Normalizer.pack(images)
        pix_d = torch.from_numpy(pix).cuda()
        nz = Normalizer(48, lib=lib)

        def window(fn):
            lines, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < MIN_WINDOW_S:
                fn()
                lines += n
            lib.call("clstm_synchronize")
            return lines / (time.perf_counter() - t0)
        run_d = lambda: nz.run_device_pixels(pix_d, w, h)
        run_h = lambda: nz._run("clstm_normalizer_run_h", pix, w, h)
        for _ in range(2):
            run_d(); run_h()
        rd, rh = [], []
        for _ in range(ALTERNATIONS):
            rd.append(window(run_d))
            rh.append(window(run_h))
        say("%4d crops of the fixture line   run_d %9.0f lines/s (spread %4.1f %%)   run_h %9.0f lines/s (spread %4.1f %%)   device bytes %d"
            % (n, np.median(rd), 100 * spread(rd), np.median(rh), 100 * spread(rh), nz.device_bytes()))
        # the host normaliser on the same lines
        raws = os.path.join(tmp, "crops%d.raw" % n)
        with open(raws, "wb") as f:
            for a in images:
                f.write(struct.pack("<ii", a.shape[0], a.shape[1]))
                f.write(a.tobytes())
        for threads in (1, 16):
            r = []
            for _ in range(ALTERNATIONS):
                out = subprocess.run([os.path.join(BIN, "clstm_hosttool"), "normalize-bench", raws, "48", str(threads)], check=True,
                                     capture_output=True, text=True).stdout.split()
                r.append(float(out[out.index("lines/s") - 1]))
            say("%4d crops, host CenterNormalizer on %2d thread(s) %9.0f lines/s (spread %4.1f %%)" % (n, threads, np.median(r), 100 * spread(r)))
        del nz


def cli_rates(say):
    from make_corpus import make_corpus
    d = tempfile.mkdtemp(prefix="prep_cli_")
    names, _ = make_corpus(d, n=512, seed=0)
    env = dict(os.environ, batch="64", ntrain="64", lrate="1e-4", nhidden="100", seed="0.222", save_name=os.path.join(d, "_m"),
               save_every="64", report_every="1000000", test_every="100000000")
    subprocess.run([os.path.join(BIN, "clstmocrtrain"), os.path.join(d, "list.txt")], env=env, check=True, capture_output=True, timeout=600)
    model = sorted(glob.glob(os.path.join(d, "_m-*.clstm")))[-1]
    rates, outs = {0: [], 1: []}, {}
    for _ in range(3):
        for g in (0, 1):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(BIN, "clstmocr"), os.path.join(d, "list.txt")],
                               env=dict(os.environ, load=model, batch="64", gpu_prep=str(g), save_text="0"), check=True, capture_output=True, timeout=600)
            rates[g].append(len(names) / (time.perf_counter() - t0))
            outs[g] = r.stdout
    say("# clstmocr batch=64 on the 512-line rendered corpus, wall time of the whole process (start-up, PNG decoding included), lines/s")
    for g in (0, 1):
        say("clstmocr batch=64 gpu_prep=%d  %s   median %.0f (spread %.1f %%)" % (g, " ".join("%.0f" % r for r in rates[g]), float(np.median(rates[g])),
                                                                                 100 * spread(rates[g])))
    m0, m1 = float(np.median(rates[0])), float(np.median(rates[1]))
    say("gpu_prep=1 / gpu_prep=0: %.2f; faster by more than the spread: %s; same stdout: %s"
        % (m1 / m0, "yes" if min(rates[1]) > max(rates[0]) else "NO", "yes" if outs[0] == outs[1] else "NO"))


def kernel_table(say, d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Name"].startswith("k_nz_"):
                rows.append((r["Name"].split("(")[0], int(r["Calls"]), float(r["TotalDurationNs"])))
    total = sum(r[2] for r in rows)
    say("# device time per kernel (rocprofv3 --kernel-trace --stats of --profile-run: run_d on 64 crops of the fixture line)")
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        say("%-18s %5d launches  %9.1f us per call of 64 lines  %5.1f %%" % (name, calls, ns / 1e3 / PROFILE_CALLS, 100 * ns / total if total else 0.0))
    say("all k_nz_* kernels: %.1f us per call of 64 lines" % (total / 1e3 / PROFILE_CALLS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-table")
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_rate.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)
    if args.kernel_table:
        kernel_table(say, args.kernel_table)
        with open(args.out, "a") as f:
            f.write("\n".join(out) + "\n")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("gpu_prep_rate.py needs a GPU")
    tmp = tempfile.mkdtemp(prefix="prep_rate_")
    if args.profile_run:
        from clstm_amd import abi
        from clstm_amd.net import Normalizer
        images = fixture_crops(64, tmp)
        pix, w, h = Normalizer.pack(images)
        pix_d = torch.from_numpy(pix).cuda()
        nz = Normalizer(48, lib=abi.load())
        for _ in range(PROFILE_CALLS):
            nz.run_device_pixels(pix_d, w, h)
        abi.load().call("clstm_synchronize")
        return
    say("# line normalisation: device (clstm_normalizer_run_*) against the host CenterNormalizer; %s" % torch.cuda.get_device_name(0))
    normaliser_rates(say, tmp)
    if not args.skip_cli:
        cli_rates(say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
