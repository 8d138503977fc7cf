"""Batched recognition in the drop-in tools: `clstmocr batch=N` and the test-set pass of `clstmocrtrain test_batch=N` must print and
write, byte for byte, what the line-by-line loops (batch=1, test_batch=1: the reference's) print and write.

The model is in the trained regime (the recipe of tests/test_corpus_decode.py with fewer lines and updates: 150 rendered lines --
not a multiple of 64 --, 800 updates of 64 lines, lrate 1e-4): at least half of the decodes must be non-empty, or the test fails
as inconclusive.  Every subprocess has a timeout."""
import glob
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "clstm_amd", "bin")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N_LINES, UPDATES, LRATE = 150, 800, "1e-4"


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from make_corpus import make_corpus
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"], timeout=900)
    d = str(tmp_path_factory.mktemp("predict_host"))
    names, texts = make_corpus(d, n=N_LINES, seed=1)
    env = dict(os.environ, batch="64", ntrain=str(64 * UPDATES), lrate=LRATE, nhidden="100", seed="0.222",
               save_name=os.path.join(d, "_m"), save_every=str(64 * UPDATES), report_every=str(64 * UPDATES), test_every="100000000")
    r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), os.path.join(d, "list.txt")], env=env, capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    models = sorted(glob.glob(os.path.join(d, "_m-*.clstm")))
    assert models, r.stdout[-2000:]
    return d, names, texts, models[-1]


def run_ocr(d, model, names, **var):
    """one clstmocr run over the whole list; returns (stdout, {file suffix: {name: sha1}}) and removes what it wrote"""
    env = dict(os.environ, load=model, **{k: str(v) for k, v in var.items()})
    r = subprocess.run([os.path.join(BIN, "clstmocr"), os.path.join(d, "list.txt")], env=env, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    written = {}
    for suffix in (".txt", ".p.png", ".lp.png"):
        written[suffix] = {}
        for n in names:
            f = n[:-len(".png")] + suffix
            if suffix == ".txt" and f.endswith(".gt.txt"):
                continue
            if os.path.exists(f):
                written[suffix][n] = hashlib.sha1(open(f, "rb").read()).hexdigest()
                os.remove(f)
    return r.stdout, written


@pytest.mark.gpu
def test_clstmocr_batch_is_byte_identical_to_line_by_line(trained):
    d, names, texts, model = trained
    assert len(names) % 64 != 0
    one, w1 = run_ocr(d, model, names, batch=1)
    many, w64 = run_ocr(d, model, names, batch=64)
    lines = one.decode("utf-8").rstrip("\n").split("\n")
    assert len(lines) == len(names)
    nonempty = sum(1 for l in lines if l.split("\t", 1)[1].strip())
    sys.stderr.write("predict_host: %d of %d decodes non-empty\n" % (nonempty, len(names)))
    assert nonempty >= len(names) / 2, "inconclusive: the model decodes almost nothing (%d of %d)" % (nonempty, len(names))
    assert many == one
    assert len(w1[".txt"]) == len(names) and w64[".txt"] == w1[".txt"]
    # a chunk size that leaves a one-line tail, few preparation threads
    odd, wodd = run_ocr(d, model, names, batch=149, prep_threads=2)
    assert odd == one and wodd[".txt"] == w1[".txt"]
    # conf=1: every line of stdout (index, frame, character, posterior)
    c1, _ = run_ocr(d, model, names, batch=1, conf=1)
    c64, _ = run_ocr(d, model, names, batch=64, conf=1)
    assert c1.count(b"\n") > len(names)
    assert c64.split(b"\n") == c1.split(b"\n")
    # output=posteriors: every .p.png; output=logs: every .lp.png
    for fmt, suffix in (("posteriors", ".p.png"), ("logs", ".lp.png")):
        _, p1 = run_ocr(d, model, names, batch=1, output=fmt)
        _, p64 = run_ocr(d, model, names, batch=64, output=fmt)
        assert len(p1[suffix]) == len(names) and p64[suffix] == p1[suffix], fmt


@pytest.mark.gpu
def test_clstmocrtrain_test_pass_batched_prints_the_same(trained):
    """the test-set pass through CLSTMOCR::predict_frames in chunks of 64 against the single-line loop, between the updates of a
    running training loop (the weights move: the model's own learning rate): same ERROR lines, same training reports around them.
    Both runs set CLSTM_OVERLAP=0.  At the default overlap mode the training loop of `clstmocrtrain batch=16` is itself not
    reproducible to the last decode on this corpus -- two IDENTICAL test_batch=1 runs printed 7 and 8 errors of 3096 at the same
    trial -- so there the comparison would measure the training loop's run-to-run noise, not the test pass; with the fused launches
    off the same runs reproduce (7 errors at any test_batch)."""
    d, names, texts, model = trained
    outs = []
    for tb in (1, 64):
        env = dict(os.environ, load=model, batch="16", test_batch=str(tb), ntrain=str(64 * UPDATES + 16 * 12), CLSTM_OVERLAP="0",
                   save_name=os.path.join(d, "_t%d" % tb), save_every="100000000", report_every="64", test_every="64")
        r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), os.path.join(d, "list.txt"), os.path.join(d, "list.txt")], env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(r.stdout.replace("_t%d" % tb, "_t"))
    assert outs[0].count("ERROR ") >= 2, outs[0][-2000:]
    assert outs[0] == outs[1]
