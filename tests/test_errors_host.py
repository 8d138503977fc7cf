"""The C++ host side of clstm_net_errors / clstm_edit_distance_batch: CLSTMOCR::errors_current through the drivers' opt-in switches
(clstmocrtrain gpu_errors=1, clstmocr errs=1) on the rendered corpus and the trained model of tests/test_predict_host.py (150 lines,
800 updates of 64).  Every figure is an integer compared with the Python referee of tests/test_edit_distance.py on the texts the
driver printed.  Every subprocess has a timeout."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_edit_distance import levenshtein, ref_edit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "clstm_amd", "bin")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N_LINES, UPDATES, LRATE = 150, 800, "1e-4"


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from make_corpus import make_corpus
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"], timeout=900)
    d = str(tmp_path_factory.mktemp("errors_host"))
    names, texts = make_corpus(d, n=N_LINES, seed=1)
    env = dict(os.environ, batch="64", ntrain=str(64 * UPDATES), lrate=LRATE, nhidden="100", seed="0.222",
               save_name=os.path.join(d, "_m"), save_every=str(64 * UPDATES), report_every=str(64 * UPDATES), test_every="100000000")
    r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), os.path.join(d, "list.txt")], env=env, capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    models = sorted(glob.glob(os.path.join(d, "_m-*.clstm")))
    assert models, r.stdout[-2000:]
    return d, names, texts, models[-1]


@pytest.mark.gpu
def test_clstmocrtrain_gpu_errors_prints_the_same(trained):
    """the batched test pass with its errors counted on the device against the host's levenshtein loop, between the updates of a
    running training loop (CLSTM_OVERLAP=0: tests/test_predict_host.py says why): same ERROR lines, same everything else.  150 test
    lines in chunks of 8: the last chunk has 6."""
    d, names, texts, model = trained
    outs = []
    for ge in (0, 1):
        env = dict(os.environ, load=model, batch="16", test_batch="8", gpu_errors=str(ge), ntrain=str(64 * UPDATES + 16 * 12),
                   CLSTM_OVERLAP="0", save_name=os.path.join(d, "_e%d" % ge), save_every="100000000", report_every="64", test_every="64")
        r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), os.path.join(d, "list.txt"), os.path.join(d, "list.txt")], env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(r.stdout.replace("_e%d" % ge, "_e"))
    assert outs[0].count("ERROR ") >= 2, outs[0][-2000:]
    assert outs[0] == outs[1]


def run_ocr(lst, model, **var):
    env = dict(os.environ, load=model, save_text="0", **{k: str(v) for k, v in var.items()})
    r = subprocess.run([os.path.join(BIN, "clstmocr"), lst], env=env, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.decode("utf-8")


def split_errs(out):
    """-> (the other lines, {file: [dist, sub, ins, del, reflen]}, {file: (dist, k)}, (dist, reflen, rate) or None, [(count, ref, out)])"""
    rest, errs, oracle, cer, conf = [], {}, {}, None, []
    for ln in out.split("\n"):
        f = ln.split(" ")
        if f[0] == "ERRS":
            errs[f[1]] = [int(x) for x in f[2:]]
        elif f[0] == "ORACLE":
            oracle[f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "CER":
            cer = (int(f[1]), int(f[2]), float(f[3]))
        elif f[0] == "CONF":
            body = ln.split(" ", 2)[2]   # "<ref> <out>": either character may be a space itself
            conf.append((int(f[1]), body[0], body[2]))
        else:
            rest.append(ln)
    return rest, errs, oracle, cer, conf


def referee(outputs, gts):
    """outputs, gts: {file: text} -> ({file: [dist, sub, ins, del, reflen]}, the CONF rows)"""
    rows, table = {}, {}
    for name, gt in gts.items():
        h, r = [ord(c) for c in outputs[name]], [ord(c) for c in gt]
        d, ops = ref_edit(h, r)
        assert d == levenshtein(h, r)
        rows[name] = [d, ops.count(1), ops.count(2), ops.count(3), len(r)]
        i = j = 0
        for op in ops:
            key = (r[j] if op != 2 else 0, h[i] if op != 3 else 0)
            table[key] = table.get(key, 0) + 1
            i, j = i + (op != 3), j + (op != 2)
    off = sorted(((n, rc, hc) for (rc, hc), n in table.items() if rc != hc), key=lambda e: (-e[0], e[1], e[2]))
    name = lambda c: "_" if c == 0 else chr(c)
    return rows, [(n, name(rc), name(hc)) for n, rc, hc in off[:20]]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 64])
def test_clstmocr_errs(trained, batch):
    d, names, texts, model = trained
    lst = os.path.join(d, "list.txt")
    plain = run_ocr(lst, model, batch=batch)
    assert "ERRS" not in plain and "CER" not in plain and "CONF" not in plain
    assert run_ocr(lst, model, batch=batch, errs=0) == plain
    rest, errs, oracle, cer, conf = split_errs(run_ocr(lst, model, batch=batch, errs=1))
    assert rest == plain.split("\n"), "without the ERRS / CER / CONF lines the output is the plain run's"
    outputs = dict(ln.split("\t", 1) for ln in plain.split("\n") if ln)
    assert sum(1 for t in outputs.values() if t.strip()) >= len(names) / 2, "inconclusive: the model decodes almost nothing"
    want, want_conf = referee(outputs, dict(zip(names, texts)))
    assert errs == want and not oracle
    assert sum(r[0] for r in want.values()) > 0, "inconclusive: no error at all"
    tot, ref = sum(r[0] for r in want.values()), sum(r[4] for r in want.values())
    assert cer[:2] == (tot, ref) and abs(cer[2] - tot / ref) <= 1e-5 * tot / ref   # (the rate is printed with 6 digits)
    assert conf == want_conf


@pytest.mark.gpu
def test_clstmocr_errs_some_lines_without_ground_truth_and_oracle(trained, tmp_path):
    """lines without a .gt.txt get no ERRS line and count nowhere; with beam=W every counted line gains its best-of-n distance"""
    d, names, texts, model = trained
    keep = 12
    listed = []
    for k in range(keep):
        png = tmp_path / ("%04d.bin.png" % k)
        shutil.copy(names[k], png)
        if k % 3 != 1:
            (tmp_path / ("%04d.gt.txt" % k)).write_text(texts[k] + "\n", encoding="utf-8")
        listed.append(str(png))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(listed) + "\n")
    gts = {n: texts[k] for k, n in enumerate(listed) if k % 3 != 1}
    for batch in (1, 5):
        plain = run_ocr(str(lst), model, batch=batch)
        rest, errs, oracle, cer, conf = split_errs(run_ocr(str(lst), model, batch=batch, errs=1))
        assert rest == plain.split("\n")
        outputs = dict(ln.split("\t", 1) for ln in plain.split("\n") if ln)
        want, want_conf = referee(outputs, gts)
        assert errs == want and conf == want_conf
        assert cer[:2] == (sum(r[0] for r in want.values()), sum(r[4] for r in want.values()))
        # beam=4 nbest=3: the smallest distance among the hypotheses the driver printed, and the first that has it
        out = run_ocr(str(lst), model, batch=batch, errs=1, beam=4, nbest=3)
        _, errs_b, oracle, _, _ = split_errs(out)
        assert errs_b == want and set(oracle) == set(gts)
        lines = out.split("\n")
        for name, gt in gts.items():
            a = lines.index("nbest " + name)
            e = lines.index("end", a)
            hyps = [ln.split("\t")[2] for ln in lines[a + 1:e]]
            dists = [levenshtein(h, gt) for h in hyps]
            assert oracle[name] == (min(dists), int(np.argmin(dists))), (name, oracle[name], dists)
