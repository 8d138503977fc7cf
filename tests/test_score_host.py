"""The C++ host side of clstm_net_score: CLSTMOCR::score / align through the drivers' opt-in switches (clstmocrtrain test_loss=1,
clstmocr align=1) on the reference's OCR fixture.  The model is a few training iterations of the drop-in driver, as in
test_gpu_e2e.py: the checks hold for any weights."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_e2e import BIN, FIXTURE, GT, ROOT, fixture_frames

NH = 20


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """two runs of clstmocrtrain with the same seed, the fixture as training and as test set: test_loss unset / test_loss=1"""
    tmp = tmp_path_factory.mktemp("score_host")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    png = tmp / "textline.bin.png"
    png.write_bytes(open(FIXTURE, "rb").read())
    (tmp / "textline.gt.txt").write_text(GT + "\n", encoding="utf-8")
    lst = tmp / "list.txt"
    lst.write_text(str(png) + "\n")
    runs = {}
    for name, extra in (("plain", {}), ("loss", {"test_loss": "1"})):
        env = dict(os.environ, ntrain="41", nhidden=str(NH), lrate="1e-2", save_name=str(tmp / ("_" + name)), seed="0.222",
                   test_every="20", save_every="20", report_every="20", **extra)
        r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), str(lst), str(lst)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = r.stdout
    model = tmp / "_loss-40.clstm"
    assert model.exists(), runs["loss"][-1000:]
    return {"tmp": tmp, "lst": lst, "png": png, "model": model, "runs": runs}


@pytest.mark.gpu
def test_clstmocrtrain_test_loss(trained):
    plain, loss = trained["runs"]["plain"], trained["runs"]["loss"]
    assert "TESTLOSS" not in plain
    lines = loss.splitlines()
    got = [ln.split() for ln in lines if ln.startswith("TESTLOSS")]
    errs = [k for k, ln in enumerate(lines) if ln.startswith("ERROR")]
    assert len(got) == len(errs) >= 2
    for k in errs:
        assert lines[k + 1].startswith("TESTLOSS " + lines[k].split()[1] + " "), lines[k:k + 2]
    for g in got:
        assert len(g) == 4 and int(g[3]) == 1 and np.isfinite(float(g[2])), g
    # everything else is what the run without the switch printed (the two runs save under different names)
    strip = lambda text: [ln.replace("_loss", "_plain") for ln in text.splitlines() if not ln.startswith("TESTLOSS")]
    assert strip(loss) == strip(plain)


def run_clstmocr(trained, **extra):
    r = subprocess.run([os.path.join(BIN, "clstmocr"), str(trained["lst"])], env=dict(os.environ, load=str(trained["model"]), **extra),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def parse_alignment(out):
    lines = out.splitlines()
    a = [k for k, ln in enumerate(lines) if ln.startswith("align ")]
    assert len(a) == 1, out
    e = next(k for k in range(a[0], len(lines)) if lines[k].startswith("end "))
    triples = [ln.split("\t") for ln in lines[a[0] + 1:e]]
    return lines[:a[0]] + lines[e + 1:], [(c, int(x0), int(x1)) for c, x0, x1 in triples], float(lines[e].split()[1])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "4"])
def test_clstmocr_align(trained, tmp_path, batch):
    T = len(fixture_frames(tmp_path))
    plain = run_clstmocr(trained, batch=batch)
    assert "align" not in plain
    rest, triples, score = parse_alignment(run_clstmocr(trained, batch=batch, align="1"))
    assert rest == plain.splitlines()
    assert [c for c, _, _ in triples] == list(GT)
    assert np.isfinite(score)
    seen = [(x0, x1) for _, x0, x1 in triples if (x0, x1) != (-1, -1)]
    assert len(seen) >= 1
    assert all(0 <= x0 <= x1 < T for x0, x1 in seen), (T, triples)
    assert all(a[0] <= b[0] and a[1] < b[0] for a, b in zip(seen, seen[1:])), triples


@pytest.mark.gpu
def test_clstmocr_align_skips_a_ground_truth_outside_the_codec(trained, tmp_path):
    """a second line whose ground truth holds a character the model never saw: a noalign note in place of its alignment, the first
    line's alignment and all recognition output as before"""
    png2 = tmp_path / "other.bin.png"
    png2.write_bytes(open(FIXTURE, "rb").read())
    (tmp_path / "other.gt.txt").write_text("per\u00e9formance\n", encoding="utf-8")
    lst = tmp_path / "two.txt"
    lst.write_text(str(trained["png"]) + "\n" + str(png2) + "\n")
    for batch in ("1", "2"):
        env = dict(os.environ, load=str(trained["model"]), batch=batch)
        plain = subprocess.run([os.path.join(BIN, "clstmocr"), str(lst)], env=env, capture_output=True, text=True, timeout=300)
        r = subprocess.run([os.path.join(BIN, "clstmocr"), str(lst)], env=dict(env, align="1"), capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0 and r.returncode == 0, r.stderr[-2000:]
        notes = [ln for ln in r.stdout.splitlines() if ln.startswith("noalign ")]
        assert len(notes) == 1 and str(png2) in notes[0], r.stdout
        rest, triples, _ = parse_alignment("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("noalign ")))
        assert rest == plain.stdout.splitlines() and [c for c, _, _ in triples] == list(GT)


@pytest.mark.gpu
def test_clstmocr_score_equals_python(trained, tmp_path, backend_hip):
    from clstm_amd.net import Network, spans
    frames = fixture_frames(tmp_path)
    raw = tmp_path / "params.raw"
    subprocess.check_call([os.path.join(BIN, "clstm_hosttool"), "params", str(trained["model"]), str(raw)])
    codec = [int(x) for x in subprocess.run([os.path.join(BIN, "clstm_hosttool"), "codec", str(trained["model"])], check=True,
                                             capture_output=True, text=True).stdout.split()]
    labels = np.array([codec.index(ord(ch)) for ch in GT], np.int32)
    net = Network(frames.shape[1], [NH], len(codec), lib=backend_hip.lib)
    net.set_params(np.fromfile(raw, np.float32))
    net.set_training(False)          # clstmocr's per-line loop: CLSTMOCR::predict = clstm_net_forward outside a training step
    net.set_inputs([frames])
    net.forward()
    s = float(net.score([labels])[0])
    path = net.align([labels])[0]
    _, triples, score = parse_alignment(run_clstmocr(trained, align="1"))
    assert abs(score - s) <= 1e-4 * max(1.0, abs(s)), (score, s)
    assert [(x0, x1) for _, x0, x1 in triples] == spans(path, len(labels))


@pytest.fixture(scope="module")
def backend_hip():
    from common import Backend
    return Backend("hip")
