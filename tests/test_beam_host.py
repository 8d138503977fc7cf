"""The C++ host side of clstm_net_beam: CLSTMOCR::predict_nbest / nbest_current through clstmocr's opt-in beam=W nbest=K, on the
reference's OCR fixture and a freshly initialised model (clstm_hosttool init-model): the checks hold for any weights."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_e2e import BIN, FIXTURE, ROOT, fixture_frames

NH, NC = 20, 83


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("beam_host")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    png = tmp / "textline.bin.png"
    png.write_bytes(open(FIXTURE, "rb").read())
    lst = tmp / "list.txt"
    lst.write_text(str(png) + "\n")
    model = tmp / "fresh.clstm"
    subprocess.check_call([os.path.join(BIN, "clstm_hosttool"), "init-model", "bidi", "48", str(NH), "0", str(NC), "0.222", str(model)])
    return {"tmp": tmp, "lst": lst, "png": png, "model": model}


def run_clstmocr(fresh, **extra):
    r = subprocess.run([os.path.join(BIN, "clstmocr"), str(fresh["lst"])], env=dict(os.environ, load=str(fresh["model"]), save_text="0", **extra),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def parse_nbest(out):
    """-> (the other lines, [(k, score, text)])"""
    lines = out.split("\n")
    a = [k for k, ln in enumerate(lines) if ln.startswith("nbest ")]
    assert len(a) == 1, out
    e = next(k for k in range(a[0], len(lines)) if lines[k] == "end")
    rows = [ln.split("\t") for ln in lines[a[0] + 1:e]]
    assert all(len(r) == 3 for r in rows), rows
    return lines[:a[0]] + lines[e + 1:], [(int(k), float(s), t) for k, s, t in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "4"])
def test_clstmocr_output_is_unchanged_without_beam(fresh, batch):
    plain = run_clstmocr(fresh, batch=batch)
    assert "nbest" not in plain
    assert run_clstmocr(fresh, batch=batch, beam="0") == plain
    rest, rows = parse_nbest(run_clstmocr(fresh, batch=batch, beam="4", nbest="3"))
    assert rest == plain.split("\n")
    assert [k for k, _, _ in rows] == [0, 1, 2]
    sc = [s for _, s, _ in rows]
    assert all(np.isfinite(sc)) and sc[0] >= sc[1] >= sc[2]
    assert len({t for _, _, t in rows}) == 3, "three different texts"


@pytest.mark.gpu
def test_clstmocr_nbest_with_align(fresh, tmp_path):
    """no ground truth beside the line: align=1 aligns the top hypothesis"""
    T = len(fixture_frames(tmp_path))
    out = run_clstmocr(fresh, beam="4", nbest="2", align="1")
    rest, rows = parse_nbest(out)
    a = [k for k, ln in enumerate(rest) if ln.startswith("align ")]
    e = [k for k, ln in enumerate(rest) if ln.startswith("end ")]
    assert len(a) == 1 and len(e) == 1, out
    triples = [ln.split("\t") for ln in rest[a[0] + 1:e[0]]]
    assert "".join(c for c, _, _ in triples) == rows[0][2]
    assert all(-1 <= int(x0) <= int(x1) < T for _, x0, x1 in triples)
    assert "align" not in run_clstmocr(fresh, align="1"), "without beam there is nothing to align"


@pytest.mark.gpu
def test_clstmocr_nbest_equals_predict_nbest_and_python(fresh, tmp_path, backend_hip):
    """the per-line loop (CLSTMOCR::predict + nbest_current), the batched path (CLSTMOCR::predict_nbest, frames normalised on the
    host and on the device) and Network.beam on the same frames and parameters give the same top text"""
    from clstm_amd.net import Network
    one = parse_nbest(run_clstmocr(fresh, beam="4", nbest="3"))[1]
    for extra in ({"batch": "4"}, {"gpu_prep": "1"}):
        rows = parse_nbest(run_clstmocr(fresh, beam="4", nbest="3", **extra))[1]
        assert rows[0][2] == one[0][2], extra
        assert all(abs(a[1] - b[1]) <= 1e-4 * max(1.0, abs(a[1])) for a, b in zip(rows, one)), (extra, rows, one)
    frames = fixture_frames(tmp_path)
    raw = tmp_path / "params.raw"
    subprocess.check_call([os.path.join(BIN, "clstm_hosttool"), "params", str(fresh["model"]), str(raw)])
    codec = [int(x) for x in subprocess.run([os.path.join(BIN, "clstm_hosttool"), "codec", str(fresh["model"])], check=True,
                                             capture_output=True, text=True).stdout.split()]
    net = Network(frames.shape[1], [NH], len(codec), lib=backend_hip.lib)
    net.set_params(np.fromfile(raw, np.float32))
    net.set_training(False)          # clstmocr's per-line loop: CLSTMOCR::predict = clstm_net_forward outside a training step
    net.set_inputs([frames])
    net.forward()
    hyps = net.beam(4, 3)[0]
    assert len(hyps) == len(one) == 3
    assert "".join(chr(codec[c]) for c in hyps[0][0]) == one[0][2]
    assert abs(hyps[0][1] - one[0][1]) <= 1e-4 * max(1.0, abs(one[0][1]))


@pytest.fixture(scope="module")
def backend_hip():
    from common import Backend
    return Backend("hip")
