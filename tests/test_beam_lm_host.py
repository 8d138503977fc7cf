"""Above the ABI of the beam search with a language model: clstm_amd.lm.CharLM (estimate, save / load), its C++ twin
clstm_amd/host/charlm.h through the clstmlm driver (the same bytes) and the stand-alone check program (address and
undefined-behaviour sanitizers, host code only), and clstmocr beam=W lm=FILE on the reference's OCR fixture with a freshly
initialised model (clstm_hosttool init-model: the checks hold for any weights)."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_gpu_e2e import BIN, FIXTURE, ROOT, fixture_frames

NH, NC = 20, 83
F32 = np.float32
# six lines over classes 1 .. 3, counted by hand below (clstm_amd/host/charlm_check.cc counts the same corpus)
CORPUS = [[1, 2], [1, 2, 3], [2], [1, 1], [], [3, 1, 2]]
K = 0.1


def lg(count, total, nc=4):
    return F32(math.log((count + K) / (total + K * nc)))


def test_estimate_against_counts_done_by_hand():
    from clstm_amd.lm import CharLM
    m = CharLM.estimate(CORPUS, 4, 2, add_k=K)
    assert m.table.shape == (4, 4) and m.end.shape == (4,) and m.table.dtype == F32
    # context 0 (line start): 1 x3, 2 x1, 3 x1, end x1 (the empty line): 6 events
    assert m.table[0, 1] == lg(3, 6) and m.table[0, 2] == lg(1, 6) and m.table[0, 3] == lg(1, 6) and m.end[0] == lg(1, 6)
    # context 1: -> 2 x3, -> 1 x1, end x1 (the line 1 1): 5 events
    assert m.table[1, 2] == lg(3, 5) and m.table[1, 1] == lg(1, 5) and m.table[1, 3] == lg(0, 5) and m.end[1] == lg(1, 5)
    # context 2: -> 3 x1, end x3;  context 3: -> 1 x1, end x1
    assert m.table[2, 3] == lg(1, 4) and m.end[2] == lg(3, 4) and m.table[3, 1] == lg(1, 2) and m.end[3] == lg(1, 2)
    assert (m.table[:, 0] == 0).all()
    m = CharLM.estimate(CORPUS, 4, 3, add_k=K)
    assert m.table.shape == (16, 4) and m.end.shape == (16,)
    # context (0, 1) = 1: -> 2 x2, -> 1 x1;  (1, 2) = 6: -> 3 x1, end x2;  (3, 1) = 13: -> 2 x1;  (2, 1) = 9: never seen
    assert m.table[1, 2] == lg(2, 3) and m.table[1, 1] == lg(1, 3) and m.table[6, 3] == lg(1, 3) and m.end[6] == lg(2, 3)
    assert m.table[13, 2] == lg(1, 1) and m.table[9, 1] == lg(0, 0) and m.end[9] == lg(0, 0)
    # the smoothed events of a context sum to one: labels and the line end
    assert np.allclose(np.exp(m.table[:, 1:].astype(np.float64)).sum(1) + np.exp(m.end.astype(np.float64)), 1.0, atol=1e-6)
    for bad in (dict(add_k=0.0), dict(add_k=-1.0), dict(add_k=float("nan")), dict(order=1), dict(order=4), dict(nc=1), dict(nc=407, order=3)):
        kw = dict(nc=4, order=2, add_k=K)
        kw.update(bad)
        with pytest.raises(ValueError):
            CharLM.estimate(CORPUS, **kw)
    with pytest.raises(ValueError):
        CharLM.estimate([[1, 4]], 4, 2)
    # the value a labelling gets: left to right, start contexts padded with 0
    m2 = CharLM.estimate(CORPUS, 4, 2, add_k=K)
    want = 0.5 * (float(m2.table[0, 1]) + float(m2.table[1, 2]) + float(m2.end[2])) + 2 * 0.25
    assert abs(m2.value([1, 2], 0.5, 0.25) - want) < 1e-12


def test_save_load_round_trip_and_broken_files(tmp_path):
    from clstm_amd.lm import MAGIC, CharLM
    for order, end in ((2, True), (3, True), (3, False)):
        m = CharLM.estimate(CORPUS, 4, order, add_k=K)
        if not end:
            m = CharLM(order, 4, m.table)
        path = str(tmp_path / "m.lm")
        m.save(path)
        data = open(path, "rb").read()
        assert data[:8] == MAGIC and len(data) == 20 + 4 * (4 ** order + (4 ** (order - 1) if end else 0))
        assert np.frombuffer(data[8:20], "<i4").tolist() == [order, 4, int(end)]
        r = CharLM.load(path)
        assert (r.order, r.nc) == (order, 4) and r.table.tobytes() == m.table.tobytes() and r.tobytes() == data
        assert (r.end is None) == (not end)
        for cut in (0, 7, 19, 20, len(data) - 1):
            open(path, "wb").write(data[:cut])
            with pytest.raises(ValueError):
                CharLM.load(path)
        open(path, "wb").write(data + b"\0")
        with pytest.raises(ValueError, match="after the tables"):
            CharLM.load(path)
        open(path, "wb").write(b"X" + data[1:])
        with pytest.raises(ValueError, match="CLSTMLM1"):
            CharLM.load(path)
        for head in ((1, 4, 1), (3, 1 << 30, 1), (3, -4, 0), (3, 4, 2), (2, 8193, 0)):
            open(path, "wb").write(MAGIC + np.asarray(head, "<i4").tobytes() + data[20:])
            with pytest.raises(ValueError, match="bad header"):
                CharLM.load(path)
        bad = bytearray(data)
        bad[20 + 4 * 5:20 + 4 * 6] = np.asarray([np.inf], "<f4").tobytes()
        open(path, "wb").write(bytes(bad))
        with pytest.raises(ValueError, match="not finite"):
            CharLM.load(path)


@pytest.fixture(scope="module")
def host_bin():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])
    return BIN


def test_the_loader_and_estimator_under_sanitizers():
    """clstm_amd/host/charlm_check.cc: charlm.h alone, built with -fsanitize=address,undefined, run on the CPU"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "check-charlm"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "charlm_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory, host_bin):
    """a model whose codec maps class i to the character chr(96 + i), and ground truths beside (absent) line images"""
    tmp = tmp_path_factory.mktemp("lm_host")
    model = tmp / "fresh.clstm"
    subprocess.check_call([os.path.join(host_bin, "clstm_hosttool"), "init-model", "bidi", "48", str(NH), "0", str(NC), "0.222", str(model)])
    rng = np.random.default_rng(3)
    seqs = [rng.integers(1, NC, n).tolist() for n in (5, 1, 12, 0, 7, 30)] + [[1, 1, 2, 1, 1, 2]]
    names = []
    for k, s in enumerate(seqs):
        (tmp / ("line%d.gt.txt" % k)).write_text("".join(chr(96 + c) for c in s) + "\n", encoding="utf-8")
        names.append(str(tmp / ("line%d.bin.png" % k)))
    lst = tmp / "gt_list.txt"
    lst.write_text("\n".join(names) + "\n")
    return {"tmp": tmp, "model": model, "seqs": seqs, "list": lst}


@pytest.mark.parametrize("order,add_k", [(2, "0.1"), (3, "0.1"), (3, "0.37")])
def test_clstmlm_writes_pythons_bytes(corpus_dir, host_bin, order, add_k):
    from clstm_amd.lm import CharLM
    out = corpus_dir["tmp"] / ("cc_%d_%s.lm" % (order, add_k))
    r = subprocess.run([os.path.join(host_bin, "clstmlm"), str(corpus_dir["list"])], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, load=str(corpus_dir["model"]), order=str(order), add_k=add_k, out=str(out), params="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    want = CharLM.estimate(corpus_dir["seqs"], NC, order, add_k=float(add_k)).tobytes()
    got = out.read_bytes()
    assert len(got) == len(want) and got == want
    assert CharLM.load(str(out)).order == order
    r = subprocess.run([os.path.join(host_bin, "clstmlm"), str(corpus_dir["list"])], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, load=str(corpus_dir["model"]), order="5", out=str(out), params="0"))
    assert r.returncode != 0 and "order must be 2 or 3" in r.stderr


# ---- clstmocr beam=W lm=FILE (GPU) -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh(corpus_dir):
    from clstm_amd.lm import CharLM
    tmp = corpus_dir["tmp"]
    png = tmp / "textline.bin.png"
    png.write_bytes(open(FIXTURE, "rb").read())
    lst = tmp / "list.txt"
    lst.write_text(str(png) + "\n")
    rng = np.random.default_rng(9)
    lm = CharLM(3, NC, rng.normal(-2.0, 1.0, (NC * NC, NC)).astype(F32), rng.normal(-2.0, 1.0, NC * NC).astype(F32))
    lm.save(str(tmp / "random3.lm"))
    return {"tmp": tmp, "lst": lst, "png": png, "model": corpus_dir["model"], "lm": tmp / "random3.lm"}


def run_clstmocr(fresh, ok=True, **extra):
    r = subprocess.run([os.path.join(BIN, "clstmocr"), str(fresh["lst"])], env=dict(os.environ, load=str(fresh["model"]), save_text="0", **extra),
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r.stdout if ok else r.stderr


def parse_nbest(out, columns):
    lines = out.split("\n")
    a = [k for k, ln in enumerate(lines) if ln.startswith("nbest ")]
    assert len(a) == 1, out
    e = next(k for k in range(a[0], len(lines)) if lines[k] == "end")
    rows = [ln.split("\t") for ln in lines[a[0] + 1:e]]
    assert all(len(r) == columns for r in rows), rows
    return lines[:a[0]] + lines[e + 1:], rows


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "4"])
def test_clstmocr_zero_weight_prints_the_beam_hypotheses_with_the_extra_column(fresh, batch):
    plain = run_clstmocr(fresh, batch=batch, beam="4")
    rest0, rows0 = parse_nbest(plain, 3)
    rest, rows = parse_nbest(run_clstmocr(fresh, batch=batch, beam="4", lm=str(fresh["lm"]), lm_weight="0"), 4)
    assert rest == rest0 and len(rows) == len(rows0) == 4
    for (k0, s0, t0), (k, s, am, t) in zip(rows0, rows):
        assert (k, s, am, t) == (k0, s0, s0, t0)
    assert "lm= needs beam=" in run_clstmocr(fresh, ok=False, batch=batch, lm=str(fresh["lm"]))
    assert run_clstmocr(fresh, batch=batch, beam="4", lm="") == plain, "without lm= the output is unchanged"


@pytest.fixture(scope="module")
def backend_hip():
    from common import Backend
    return Backend("hip")


@pytest.mark.gpu
def test_clstmocr_with_a_weight_equals_network_beam_lm(fresh, tmp_path, backend_hip):
    from clstm_amd.lm import CharLM
    from clstm_amd.net import Network
    one = parse_nbest(run_clstmocr(fresh, beam="4", nbest="3", lm=str(fresh["lm"]), lm_weight="0.6", lm_bonus="0.25"), 4)[1]
    for extra in ({"batch": "4"}, {"gpu_prep": "1"}):
        rows = parse_nbest(run_clstmocr(fresh, beam="4", nbest="3", lm=str(fresh["lm"]), lm_weight="0.6", lm_bonus="0.25", **extra), 4)[1]
        assert [r[3] for r in rows] == [r[3] for r in one], extra
        assert all(abs(float(a[j]) - float(b[j])) <= 1e-4 * max(1.0, abs(float(a[j]))) for a, b in zip(rows, one) for j in (1, 2)), (extra, rows, one)
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
    lm = CharLM.load(str(fresh["lm"]), lib=backend_hip.lib)
    hyps = net.beam_lm(lm, 0.6, 0.25, beam=4, nbest=3)[0]
    assert len(hyps) == len(one) == 3
    for (lab, s, am), (k, s1, am1, text) in zip(hyps, one):
        assert "".join(chr(codec[c]) for c in lab) == text
        assert abs(s - float(s1)) <= 1e-4 * max(1.0, abs(s)) and abs(am - float(am1)) <= 1e-4 * max(1.0, abs(am))
    plain = net.beam(4, 3)[0]
    assert [h[0].tolist() for h in hyps] != [h[0].tolist() for h in plain] or any(abs(a[1] - b[1]) > 1e-3 for a, b in zip(hyps, plain))
