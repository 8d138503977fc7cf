"""Line normalisation on the device (clstm_normalizer_*, clstm_amd/csrc/normalize.h): raw line images in, input frames out.
The acceptance property is identity with the host CenterNormalizer (clstm_amd/host/normalizer.h): the referee everywhere is
`clstm_hosttool normalize-raw`, frames are compared AS BYTES, T and r exactly.  Every case runs on the host emulator (CPU suite)
and, marked gpu, on the MI355X."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from common import synth_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "clstm_amd", "bin", "clstm_hosttool")
FIXTURE = os.path.join(ROOT, "tests", "golden", "textline.bin.png")
NORMALIZED = 25      # clstm_debug_path_count: lines normalised on the device


@pytest.fixture(scope="module", autouse=True)
def build_tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"])


def write_raw(path, img):
    img = np.ascontiguousarray(img, np.float32)
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", img.shape[0], img.shape[1]))
        f.write(img.tobytes())


def read_raw(path):
    data = open(path, "rb").read()
    w, h = struct.unpack("<ii", data[:8])
    return np.frombuffer(data[8:], np.float32).reshape(w, h)


_REFEREE = {}


def referee(tmp, img, height=48, params=None):
    """the host CenterNormalizer on one image -> (T, r, frames [T][height]); computed once per (image, parameters)"""
    img = np.ascontiguousarray(img, np.float32)
    key = (img.shape, img.tobytes(), height, params)
    if key not in _REFEREE:
        src, dst = os.path.join(tmp, "in.raw"), os.path.join(tmp, "out.raw")
        write_raw(src, img)
        args = [TOOL, "normalize-raw", src, dst, str(height)] + ([repr(float(p)) for p in params] if params else [])
        out = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split()
        frames = read_raw(dst)
        assert out[0] == "r" and out[2] == "width" and int(out[3]) == frames.shape[0] and frames.shape[1] == height
        _REFEREE[key] = (frames.shape[0], float(out[1]), frames)
    return _REFEREE[key]


def count(backend, which):
    out = ctypes.c_longlong(0)
    backend.lib.call("clstm_debug_path_count", which, ctypes.byref(out))
    return out.value


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_against_referee(tmp, nz, images, height=48, params=None):
    """one call on `images`: T, r and every line's frames against the referee"""
    T, r, frames = nz.run(images)
    assert frames.shape == (int(T.sum()), height)
    o = 0
    for b, img in enumerate(images):
        wt, wr, wf = referee(tmp, img, height, params)
        assert T[b] == wt and r[b] == np.float32(wr), (b, img.shape, T[b], wt, r[b], wr)
        got = frames[o:o + T[b]]
        assert same_bytes(got, wf), "line %d (%d x %d): %d of %d frame values differ, max |d| %g" % (
            b, img.shape[0], img.shape[1], int((got != wf).sum()), wf.size, float(np.abs(got - wf).max()))
        o += T[b]
    return T, r, frames


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("normalize"))


@pytest.fixture(scope="module")
def fixture_line(tmp):
    raw = os.path.join(tmp, "fixture.raw")
    subprocess.run([TOOL, "png2raw", FIXTURE, raw], check=True)
    img = np.float32(1.0) - read_raw(raw)             # ink = 1, as clstmocrtrain.cc:73 leaves it (v = -v + 1.0f)
    assert img.shape == (819, 88)
    return img


def grey(rng, w, h):
    """values k/255 from a seeded generator: float summation order matters"""
    return (rng.integers(0, 256, (w, h)).astype(np.float32) / np.float32(255.0)).astype(np.float32)


RAGGED = [(1, 1), (2, 3), (7, 2), (40, 150), (1500, 20), (333, 48), (64, 88), (65, 88)]


# ---- 1. the golden fixture -------------------------------------------------------------------------------------------
def test_fixture_line(backend, tmp, fixture_line):
    """the whole 819 x 88 line on the GPU, its first 160 columns on the emulator (to bound its time)"""
    from clstm_amd.net import Normalizer
    img = fixture_line if backend.kind == "hip" else fixture_line[:160]
    T, r, _ = check_against_referee(tmp, Normalizer(48, lib=backend.lib), [img])
    if backend.kind == "hip":
        assert 300 < T[0] < 450, T


# ---- 2. ragged batch of grey images ----------------------------------------------------------------------------------
def test_ragged_batch_and_one_per_call(backend, tmp):
    """rows shorter than the mask's reach (clamping dominates), a column taller than a wave, a row wider than any tile with
    halos on both sides, two lines sharing one h (a cached mask) and several distinct h; then the same images one per call"""
    from clstm_amd.net import Normalizer
    rng = np.random.default_rng(41)
    images = [grey(rng, w, h) for w, h in RAGGED]
    nz = Normalizer(48, lib=backend.lib)
    c0 = count(backend, NORMALIZED)
    T, r, frames = check_against_referee(tmp, nz, images)
    assert count(backend, NORMALIZED) == c0 + len(images)
    o = 0
    for b, img in enumerate(images):
        T1, r1, f1 = nz.run([img])
        assert T1[0] == T[b] and r1[0] == r[b] and same_bytes(f1, frames[o:o + T[b]]), b
        o += T[b]
    # pixels resident on the device: the same bytes
    pix, w, h = Normalizer.pack(images)
    Td, rd, _ = nz.run_device_pixels(backend.up(pix), w, h)
    assert np.array_equal(Td, T) and same_bytes(rd, r) and same_bytes(nz.frames(), frames)


# ---- 3. argmax ties --------------------------------------------------------------------------------------------------
def test_empty_and_constant_columns(backend, tmp):
    """columns partly empty and partly constant: ties in the per-column argmax go to the last row, the smear decides the rest"""
    from clstm_amd.net import Normalizer
    img = np.zeros((50, 20), np.float32)
    img[10:20, :] = 1.0
    img[30:40, 5:15] = 0.5
    img[44, 3] = 0.25
    check_against_referee(tmp, Normalizer(48, lib=backend.lib), [img, img[:25], img[25:]])


# ---- 4. parameters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,params", [(48, None), (32, None), (5, None), (48, (1.0, 0.5, 2.0)), (5, (0.7, 0.5, 2.0))],
                         ids=["h48", "h32", "h5", "range2_smooth1d_half", "h5_all_params"])
def test_target_height_and_parameters(backend, tmp, height, params):
    from clstm_amd.net import Normalizer
    rng = np.random.default_rng(43)
    images = [grey(rng, 90, 31), grey(rng, 33, 64)]
    images[0][:, :9] = 0.0
    images[0][:, 22:] = 0.0
    nz = Normalizer(height, *(params or ()), lib=backend.lib)
    check_against_referee(tmp, nz, images, height, params)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_blank_line_is_refused_by_index(backend, tmp):
    from clstm_amd.abi import ClstmError
    from clstm_amd.net import Normalizer
    rng = np.random.default_rng(47)
    good = [grey(rng, 60, 24), grey(rng, 35, 24)]
    nz = Normalizer(48, lib=backend.lib)
    nz.run(good)
    c0 = count(backend, NORMALIZED)
    with pytest.raises(ClstmError, match="line 1 "):
        nz.run_device([good[0], np.zeros((17, 24), np.float32), good[1]])
    assert b"line 1 " in backend.lib.dll.clstm_last_error()
    assert count(backend, NORMALIZED) == c0
    with pytest.raises(ClstmError, match="no frames"):       # no frames were produced for the call
        nz.lib.call("clstm_normalizer_get_frames_h", nz.h, np.zeros(1 << 16, np.float32).ctypes.data)
    T, r, frames = nz.run(good)
    Tf, rf, ff = Normalizer(48, lib=backend.lib).run(good)
    assert np.array_equal(T, Tf) and same_bytes(r, rf) and same_bytes(frames, ff)
    check_against_referee(tmp, nz, good)


def test_bad_arguments_are_refused_before_anything_is_touched(backend):
    from clstm_amd.abi import ClstmError, f32, i32, ptr
    from clstm_amd.net import Normalizer
    with pytest.raises(ClstmError, match="target_height"):
        Normalizer(0, lib=backend.lib)
    rng = np.random.default_rng(53)
    nz = Normalizer(48, lib=backend.lib)
    _, _, frames = nz.run([grey(rng, 20, 10)])
    b0, c0 = nz.device_bytes(), count(backend, NORMALIZED)
    pix, T, out = f32(np.ones(64)), np.zeros(2, np.int32), ctypes.c_void_p()
    for w, h, bs, what in (([4, 0], [4, 4], 2, "width 0"), ([4, 4], [0, 4], 2, "height 0"), ([4], [4], 0, "bs")):
        wa, ha = i32(w), i32(h)
        with pytest.raises(ClstmError, match=what):
            backend.lib.call("clstm_normalizer_run_h", nz.h, ptr(pix), ptr(wa), ptr(ha), bs, ptr(T), None, ctypes.byref(out))
    wa, ha = i32([1]), i32([600])
    with pytest.raises(ClstmError, match="NZ_MAXRANGE"):     # the stated limit, refused by name
        backend.lib.call("clstm_normalizer_run_h", nz.h, ptr(pix), ptr(wa), ptr(ha), 1, ptr(T), None, ctypes.byref(out))
    assert nz.device_bytes() == b0 and count(backend, NORMALIZED) == c0
    assert same_bytes(nz.frames(), frames)                   # the last good call's frames are still there


# ---- 6. chaining -----------------------------------------------------------------------------------------------------
def chain_images(rng):
    return [grey(rng, w, 30) for w in (61, 118, 90)]


def test_run_then_predict_equals_host_frames(backend, tmp):
    from clstm_amd.abi import i32, ptr
    from clstm_amd.net import Normalizer
    from test_predict import make_net, raw_predict, varied_params
    ni, nh, nc = 48, [8], 11
    rng = np.random.default_rng(59)
    images = chain_images(rng)
    lines = [referee(tmp, img)[2] for img in images]
    params = varied_params(backend, ni, nh, nc, lines)
    host, dev = make_net(backend, ni, nh, nc, params), make_net(backend, ni, nh, nc, params)
    cls_h, loc_h, conf_h, cnt_h = raw_predict(host, lines)
    z_h = host.outputs()
    nz = Normalizer(ni, lib=backend.lib)
    c0 = count(backend, NORMALIZED)
    T, _, frames_d = nz.run_device(images)
    assert count(backend, NORMALIZED) == c0 + len(images)
    assert T.tolist() == [len(x) for x in lines]
    N = int(T.sum())
    cls, loc = np.full(N, -7, np.int32), np.full(N, -7, np.int32)
    conf, cnt = np.full(N, -7.0, np.float32), np.full(len(T), -7, np.int32)
    backend.lib.call("clstm_net_predict", dev.h, ptr(i32(T)), len(T), frames_d, ptr(cls), ptr(loc), ptr(conf), ptr(cnt))
    dev.T, dev.N = [int(t) for t in T], N
    assert same_bytes(dev.outputs(), z_h) and np.array_equal(cnt, cnt_h) and cnt.sum() > 0
    off = np.concatenate([[0], np.cumsum(T)])
    for b in range(len(T)):
        o, k = off[b], cnt[b]
        assert np.array_equal(cls[o:o + k], cls_h[o:o + k]) and np.array_equal(loc[o:o + k], loc_h[o:o + k])
        assert same_bytes(conf[o:o + k], conf_h[o:o + k])
    # the Python chain gives the same decodes
    dec, locs, confs = dev.predict_images(images, nz)
    for b in range(len(T)):
        o, k = off[b], cnt[b]
        assert np.array_equal(dec[b], cls_h[o:o + k]) and same_bytes(confs[b], conf_h[o:o + k])


def test_run_then_train_step_equals_host_frames(backend, tmp):
    from clstm_amd.init import init_params
    from clstm_amd.net import Network, Normalizer
    ni, nh, nc = 48, [8], 11
    rng = np.random.default_rng(61)
    p0 = init_params(ni, nh, nc, seed=0.222) * 20
    host, dev = Network(ni, nh, nc, lib=backend.lib), Network(ni, nh, nc, lib=backend.lib)
    for n in (host, dev):
        n.set_params(p0)
        n.setLearningRate(1e-2, 0.9)
    nz = Normalizer(ni, lib=backend.lib)
    for step in range(2):
        images = chain_images(rng)
        lines = [referee(tmp, img)[2] for img in images]
        T = [len(x) for x in lines]
        trs = synth_labels(rng, len(T), 5, nc)
        x = backend.up(np.concatenate(lines, 0))      # (kept alive until the sync below: the step is asynchronous)
        host.train_step(T, x, trs)
        Td, _, frames_d = nz.run_device(images)
        assert Td.tolist() == T
        dev.train_step(T, frames_d, trs)
        backend.sync()
        assert same_bytes(dev.get_params(), host.get_params()), step
        assert same_bytes(dev.get_derivs(), host.get_derivs()), step
    assert not np.array_equal(host.get_params(), p0.astype(np.float32))
