"""Above the ABI of the lexicon-constrained beam search: clstm_amd.lexicon.Lexicon and its C++ twin clstm_amd/host/lexicon.h (the same
words and word classes from the same word-list file, through clstm_hosttool lexicon), the stand-alone check program (address and
undefined-behaviour sanitizers, host code only: the loader and the trie builder), and clstmocr beam=W lexicon=FILE on the
reference's OCR fixture with the small model tests/test_gpu_e2e.py trains on it (201 updates on the one line)."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_e2e import BIN, FIXTURE, GT, ROOT

NH, NC = 20, 83


def test_the_loader_and_the_trie_builder_under_sanitizers():
    """clstm_amd/host/lexicon_check.cc: lexicon.h and csrc/lexicon_trie.h alone, built with -fsanitize=address,undefined, run on the CPU"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "check-lexicon"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lexicon_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def host_bin():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"], timeout=900)
    return BIN


WORD_LIST = (b"cab\r\n  bad\t\r\ncab\n\nd\xc3\xa9j\xc3\xa0\nwith space\nZZZ\nbroken\xff\n" + b"a" * 300 + b"\nface")   # (no newline at the end)


@pytest.fixture(scope="module")
def fresh_model(tmp_path_factory, host_bin):
    """a model whose codec maps class i to the character chr(96 + i): a .. z are classes 1 .. 26"""
    tmp = tmp_path_factory.mktemp("lex_host")
    model = tmp / "fresh.clstm"
    subprocess.check_call([os.path.join(host_bin, "clstm_hosttool"), "init-model", "bidi", "48", str(NH), "0", str(NC), "0.222", str(model)])
    words = tmp / "words.txt"
    words.write_bytes(WORD_LIST)
    return tmp, model, words


def hosttool_lexicon(host_bin, model, words, word_chars=None):
    r = subprocess.run([os.path.join(host_bin, "clstm_hosttool"), "lexicon", str(model), str(words)] + ([word_chars] if word_chars is not None else []),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip("\n").split("\n")
    head = lines[0].split()
    counts = {head[k]: int(head[k + 1]) for k in (0, 2, 4)}
    classes = [int(x) for x in lines[1].split()[1:]]
    return counts, classes, [tuple(int(x) for x in ln.split()[1:]) for ln in lines[2:]]


@pytest.mark.parametrize("word_chars", [None, "abcdef", "abcdeé"])
def test_python_and_cpp_derive_the_same_words_and_classes(fresh_model, host_bin, word_chars):
    from clstm_amd.lexicon import Lexicon, read_word_list
    tmp, model, words = fresh_model
    codec = [int(x) for x in subprocess.run([os.path.join(host_bin, "clstm_hosttool"), "codec", str(model)], check=True,
                                             capture_output=True, text=True).stdout.split()]
    enc = {cp: c for c, cp in enumerate(codec)}
    lx = Lexicon.from_file(str(words), lambda ch: enc.get(ord(ch)), len(codec), word_chars)
    counts, classes, cwords = hosttool_lexicon(host_bin, model, words, word_chars)
    assert cwords == lx.words and classes == np.flatnonzero(lx.word_class).tolist()
    nlines = len(read_word_list(str(words))) + 1   # (the line that is not UTF-8: counted by the C++ loader, skipped by the reader)
    assert counts == {"lines": nlines, "kept": len(lx.words), "dropped": lx.dropped + 1}
    if word_chars is None:
        # cab, bad, cab, face; dropped: deja (its accents are not in this codec), "with space", ZZZ, the broken line, 300 a
        assert lx.words == [(3, 1, 2), (2, 1, 4), (3, 1, 2), (6, 1, 3, 5)] and classes == [1, 2, 3, 4, 5, 6] and lx.dropped == 4
    elif word_chars == "abcdef":
        assert lx.words == [(3, 1, 2), (2, 1, 4), (3, 1, 2), (6, 1, 3, 5)] and classes == [1, 2, 3, 4, 5, 6]
    else:
        assert lx.words == [(3, 1, 2), (2, 1, 4), (3, 1, 2)] and classes == [1, 2, 3, 4, 5] and lx.dropped == 5   # face: f is no word character


# ---- clstmocr beam=W lexicon=FILE (GPU) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """tests/test_gpu_e2e.py's model: 201 updates on the fixture line; the list names the line twice"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "clstm_amd", "host"), "-s", "all"], timeout=900)
    tmp = tmp_path_factory.mktemp("lex_ocr")
    png = tmp / "textline.bin.png"
    png.write_bytes(open(FIXTURE, "rb").read())
    (tmp / "textline.gt.txt").write_text(GT + "\n", encoding="utf-8")
    one = tmp / "one.txt"
    one.write_text(str(png) + "\n")
    env = dict(os.environ, ntrain="201", hidden="50", lrate="1e-2", save_name=str(tmp / "_lex"), seed="0.222")
    r = subprocess.run([os.path.join(BIN, "clstmocrtrain"), str(one)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lst = tmp / "list.txt"
    lst.write_text(str(png) + "\n" + str(png) + "\n")
    return {"tmp": tmp, "model": tmp / "_lex-200.clstm", "lst": lst}


def run_clstmocr(t, ok=True, **extra):
    r = subprocess.run([os.path.join(BIN, "clstmocr"), str(t["lst"])], env=dict(os.environ, load=str(t["model"]), save_text="0", **extra),
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r.stdout, r.stderr


def nbest_blocks(out):
    """-> [rows of every "nbest" block], the other lines"""
    lines, blocks, rest, k = out.split("\n"), [], [], 0
    while k < len(lines):
        if lines[k].startswith("nbest "):
            e = next(j for j in range(k, len(lines)) if lines[j] == "end")
            blocks.append([ln.split("\t") for ln in lines[k + 1:e]])
            k = e + 1
        else:
            rest.append(lines[k])
            k += 1
    return blocks, rest


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "2"])
def test_clstmocr_lexicon(trained, batch):
    tmp = trained["tmp"]
    plain, _ = run_clstmocr(trained, batch=batch, beam="4", nbest="3")
    pblocks, prest = nbest_blocks(plain)
    assert len(pblocks) == 2 and pblocks[0][0][2] == GT == "performance analysis"
    # a lexicon that lacks "performance": every reported transcript splits into its words; a line on which nothing admissible survived
    # is marked, shows the plain search's hypotheses and is counted
    words = ["perform", "performs", "an", "analysis", "analyses", "a", "per", "form", "once", "romance", "lysis", "p", "e", "r", "f",
             "o", "m", "n", "c", "s", "y", "l", "i"]
    wl = tmp / "words.txt"
    wl.write_text("\n".join(words) + "\n", encoding="utf-8")
    out, err = run_clstmocr(trained, batch=batch, beam="4", nbest="3", lexicon=str(wl))
    blocks, rest = nbest_blocks(out)
    assert rest == prest and len(blocks) == 2 and blocks[0] == blocks[1]
    assert "lexicon: %d words, 0 lines" % len(words) in err
    missed = 0
    for got, want in zip(blocks, pblocks):
        if got and got[0][0] == "LEXMISS":
            missed += 1
            assert all(r[0] == "LEXMISS" for r in got) and [r[1:] for r in got] == want
            continue
        assert got and all(len(r) == 3 for r in got)
        for k, score, text in got:
            assert all(w in words for w in text.split(" ") if w), text
        assert got[0][2] != GT
    assert "lexicon: %d lines without an admissible transcript (LEXMISS)" % missed in err
    # the full lexicon keeps the top transcript (its score may move: a beam that holds only admissible prefixes gathers other paths)
    wl.write_text("performance\nanalysis\n", encoding="utf-8")
    out, err = run_clstmocr(trained, batch=batch, beam="4", nbest="3", lexicon=str(wl))
    full = nbest_blocks(out)[0]
    assert full[0][0][2] == GT and "lexicon: 0 lines without" in err
    assert all(w in ("performance", "analysis") for r in full[0] for w in r[2].split(" ") if w)
    # word_chars="p" and one word the line is too short to finish (256 p through 255 blanks need 511 frames): after the first p no
    # separator is allowed any more, so with beam=1 nothing admissible survives: LEXMISS, and the hypotheses of the plain search
    wl.write_text("p" * 256 + "\n", encoding="utf-8")
    plain1, _ = run_clstmocr(trained, batch=batch, beam="1")
    out, err = run_clstmocr(trained, batch=batch, beam="1", lexicon=str(wl), word_chars="p")
    blocks, rest = nbest_blocks(out)
    p1, prest1 = nbest_blocks(plain1)
    assert rest == prest1 and len(blocks) == 2
    for got, want in zip(blocks, p1):
        assert got and all(r[0] == "LEXMISS" for r in got) and [r[1:] for r in got] == want
    assert "lexicon: 2 lines without an admissible transcript (LEXMISS)" in err
    _, err = run_clstmocr(trained, ok=False, batch=batch, lexicon=str(wl))
    assert "lexicon= needs beam=" in err
    assert run_clstmocr(trained, batch=batch, beam="4", nbest="3", lexicon="")[0] == plain, "without lexicon= the output is unchanged"
