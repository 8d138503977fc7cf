"""Lexicons for the beam search (clstm_ctc_beam_lex_batch / clstm_net_beam_lex, include/clstm_abi.h).

A lexicon over nc classes is a flag per class -- word_class[c]: words are made of it; class 0 (blank) never is, the other classes
without the flag are separators -- and a set of words, label sequences over word classes.  A labelling is admissible when every
maximal run of word classes in it is one of the words.  clstm_amd/csrc/ctc_beam.h (third part) states how the search uses it; the
library builds the trie and owns the device copy.  clstm_amd/host/lexicon.h reads the same word-list files in C++ (UTF-8, one word
per line) and derives the same word classes.
"""
import ctypes as C

import numpy as np

from .abi import i32, load, ptr

MAX_WORD = 256   # code points: a longer line of a word list is dropped (clstm_amd/host/lexicon.h)


def read_word_list(path):
    """-> the words of a UTF-8 word list, one per line: line ends LF or CRLF, blanks around a word dropped, empty lines skipped.
    A line that is not valid UTF-8 is dropped (lexicon.h counts it)."""
    out = []
    with open(path, "rb") as f:
        for raw in f.read().split(b"\n"):
            try:
                w = raw.decode("utf-8")
            except UnicodeDecodeError:
                continue
            w = w.strip(" \t\r")
            if w:
                out.append(w)
    return out


class Lexicon:
    def __init__(self, nc, word_class, words, lib=None):
        """word_class: one flag per class; words: label sequences over the flagged classes"""
        nc = int(nc)
        if nc < 2:
            raise ValueError("Lexicon: nc must be at least 2")
        wc = np.asarray(word_class).reshape(-1)
        if wc.shape != (nc,):
            raise ValueError("Lexicon: word_class holds one flag per class")
        self.nc, self.word_class = nc, np.ascontiguousarray(wc != 0, np.uint8)
        if self.word_class[0]:
            raise ValueError("Lexicon: class 0 (blank) cannot be a word class")
        self.words = [tuple(int(c) for c in w) for w in words]
        for w in self.words:
            if not w:
                raise ValueError("Lexicon: an empty word")
            if any(c < 1 or c >= nc or not self.word_class[c] for c in w):
                raise ValueError("Lexicon: a word holds a label that is not a word class of 1 .. nc-1")
        self.lib, self._h = lib, None

    @classmethod
    def from_strings(cls, words, encode, nc, word_chars=None, lib=None):
        """words: strings; encode(ch) -> the class of a character, or None / a value outside 1 .. nc-1 when the codec lacks it.
        A word with such a character is dropped and counted (self.dropped).  word_chars (a string) names the word characters;
        the default: a class is a word class iff it occurs in a kept word -- the rule of clstm_amd/host/lexicon.h."""
        kept, dropped = [], 0
        for w in words:
            lab = [encode(ch) for ch in w]
            if len(lab) > MAX_WORD or not lab or any(c is None or c < 1 or c >= nc for c in lab):
                dropped += 1
                continue
            kept.append(tuple(int(c) for c in lab))
        flags = np.zeros(nc, np.uint8)
        if word_chars is None:
            for w in kept:
                flags[list(w)] = 1
        else:
            for ch in word_chars:
                c = encode(ch)
                if c is not None and 1 <= c < nc:
                    flags[c] = 1
            ok = [w for w in kept if all(flags[c] for c in w)]   # a word with a character that is no word character cannot be written
            dropped += len(kept) - len(ok)
            kept = ok
        lx = cls(nc, flags, kept, lib=lib)
        lx.dropped = dropped
        return lx

    @classmethod
    def from_file(cls, path, encode, nc, word_chars=None, lib=None):
        return cls.from_strings(read_word_list(path), encode, nc, word_chars, lib)

    # ---- the device copy ----
    def handle(self, lib=None):
        """the clstm_lexicon of this lexicon in `lib` (made at the first call; a lexicon lives in one library)"""
        if self._h is None:
            self.lib = lib or self.lib or load()
            flat = i32([c for w in self.words for c in w] or [0])
            off = i32(np.concatenate([[0], np.cumsum([len(w) for w in self.words])]))
            h = C.c_void_p()
            self.lib.call("clstm_lexicon_create", C.byref(h), self.nc, ptr(self.word_class), ptr(flat), ptr(off), len(self.words))
            self._h = h
        elif lib is not None and lib is not self.lib:
            raise ValueError("Lexicon: the device copy belongs to another library")
        return self._h

    def info(self, lib=None):
        """-> dict(words, nodes, edges, device_bytes): distinct words, trie nodes with the root, edges, bytes on the device"""
        out = np.zeros(4, np.int64)
        h = self.handle(lib)
        self.lib.call("clstm_lexicon_info", h, ptr(out))
        return dict(zip(("words", "nodes", "edges", "device_bytes"), (int(v) for v in out)))

    def admits(self, labels, lib=None):
        """0: not an admissible prefix; 1: an admissible prefix whose last run is unfinished; 2: an admissible labelling
        (clstm_lexicon_admits: the library's walk over the arrays it uploaded)"""
        lab = i32(list(labels) or [0])
        out = C.c_int(-1)
        h = self.handle(lib)
        self.lib.call("clstm_lexicon_admits", h, ptr(lab), len(labels), C.byref(out))
        return out.value

    def close(self):
        if self._h is not None:
            self.lib.call("clstm_lexicon_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
