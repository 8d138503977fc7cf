"""Character n-gram language models for the beam search (clstm_ctc_beam_lm_batch / clstm_net_beam_lm, include/clstm_abi.h).

A model is a dense float32 table lm[ctx][c] of order 2 or 3 -- nc^(order-1) rows of nc columns, labels 1 .. nc-1, 0 = "no label
yet"; order 2: ctx = the last label, order 3: ctx = nc * (the label before last) + the last label -- and an optional end table
end[ctx].  clstm_amd/csrc/ctc_beam.h states how the search uses it.  This module estimates, stores and loads such tables and owns
the device copy; clstm_amd/host/charlm.h is the same estimator and file format in C++ (the two write the same bytes).

File format (little endian): 8 bytes magic "CLSTMLM1", int32 order, int32 nc, int32 end flag (0 | 1), nc^order float32 of the
table row by row, then nc^(order-1) float32 of the end table when the flag is 1.
"""
import ctypes as C
import math
import struct

import numpy as np

from .abi import f32, load, ptr

MAGIC = b"CLSTMLM1"
MAX_FLOATS = 1 << 26


def context_of(prefix, order, nc):
    """ctx(prefix) as the search keeps it: start contexts are padded with 0"""
    last = int(prefix[-1]) if len(prefix) >= 1 else 0
    if order == 2:
        return last
    before = int(prefix[-2]) if len(prefix) >= 2 else 0
    return nc * before + last


class CharLM:
    def __init__(self, order, nc, table, end=None, lib=None):
        order, nc = int(order), int(nc)
        if order not in (2, 3):
            raise ValueError("CharLM: order must be 2 or 3")
        if nc < 2 or nc ** order > MAX_FLOATS:
            raise ValueError("CharLM: nc must be at least 2 and the table at most 2^26 floats")
        self.order, self.nc, self.nctx = order, nc, nc ** (order - 1)
        self.table = f32(table).reshape(self.nctx, nc)
        self.end = None if end is None else f32(end).reshape(self.nctx)
        if not np.isfinite(self.table).all() or (self.end is not None and not np.isfinite(self.end).all()):
            raise ValueError("CharLM: a table entry is not finite")
        self.lib, self._h = lib, None

    # ---- the device copy ----
    def handle(self, lib=None):
        """the clstm_charlm of this model in `lib` (made at the first call; a model lives in one library)"""
        if self._h is None:
            self.lib = lib or self.lib or load()
            h = C.c_void_p()
            self.lib.call("clstm_charlm_create", C.byref(h), self.order, self.nc, ptr(self.table), ptr(self.end))
            self._h = h
        elif lib is not None and lib is not self.lib:
            raise ValueError("CharLM: the device copy belongs to another library")
        return self._h

    def close(self):
        if self._h is not None:
            self.lib.call("clstm_charlm_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the value the search gives a labelling (a host restatement, float64: for inspection and tests) ----
    def value(self, labels, weight, bonus=0.0, with_end=True):
        v = 0.0
        for j, c in enumerate(labels):
            v += weight * float(self.table[context_of(labels[:j], self.order, self.nc), int(c)]) + bonus
        if with_end and self.end is not None:
            v += weight * float(self.end[context_of(labels, self.order, self.nc)])
        return v

    # ---- estimation ----
    @staticmethod
    def counts(label_sequences, nc, order):
        """-> (count[ctx][c], endcount[ctx]) as int64; labels outside 1 .. nc-1 are an error"""
        nctx = nc ** (order - 1)
        cnt, endc = np.zeros((nctx, nc), np.int64), np.zeros(nctx, np.int64)
        for seq in label_sequences:
            seq = [int(c) for c in seq]
            if any(c < 1 or c >= nc for c in seq):
                raise ValueError("CharLM.estimate: a label lies outside 1 .. nc-1")
            for j, c in enumerate(seq):
                cnt[context_of(seq[:j], order, nc), c] += 1
            endc[context_of(seq, order, nc)] += 1
        return cnt, endc

    @classmethod
    def estimate(cls, label_sequences, nc, order, add_k=0.1, lib=None):
        """add-k smoothed log relative frequencies.  The events of a context are the nc - 1 labels and the line end:
        lm[ctx][c] = log((count[ctx][c] + k) / (total[ctx] + k nc)), end[ctx] the same with the count of lines that ended in
        ctx, total[ctx] = all of them; column 0 is 0.  Quotient and logarithm in float64 (the C library's log), rounded to
        float32 once."""
        add_k = float(add_k)
        if not (add_k > 0.0 and math.isfinite(add_k)):
            raise ValueError("CharLM.estimate: add_k must be positive and finite")
        nc, order = int(nc), int(order)
        if order not in (2, 3) or nc < 2 or nc ** order > MAX_FLOATS:
            raise ValueError("CharLM.estimate: order must be 2 or 3, nc at least 2, the table at most 2^26 floats")
        cnt, endc = cls.counts(label_sequences, nc, order)
        den = (cnt.sum(1) + endc).astype(np.float64) + add_k * float(nc)
        q = np.concatenate([(cnt.astype(np.float64) + add_k) / den[:, None], ((endc.astype(np.float64) + add_k) / den)[:, None]], 1)
        uq, inv = np.unique(q, return_inverse=True)
        logs = np.array([math.log(x) for x in uq], np.float64)[inv.reshape(q.shape)].astype(np.float32)
        table = np.ascontiguousarray(logs[:, :nc])
        table[:, 0] = 0.0
        return cls(order, nc, table, np.ascontiguousarray(logs[:, nc]), lib=lib)

    # ---- the file ----
    def tobytes(self):
        head = MAGIC + struct.pack("<iii", self.order, self.nc, 0 if self.end is None else 1)
        return head + self.table.astype("<f4").tobytes() + (b"" if self.end is None else self.end.astype("<f4").tobytes())

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.tobytes())

    @classmethod
    def load(cls, path, lib=None):
        with open(path, "rb") as f:
            data = f.read(20)
            if len(data) != 20 or data[:8] != MAGIC:
                raise ValueError("%s: not a CLSTMLM1 file" % path)
            order, nc, flag = struct.unpack("<iii", data[8:])
            if order not in (2, 3) or nc < 2 or nc ** order > MAX_FLOATS or flag not in (0, 1):
                raise ValueError("%s: bad header (order %d, nc %d, end flag %d)" % (path, order, nc, flag))
            nctx = nc ** (order - 1)
            want = 4 * (nctx * nc + (nctx if flag else 0))
            body = f.read(want + 1)
        if len(body) != want:
            raise ValueError("%s: %s" % (path, "truncated" if len(body) < want else "bytes after the tables"))
        vals = np.frombuffer(body, "<f4")
        return cls(order, nc, vals[:nctx * nc], vals[nctx * nc:] if flag else None, lib=lib)
