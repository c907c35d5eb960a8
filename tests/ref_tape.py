"""The reference's answers for the tests that compare against its own code.

Where oracle/_ref is built (the reference checkout was present at build time) every call goes to
the compiled reference and its answer is checked against the recorded one under
tests/golden/ref_tape/.  Elsewhere the recorded answer is replayed, after checking that the
inputs are byte for byte the ones the reference was given when it was recorded.  So the tests
check the same thing on every machine, and a recording that drifts from the reference fails.

Recording (where oracle/_ref is built):

    VAQ_RECORD_REF_TAPE=1 python -m pytest tests -m "not gpu" -k reference
"""
from __future__ import annotations

import hashlib
import os
import re

import numpy as np

TAPE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tape")


def _digest(inputs) -> str:
    h = hashlib.sha256()
    for a in inputs:
        a = np.ascontiguousarray(np.asarray(a))
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


class RefTape:
    """One test's sequence of reference calls: call(fn, *inputs) returns fn()'s answer (a numpy
    array, a number or a tuple of them), live or replayed."""

    def __init__(self, oracle, test_name: str):
        self.live = oracle.have_ref()
        self.record = bool(os.environ.get("VAQ_RECORD_REF_TAPE"))
        if self.record and not self.live:
            raise RuntimeError("VAQ_RECORD_REF_TAPE needs oracle/_ref (built from the reference checkout)")
        self.path = os.path.join(TAPE_DIR, re.sub(r"[^A-Za-z0-9_.-]+", "_", test_name).strip("_") + ".npz")
        self.i = 0
        self.saved = {}
        if not self.record:
            assert os.path.exists(self.path), \
                f"{self.path} is missing: record it with VAQ_RECORD_REF_TAPE=1 where oracle/_ref is built"
            with np.load(self.path) as z:
                self.saved = {k: z[k] for k in z.files}

    def call(self, fn, *inputs):
        key = "c%d" % self.i
        self.i += 1
        digest = _digest(inputs)
        if self.record:
            out = fn()
            outs = out if isinstance(out, tuple) else (out,)
            self.saved[key + "_digest"] = np.array(digest)
            self.saved[key + "_n"] = np.array(len(outs) if isinstance(out, tuple) else -1)
            for j, o in enumerate(outs):
                self.saved["%s_out%d" % (key, j)] = np.asarray(o)
            os.makedirs(TAPE_DIR, exist_ok=True)
            np.savez_compressed(self.path, **self.saved)
            return out
        assert key + "_digest" in self.saved, f"{self.path}: no recorded call {key} (re-record the tape)"
        assert str(self.saved[key + "_digest"]) == digest, \
            f"{self.path}: the inputs of call {key} differ from the recorded ones (re-record the tape)"
        n = int(self.saved[key + "_n"])
        rec = tuple(self.saved["%s_out%d" % (key, j)] for j in range(max(n, 1)))
        if self.live:
            out = fn()
            outs = out if isinstance(out, tuple) else (out,)
            assert len(outs) == len(rec)
            for o, r in zip(outs, rec):
                o = np.asarray(o)
                assert o.dtype == r.dtype and o.shape == r.shape and o.tobytes() == r.tobytes(), \
                    f"{self.path}: the reference's answer to call {key} differs from the recorded one"
            return out
        if n < 0:
            r = rec[0]
            return r.item() if r.ndim == 0 else r
        return tuple(r.item() if r.ndim == 0 else r for r in rec)
