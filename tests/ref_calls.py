"""What the reference's own Fortran modules (oracle/_ref/libkiwi_ref.so, plus the CRUST2.0 tables of the reference tree) answered
to the seeded inputs of the tests that compare against them, committed as tests/golden/ref_calls_<name>.npz.  Those tests run
everywhere: with the reference build present every call goes to the live library and its answer must equal the recorded one;
without it the recorded answer stands in for the call.  Each recorded call carries a digest of its inputs, so a recording is
never replayed to a question it was not the answer to.

Recording (where oracle/_ref and the reference's aux data exist):
    KIWI_REF_RECORD=1 python -m pytest tests/test_oracle_vs_ref.py tests/test_oracle_eikonal.py tests/test_lm_minpack.py
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _digest(inputs):
    h = hashlib.sha256()
    for v in inputs:
        a = np.ascontiguousarray(v)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest()[:8], np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class RefCalls:
    """calls(key, fn, *inputs) -> the reference's outputs (a tuple of numbers / arrays) for `inputs`: fn() where `live`, else the
    recording.  The i-th call under a key is matched to the i-th recorded one."""

    def __init__(self, name, live):
        self.path = os.path.join(GOLDEN, "ref_calls_%s.npz" % name)
        self.live = bool(live)
        self.record = self.live and os.environ.get("KIWI_REF_RECORD") == "1"
        self.rec = {}
        if os.path.exists(self.path) and not self.record:
            with np.load(self.path) as z:
                self.rec = self._decode(z)
        self.count = {}
        self.new = {}

    def __call__(self, key, fn, *inputs):
        i = self.count.get(key, 0)
        self.count[key] = i + 1
        h = _digest(inputs)
        want = self.rec.get(key)
        if want is not None and i < len(want[0]):
            assert np.array_equal(want[0][i], h), "%s #%d: the inputs differ from the recorded ones" % (key, i)
        if self.live:
            out = tuple(np.asarray(v) for v in fn())
            if self.record:
                self.new.setdefault(key, ([], []))
                self.new[key][0].append(h)
                self.new[key][1].append(out)
            elif want is not None:
                assert i < len(want[0]) and all(_same(a, b) for a, b in zip(out, want[1][i])), \
                    "%s #%d: the live reference differs from its recording" % (key, i)
            return tuple(v[()] if v.ndim == 0 else v for v in out)
        assert want is not None and i < len(want[0]), "%s #%d: not recorded (%s)" % (key, i, os.path.basename(self.path))
        return tuple(v[()] if v.ndim == 0 else v.copy() for v in want[1][i])

    def save(self):
        """(recording runs only) write what the live library answered"""
        if not self.record or not self.new:
            return
        z = {}
        for key, (hs, outs) in self.new.items():
            z[key + ":h"] = np.stack(hs)
            for j in range(len(outs[0])):
                arrs = [np.asarray(o[j]) for o in outs]
                z["%s:%d:d" % (key, j)] = np.concatenate([a.ravel() for a in arrs])
                z["%s:%d:s" % (key, j)] = np.array([a.shape for a in arrs], np.int64).reshape(len(arrs), arrs[0].ndim)
        np.savez_compressed(self.path, **z)

    @staticmethod
    def _decode(z):
        rec = {}
        keys = sorted(set(k.split(":")[0] for k in z.files))
        for key in keys:
            hs = z[key + ":h"]
            outs = [[] for _ in range(len(hs))]
            j = 0
            while "%s:%d:d" % (key, j) in z.files:
                d, shapes = z["%s:%d:d" % (key, j)], z["%s:%d:s" % (key, j)]
                off = 0
                for i, s in enumerate(shapes):
                    s = tuple(int(v) for v in s)
                    n = int(np.prod(s)) if s else 1
                    outs[i].append(d[off:off + n].reshape(s))
                    off += n
                j += 1
            rec[key] = (list(hs), [tuple(o) for o in outs])
        return rec
