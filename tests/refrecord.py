"""The reference's outputs for the bit-exact oracle tests, recorded as digests under tests/golden/.

A test body takes a side (`Oracle()` or `Reference()`, the same calls on either library) and returns the
named arrays it compares.  `check` runs the body on the oracle and compares every array, bit for bit, with
the SHA-256 digest of the reference's array recorded in tests/golden/ref_digests.json.  Where the reference
build (oracle/_ref) is present, the same body also runs on the reference and its arrays must match the
record too.  `python tests/golden/make_golden.py digests` writes the record from the reference build.

Test infrastructure only: nothing under dsurftomo_amd/ imports this module.
"""
import hashlib
import json
import os

import numpy as np

import _libs as L

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")


def digest(a):
    """dtype, shape and every byte of the array"""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def canonical_solve(s):
    """the parts of a solve the tests compare: the coarse field, where the refined box is live / dead / zero,
    and the refined times where it is live"""
    sign = np.sign(s["Sr"]).clip(-1, 1).astype(np.int8)
    return {"T": np.asarray(s["T"], np.float32), "Sr": sign,
            "Tr": np.where(s["Sr"] >= 0, s["Tr"], np.float32(0)).astype(np.float32)}


class _OracleGrid:
    """the oracle's white-box calls with the interface of L.RefWB"""

    def __init__(self, nx, ny, goxd, gozd, dvxd, dvzd, gd=8):
        self.g = L.grid(nx, ny, goxd, gozd, dvxd, dvzd, gd)
        self.nnx, self.nnz = self.g.nnx, self.g.nnz
        self.gox, self.goz, self.dnx, self.dnz = [np.float32(v) for v in (self.g.gox, self.g.goz, self.g.dnx, self.g.dnz)]
        self.veln = self.pv = self.sol = None

    def gridder(self, pv):
        self.pv, self.veln = pv, L.o_gridder(self.g, pv)
        return self.veln

    def solve(self, x, z):
        self.sol = L.o_solve(self.g, self.pv, self.veln, x, z)
        return self.sol

    def srtimes(self, sx, sz, rx, rz):
        return L.o_srtimes(self.g, self.veln, self.sol["T"], sx, sz, rx, rz)

    def rpaths(self, sx, sz, rx, rz):
        return L.o_rpaths(self.g, self.sol, self.veln, sx, sz, rx, rz)[0]

    def close(self):
        pass


class Oracle:
    name = "oracle"

    def __init__(self):
        O = self.lib = L.oracle()
        self.calsurfg, self.synthetic, self.aprod, self.lsmr = O.dso_calsurfg, O.dso_synthetic, O.dso_aprod, O.dso_lsmr
        self.grid = _OracleGrid


class Reference:
    name = "ref"

    def __init__(self):
        R = self.lib = L.ref()
        assert R is not None, "reference build not available (make -C oracle ref)"
        self.calsurfg, self.synthetic, self.aprod, self.lsmr = R.calsurfg_, R.synthetic_, R.aprod_, R.ref_wb_lsmr
        self.grid = L.RefWB


_record = None


def recorded(name):
    global _record
    if _record is None:
        with open(RECORD) as f:
            _record = json.load(f)
    assert name in _record, "%s: no recorded reference outputs (python tests/golden/make_golden.py digests)" % name
    return _record[name]


def _mismatch(want, got):
    keys = sorted(set(want) | set(got))
    return [k for k in keys if want.get(k) != got.get(k)]


def check(name, body):
    """run `body` on the oracle and compare with the reference's record; also on the reference where it is built.
    Returns the oracle's arrays."""
    want = recorded(name)
    out = body(Oracle())
    bad = _mismatch(want, {k: digest(v) for k, v in out.items()})
    assert bad == [], "%s: the oracle differs from the reference in %d of %d arrays: %s" % (name, len(bad), len(want), bad[:12])
    if L.ref() is not None:
        live = {k: digest(v) for k, v in body(Reference()).items()}
        bad = _mismatch(want, live)
        assert bad == [], "%s: the reference build differs from its record in %s (regenerate tests/golden/ref_digests.json)" % (name, bad[:12])
    return out


def record(cases, path=RECORD):
    """cases: iterable of (name, body).  Runs every body on the reference and writes the digests."""
    ref = Reference()
    data = {name: {k: digest(v) for k, v in body(ref).items()} for name, body in cases}
    with open(path, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    return data
