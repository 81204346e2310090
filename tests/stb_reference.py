"""The reference's stb_image decode of a file, for the decoder tests.  Live from oracle/_ref (the reference's vendored stb_image translation unit,
`make -C oracle ref`) where that library is built; elsewhere from tests/golden/ref_stb_digests.json, the digests of what that build returned for
every file the tests write (tests/golden/make_ref_stb_golden.py records them).  A file is known by the sha256 of its bytes, a decode by its dtype,
shape and the sha256 of its bytes (128 bits of each): held against the digest, a decoder's output must still be bit for bit what the reference returned."""
import atexit
import hashlib
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_stb_digests.json")
RECORD = os.environ.get("PTC_RECORD_REF_STB")          # set by tests/golden/make_ref_stb_golden.py: collect the live decodes' digests

_table = None
_recorded = {}


def _key(kind, data):
    return f"{kind}:{hashlib.sha256(data).hexdigest()[:32]}"


def _digest(a):
    return f"{a.dtype.str}{list(a.shape)}:{hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]}"


def _recorded_digest(kind, data):
    global _table
    if _table is None:
        with open(GOLD) as f:
            _table = json.load(f)
    k = _key(kind, data)
    assert k in _table, f"{k}: no decode of this file recorded (a changed writer needs tests/golden/make_ref_stb_golden.py run where oracle/_ref is built)"
    return _table[k]


def equals_reference(ora, data, got, floats=False):
    """`got` is bit for bit what the reference's stb build makes of `data`: stbi_load_from_memory(..., 4) (uint8 RGBA), or with `floats`
    stbi_loadf_from_memory(..., 3) (float32 RGB)."""
    kind = "f3" if floats else "u4"
    if ora.have_ref_stb():
        want = ora.ref_stb_decode_float(data) if floats else ora.ref_stb_decode(data)
        if RECORD:
            _recorded[_key(kind, data)] = _digest(want)
        return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    return _digest(np.asarray(got)) == _recorded_digest(kind, data)


def refused_by_reference(ora, data, floats=False):
    """the reference's stb build refuses `data` (its decode raises ValueError)"""
    kind = "f3" if floats else "u4"
    if ora.have_ref_stb():
        try:
            ora.ref_stb_decode_float(data) if floats else ora.ref_stb_decode(data)
        except ValueError:
            if RECORD:
                _recorded[_key(kind, data)] = "refused"
            return True
        return False
    return _recorded_digest(kind, data) == "refused"


@atexit.register
def _write_record():
    if RECORD and _recorded:
        old = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        old.update(_recorded)
        with open(RECORD, "w") as f:
            json.dump(dict(sorted(old.items())), f, indent=0)
            f.write("\n")
