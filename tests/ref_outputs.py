#!/usr/bin/env python3
"""The reference's answers to the tests that compare against it (test_oracle.py, test_host.py), recorded in
tests/golden/ref_outputs.json so that those tests run wherever the repository is checked out; where the reference
is built in place (oracle/_ref) they check it live as well.  Arrays are kept as SHA-256 digests of their bytes,
so a comparison with the recording is as strict as the bit-for-bit one against the live reference.  Regenerate
from the reference itself:

    make -C oracle all && python tests/ref_outputs.py
"""
import base64
import ctypes as C
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _checkers import Params, REF_CLI  # noqa: E402
from steganosaurus_amd.synth import cover_rgb  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ref_outputs.json")
HELLO_PNG = os.path.join(HERE, "golden", "cli_256_hello.png")
COVER_HASH_CASES = [(64, 64, 5, 0), (100, 30, 6, 1), (333, 200, 7, 0), (8, 8, 8, 1), (7, 300, 9, 0)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def checker_outputs(chk, variants):
    """test_oracle.py::test_against_live_reference: keys, keystream, 1-D FFTs, forward transform, walk, embed and extract in
    every parameter variant, capacity"""
    rng = np.random.default_rng(11)
    pk = hashlib.sha256(b"another pass").digest()
    out = {"subkeys": [k.hex() for k in chk.subkeys(pk)]}
    kw = chk.subkeys(pk)[0]
    out["ks_bytes"] = digest(chk.ks_bytes(kw, 5000))
    for n in (2, 8, 128, 1024):
        a = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        out["fft1d_%d" % n] = [digest(chk.fft1d(a)), digest(chk.fft1d(a, True))]
    for (W, H) in [(33, 17), (128, 64), (200, 120)]:
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        case = "%dx%d_" % (W, H)
        out[case + "forward"] = [digest(x) for x in chk.forward_rgb8(img)]
        _, bins, sk, ctr, start = chk.walk(kw, chk.next_pow2(H), chk.next_pow2(W), 150)
        out[case + "walk"] = [digest(bins), sk, ctr, start.tolist()]
        bits = rng.integers(0, 2, 150).astype(np.uint8)
        for name, kwargs in variants.items():
            P = Params(**kwargs)
            e = chk.embed_rgb8(img, pk, bits, P, True, True)
            out[case + name] = [digest(x) for x in e] + [digest(chk.extract_bits(e[0], pk, 150, P))]
        out[case + "capacity"] = chk.capacity_rgb8(img)[0]
    return out


def cover_hash_outputs(chk):
    """test_oracle.py::test_cover_hash_against_live_reference: region, hash, magnitudes, quantised bytes"""
    out = {}
    for (w, h, idx, center) in COVER_HASH_CASES:
        region, hsh, mags, q = chk.cover_hash(cover_rgb(w, h, idx), center)
        out["%dx%d_%d_c%d" % (w, h, idx, center)] = [region, hsh.hex(), digest(mags), q.tolist()]
    return out


def png_test_image():
    return np.random.default_rng(5).integers(0, 256, (37, 41, 3), dtype=np.uint8)


def png_content(path):
    """What a PNG decoder's result depends on: the signature, every chunk but IDAT as stored and the inflated image data
    (the deflate bytes themselves may differ between zlib builds)."""
    data = open(path, "rb").read()
    pos, parts, idat = 8, [data[:8]], b""
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        parts.append(kind)
        if kind == b"IDAT":
            idat += body
        else:
            parts.append(body)
        pos += 12 + n
    return hashlib.sha256(b"".join(parts) + zlib.decompress(idat)).hexdigest()


def unwraps(host, key_b64, wrapped_b64):
    """test_host.py::test_wrapped_key_from_reference_cli_unwraps: a key file the reference's gen-key wrapped with --wrap-pass pw
    (--pbkdf2_iter 1000) opens with the reference-compatible AEAD variant only, to the key it printed"""
    key, blob = base64.b64decode(key_b64), base64.b64decode(wrapped_b64)
    assert len(blob) == 80 and blob[:4] == b"TFKW"
    derived = hashlib.pbkdf2_hmac("sha256", b"pw", blob[4:20], 1000, 44)
    out = C.create_string_buffer(32)
    assert host.tfh_aead_open_turtle(derived[:32], blob[20:32], None, C.c_size_t(0), blob[32:64], C.c_size_t(32), blob[64:80], out) == 1
    assert out.raw == key
    assert host.tfh_aead_open(derived[:32], blob[20:32], None, C.c_size_t(0), blob[32:64], C.c_size_t(32), blob[64:80], out) == 0


def reference_gen_key(tmp):
    """(printed key, wrapped key file) of one run of the reference CLI's gen-key"""
    kf = os.path.join(tmp, "w.txt")
    r = subprocess.run([REF_CLI, "gen-key", "--key-out", kf, "--wrap-pass", "pw", "--pbkdf2_iter", "1000"],
                       capture_output=True, text=True, check=True)
    return re.search(r"Base64: (\S+)", r.stdout).group(1), open(kf).read().strip()


def main():
    from _checkers import Checker
    from test_oracle import VARIANTS
    R = Checker("ref")
    host = C.CDLL(os.path.join(os.path.dirname(HERE), "steganosaurus_amd", "libtfhost.so"))
    with tempfile.TemporaryDirectory() as tmp:
        img = png_test_image()
        q = os.path.join(tmp, "ours.png")
        assert host.tfh_png_write(q.encode(), img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0]) == 0
        assert np.array_equal(R.png_read(q), img)          # the reference's decoder reads what our writer wrote
        png = {"cli_256_hello": digest(R.png_read(HELLO_PNG)), "written_37x41": png_content(q)}
        key_b64, wrapped = reference_gen_key(tmp)
    out = {"source": "oracle/_ref (the reference compiled in place), tests/ref_outputs.py",
           "checker": checker_outputs(R, VARIANTS), "cover_hash": cover_hash_outputs(R), "png": png,
           "gen_key": {"key_b64": key_b64, "wrapped": wrapped}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
