#!/usr/bin/env python3
"""Records tests/golden/aead_vectors.json from the system libcrypto
(tests/aead_libcrypto.py): ChaCha20-Poly1305 (IETF) vectors from
EVP_chacha20_poly1305, HChaCha20 vectors from the raw EVP_chacha20 block minus
the state, and XChaCha20-Poly1305 records by composition of the two.  Inputs
are seeded; the keys include the reference's two test keys
(encrypt_test.go:14-15).  Nothing here uses tests/aead_ref.py: the file is the
independent pin test_aead_host.py holds the reference to.

    python tools/aead_vectors.py            # rewrites the golden file
"""
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import aead_libcrypto  # noqa: E402

KEYS = ("6368616e676520746869732070617373776f726420746f206120736563726574",
        "746f74616c6c7920646966666572656e74206b65792075736564206865726521")
SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 300)


def main():
    lc = aead_libcrypto.load()
    if lc is None:
        sys.exit("libcrypto cannot be loaded")
    rng = random.Random(20250)
    keys = [bytes.fromhex(k) for k in KEYS] + [rng.randbytes(32), bytes(32), b"\xff" * 32]
    ietf, hch, xch = [], [], []
    for n, size in enumerate(SIZES):
        key = keys[n % len(keys)]
        nonce = rng.randbytes(24)
        pt = rng.randbytes(size)
        ietf.append({"key": key.hex(), "nonce": nonce[:12].hex(), "pt": pt.hex(),
                     "sealed": lc.ietf_seal(key, nonce[:12], pt).hex()})
        xch.append({"key": key.hex(), "nonce": nonce.hex(), "pt": pt.hex(),
                    "record": lc.xseal(key, nonce, pt).hex()})
    for key in keys:
        nonce = rng.randbytes(16)
        hch.append({"key": key.hex(), "nonce": nonce.hex(), "subkey": lc.hchacha20(key, nonce).hex()})
    # draft-irtf-cfrg-xchacha 2.2.1, kept only because libcrypto reproduces it
    pub = {"key": bytes(range(32)).hex(), "nonce": "000000090000004a0000000031415927",
           "subkey": "82413b4227b27bfed30e42508a877d73a0f9e4d58a74a853c12ec41326d3ecdc"}
    assert lc.hchacha20(bytes.fromhex(pub["key"]), bytes.fromhex(pub["nonce"])).hex() == pub["subkey"]
    out = {"source": "libcrypto (EVP_chacha20_poly1305, EVP_chacha20), tools/aead_vectors.py",
           "test_keys": list(KEYS), "ietf": ietf, "hchacha20": hch, "published_hchacha20": [pub],
           "xchacha20poly1305": xch}
    path = os.path.join(REPO, "tests", "golden", "aead_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
