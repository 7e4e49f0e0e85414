"""The AEAD store converter (dsx_aead_*, desync_amd.encrypt): what can be checked
without a GPU -- the CPU reference (aead_ref.py) against the recorded vectors
and against libcrypto, the converter's names and validation
(encrypt_test.go), the exports, and the refusals that come before any device
work."""
import ctypes
import json
import os
import random

import pytest

import aead_libcrypto
import aead_ref
import desync_amd
from desync_amd import _lib
from desync_amd.store import chunk_file_name, chunk_id_from_filename

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# encrypt_test.go:14-15
TEST_KEY = "6368616e676520746869732070617373776f726420746f206120736563726574"
OTHER_KEY = "746f74616c6c7920646966666572656e74206b65792075736564206865726521"
NEW = ("dsx_aead_seal", "dsx_aead_open", "dsx_selftest_poly1305")


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(GOLDEN, "aead_vectors.json")) as f:
        return json.load(f)


def _b(v, *names):
    return [bytes.fromhex(v[n]) for n in names]


def test_reference_gives_the_recorded_ietf_vectors(vectors):
    assert len(vectors["ietf"]) >= 10
    for v in vectors["ietf"]:
        key, nonce, pt, sealed = _b(v, "key", "nonce", "pt", "sealed")
        assert aead_ref.ietf_seal(key, nonce, pt) == sealed
        assert aead_ref.ietf_open(key, nonce, sealed) == pt


def test_reference_gives_the_recorded_hchacha20_vectors(vectors):
    for v in vectors["hchacha20"] + vectors["published_hchacha20"]:
        key, nonce, sub = _b(v, "key", "nonce", "subkey")
        assert aead_ref.hchacha20(key, nonce) == sub


def test_reference_gives_the_recorded_xchacha_records(vectors):
    keys = set()
    for v in vectors["xchacha20poly1305"]:
        key, nonce, pt, rec = _b(v, "key", "nonce", "pt", "record")
        keys.add(v["key"])
        assert len(rec) == len(pt) + aead_ref.OVERHEAD and rec[:24] == nonce
        assert aead_ref.seal(key, nonce, pt) == rec
        assert aead_ref.open(key, rec) == pt
    assert {TEST_KEY, OTHER_KEY} <= keys and vectors["test_keys"] == [TEST_KEY, OTHER_KEY]


def test_reference_batch_form_equals_the_single_form():
    rng = random.Random(5)
    sizes = [0, 1, 63, 64, 65, 0, 200, 1000, 16, 4096 + 7]
    blob = rng.randbytes(11 + sum(sizes))
    ends, e = [], 11
    for s in sizes:
        e += s
        ends.append(e)
    key, nonces = rng.randbytes(32), rng.randbytes(24 * len(sizes))
    recs, rec_ends = aead_ref.seal_many(key, nonces, blob, ends, 11)
    prev, want = 11, b""
    for i, e in enumerate(ends):
        want += aead_ref.seal(key, nonces[24 * i:24 * i + 24], blob[prev:e])
        prev = e
        assert rec_ends[i] == len(want)
    assert recs == want


def test_reference_refuses_what_the_converter_refuses(vectors):
    v = vectors["xchacha20poly1305"][4]
    key, rec = _b(v, "key", "record")
    with pytest.raises(ValueError, match="no nonce prefix found in chunk, not encrypted or wrong algorithm"):
        aead_ref.open(key, rec[:23])
    for broken in (rec[:24], rec[:39], rec[:-1], bytes([rec[0] ^ 1]) + rec[1:], rec[:-1] + bytes([rec[-1] ^ 0x80])):
        with pytest.raises(aead_ref.AuthError, match="chacha20poly1305: message authentication failed"):
            aead_ref.open(key, broken)
    with pytest.raises(aead_ref.AuthError):
        aead_ref.open(bytes.fromhex(OTHER_KEY), rec)


def test_poly1305_edge_cases_of_the_reference():
    """r = 1, s = 0 and all-0xFF blocks: each block adds 2^129 - 1, so the sums
    pass 2^130 - 5; worked by hand here, independent of the loop in aead_ref."""
    otk = (1).to_bytes(16, "little") + bytes(16)
    p = (1 << 130) - 5
    for blocks in range(1, 7):
        want = (blocks * ((1 << 129) - 1)) % p % (1 << 128)
        assert aead_ref.poly1305(otk, b"\xff" * (16 * blocks)) == want.to_bytes(16, "little")
    # s all 0xFF: the carry out of 2^128 is dropped
    otk = (1).to_bytes(16, "little") + b"\xff" * 16
    want = (((1 << 129) - 1) + (1 << 128) - 1) % (1 << 128)
    assert aead_ref.poly1305(otk, b"\xff" * 16) == want.to_bytes(16, "little")


def test_reference_against_libcrypto():
    lc = aead_libcrypto.load()
    if lc is None:
        pytest.skip("libcrypto cannot be loaded (the recorded vectors still pin the reference)")
    rng = random.Random(8439)
    for size in (0, 1, 31, 64, 100, 1000, 4097, 70000):
        key, nonce, pt = rng.randbytes(32), rng.randbytes(24), rng.randbytes(size)
        rec = aead_ref.seal(key, nonce, pt)
        assert rec == lc.xseal(key, nonce, pt)
        assert lc.xopen(key, rec) == pt and aead_ref.open(key, rec) == pt
        assert aead_ref.hchacha20(key, nonce[:16]) == lc.hchacha20(key, nonce[:16])
        assert aead_ref.ietf_seal(key, nonce[:12], pt) == lc.ietf_seal(key, nonce[:12], pt)
        if size:
            assert lc.xopen(key, rec[:30] + bytes([rec[30] ^ 4]) + rec[31:]) is None


def test_extension_carries_the_key_id():
    """TestAES256GCMExtension's key handle (encrypt_test.go:94-106), for the
    algorithm that is built: the leading 4 bytes of SHA-256(key)."""
    enc = desync_amd.NewXChaCha20Poly1305(bytes.fromhex(TEST_KEY))
    assert enc.storageExtension() == ".xchacha20-poly1305-50d64035" == enc.extension
    assert desync_amd.NewXChaCha20Poly1305(bytes.fromhex(TEST_KEY)).extension == enc.extension
    other = desync_amd.NewXChaCha20Poly1305(bytes.fromhex(OTHER_KEY))
    import hashlib
    assert other.extension == ".xchacha20-poly1305-" + hashlib.sha256(bytes.fromhex(OTHER_KEY)).hexdigest()[:8]
    assert other.extension != enc.extension
    assert desync_amd.EncryptionKeySize == 32


def test_key_validation_uses_the_references_message():
    for new in (desync_amd.NewXChaCha20Poly1305, desync_amd.NewAES256GCM):
        with pytest.raises(ValueError, match="encryption key must be 32 bytes, got 9"):
            new(b"too short")
    with pytest.raises(NotImplementedError, match="not built"):
        desync_amd.NewAES256GCM(bytes.fromhex(TEST_KEY))


@pytest.mark.parametrize("opt,err", [
    # encrypt_test.go:141-146
    (dict(EncryptionKey=TEST_KEY), "without setting encryption to true"),
    (dict(EncryptionAlgorithm="aes-256-gcm"), "without setting encryption to true"),
    (dict(Encryption=True), "no encryption key configured"),
    (dict(Encryption=True, EncryptionKey="not-hex"), "invalid encryption key"),
    (dict(Encryption=True, EncryptionKey=TEST_KEY, EncryptionAlgorithm="rot13"), "unsupported encryption algorithm"),
    (dict(Encryption=True, EncryptionKey=TEST_KEY), ""),
], ids=["key without encryption flag", "algorithm without encryption flag", "encryption without key",
        "invalid key encoding", "unsupported algorithm", "valid"])
def test_storage_converters_validation(opt, err):
    o = desync_amd.StoreOptions(**opt)
    if err:
        with pytest.raises(ValueError) as e:
            o.StorageConverters()
        assert err in str(e.value)
        return
    c = o.StorageConverters()
    assert [type(x).__name__ for x in c] == ["Compressor", "AEADConverter"]
    assert c.storageExtension() == ".cacnk.xchacha20-poly1305-50d64035"
    plain = desync_amd.StoreOptions(Uncompressed=True, **opt).StorageConverters()
    assert plain.storageExtension() == ".xchacha20-poly1305-50d64035" and len(plain) == 1
    assert desync_amd.StoreOptions(Uncompressed=True).StorageConverters().storageExtension() == ""
    assert desync_amd.StoreOptions().StorageConverters().storageExtension() == ".cacnk"


def test_equal_semantics():
    """encrypt_test.go:72-92, for the converters that exist here."""
    enc1 = desync_amd.NewXChaCha20Poly1305(bytes.fromhex(TEST_KEY))
    enc2 = desync_amd.NewXChaCha20Poly1305(bytes.fromhex(TEST_KEY))
    diff = desync_amd.NewXChaCha20Poly1305(bytes.fromhex(OTHER_KEY))
    assert enc1.equal(enc2) and enc2.equal(enc1)
    assert not diff.equal(enc1) and not enc1.equal(diff)
    # a different algorithm with the same key must not be equal either
    alg = desync_amd.AEADConverter("aes-256-gcm", bytes.fromhex(TEST_KEY))
    assert not enc1.equal(alg) and not alg.equal(enc1)
    comp = desync_amd.Compressor()
    assert comp.equal(desync_amd.Compressor()) and not comp.equal(enc1) and not enc1.equal(comp)
    assert comp.storageExtension() == ".cacnk"
    for call in (comp.toStorage, comp.fromStorage):
        with pytest.raises(NotImplementedError, match="zstd is not available"):
            call(b"x")
    a, b = desync_amd.Converters([comp, enc1]), desync_amd.Converters([comp, diff])
    assert a.commonPrefix(b) == 1 and a.commonPrefix(a) == 2


def test_new_entry_points_are_bound_and_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert (_lib.DSX_AEAD_XCHACHA20_POLY1305, _lib.DSX_AEAD_NONCE, _lib.DSX_AEAD_OVERHEAD) == (0, 24, 40)
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dsx.h")) as f:
        header = f.read()
    for name in NEW:
        assert f"int {name}(" in header
    assert f"#define DSX_AEAD_TILE {_lib.DSX_AEAD_TILE}u" in header
    for name in ("NewXChaCha20Poly1305", "NewAES256GCM", "Compressor", "Converters", "StoreOptions",
                 "EncryptionKeySize"):
        assert name in desync_amd.__all__ and hasattr(desync_amd, name), name
    for name in ("Seal", "PutSealed", "WriteLocal", "ReadLocal"):
        assert callable(getattr(desync_amd.DeviceStore, name)), name


def test_abi_version_stays():
    assert _lib.lib().dsx_abi_version() == 5


def test_null_arguments_are_invalid_before_hip():
    """A NULL context is refused before HIP is touched (without a GPU a HIP
    call would fail with another code)."""
    L = _lib.lib()
    E = _lib.DSX_E_INVAL
    key = bytes(32)
    ends = (ctypes.c_uint64 * 1)(5)
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the context is NULL
    n_bad = ctypes.c_uint64()
    tag = (ctypes.c_uint8 * 16)()
    assert L.dsx_aead_seal(None, 0, key, fake, 5, ends, 0, 1, None, fake, 45, None, 0) == E
    assert L.dsx_aead_seal(None, 0, None, None, 0, None, 0, 0, None, None, 0, None, 0) == E
    assert L.dsx_aead_open(None, 0, key, fake, 45, ends, 0, 1, fake, 5, None, None, 0,
                           ctypes.byref(n_bad), 0) == E
    assert L.dsx_selftest_poly1305(None, key, fake, 5, tag) == E
    assert L.dsx_selftest_poly1305(None, None, None, 0, None) == E


def test_local_store_path_naming():
    """nameFromID (local.go:234-239) and chunkIDFromFilename (types.go:44-54)."""
    cid = bytes(range(7, 39))
    ext = ".xchacha20-poly1305-50d64035"
    d, p = chunk_file_name("/srv/store", cid, ext)
    assert d == "/srv/store/0708" and p == f"/srv/store/0708/{cid.hex()}{ext}"
    assert chunk_file_name("base", cid) == ("base/0708", f"base/0708/{cid.hex()}")
    assert chunk_id_from_filename(cid.hex() + ext, ext) == cid
    assert chunk_id_from_filename(cid.hex(), "") == cid
    # other settings' files are skipped, not errors (local.go:148-150)
    assert chunk_id_from_filename(cid.hex() + ".cacnk", ext) is None
    assert chunk_id_from_filename(cid.hex() + ext, "") is None
    assert chunk_id_from_filename(".tmp-cacnk123" + ext, ext) is None
    assert chunk_id_from_filename(cid.hex()[:-2] + ext, ext) is None
    assert chunk_id_from_filename("zz" + cid.hex()[2:] + ext, ext) is None


def test_local_converters_refuse_a_compressor():
    from desync_amd.store import _local_converters
    enc = desync_amd.NewXChaCha20Poly1305(bytes.fromhex(TEST_KEY))
    assert _local_converters(()).storageExtension() == ""
    assert _local_converters([enc]).storageExtension() == enc.extension
    with pytest.raises(ValueError, match="zstd is not available"):
        _local_converters(desync_amd.StoreOptions(Encryption=True, EncryptionKey=TEST_KEY).StorageConverters())
    with pytest.raises(ValueError, match="one AEAD converter"):
        _local_converters([enc, enc])
